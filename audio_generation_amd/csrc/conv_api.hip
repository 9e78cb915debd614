// C-ABI entry points of the convolution family: shape checks + kernel dispatch.
#include "conv_kernels.hpp"

namespace agx {
// dx *= gelu'(pre)  (exact erf GELU)
__global__ __launch_bounds__(256) void gelu_grad_mul_kernel(float *__restrict__ dx, const float *__restrict__ pre, int64_t n) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = pre[i];
    dx[i] *= 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
}

// Which family runs a lowered 1-D plan (forward, backward-data, the two launches of the residual-block fallback): launcher and
// name query both read it.  A negative result is a refusal (error code, message set); ring = false leaves the ring kernels out.
enum ConvKernel { CONV_P, CONV_B3, CONV_MFMA, CONV_DIRECT };
static int conv_kernel(const ConvPlan &p, int impl, bool ring = true) {
    ring = ring && tuning().conv_impl == 1;
    if ((impl == AGX_IMPL_AUTO || impl == AGX_IMPL_MFMA) && ring && conv_p_supported(p)) return CONV_P;
    if (impl == AGX_IMPL_MFMA_BF16X3 && ring && conv_b3_supported(p)) return CONV_B3;
    if (impl == AGX_IMPL_AUTO) return conv_mfma_supported(p) ? CONV_MFMA : CONV_DIRECT;
    if (impl == AGX_IMPL_MFMA || impl == AGX_IMPL_MFMA_BF16X3) return CONV_MFMA;
    if (impl == AGX_IMPL_DIRECT) return CONV_DIRECT;
    return fail(AGX_ERR_BAD_SHAPE, "conv: unknown impl %d", impl);
}

static int run_conv(const ConvPlan &p, int impl, const float *x, const float *wp, const float *bias,
                    const float *res, float *y, hipStream_t st) {
    const int k = conv_kernel(p, impl);
    switch (k) {
        case CONV_P: return launch_conv_p(p, x, wp, bias, res, y, st);
        case CONV_B3: return launch_conv_b3(p, x, wp, bias, y, st);
        case CONV_MFMA: return launch_conv_mfma(p, x, wp, bias, res, y, st);
        case CONV_DIRECT: return launch_conv_direct(p, x, wp, bias, res, y, st);
        default: return k;
    }
}

// "<prefix><variant>[:bf16x3]" of the family conv_kernel picks
static int conv_name(const ConvPlan &p, int impl, bool ring, const char *prefix, char *buf, size_t buf_len) {
    const int k = conv_kernel(p, impl, ring);
    if (k < 0) return k;
    const char *v = k == CONV_P ? conv_p_variant(p) : k == CONV_B3 ? conv_b3_variant(p) : k == CONV_MFMA ? conv_mfma_variant(p)
                                                                                                          : conv_direct_variant(p);
    snprintf(buf, buf_len, "%s%s%s", prefix, v, impl == AGX_IMPL_MFMA_BF16X3 ? ":bf16x3" : "");
    return AGX_OK;
}

// The layer's bf16x3 ring kernel reads pre-split planes (1), and can write them as well (2): conv_b3_planes
static int conv_takes_planes(const ConvPlan &p, int impl) {
    return conv_kernel(p, impl) == CONV_B3 ? conv_b3_planes(p) : 0;
}

// Plan of the residual block `d` describes (its first conv with the LeakyReLU epilogue), for the launcher and the name query
static int lower_resblock(const agx_conv_desc *d, ConvPlan *p) {
    if (!d) return fail(AGX_ERR_NULL_POINTER, "resblock: NULL descriptor");
    if (d->kind != AGX_CONV_CAUSAL || d->stride != 1 || d->c_in != d->c_out)
        return fail(AGX_ERR_BAD_SHAPE, "resblock: needs a stride-1 causal conv with c_in == c_out");
    agx_conv_desc d1 = *d;
    d1.epilogue = AGX_EPI_LEAKY_PRE;
    return lower_conv(&d1, p);
}

// Form of the residual block: one kernel (fp32 ring / bf16x3 ring / staged MFMA tiles) or two conv launches
enum ResblockKernel { RB_P, RB_B3, RB_FUSED, RB_TWO };
static ResblockKernel resblock_kernel(const ConvPlan &p, int impl) {
    const bool ring = tuning().rb_impl == 1;
    if (impl != AGX_IMPL_DIRECT && ring && resblock_p_supported(p)) return RB_P;
    if (ring && resblock_b3_supported(p)) return RB_B3;
    if (impl != AGX_IMPL_DIRECT && resblock_fused_supported(p)) return RB_FUSED;
    return RB_TWO;
}
}  // namespace agx

extern "C" {

int agx_conv_forward(const agx_conv_desc *d, const float *x, const float *packed, const float *bias,
                     const float *res, float *y, void *stream) {
    using namespace agx;
    ConvPlan p;
    int rc = lower_conv(d, &p);
    if (rc != AGX_OK) return rc;
    if (!x || !packed || !y) return fail(AGX_ERR_NULL_POINTER, "agx_conv_forward: NULL pointer");
    if ((p.epilogue & AGX_EPI_RESIDUAL) && !res)
        return fail(AGX_ERR_NULL_POINTER, "agx_conv_forward: residual epilogue without res");
    return run_conv(p, d->impl, x, packed, bias, res, y, static_cast<hipStream_t>(stream));
}

size_t agx_planes_bytes(int32_t batch, int32_t channels, int32_t length) {
    if (batch <= 0 || channels <= 0 || length <= 0 || channels % 8 != 0) return 0;
    return size_t(batch) * (channels / 8) * 3 * size_t(length) * 16;
}

int agx_planes_split(const float *x, void *planes, int32_t batch, int32_t channels, int32_t length, void *stream) {
    using namespace agx;
    if (batch <= 0 || channels <= 0 || length <= 0 || channels % 8 != 0)
        return fail(AGX_ERR_BAD_SHAPE, "agx_planes_split: bad shape B=%d C=%d L=%d (C must be a multiple of 8)", batch, channels, length);
    if (!x || !planes) return fail(AGX_ERR_NULL_POINTER, "agx_planes_split: NULL pointer");
    return launch_planes_split(x, planes, batch, channels, length, static_cast<hipStream_t>(stream));
}

int agx_conv_forward_planes(const agx_conv_desc *d, const void *x_planes, const float *packed, const float *bias, float *y,
                            void *y_planes, void *stream) {
    using namespace agx;
    ConvPlan p;
    int rc = lower_conv(d, &p);
    if (rc != AGX_OK) return rc;
    if (!x_planes || !packed || (!y && !y_planes)) return fail(AGX_ERR_NULL_POINTER, "agx_conv_forward_planes: NULL pointer");
    if (!conv_takes_planes(p, d->impl))
        return fail(AGX_ERR_UNSUPPORTED, "agx_conv_forward_planes: the layer has no plane-fed bf16x3 ring form (ask agx_conv_planes_supported first)");
    return launch_conv_b3_planes(p, x_planes, packed, bias, y, y_planes, static_cast<hipStream_t>(stream));
}

int agx_conv_planes_supported(const agx_conv_desc *d) {
    using namespace agx;
    ConvPlan p;
    if (lower_conv(d, &p) != AGX_OK) return 0;
    return conv_takes_planes(p, d->impl);      // 2: the layer can also WRITE planes (one output phase)
}

int agx_conv_bwd_data(const agx_conv_desc *d, const float *dy, const float *packed_bwd, const float *add,
                      const float *mask, float slope, float *dx, void *stream) {
    using namespace agx;
    ConvPlan p;
    int rc = lower_conv_bwd_data(d, &p);
    if (rc != AGX_OK) return rc;
    if (!dy || !packed_bwd || !dx) return fail(AGX_ERR_NULL_POINTER, "agx_conv_bwd_data: NULL pointer");
    p.epilogue = (add ? AGX_EPI_RESIDUAL : 0) | (mask ? AGX_EPI_MASK : 0);
    p.mask = mask;
    p.slope = slope;
    return run_conv(p, d->impl, dy, packed_bwd, nullptr, add, dx, static_cast<hipStream_t>(stream));
}

int agx_conv_bwd_data_gelu(const agx_conv_desc *d, const float *dy, const float *packed_bwd, const float *add,
                           const float *pre, float *dx, void *stream) {
    using namespace agx;
    ConvPlan p;
    int rc = lower_conv_bwd_data(d, &p);
    if (rc != AGX_OK) return rc;
    if (!dy || !packed_bwd || !dx || !pre) return fail(AGX_ERR_NULL_POINTER, "agx_conv_bwd_data_gelu: NULL pointer");
    p.epilogue = add ? AGX_EPI_RESIDUAL : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = run_conv(p, d->impl, dy, packed_bwd, nullptr, add, dx, st);
    if (rc != AGX_OK) return rc;
    // the GELU gradient as a second (elementwise) launch: erf + exp in the conv epilogue cost the MFMA kernels
    // their register budget (spills in every instantiation), and this op only exists on the 225-frame bottleneck
    const int64_t n = int64_t(p.B) * p.Cout * p.Lout;
    hipLaunchKernelGGL(gelu_grad_mul_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, dx, pre, n);
    return check_launch("agx_conv_bwd_data_gelu");
}

int agx_conv_kernel_name(const agx_conv_desc *d, char *buf, size_t buf_len) {
    using namespace agx;
    ConvPlan p;
    int rc = lower_conv(d, &p);
    if (rc != AGX_OK) return rc;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "agx_conv_kernel_name: NULL buffer");
    return conv_name(p, d->impl, true, "", buf, buf_len);
}

size_t agx_resblock_workspace_bytes(const agx_conv_desc *d) {
    if (!d || d->batch <= 0 || d->c_out <= 0 || d->l_in <= 0) return 0;
    return size_t(d->batch) * d->c_out * d->l_in * sizeof(float);
}

int agx_resblock_kernel_name(const agx_conv_desc *d, char *buf, size_t buf_len) {
    using namespace agx;
    ConvPlan p;
    int rc = lower_resblock(d, &p);
    if (rc != AGX_OK) return rc;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "agx_resblock_kernel_name: NULL pointer");
    switch (resblock_kernel(p, d->impl)) {
        case RB_P: snprintf(buf, buf_len, "%s", resblock_p_variant(p)); return AGX_OK;
        case RB_B3: snprintf(buf, buf_len, "%s:bf16x3", resblock_b3_variant(p)); return AGX_OK;
        case RB_FUSED: snprintf(buf, buf_len, "%s%s", resblock_variant(p), p.prec ? ":bf16x3" : ""); return AGX_OK;
        case RB_TWO: return conv_name(p, d->impl, false, "2x:", buf, buf_len);   // (the plan's tile family, as the name always was)
    }
    return AGX_OK;
}

int agx_resblock_forward(const agx_conv_desc *d, const float *x, const float *packed1,
                         const float *bias1, const float *packed2, const float *bias2, float *y,
                         int32_t post_act, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace agx;
    ConvPlan p1;
    int rc = lower_resblock(d, &p1);
    if (rc != AGX_OK) return rc;
    if (!x || !packed1 || !packed2 || !y) return fail(AGX_ERR_NULL_POINTER, "agx_resblock_forward: NULL pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (resblock_kernel(p1, d->impl)) {
        case RB_P: return launch_resblock_p(p1, x, packed1, bias1, packed2, bias2, y, post_act, st);
        case RB_B3: return launch_resblock_b3(p1, x, packed1, bias1, packed2, bias2, y, post_act, st);
        case RB_FUSED: return launch_resblock_fused(p1, x, packed1, bias1, packed2, bias2, y, post_act, st);
        case RB_TWO: break;
    }
    // two launches: h = leaky(conv1(x)+b1) -> workspace;  y = [leaky](x + conv2(h) + b2)
    if (!workspace || workspace_bytes < agx_resblock_workspace_bytes(d))
        return fail(AGX_ERR_WORKSPACE, "resblock: workspace too small (%zu < %zu)", workspace_bytes,
                    agx_resblock_workspace_bytes(d));
    float *h = static_cast<float *>(workspace);
    rc = run_conv(p1, d->impl, x, packed1, bias1, nullptr, h, st);
    if (rc != AGX_OK) return rc;
    agx_conv_desc d2 = *d;
    d2.kernel = 1;
    d2.dilation = 1;
    d2.epilogue = AGX_EPI_RESIDUAL | (post_act ? AGX_EPI_LEAKY_POST : 0);
    ConvPlan p2;
    rc = lower_conv(&d2, &p2);
    if (rc != AGX_OK) return rc;
    return run_conv(p2, d->impl, h, packed2, bias2, x, y, st);
}

int agx_resblock_q4_supported(const agx_conv_desc *d) {
    using namespace agx;
    ConvPlan p;
    if (lower_resblock(d, &p) != AGX_OK) return 0;
    return resblock_kernel(p, d->impl) == RB_P && resblock_p_quads(p) ? 1 : 0;
}

int agx_resblock_forward_q4(const agx_conv_desc *d, const float *x, const float *packed1, const float *bias1,
                            const float *packed2, const float *bias2, float *y, int32_t post_act, int32_t x_is_q4,
                            int32_t y_is_q4, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace agx;
    (void)workspace, (void)workspace_bytes;   // one launch: the workspace of the two-launch form is never needed here
    ConvPlan p1;
    int rc = lower_resblock(d, &p1);
    if (rc != AGX_OK) return rc;
    if (!x || !packed1 || !packed2 || !y) return fail(AGX_ERR_NULL_POINTER, "agx_resblock_forward_q4: NULL pointer");
    if (resblock_kernel(p1, d->impl) != RB_P || !resblock_p_quads(p1))
        return fail(AGX_ERR_UNSUPPORTED, "agx_resblock_forward_q4: the block has no channel-quad form (ask agx_resblock_q4_supported first)");
    return launch_resblock_p_quads(p1, x, packed1, bias1, packed2, bias2, y, post_act, x_is_q4 != 0, y_is_q4 != 0,
                                   static_cast<hipStream_t>(stream));
}

}  // extern "C"
