// Streaming step of the codec's conv stacks: one chunk of n latent frames through one layer whose state is a ring of its own
// INPUT (include/agx.h "Streaming conv stacks").  The step kernel and its launch tables are in conv_stream.hpp, which the steps of
// the wavelet decoder block (wavelet_stream.hip) share; here: the kernel choice, the conv entry points and the ring plumbing.
#include "conv_stream.hpp"

namespace agx {

// buf[b, c, (pos[b] * rate + t) mod cap] = src[b, c, t], t < n_cols: a stack's input chunk into its first ring.  CNT: only the
// columns of the row's first clamp(counts[b], 0, n_cols / rate) frames; the others are neither read nor written.
template <bool CNT>
__global__ __launch_bounds__(256) void ring_write_rate_kernel(float *__restrict__ buf, const float *__restrict__ src,
                                                              const int64_t *__restrict__ pos, const int64_t *__restrict__ counts, int C,
                                                              int n_cols, int cap, int rate) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= C * n_cols) return;
    const int c = e / n_cols, t = e - c * n_cols;
    if (CNT) {
        const int64_t cb = counts[b], n = n_cols / rate;
        if (t >= int(cb < 0 ? 0 : cb > n ? n : cb) * rate) return;
    }
    buf[(size_t(b) * C + c) * cap + floor_mod(pos[b] * rate + t, cap)] = src[size_t(b) * C * n_cols + e];
}

// end[r] = pos[r] for the listed rows (or every row)
__global__ __launch_bounds__(256) void stream_mark_end_kernel(const int64_t *__restrict__ pos, int64_t *__restrict__ end,
                                                              const int64_t *__restrict__ rows, int n_rows, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const int64_t r = rows ? rows[i] : i;
    if (r >= 0 && r < B) end[r] = pos[r];
}

// ------------------------------------------------------------------ host side
// The split of the (g, j) reduction over the waves of a workgroup: a function of the layer alone.
static int stream_split(int c_in, int J) {
    const int gj = ceil_div(c_in, kWG) * J;
    int ks = 1;
    while (ks < 16 && ks * 2 * 4 <= gj) ks *= 2;
    return ks;
}

StreamPick stream_pick(const char *op, int kind, int c_in, int c_out, int kernel, int stride, int dilation, int batch, int n,
                       int rate_in, int64_t delay_in, bool same_ok) {
    StreamPick k{};
    if (batch <= 0 || n <= 0) {
        k.empty = true;
        return k;
    }
    if (c_in <= 0 || c_out <= 0 || kernel <= 0 || stride <= 0 || dilation <= 0 || rate_in <= 0 || delay_in < 0) {
        k.code = fail(AGX_ERR_BAD_SHAPE, "%s: non-positive dimension (Cin=%d Cout=%d K=%d s=%d d=%d rate_in=%d delay_in=%lld)", op, c_in,
                      c_out, kernel, stride, dilation, rate_in, (long long)delay_in);
        return k;
    }
    agx_conv_desc d{};
    d.kind = kind, d.batch = 1, d.c_in = c_in, d.c_out = c_out, d.l_in = 1 << 20, d.kernel = kernel, d.stride = stride;
    d.dilation = dilation, d.groups = 1;
    ConvPlan p;
    if ((k.code = lower_conv(&d, &p)) != AGX_OK) return k;
    StreamArgs &a = k.a;
    a.Cin = c_in, a.Cout = c_out, a.M = p.M, a.q = p.q, a.J = p.J, a.s = p.s, a.d = p.d, a.P = p.P;
    a.first_off = 0;
    switch (kind) {
        case AGX_CONV_CAUSAL:
            if (p.P < 0) {
                k.code = fail(AGX_ERR_UNSUPPORTED, "%s: causal conv with stride > dilation (K - 1) + 1 reads nothing of its past", op);
                return k;
            }
            if (rate_in % stride || delay_in % stride) {
                k.code = fail(AGX_ERR_BAD_SHAPE, "%s: stride %d does not divide rate_in=%d / delay_in=%lld", op, stride, rate_in,
                              (long long)delay_in);
                return k;
            }
            a.rt = rate_in / stride, a.Dt = delay_in / stride;
            break;
        case AGX_CONV_TRANSPOSED:
            if (stride != 1) {
                k.code = fail(AGX_ERR_UNSUPPORTED, "%s: a transposed conv streams with stride 1 only (got %d)", op, stride);
                return k;
            }
            a.rt = rate_in, a.Dt = delay_in;
            break;
        case AGX_CONV_UPSAMPLE:
            if (kernel != 2 * stride + 1) {
                k.code = fail(AGX_ERR_UNSUPPORTED, "%s: an upsampling conv streams with kernel 2 stride + 1 only (K=%d s=%d)", op, kernel,
                              stride);
                return k;
            }
            a.rt = rate_in, a.Dt = delay_in + 1, a.first_off = 1;   // output t reads t - 1 .. t + 1: one base position behind
            break;
        case AGX_CONV_SAME:
            if (same_ok) {      // the wavelet block's steps only: output t reads t - P .. t + P, P base positions behind
                if (kernel % 2 == 0 || dilation != 1) {
                    k.code = fail(AGX_ERR_UNSUPPORTED, "%s: a \"same\" conv streams with an odd kernel and dilation 1 (K=%d d=%d)", op,
                                  kernel, dilation);
                    return k;
                }
                a.rt = rate_in, a.Dt = delay_in + p.P, a.first_off = p.P;
                break;
            }
            [[fallthrough]];
        default:
            k.code = fail(AGX_ERR_UNSUPPORTED, "%s: conv kind %d has no streaming step", op, kind);
            return k;
    }
    if (int64_t(n) * a.rt * a.q > (1 << 24) || int64_t(batch) > 65535) {
        k.code = fail(AGX_ERR_BAD_SHAPE, "%s: a step of %d frames at rate %d (batch %d) is beyond the grid", op, n, a.rt * a.q, batch);
        return k;
    }
    a.nt = n * a.rt;
    a.n_in = n * rate_in;
    a.rate_out = a.rt * a.q;
    k.ks = stream_split(c_in, p.J);
    k.nt_tile = a.nt <= 1 ? 1 : a.nt <= 4 ? 4 : 8;
    return k;
}

// The one launcher of both entry points: counts == nullptr is the uncounted step, the instances without the count.
int stream_step(const char *op, int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation,
                int32_t epilogue, float slope, const float *packed, const float *bias, const float *src, int32_t src_cap,
                const float *res, int32_t res_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end,
                const int64_t *counts, int32_t batch, int32_t n, int32_t rate_in, int64_t delay_in, void *stream, bool same_ok,
                bool affine, const float *scale, const float *shift) {
    // the operand policy of a depthwise block's dilated conv (the padding lies behind the affine): refused by kind before anything else
    if (affine && batch > 0 && n > 0 && (kind != AGX_CONV_CAUSAL || stride != 1 || src_cap == 0))
        return fail(AGX_ERR_UNSUPPORTED, "%s: the per-channel affine is the operand of a stride-1 causal conv reading a ring (kind=%d s=%d "
                    "src_cap=%d)", op, kind, stride, src_cap);
    StreamPick k = stream_pick(op, kind, c_in, c_out, kernel, stride, dilation, batch, n, rate_in, delay_in, same_ok);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    StreamArgs &a = k.a;
    if (epilogue & ~(AGX_EPI_LEAKY_PRE | AGX_EPI_RESIDUAL | AGX_EPI_LEAKY_POST))
        return fail(AGX_ERR_UNSUPPORTED, "%s: epilogue %d (bias, LeakyReLU before / after and the residual are fused)", op, epilogue);
    const int reach = a.P + int(a.first_off);                 // input columns read before the step's first new one
    if (src_cap < 0 || res_cap < 0 || dst_cap < 0) return fail(AGX_ERR_BAD_SHAPE, "%s: negative ring capacity", op);
    if (src_cap == 0 && (reach != 0 || a.s != 1 || a.J != 1))
        return fail(AGX_ERR_BAD_SHAPE, "%s: a plain source holds no history: kernel 1 / stride 1 only (K=%d s=%d)", op, kernel, stride);
    if (src_cap && int64_t(src_cap) < int64_t(reach) + a.n_in)
        return fail(AGX_ERR_BAD_SHAPE, "%s: src_cap=%d < reach %d + %d new columns (the step's writes would alias its history)", op,
                    src_cap, reach, a.n_in);
    const int64_t n_out = int64_t(a.nt) * a.q;
    if (dst_cap && dst_cap < n_out)
        return fail(AGX_ERR_BAD_SHAPE, "%s: dst_cap=%d < %lld new columns (a column would be written twice)", op, dst_cap, (long long)n_out);
    if (epilogue & AGX_EPI_RESIDUAL) {
        if (a.q != 1 || a.s != 1) return fail(AGX_ERR_BAD_SHAPE, "%s: the residual needs a stride-1 layer", op);
        if (res_cap < n_out) return fail(AGX_ERR_BAD_SHAPE, "%s: res_cap=%d < %lld new columns", op, res_cap, (long long)n_out);
        if (!res) return fail(AGX_ERR_NULL_POINTER, "%s: NULL residual ring", op);
    }
    if (affine && (!scale || !shift)) return fail(AGX_ERR_NULL_POINTER, "%s: NULL scale or shift", op);
    if (!packed || !src || !dst || !pos) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    if (dst == src || dst == res) return fail(AGX_ERR_BAD_SHAPE, "%s: the destination is one of the sources", op);
    a.W = packed, a.bias = bias, a.src = src, a.res = (epilogue & AGX_EPI_RESIDUAL) ? res : nullptr, a.dst = dst, a.pos = pos, a.end = end;
    a.counts = counts, a.n = n;
    a.src_cap = src_cap, a.res_cap = res_cap, a.dst_cap = dst_cap, a.epilogue = epilogue, a.slope = slope;
    a.scale = scale, a.shift = shift;
    const dim3 grid(ceil_div(a.M, 64), ceil_div(a.nt, k.nt_tile), batch);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (affine) {
        if (counts)
            stream_launch<true, false, true>(k, grid, st);
        else
            stream_launch<false, false, true>(k, grid, st);
        return check_launch(op);
    }
    if (counts)
        stream_launch<true, false>(k, grid, st);
    else
        stream_launch<false, false>(k, grid, st);
    return check_launch(op);
}

static int ring_write_rate(const char *op, float *buf, const float *src, const int64_t *pos, const int64_t *counts, int32_t batch,
                           int32_t rows, int32_t n_cols, int32_t cap, int32_t rate, void *stream) {
    if (batch <= 0 || rows <= 0 || n_cols <= 0) return AGX_OK;
    if (batch > 65535) return fail(AGX_ERR_BAD_SHAPE, "%s: grid too large", op);
    if (rate < 1) return fail(AGX_ERR_BAD_SHAPE, "%s: rate=%d < 1", op, rate);
    if (n_cols > cap) return fail(AGX_ERR_BAD_SHAPE, "%s: n_cols=%d > cap=%d (a column would be written twice)", op, n_cols, cap);
    if (int64_t(rows) * n_cols + 256 > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: rows * n_cols is beyond int32", op);
    if (!buf || !src || !pos) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    const dim3 grid(ceil_div(rows * n_cols, 256), batch);
    if (counts)
        hipLaunchKernelGGL(ring_write_rate_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), buf, src, pos, counts, rows,
                           n_cols, cap, rate);
    else
        hipLaunchKernelGGL(ring_write_rate_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), buf, src, pos, counts, rows,
                           n_cols, cap, rate);
    return check_launch(op);
}

}  // namespace agx

extern "C" {

int agx_conv_stream_step(int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation, int32_t epilogue,
                         float slope, const float *packed, const float *bias, const float *src, int32_t src_cap, const float *res,
                         int32_t res_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end, int32_t batch, int32_t n,
                         int32_t rate_in, int64_t delay_in, void *stream) {
    return agx::stream_step("conv_stream_step", kind, c_in, c_out, kernel, stride, dilation, epilogue, slope, packed, bias, src, src_cap, res,
                            res_cap, dst, dst_cap, pos, end, nullptr, batch, n, rate_in, delay_in, stream);
}

int agx_conv_stream_step_counted(int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation,
                                 int32_t epilogue, float slope, const float *packed, const float *bias, const float *src, int32_t src_cap,
                                 const float *res, int32_t res_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end,
                                 const int64_t *counts, int32_t batch, int32_t n, int32_t rate_in, int64_t delay_in, void *stream) {
    if (!counts && batch > 0 && n > 0) return agx::fail(AGX_ERR_NULL_POINTER, "conv_stream_step_counted: NULL counts");
    return agx::stream_step("conv_stream_step_counted", kind, c_in, c_out, kernel, stride, dilation, epilogue, slope, packed, bias, src,
                            src_cap, res, res_cap, dst, dst_cap, pos, end, counts, batch, n, rate_in, delay_in, stream);
}

int agx_conv_stream_step_affine(int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation,
                                int32_t epilogue, float slope, const float *packed, const float *bias, const float *scale,
                                const float *shift, const float *src, int32_t src_cap, const float *res, int32_t res_cap, float *dst,
                                int32_t dst_cap, const int64_t *pos, const int64_t *end, int32_t batch, int32_t n, int32_t rate_in,
                                int64_t delay_in, void *stream) {
    return agx::stream_step("conv_stream_step_affine", kind, c_in, c_out, kernel, stride, dilation, epilogue, slope, packed, bias, src,
                            src_cap, res, res_cap, dst, dst_cap, pos, end, nullptr, batch, n, rate_in, delay_in, stream, false, true, scale,
                            shift);
}

int agx_conv_stream_step_affine_counted(int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation,
                                        int32_t epilogue, float slope, const float *packed, const float *bias, const float *scale,
                                        const float *shift, const float *src, int32_t src_cap, const float *res, int32_t res_cap,
                                        float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end, const int64_t *counts,
                                        int32_t batch, int32_t n, int32_t rate_in, int64_t delay_in, void *stream) {
    if (!counts && batch > 0 && n > 0) return agx::fail(AGX_ERR_NULL_POINTER, "conv_stream_step_affine_counted: NULL counts");
    return agx::stream_step("conv_stream_step_affine_counted", kind, c_in, c_out, kernel, stride, dilation, epilogue, slope, packed, bias,
                            src, src_cap, res, res_cap, dst, dst_cap, pos, end, counts, batch, n, rate_in, delay_in, stream, false, true,
                            scale, shift);
}

int agx_conv_stream_kernel_name(int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation, int32_t n,
                                int32_t rate_in, char *buf, size_t buf_len) {
    using namespace agx;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "agx_conv_stream_kernel_name: NULL buffer");
    const StreamPick k = stream_pick("agx_conv_stream_kernel_name", kind, c_in, c_out, kernel, stride, dilation, 1, n, rate_in, 0);
    if (k.code) return k.code;
    if (k.empty)
        snprintf(buf, buf_len, "none");
    else
        snprintf(buf, buf_len, "conv_stream<%d,%d>", k.ks, k.nt_tile);
    return AGX_OK;
}

int agx_ring_write_rate(float *buf, const float *src, const int64_t *pos, int32_t batch, int32_t rows, int32_t n_cols, int32_t cap,
                        int32_t rate, void *stream) {
    return agx::ring_write_rate("ring_write_rate", buf, src, pos, nullptr, batch, rows, n_cols, cap, rate, stream);
}

int agx_ring_write_rate_counted(float *buf, const float *src, const int64_t *pos, const int64_t *counts, int32_t batch, int32_t rows,
                                int32_t n_cols, int32_t cap, int32_t rate, void *stream) {
    if (!counts && batch > 0 && rows > 0 && n_cols > 0) return agx::fail(AGX_ERR_NULL_POINTER, "ring_write_rate_counted: NULL counts");
    return agx::ring_write_rate("ring_write_rate_counted", buf, src, pos, counts, batch, rows, n_cols, cap, rate, stream);
}

int agx_stream_mark_end(const int64_t *pos, int64_t *end, const int64_t *rows, int32_t n_rows, int32_t batch, void *stream) {
    using namespace agx;
    const int count = rows ? n_rows : batch;
    if (batch <= 0 || count <= 0) return AGX_OK;
    if (!pos || !end) return fail(AGX_ERR_NULL_POINTER, "stream_mark_end: NULL pointer");
    hipLaunchKernelGGL(stream_mark_end_kernel, dim3(ceil_div(count, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pos, end, rows,
                       count, batch);
    return check_launch("stream_mark_end");
}

}  // extern "C"
