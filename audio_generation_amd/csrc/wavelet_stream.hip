// Streaming steps of a wavelet decoder block (include/agx.h "Streaming wavelet blocks"): conv_in as a "same"-conv
// step into a ring of the hidden activation h, and conv_out with the polyphase fold fused into its operand fetch -- y, the folded
// signal at s columns per column of h, is never stored.  Both are instances of conv_stream_kernel (conv_stream.hpp): the in-step
// the plain one through the private "same" path of the conv launcher, the out-step the FOLD operand policy.  The per-channel
// phase sums and tail taps come from a small table that agx_wavelet_fold_table writes with the code of the plain fold.
#include "conv_stream.hpp"
#include "wavelet_fold.hpp"

namespace agx {

// table[c] = [S_hi[0 .. s) | S_lo[0 .. s) | kern[P - (s - 1) .. P)], one workgroup per channel
__global__ __launch_bounds__(256) void wavelet_fold_table_kernel(const float *__restrict__ space, const float *__restrict__ sigma,
                                                                 int sigma_len, float *__restrict__ table, int P, int scale) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *kern = sm;            // [P]
    float *s_lo = sm + P;        // [scale]
    float *s_hi = s_lo + scale;  // [scale]
    const int c = blockIdx.x, tid = threadIdx.x;
    wavelet_phase_sums(space, sigma[sigma_len == 1 ? 0 : c], P, scale, kern, s_lo, s_hi);
    float *row = table + size_t(c) * (3 * scale - 1);
    if (tid < scale) {
        row[tid] = s_hi[tid];
        row[scale + tid] = s_lo[tid];
    }
    if (tid < scale - 1) row[2 * scale + tid] = kern[P - (scale - 1) + tid];
}

// Geometry of the out-step: a "same" conv of k taps over y, which runs at rate_h s columns per frame and lags by delay_h s + s.
static StreamPick out_pick(const char *op, int hidden, int c_out, int kernel, int scale, int batch, int n, int rate_h, int64_t delay_h) {
    StreamPick k{};
    if (batch <= 0 || n <= 0) {
        k.empty = true;
        return k;
    }
    if (scale < 2 || scale > 256) {
        k.code = fail(AGX_ERR_BAD_SHAPE, "%s: scale=%d outside 2 .. 256", op, scale);
        return k;
    }
    if (rate_h <= 0 || delay_h < 0 || int64_t(rate_h) * scale > (1 << 24) || delay_h > (int64_t(1) << 40)) {
        k.code = fail(AGX_ERR_BAD_SHAPE, "%s: rate_h=%d / delay_h=%lld", op, rate_h, (long long)delay_h);
        return k;
    }
    return stream_pick(op, AGX_CONV_SAME, hidden, c_out, kernel, 1, 1, batch, n, rate_h * scale, delay_h * scale + scale, true);
}

static int in_step(const char *op, int32_t c_in, int32_t hidden, int32_t kernel, const float *packed, const float *bias, const float *src,
                   int32_t src_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end, const int64_t *counts,
                   int32_t batch, int32_t n, int32_t rate_in, int64_t delay_in, void *stream) {
    if (batch > 0 && n > 0) {
        if (src_cap <= 0 || dst_cap <= 0) return fail(AGX_ERR_BAD_SHAPE, "%s: src and dst are rings (src_cap=%d dst_cap=%d)", op, src_cap, dst_cap);
        if (!end) return fail(AGX_ERR_NULL_POINTER, "%s: NULL end (h is stored as 0 outside the signal)", op);
    }
    return stream_step(op, AGX_CONV_SAME, c_in, hidden, kernel, 1, 1, 0, 0.f, packed, bias, src, src_cap, nullptr, 0, dst, dst_cap, pos, end,
                       counts, batch, n, rate_in, delay_in, stream, true);
}

static int out_step(const char *op, int32_t hidden, int32_t c_out, int32_t kernel, int32_t scale, int32_t epilogue, float slope,
                    const float *packed, const float *bias, const float *table, const float *h, int32_t h_cap, float *dst, int32_t dst_cap,
                    const int64_t *pos, const int64_t *end, const int64_t *counts, int32_t batch, int32_t n, int32_t rate_h,
                    int64_t delay_h, void *stream) {
    StreamPick k = out_pick(op, hidden, c_out, kernel, scale, batch, n, rate_h, delay_h);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    StreamArgs &a = k.a;
    if (epilogue & ~AGX_EPI_LEAKY_PRE) return fail(AGX_ERR_UNSUPPORTED, "%s: epilogue %d (bias and AGX_EPI_LEAKY_PRE are fused)", op, epilogue);
    const int reach = 1 + ceil_div(kernel - 1, scale);        // columns of h read before the step's first new one
    const int64_t n_h = int64_t(n) * rate_h;
    if (h_cap <= 0 || int64_t(h_cap) < reach + n_h)
        return fail(AGX_ERR_BAD_SHAPE, "%s: h_cap=%d < reach %d + %lld new columns (the in-step's writes would alias its history)", op, h_cap,
                    reach, (long long)n_h);
    if (dst_cap < 0 || (dst_cap && dst_cap < a.nt))
        return fail(AGX_ERR_BAD_SHAPE, "%s: dst_cap=%d < %d new columns (a column would be written twice)", op, dst_cap, a.nt);
    if (!packed || !table || !h || !dst || !pos || !end) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    if (dst == h || dst == table) return fail(AGX_ERR_BAD_SHAPE, "%s: the destination is one of the sources", op);
    a.W = packed, a.bias = bias, a.src = h, a.res = nullptr, a.dst = dst, a.pos = pos, a.end = end, a.counts = counts, a.n = n;
    a.src_cap = h_cap, a.res_cap = 0, a.dst_cap = dst_cap, a.epilogue = epilogue, a.slope = slope;
    a.tab = table, a.fold_s = scale, a.fold_rate = rate_h;
    const dim3 grid(ceil_div(a.M, 64), ceil_div(a.nt, k.nt_tile), batch);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (counts)
        stream_launch<true, true>(k, grid, st);
    else
        stream_launch<false, true>(k, grid, st);
    return check_launch(op);
}

}  // namespace agx

extern "C" {

int agx_wavelet_fold_table(const float *space, const float *sigma, int32_t sigma_len, float *table, int32_t channels, int32_t n_points,
                           int32_t scale, void *stream) {
    using namespace agx;
    if (channels <= 0 || n_points <= 0 || scale < 2 || n_points % scale != 0)
        return fail(AGX_ERR_BAD_SHAPE, "wavelet_fold_table: bad shape (scale >= 2 must divide n_points; C=%d P=%d s=%d)", channels, n_points,
                    scale);
    if (n_points > 256 || scale > 256) return fail(AGX_ERR_UNSUPPORTED, "wavelet_fold_table: n_points/scale > 256");
    if (sigma_len != 1 && sigma_len != channels) return fail(AGX_ERR_BAD_SHAPE, "wavelet_fold_table: sigma_len must be 1 or C");
    if (!space || !sigma || !table) return fail(AGX_ERR_NULL_POINTER, "wavelet_fold_table: NULL pointer");
    const size_t lds = (n_points + 2 * scale) * sizeof(float);
    hipLaunchKernelGGL(wavelet_fold_table_kernel, dim3(channels), dim3(256), lds, static_cast<hipStream_t>(stream), space, sigma, sigma_len,
                       table, n_points, scale);
    return check_launch("wavelet_fold_table");
}

int agx_wavelet_stream_in_step(int32_t c_in, int32_t hidden, int32_t kernel, const float *packed, const float *bias, const float *src,
                               int32_t src_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end, int32_t batch, int32_t n,
                               int32_t rate_in, int64_t delay_in, void *stream) {
    return agx::in_step("wavelet_stream_in_step", c_in, hidden, kernel, packed, bias, src, src_cap, dst, dst_cap, pos, end, nullptr, batch, n,
                        rate_in, delay_in, stream);
}

int agx_wavelet_stream_in_step_counted(int32_t c_in, int32_t hidden, int32_t kernel, const float *packed, const float *bias, const float *src,
                                       int32_t src_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end,
                                       const int64_t *counts, int32_t batch, int32_t n, int32_t rate_in, int64_t delay_in, void *stream) {
    if (!counts && batch > 0 && n > 0) return agx::fail(AGX_ERR_NULL_POINTER, "wavelet_stream_in_step_counted: NULL counts");
    return agx::in_step("wavelet_stream_in_step_counted", c_in, hidden, kernel, packed, bias, src, src_cap, dst, dst_cap, pos, end, counts,
                        batch, n, rate_in, delay_in, stream);
}

int agx_wavelet_stream_out_step(int32_t hidden, int32_t c_out, int32_t kernel, int32_t scale, int32_t epilogue, float slope,
                                const float *packed, const float *bias, const float *table, const float *h, int32_t h_cap, float *dst,
                                int32_t dst_cap, const int64_t *pos, const int64_t *end, int32_t batch, int32_t n, int32_t rate_h,
                                int64_t delay_h, void *stream) {
    return agx::out_step("wavelet_stream_out_step", hidden, c_out, kernel, scale, epilogue, slope, packed, bias, table, h, h_cap, dst,
                         dst_cap, pos, end, nullptr, batch, n, rate_h, delay_h, stream);
}

int agx_wavelet_stream_out_step_counted(int32_t hidden, int32_t c_out, int32_t kernel, int32_t scale, int32_t epilogue, float slope,
                                        const float *packed, const float *bias, const float *table, const float *h, int32_t h_cap,
                                        float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end, const int64_t *counts,
                                        int32_t batch, int32_t n, int32_t rate_h, int64_t delay_h, void *stream) {
    if (!counts && batch > 0 && n > 0) return agx::fail(AGX_ERR_NULL_POINTER, "wavelet_stream_out_step_counted: NULL counts");
    return agx::out_step("wavelet_stream_out_step_counted", hidden, c_out, kernel, scale, epilogue, slope, packed, bias, table, h, h_cap,
                         dst, dst_cap, pos, end, counts, batch, n, rate_h, delay_h, stream);
}

int agx_wavelet_stream_in_kernel_name(int32_t c_in, int32_t hidden, int32_t kernel, int32_t n, int32_t rate_in, char *buf, size_t buf_len) {
    using namespace agx;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "agx_wavelet_stream_in_kernel_name: NULL buffer");
    const StreamPick k = stream_pick("agx_wavelet_stream_in_kernel_name", AGX_CONV_SAME, c_in, hidden, kernel, 1, 1, 1, n, rate_in, 0, true);
    if (k.code) return k.code;
    if (k.empty)
        snprintf(buf, buf_len, "none");
    else
        snprintf(buf, buf_len, "conv_stream<%d,%d>", k.ks, k.nt_tile);
    return AGX_OK;
}

int agx_wavelet_stream_out_kernel_name(int32_t hidden, int32_t c_out, int32_t kernel, int32_t scale, int32_t n, int32_t rate_h, char *buf,
                                       size_t buf_len) {
    using namespace agx;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "agx_wavelet_stream_out_kernel_name: NULL buffer");
    const StreamPick k = out_pick("agx_wavelet_stream_out_kernel_name", hidden, c_out, kernel, scale, 1, n, rate_h, 0);
    if (k.code) return k.code;
    if (k.empty)
        snprintf(buf, buf_len, "none");
    else
        snprintf(buf, buf_len, "wavelet_stream_out<%d,%d>", k.ks, k.nt_tile);
    return AGX_OK;
}

}  // extern "C"
