// Streaming step of the codec's conv stacks: one chunk of n latent frames through one layer whose state is a ring of its own
// INPUT (include/agx.h "Streaming conv stacks").  Every layer kind is the polyphase form of core.hip: lower_conv on the standard
// packed image of agx_conv_pack,
//     y[co, q t + ph] = epilogue(bias[co] + sum_{g, j, c} Wp[(g J + j) M + co q + ph][c] * x[16 g + c, t s + j d - P]),
// with t running over the n * rt base positions of the step, t0 = pos[b] * rt - Dt, and x read from the ring at (index mod cap).
//
// One chain per output, whatever the schedule.  A lane owns one row m = co q + ph and NT base positions; the KS waves of a
// workgroup own KS fixed contiguous ranges of the (g, j) reduction, each an fmaf chain from 0 in (g, j, c) order, and wave 0 adds
// the KS partial sums in ascending order, then the bias.  KS is a function of the layer alone (stream_split); NT (how many columns
// a lane carries) and the grid only decide which thread runs a chain, never what the chain is.  A wave streams its 64 rows of the
// image (4 KiB contiguous per (g, j)) against operands it loads once and broadcasts across its lanes: at the bottleneck, where a
// chunk is a handful of columns against megabytes of weights, the image stream is what bounds the step.
#include "common.hpp"

namespace agx {

struct StreamArgs {
    const float *W, *bias, *src, *res;
    float *dst;
    const int64_t *pos, *end;
    const int64_t *counts;   // counted form: row b takes its first clamp(counts[b], 0, n) frames
    int n;                   // frames of the step
    int Cin, Cout, M, q, J, s, d, P;
    int nt;            // base positions of the step (n * rt)
    int rt;            // base positions per frame
    int64_t Dt;        // delay in base positions
    int n_in;          // input columns of the step (n * rate_in): the extent of a plain source
    int64_t first_off; // first new input column minus t0 * s (0, or 1 for the upsampling kind)
    int src_cap, res_cap, dst_cap;   // 0 = plain tensor
    int rate_out;
    int epilogue;
    float slope;
};

__device__ __forceinline__ int floor_mod(int64_t a, int cap) {
    const int64_t r = a % cap;
    return int(r < 0 ? r + cap : r);
}

// CNT, the counted form (include/agx.h "Per-row frame counts"): row b takes lim = clamp(counts[b], 0, n) rt of the step's base
// positions.  The count only decides which outputs are stored -- a plain destination gets exact 0 past lim, a ring destination is
// left alone -- never what a chain is: KS, NT and the grid are those of the uncounted step.  The uncounted instances compile it out.
template <int KS, int NT, bool CNT>
__global__ __launch_bounds__(64 * KS) void conv_stream_kernel(const StreamArgs a) {
    __shared__ float red[KS > 1 ? KS * NT * 64 : 1];
    const int lane = threadIdx.x & 63;
    const int ks = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.z;
    const int m = blockIdx.x * 64 + lane;
    const int tb = blockIdx.y * NT;
    const int64_t t0 = a.pos[b] * a.rt - a.Dt;           // workgroup-uniform
    const int mr = m < a.M ? m : a.M - 1;               // lanes past the last row repeat it and store nothing
    int lim = a.nt;                                      // workgroup-uniform: the base positions row b takes
    if (CNT) {
        const int64_t c = a.counts[b];
        lim = int(c < 0 ? 0 : c > a.n ? a.n : c) * a.rt;
        if (tb >= lim) {      // nothing of this tile is taken: the whole workgroup leaves here, before the KS > 1 barrier
            if (!a.dst_cap && ks == 0 && m < a.M) {
                const int co = m / a.q, ph = m - co * a.q;
                for (int i = 0; i < NT && tb + i < a.nt; ++i)
                    a.dst[(size_t(b) * a.Cout + co) * (size_t(a.nt) * a.q) + (tb + i) * a.q + ph] = 0.f;
            }
            return;
        }
    }

    // The NV = 16 NT activation values of one (g, j) -- 16 channels x NT columns -- are loaded once per wave, value v = c NT + i by
    // lane (v mod 64) into register (v / 64), and broadcast to the fmaf chain by v_readlane: 6 memory instructions per (g, j)
    // instead of one per multiply.  A lane therefore tracks ONE column, i = lane mod NT, and 1 or 2 channels.
    constexpr int NV = kWG * NT, NR = (NV + 63) / 64, CSTEP = 64 / NT;
    const int my_i = lane % NT, my_c = lane / NT;
    const int64_t my_idx = (t0 + tb + my_i) * a.s - a.P;
    // ring column (or plain offset) of tap 0 of the lane's column; taps add j d < cap
    const int col0 = a.src_cap ? floor_mod(my_idx, a.src_cap) : int(my_idx - (t0 * a.s + a.first_off));
    const int xpitch = a.src_cap ? a.src_cap : a.n_in;
    const float *__restrict__ xb = a.src + size_t(b) * a.Cin * xpitch;
    const float *__restrict__ W = a.W;

    float acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = 0.f;

    const int G = (a.Cin + kWG - 1) / kWG;
    const int GJ = G * a.J;
    const int chunk = (GJ + KS - 1) / KS;
    const int gj_end = min(GJ, (ks + 1) * chunk);
    // operands of one (g, j): the lane's 16 weights and its 1 or 2 activation values
    auto fetch = [&](int gj, float4 (&wq)[4], int (&xr)[NR]) {
        const int g = gj / a.J, j = gj - g * a.J;
        const float4 *wp = reinterpret_cast<const float4 *>(W + (size_t(gj) * a.M + mr) * kWG);
#pragma unroll
        for (int k = 0; k < 4; ++k) wq[k] = wp[k];
        int col = col0 + j * a.d;
        bool ok = true;
        if (a.src_cap) {
            col = col >= a.src_cap ? col - a.src_cap : col;
        } else {
            ok = col >= 0 && col < a.n_in;       // a plain source holds the step's own columns only
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int ch = g * kWG + my_c + r * CSTEP;            // channels past Cin meet the image's zero padding
            const bool have = ok && lane + 64 * r < NV && ch < a.Cin;
            xr[r] = have ? __float_as_int(xb[size_t(ch) * xpitch + col]) : 0;
        }
    };
    // the loads of (g, j) + 1 are in flight while the chain takes (g, j): the waves of a small step are few and latency-bound
    float4 wn[4];
    int xn[NR];
    int gj = ks * chunk;
    if (gj < gj_end) fetch(gj, wn, xn);
    for (; gj < gj_end; ++gj) {
        float4 wq[4];
        int xr[NR];
#pragma unroll
        for (int k = 0; k < 4; ++k) wq[k] = wn[k];
#pragma unroll
        for (int r = 0; r < NR; ++r) xr[r] = xn[r];
        if (gj + 1 < gj_end) fetch(gj + 1, wn, xn);
        const float w[kWG] = {wq[0].x, wq[0].y, wq[0].z, wq[0].w, wq[1].x, wq[1].y, wq[1].z, wq[1].w,
                              wq[2].x, wq[2].y, wq[2].z, wq[2].w, wq[3].x, wq[3].y, wq[3].z, wq[3].w};
#pragma unroll
        for (int c = 0; c < kWG; ++c)
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int v = c * NT + i;
                acc[i] = fmaf(w[c], __int_as_float(__builtin_amdgcn_readlane(xr[v >> 6], v & 63)), acc[i]);
            }
    }

    if (KS > 1) {
#pragma unroll
        for (int i = 0; i < NT; ++i) red[(ks * NT + i) * 64 + lane] = acc[i];
        __syncthreads();
        if (ks != 0) return;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            float v = red[i * 64 + lane];
            for (int k = 1; k < KS; ++k) v += red[(k * NT + i) * 64 + lane];
            acc[i] = v;
        }
    }
    if (m >= a.M) return;

    const int co = m / a.q, ph = m - co * a.q;
    const float bias = a.bias ? a.bias[co] : 0.f;
    const int64_t end = a.end ? a.end[b] : 0;
    const int n_out = a.nt * a.q;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        if (tb + i >= a.nt) break;
        if (CNT && tb + i >= lim) {                      // past the row's count: zero to a plain tensor, a ring is not written
            if (!a.dst_cap) a.dst[(size_t(b) * a.Cout + co) * n_out + (tb + i) * a.q + ph] = 0.f;
            continue;
        }
        const int64_t jo = (t0 + tb + i) * a.q + ph;     // the output's stream index
        float v = acc[i] + bias;
        if (a.epilogue & AGX_EPI_LEAKY_PRE) v = v > 0.f ? v : v * a.slope;
        if (a.epilogue & AGX_EPI_RESIDUAL) v += a.res[(size_t(b) * a.Cout + co) * a.res_cap + floor_mod(jo, a.res_cap)];
        if (a.epilogue & AGX_EPI_LEAKY_POST) v = v > 0.f ? v : v * a.slope;
        if (a.end && !(jo >= 0 && jo / a.rate_out < end)) v = 0.f;
        if (a.dst_cap)
            a.dst[(size_t(b) * a.Cout + co) * a.dst_cap + floor_mod(jo, a.dst_cap)] = v;
        else
            a.dst[(size_t(b) * a.Cout + co) * n_out + (tb + i) * a.q + ph] = v;
    }
}

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
struct StreamPick {
    int code;       // AGX_OK or the refusal
    bool empty;
    int ks, nt_tile;
    StreamArgs a;
};

// The split of the (g, j) reduction over the waves of a workgroup: a function of the layer alone.
static int stream_split(int c_in, int J) {
    const int gj = ceil_div(c_in, kWG) * J;
    int ks = 1;
    while (ks < 16 && ks * 2 * 4 <= gj) ks *= 2;
    return ks;
}

static StreamPick stream_pick(const char *op, int kind, int c_in, int c_out, int kernel, int stride, int dilation, int batch, int n,
                              int rate_in, int64_t delay_in) {
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

template <int KS, bool CNT>
static void stream_launch_nt(const StreamPick &k, dim3 grid, hipStream_t st) {
    switch (k.nt_tile) {
        case 1: hipLaunchKernelGGL((conv_stream_kernel<KS, 1, CNT>), grid, dim3(64 * KS), 0, st, k.a); break;
        case 4: hipLaunchKernelGGL((conv_stream_kernel<KS, 4, CNT>), grid, dim3(64 * KS), 0, st, k.a); break;
        default: hipLaunchKernelGGL((conv_stream_kernel<KS, 8, CNT>), grid, dim3(64 * KS), 0, st, k.a); break;
    }
}

template <bool CNT>
static void stream_launch(const StreamPick &k, dim3 grid, hipStream_t st) {
    switch (k.ks) {
        case 1: stream_launch_nt<1, CNT>(k, grid, st); break;
        case 2: stream_launch_nt<2, CNT>(k, grid, st); break;
        case 4: stream_launch_nt<4, CNT>(k, grid, st); break;
        case 8: stream_launch_nt<8, CNT>(k, grid, st); break;
        default: stream_launch_nt<16, CNT>(k, grid, st); break;
    }
}

// The one launcher of both entry points: counts == nullptr is the uncounted step, the instances without the count.
static int stream_step(const char *op, int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation,
                       int32_t epilogue, float slope, const float *packed, const float *bias, const float *src, int32_t src_cap,
                       const float *res, int32_t res_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end,
                       const int64_t *counts, int32_t batch, int32_t n, int32_t rate_in, int64_t delay_in, void *stream) {
    StreamPick k = stream_pick(op, kind, c_in, c_out, kernel, stride, dilation, batch, n, rate_in, delay_in);
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
    if (!packed || !src || !dst || !pos) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    if (dst == src || dst == res) return fail(AGX_ERR_BAD_SHAPE, "%s: the destination is one of the sources", op);
    a.W = packed, a.bias = bias, a.src = src, a.res = (epilogue & AGX_EPI_RESIDUAL) ? res : nullptr, a.dst = dst, a.pos = pos, a.end = end;
    a.counts = counts, a.n = n;
    a.src_cap = src_cap, a.res_cap = res_cap, a.dst_cap = dst_cap, a.epilogue = epilogue, a.slope = slope;
    const dim3 grid(ceil_div(a.M, 64), ceil_div(a.nt, k.nt_tile), batch);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (counts)
        stream_launch<true>(k, grid, st);
    else
        stream_launch<false>(k, grid, st);
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
