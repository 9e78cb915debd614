// Streaming step of a CausalMultiresConv1d (include/agx.h "Streaming multires layers and depthwise residual blocks"):
// one chunk of n frames of the layer's input ring through the whole cascade of multires_kernel (wavelet.hip), one launch.
//
// The cascade is per channel, so there is no image to stream and no reduction to split: the work is the columns.  At the
// bottleneck a step is 1 to 4 columns per channel row, at the waveform side hundreds -- so rows are packed into a workgroup by
// outputs (as agx_glu_dwconv_step packs them) and long steps are tiled with the receptive field as left halo (as the plain kernel
// tiles a clip).  A workgroup owns R channel rows of one batch entry and one tile of TT columns; per row two LDS rows of
// W = halo + TT floats hold the level's input and its low-pass.
//
// One chain per output, whatever the schedule.  Every value of every level is an fmaf chain from 0 over the taps in ascending k
// on the values of the level below; which thread forms it, R, TT and the ring phase change no operand and no order.  A tile
// position left of the halo's own reach sees a truncated field (the "src >= 0" select below); such a value never reaches a kept
// output, because the halo is the reach of the whole cascade.
//
// No select on the stream index: a column of index < 0 holds 0 in the ring -- the ring starts zero-filled (and reset() zero-fills
// it), and the producer stores exact 0 where its own output index is negative -- which is the cascade's causal zero padding.
#include "mfma_tile.hpp"
#include "conv_stream.hpp"

namespace agx {

constexpr int MRS_THREADS = 256;
constexpr int MRS_U = AGX_MULTIRES_STREAM_TILE / MRS_THREADS;      // outputs a thread carries at most

struct MultiresStreamArgs {
    const float *h0, *h1, *w, *src;
    float *dst;
    const int64_t *pos, *end, *counts;
    int C, n, K, depth, rate, halo;
    int64_t delay;
    int ncols;          // n * rate: the step's columns
    int TT, R;          // tile width, channel rows per workgroup
    int src_cap, dst_cap;
};

template <bool CNT>
__global__ __launch_bounds__(MRS_THREADS) void multires_stream_kernel(const MultiresStreamArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int W = a.halo + a.TT;
    float *lo_a = sm;                          // [R][W]
    float *lo_b = sm + size_t(a.R) * W;        // [R][W]
    float *hk0 = lo_b + size_t(a.R) * W;       // [R][K]
    float *hk1 = hk0 + a.R * a.K;              // [R][K]
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int c0 = blockIdx.x * a.R;
    const int rows = min(a.R, a.C - c0);       // the last workgroup of a batch entry may hold fewer rows
    const int tb = blockIdx.y * a.TT;
    const int64_t j0 = a.pos[b] * a.rate - a.delay;     // stream index of the step's column 0 (workgroup-uniform)
    int lim = a.ncols;                                   // the columns row b takes
    if (CNT) {
        const int64_t c = a.counts[b];
        lim = int(c < 0 ? 0 : c > a.n ? a.n : c) * a.rate;
    }
    const int n_own = min(a.TT, a.ncols - tb);           // columns of this tile
    const int n_out = rows * n_own;

    if (tb >= lim) {      // nothing of this tile is taken (counted form only): zero to a plain tensor, a ring is not written
        if (!a.dst_cap)
            for (int e = tid; e < n_out; e += MRS_THREADS) {
                const int r = e / n_own, t = tb + (e - r * n_own);
                a.dst[(size_t(b) * a.C + c0 + r) * a.ncols + t] = 0.f;
            }
        return;
    }

    // The tile: position i of a row is step column tb - halo + i, stream index j0 + tb - halo + i.  Columns at and behind the
    // row's count (and behind the step's last column, in a ragged tile) are not read: they are staged as 0, and the cascade is
    // causal, so no taken output sees them.
    const int64_t g0 = j0 + tb - a.halo;
    const int base = floor_mod(g0, a.src_cap);
    const int n_live = min(W, lim - tb + a.halo);        // tile positions whose column is below the count
    for (int e = tid; e < rows * W; e += MRS_THREADS) {
        const int r = e / W, i = e - r * W;
        float v = 0.f;
        if (i < n_live) {
            int col = base + i;                          // < 2 src_cap: W <= reach + n rate <= src_cap
            col = col >= a.src_cap ? col - a.src_cap : col;
            v = a.src[(size_t(b) * a.C + c0 + r) * a.src_cap + col];
        }
        lo_a[size_t(r) * W + i] = v;
    }
    for (int e = tid; e < rows * a.K; e += MRS_THREADS) {
        const int r = e / a.K, k = e - r * a.K;
        hk0[e] = a.h0[size_t(c0 + r) * a.K + k];
        hk1[e] = a.h1[size_t(c0 + r) * a.K + k];
    }
    __syncthreads();

    // a thread's outputs: e = tid + 256 u < rows * n_own, row r = e / n_own, tile position halo + (e mod n_own)
    int orow[MRS_U], opos[MRS_U];
    float acc[MRS_U], xin[MRS_U];
#pragma unroll
    for (int u = 0; u < MRS_U; ++u) {
        const int e = tid + MRS_THREADS * u;
        const bool own = e < n_out;
        orow[u] = own ? e / n_own : 0;
        opos[u] = own ? a.halo + (e - orow[u] * n_own) : a.halo;
        acc[u] = 0.f;
        xin[u] = lo_a[size_t(orow[u]) * W + opos[u]];
    }
    float *cur = lo_a, *nxt = lo_b;
    int dil = 1;
    for (int lvl = a.depth; lvl >= 1; --lvl) {
        // high-pass only where it is kept: the tile's own columns
#pragma unroll
        for (int u = 0; u < MRS_U; ++u) {
            if (tid + MRS_THREADS * u >= n_out) break;
            const float *row = cur + size_t(orow[u]) * W;
            const float *hk = hk1 + orow[u] * a.K;
            float hi = 0.f;
            for (int k = 0; k < a.K; ++k) {
                const int s = opos[u] - (a.K - 1 - k) * dil;
                hi = fmaf(hk[k], s >= 0 ? row[s] : 0.f, hi);
            }
            acc[u] = fmaf(a.w[size_t(c0 + orow[u]) * (a.depth + 2) + lvl], hi, acc[u]);
        }
        // low-pass over the whole tile: the next level's input
        for (int e = tid; e < rows * W; e += MRS_THREADS) {
            const int r = e / W, i = e - r * W;
            const float *row = cur + size_t(r) * W;
            const float *hk = hk0 + r * a.K;
            float lo = 0.f;
            for (int k = 0; k < a.K; ++k) {
                const int s = i - (a.K - 1 - k) * dil;
                lo = fmaf(hk[k], s >= 0 ? row[s] : 0.f, lo);
            }
            nxt[e] = lo;
        }
        __syncthreads();
        float *tmp = cur;
        cur = nxt;
        nxt = tmp;
        dil *= 2;
    }

    const int64_t end = a.end ? a.end[b] : 0;
#pragma unroll
    for (int u = 0; u < MRS_U; ++u) {
        if (tid + MRS_THREADS * u >= n_out) break;
        const int r = orow[u], t = tb + opos[u] - a.halo;
        const int c = c0 + r;
        const float *wc = a.w + size_t(c) * (a.depth + 2);
        if (CNT && t >= lim) {                           // past the row's count: zero to a plain tensor, a ring is not written
            if (!a.dst_cap) a.dst[(size_t(b) * a.C + c) * a.ncols + t] = 0.f;
            continue;
        }
        float v = fmaf(wc[0], cur[size_t(r) * W + opos[u]], acc[u]);
        v = fmaf(xin[u], wc[a.depth + 1], v);
        v = gelu_erf(v);
        const int64_t jo = j0 + t;                       // the output's stream index
        if (jo < 0 || (a.end && jo / a.rate >= end)) v = 0.f;
        if (a.dst_cap)
            a.dst[(size_t(b) * a.C + c) * a.dst_cap + floor_mod(jo, a.dst_cap)] = v;
        else
            a.dst[(size_t(b) * a.C + c) * a.ncols + t] = v;
    }
}

static int multires_stream_step(const char *op, const float *h0, const float *h1, const float *w, const float *src, int32_t src_cap,
                                float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end, const int64_t *counts, int32_t batch,
                                int32_t channels, int32_t n, int32_t kernel, int32_t depth, int32_t rate, int64_t delay, void *stream) {
    if (batch <= 0 || n <= 0) return AGX_OK;
    if (channels <= 0 || kernel <= 0 || depth < 0 || depth > 20 || rate <= 0 || delay < 0 || delay > (int64_t(1) << 40))
        return fail(AGX_ERR_BAD_SHAPE, "%s: bad shape (C=%d K=%d depth=%d rate=%d delay=%lld)", op, channels, kernel, depth, rate,
                    (long long)delay);
    const int64_t ncols = int64_t(n) * rate;
    if (ncols > (1 << 24) || batch > 65535 || int64_t(channels) * ncols > 0x7fffffffLL)
        return fail(AGX_ERR_BAD_SHAPE, "%s: a step of %d frames at rate %d (batch %d, C=%d) is beyond the grid", op, n, rate, batch, channels);
    const int64_t halo = int64_t(kernel - 1) * ((int64_t(1) << depth) - 1);
    const int tt = int(ncols < AGX_MULTIRES_STREAM_TILE ? ncols : AGX_MULTIRES_STREAM_TILE);
    const int64_t row_floats = 2 * (halo + tt) + 2 * int64_t(kernel);      // LDS of one channel row
    if (row_floats * int64_t(sizeof(float)) > AGX_MULTIRES_STREAM_LDS_BYTES)
        return fail(AGX_ERR_UNSUPPORTED, "%s: reach %lld + tile %d does not fit %d bytes of LDS", op, (long long)halo, tt,
                    AGX_MULTIRES_STREAM_LDS_BYTES);
    if (src_cap <= 0 || int64_t(src_cap) < halo + ncols)
        return fail(AGX_ERR_BAD_SHAPE, "%s: src_cap=%d < reach %lld + %lld new columns (the step's writes would alias its history)", op,
                    src_cap, (long long)halo, (long long)ncols);
    if (dst_cap < 0 || (dst_cap && dst_cap < ncols))
        return fail(AGX_ERR_BAD_SHAPE, "%s: dst_cap=%d < %lld new columns (a column would be written twice)", op, dst_cap, (long long)ncols);
    if (!h0 || !h1 || !w || !src || !dst || !pos) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    if (dst == src) return fail(AGX_ERR_BAD_SHAPE, "%s: the destination is the source", op);
    MultiresStreamArgs a{};
    a.h0 = h0, a.h1 = h1, a.w = w, a.src = src, a.dst = dst, a.pos = pos, a.end = end, a.counts = counts;
    a.C = channels, a.n = n, a.K = kernel, a.depth = depth, a.rate = rate, a.halo = int(halo), a.delay = delay;
    a.ncols = int(ncols), a.TT = tt, a.src_cap = src_cap, a.dst_cap = dst_cap;
    // rows per workgroup: fill the 256 threads with outputs, within the LDS budget and the channel count
    int r = MRS_THREADS / tt;
    const int fit = int(AGX_MULTIRES_STREAM_LDS_BYTES / (row_floats * int64_t(sizeof(float))));
    r = r < 1 ? 1 : r;
    r = r > fit ? fit : r;
    r = r > channels ? channels : r;
    a.R = r;
    const size_t lds = size_t(r) * row_floats * sizeof(float);
    const dim3 grid(ceil_div(channels, r), ceil_div(a.ncols, tt), batch);
    if (grid.y > 65535) return fail(AGX_ERR_BAD_SHAPE, "%s: too many tiles", op);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (counts)
        hipLaunchKernelGGL(multires_stream_kernel<true>, grid, dim3(MRS_THREADS), lds, st, a);
    else
        hipLaunchKernelGGL(multires_stream_kernel<false>, grid, dim3(MRS_THREADS), lds, st, a);
    return check_launch(op);
}

}  // namespace agx

extern "C" {

int agx_multires_stream_step(const float *h0, const float *h1, const float *w, const float *src, int32_t src_cap, float *dst,
                             int32_t dst_cap, const int64_t *pos, const int64_t *end, int32_t batch, int32_t channels, int32_t n,
                             int32_t kernel, int32_t depth, int32_t rate, int64_t delay, void *stream) {
    return agx::multires_stream_step("multires_stream_step", h0, h1, w, src, src_cap, dst, dst_cap, pos, end, nullptr, batch, channels, n,
                                     kernel, depth, rate, delay, stream);
}

int agx_multires_stream_step_counted(const float *h0, const float *h1, const float *w, const float *src, int32_t src_cap, float *dst,
                                     int32_t dst_cap, const int64_t *pos, const int64_t *end, const int64_t *counts, int32_t batch,
                                     int32_t channels, int32_t n, int32_t kernel, int32_t depth, int32_t rate, int64_t delay,
                                     void *stream) {
    if (!counts && batch > 0 && n > 0) return agx::fail(AGX_ERR_NULL_POINTER, "multires_stream_step_counted: NULL counts");
    return agx::multires_stream_step("multires_stream_step_counted", h0, h1, w, src, src_cap, dst, dst_cap, pos, end, counts, batch,
                                     channels, n, kernel, depth, rate, delay, stream);
}

}  // extern "C"
