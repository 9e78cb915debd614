// The step kernel of the streaming conv stacks and its launch tables, shared by conv_stream.hip (the conv layers of a stack) and
// wavelet_stream.hip (the two steps of a wavelet decoder block).  include/agx.h "Streaming conv stacks", "Streaming wavelet blocks".
//
// Every layer kind is the polyphase form of core.hip: lower_conv on the standard packed image of agx_conv_pack,
//     y[co, q t + ph] = epilogue(bias[co] + sum_{g, j, c} Wp[(g J + j) M + co q + ph][c] * x[16 g + c, t s + j d - P]),
// with t running over the n * rt base positions of the step, t0 = pos[b] * rt - Dt, and x read from the ring at (index mod cap).
//
// One chain per output, whatever the schedule.  A lane owns one row m = co q + ph and NT base positions; the KS waves of a
// workgroup own KS fixed contiguous ranges of the (g, j) reduction, each an fmaf chain from 0 in (g, j, c) order, and wave 0 adds
// the KS partial sums in ascending order, then the bias.  KS is a function of the layer alone (stream_split); NT (how many columns
// a lane carries) and the grid only decide which thread runs a chain, never what the chain is.  A wave streams its 64 rows of the
// image (4 KiB contiguous per (g, j)) against operands it loads once and broadcasts across its lanes: at the bottleneck, where a
// chunk is a handful of columns against megabytes of weights, the image stream is what bounds the step.
#pragma once
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
    int64_t first_off; // first new input column minus t0 * s (0, 1 for the upsampling kind, P for the "same" kind)
    int src_cap, res_cap, dst_cap;   // 0 = plain tensor
    int rate_out;
    int epilogue;
    float slope;
    // FOLD, the operand policy of the wavelet out-step: src is the ring of h (rate fold_rate columns per frame), the conv's
    // operand y[c, v] is formed from it, the per-channel table (Cin, 3 fold_s - 1) = [S_hi | S_lo | tail taps] and end[b]
    const float *tab;
    int fold_s, fold_rate;
    // AFF, the operand policy of a depthwise residual block's dilated conv: the per-channel affine of the grouped k = 1 conv
    const float *scale, *shift;
};

__device__ __forceinline__ int floor_mod(int64_t a, int cap) {
    const int64_t r = a % cap;
    return int(r < 0 ? r + cap : r);
}

// CNT, the counted form (include/agx.h "Per-row frame counts"): row b takes lim = clamp(counts[b], 0, n) rt of the step's base
// positions.  The count only decides which outputs are stored -- a plain destination gets exact 0 past lim, a ring destination is
// left alone -- never what a chain is: KS, NT and the grid are those of the uncounted step.  The uncounted instances compile it out.
//
// FOLD (include/agx.h "Streaming wavelet blocks"): the operand of column v is not loaded but formed from the ring of h, in one
// fixed order: with l0 = floor(v / s), ph = v - l0 s and L = end[b] fold_rate (infinite while the row is live),
//     v < 0 or v >= L s        0
//     v <  (L - 1) s + 1       ph == 0 ? h[l0] S_hi[0] : fmaf(h[l0 + 1], S_lo[ph], h[l0] * S_hi[ph])
//     else                     tail[v - ((L - 1) s + 1)] * h[L - 1]
// Every case is a select on the index: the column l0 + 1 behind ph == 0 may be one the ring has not received yet, and it is
// never read, let alone multiplied by the 0 that S_lo[0] holds.
//
// AFF (include/agx.h "Streaming multires layers and depthwise residual blocks"): the operand of channel c at stream column i is
//     i >= 0 && c < Cin ? fmaf(scale[c], x[c, i], shift[c]) : 0
// -- the causal zero padding lies behind the affine, so a column before the start of the stream gives 0 and not shift[c], and so
// does a channel that pads the last group of 16 (the plain fetch leaves those to the image's zero padding; shift would bias them).
// A select on the index, like FOLD's cases.  Causal, stride 1, ring source: the host refuses everything else.
template <int KS, int NT, bool CNT, bool FOLD = false, bool AFF = false>
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
    int col0 = 0;
    if (!FOLD) col0 = a.src_cap ? floor_mod(my_idx, a.src_cap) : int(my_idx - (t0 * a.s + a.first_off));
    const int xpitch = a.src_cap ? a.src_cap : a.n_in;
    const float *__restrict__ xb = a.src + size_t(b) * a.Cin * xpitch;
    const float *__restrict__ W = a.W;

    // FOLD: the lane's column of tap 0 is v = my_idx (s = d = 1); its frame, phase and ring column, and the row's end
    const int TW = FOLD ? 3 * a.fold_s - 1 : 0;
    int64_t f_l0 = 0, f_live_end = 0, f_tail0 = 0;
    int f_ph0 = 0, f_col0 = 0, f_last = 0;
    bool f_live = true;
    if (FOLD) {
        f_l0 = my_idx / a.fold_s;
        if (f_l0 * a.fold_s > my_idx) --f_l0;                      // floor
        f_ph0 = int(my_idx - f_l0 * a.fold_s);
        f_col0 = floor_mod(f_l0, a.src_cap);
        const int64_t e = a.end[b];
        f_live = e == AGX_STREAM_LIVE;
        if (!f_live) {
            const int64_t L = (e < 0 ? 0 : e) * a.fold_rate;
            f_live_end = L * a.fold_s;                             // first column past the signal
            f_tail0 = (L - 1) * a.fold_s + 1;                      // first of the s - 1 raw tail columns
            f_last = floor_mod(L - 1, a.src_cap);                  // ring column of h[L - 1]
        }
    }

    float acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = 0.f;

    const int G = (a.Cin + kWG - 1) / kWG;
    const int GJ = G * a.J;
    const int chunk = (GJ + KS - 1) / KS;
    const int gj_end = min(GJ, (ks + 1) * chunk);
    // operands of one (g, j): the lane's 16 weights and its 1 or 2 activation values
    // (AFF: also the lane's scale and shift, sc / sh -- the affine is applied where the value is used, so that the load stays in flight)
    auto fetch = [&](int gj, float4 (&wq)[4], int (&xr)[NR], float (&sc)[NR], float (&sh)[NR]) {
        const int g = gj / a.J, j = gj - g * a.J;
        const float4 *wp = reinterpret_cast<const float4 *>(W + (size_t(gj) * a.M + mr) * kWG);
#pragma unroll
        for (int k = 0; k < 4; ++k) wq[k] = wp[k];
        if (FOLD) {
            const int64_t v = my_idx + j;
            int ph = f_ph0 + j;
            const int dl = ph / a.fold_s;
            ph -= dl * a.fold_s;
            const int c0 = (f_col0 + dl) % a.src_cap;
            const int c1 = c0 + 1 == a.src_cap ? 0 : c0 + 1;
            const bool in = v >= 0 && (f_live || v < f_live_end);
            const bool tail = in && !f_live && v >= f_tail0;
            const int te = tail ? 2 * a.fold_s + int(v - f_tail0) : 0;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int ch = g * kWG + my_c + r * CSTEP;
                const bool have = in && lane + 64 * r < NV && ch < a.Cin;
                float y = 0.f;
                if (have) {
                    const float *hr = xb + size_t(ch) * xpitch;
                    const float *tr = a.tab + size_t(ch) * TW;
                    if (tail) {
                        y = tr[te] * hr[f_last];
                    } else {
                        y = hr[c0] * tr[ph];
                        if (ph > 0) y = fmaf(hr[c1], tr[a.fold_s + ph], y);
                    }
                }
                xr[r] = __float_as_int(y);
            }
            return;
        }
        int col = col0 + j * a.d;
        bool ok = true;
        if (AFF) ok = my_idx + int64_t(j) * a.d >= 0;      // the column's stream index, not only its ring column
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
            if (AFF) {      // the select picks all three operands -- x is not read -- so fmaf(0, 0, 0) is the padding's exact 0
                sc[r] = have ? a.scale[ch] : 0.f;
                sh[r] = have ? a.shift[ch] : 0.f;
            }
        }
    };
    // the loads of (g, j) + 1 are in flight while the chain takes (g, j): the waves of a small step are few and latency-bound
    float4 wn[4];
    int xn[NR];
    float scn[NR], shn[NR];
    int gj = ks * chunk;
    if (gj < gj_end) fetch(gj, wn, xn, scn, shn);
    for (; gj < gj_end; ++gj) {
        float4 wq[4];
        int xr[NR];
#pragma unroll
        for (int k = 0; k < 4; ++k) wq[k] = wn[k];
#pragma unroll
        for (int r = 0; r < NR; ++r) xr[r] = AFF ? __float_as_int(fmaf(scn[r], __int_as_float(xn[r]), shn[r])) : xn[r];
        if (gj + 1 < gj_end) fetch(gj + 1, wn, xn, scn, shn);
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

// ------------------------------------------------------------------ host side
struct StreamPick {
    int code;       // AGX_OK or the refusal
    bool empty;
    int ks, nt_tile;
    StreamArgs a;
};

// The kernel choice and index geometry of a layer's step (conv_stream.hip).  same_ok: the private path of the wavelet block's
// steps -- AGX_CONV_SAME (odd kernel, dilation 1): rt = rate_in, Dt = delay_in + (kernel - 1) / 2, reach kernel - 1.  The public
// conv entry points pass false and keep refusing the kind.
StreamPick stream_pick(const char *op, int kind, int c_in, int c_out, int kernel, int stride, int dilation, int batch, int n,
                       int rate_in, int64_t delay_in, bool same_ok = false);

// The one launcher of the conv entry points: counts == nullptr is the uncounted step, the instances without the count.
int stream_step(const char *op, int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation,
                int32_t epilogue, float slope, const float *packed, const float *bias, const float *src, int32_t src_cap,
                const float *res, int32_t res_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end,
                const int64_t *counts, int32_t batch, int32_t n, int32_t rate_in, int64_t delay_in, void *stream, bool same_ok = false,
                bool affine = false, const float *scale = nullptr, const float *shift = nullptr);

template <int KS, bool CNT, bool FOLD, bool AFF>
static void stream_launch_nt(const StreamPick &k, dim3 grid, hipStream_t st) {
    switch (k.nt_tile) {
        case 1: hipLaunchKernelGGL((conv_stream_kernel<KS, 1, CNT, FOLD, AFF>), grid, dim3(64 * KS), 0, st, k.a); break;
        case 4: hipLaunchKernelGGL((conv_stream_kernel<KS, 4, CNT, FOLD, AFF>), grid, dim3(64 * KS), 0, st, k.a); break;
        default: hipLaunchKernelGGL((conv_stream_kernel<KS, 8, CNT, FOLD, AFF>), grid, dim3(64 * KS), 0, st, k.a); break;
    }
}

template <bool CNT, bool FOLD, bool AFF = false>
static void stream_launch(const StreamPick &k, dim3 grid, hipStream_t st) {
    switch (k.ks) {
        case 1: stream_launch_nt<1, CNT, FOLD, AFF>(k, grid, st); break;
        case 2: stream_launch_nt<2, CNT, FOLD, AFF>(k, grid, st); break;
        case 4: stream_launch_nt<4, CNT, FOLD, AFF>(k, grid, st); break;
        case 8: stream_launch_nt<8, CNT, FOLD, AFF>(k, grid, st); break;
        default: stream_launch_nt<16, CNT, FOLD, AFF>(k, grid, st); break;
    }
}

}  // namespace agx
