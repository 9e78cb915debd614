// Sliding-window causal self-attention with the one-sided ALiBi bias: a query at absolute position p = i + q_pos0 sees the
// last W keys, j in [max(0, p - W + 1), p], and nothing else.
//
//     out[b,h,:,i] = sum_j softmax_j( q_i . k_j / scale_div - slope_h (p - j) ) v_j,    j in [max(0, p - W + 1), p]
//
// Build-defined, like the causal form it narrows (attention_causal.hip): W >= p + 1 for every query IS causal attention, W = 1
// returns v_p.  ALiBi needs p - j only, never an absolute position, so the keys may live in a ring: key j sits in column
// j mod ring of a kv row (ring = 0: the linear form, column j), and a stream has no end.
//
// Layouts (channel-major fp32):  q (B, H*Dh, Tq), rows of pitch Tq;  kv (B, 2*H*Dh, .), K rows first, then V rows, rows of
// pitch kv_row_stride;  out (B, H*Dh, Tq).  q and kv have their own base pointers and batch strides, so a (B, 3*H*Dh, T) qkv
// tensor is read in place (linear, q_pos0 = 0).  The keys are the positions 0 .. q_pos0 + Tq - 1: linear needs
// kv_row_stride >= q_pos0 + Tq, a ring needs Tq + min(W - 1, q_pos0) <= ring <= kv_row_stride -- the oldest key the first query
// sees, max(0, q_pos0 - W + 1), must not have been overwritten by the newest, q_pos0 + Tq - 1 (at the start of a stream there is
// nothing older than key 0 to keep).
//
// TWIN CODE: the forward is a copy of attention_causal_kernel<DVT> of attention_causal.hip and the three backward kernels are
// copies of attn_causal_bwd_stats / _dq / _dkv (same tiling, same arithmetic, same fmaf logit helper; the lower edge of the
// mask, the first block of the loops, the ring column and the two hazards below are what differs), kept apart so that the
// causal kernels stay the code they were.  A fix to one belongs in the other too.
//
// Block bounds.  Keys come in blocks of 64 ALIGNED TO ABSOLUTE POSITIONS, block = j / 64, so what a query adds up, and in
// which order, does not depend on the chunk that delivered it.  A workgroup of 128 queries starting at q0 covers the positions
// pmin = q0 + q_pos0 .. pmax = min(q0 + 127, Tq - 1) + q_pos0 and walks the blocks jlo / 64 .. pmax / 64 with
// jlo = max(0, pmin - W + 1): functions of blockIdx alone, so the loop bounds and the V prefetch are workgroup-uniform and
// every thread meets every __syncthreads.  A 64-key block may wrap the ring: K gathers and V staging compute the column per
// element (one add and one conditional subtract from the workgroup's base column; no division in the loop).
//
// Two hazards the causal kernels did not have, and what is done about them:
//  * Leading all-masked blocks.  The causal kernel relies on key 0 being visible to every query: after block 0 its running
//    maximum m is finite.  Here a row can meet a block in which every key is masked BEFORE it has seen any key (T = 130, W = 3:
//    query 127 sees keys 125..127, block 0 is empty for it), and m = -inf, bm = -inf would form (-inf) - (-inf) = NaN.  The
//    exponentials are therefore taken against ms = (mn == -inf ? 0 : mn): for such a block alpha = exp(-inf - 0) = 0 scales
//    l = 0 and o = 0 to themselves, every pe = exp(-inf - 0) = 0, and m stays -inf: the exact identity on (m, l, o).  Once a row
//    has seen a key, mn is finite, ms = mn, and the update is the causal kernel's to the bit.  Every query sees key p (W >= 1),
//    so l > 0 at the end.  (The backward's stats kernel carries a finite sentinel instead of -inf: see there.)
//  * Stale ring columns.  A ring column outside the window holds an older frame, or unwritten memory at the start of a stream.
//    A masked probability is exactly 0, but 0 * NaN = NaN in the PV product: V is staged as zeros wherever the position is
//    outside [jlo, pmax] of the workgroup; K gathers clamp the position into [jlo, pmax] (columns that hold what they should)
//    and the masked score is replaced by -inf with a select, whatever it was.  Inside [jlo, pmax] every column is a frame of
//    this stream, finite, and a masked one meets p = 0: 0 * finite = 0.
#include "mfma_tile.hpp"

namespace agx {

template <int DVT>
__global__ __launch_bounds__(256) void attention_window_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                               int64_t sq, int64_t skv, int krs,
                                                               const float *__restrict__ slopes, float *__restrict__ out, int H,
                                                               int Dh, int Tq, int q_pos0, int W, int ring, float scale_div) {
    constexpr int KB = 64;         // keys per block (two 32-key accumulator tiles)
    constexpr int DH = 32 * DVT;   // head_dim rounded up to the tile
    constexpr int VP = KB + 1;     // LDS pitch of the V block
    extern __shared__ __attribute__((aligned(16))) float vs[];   // [2][DH][VP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int HD = H * Dh;
    const float *qb = q + size_t(b) * sq + size_t(h) * Dh * Tq;
    const float *kb = kv + size_t(b) * skv + size_t(h) * Dh * krs;
    const float *vb = kb + size_t(HD) * krs;
    const int q0 = blockIdx.x * 128;
    const int i = q0 + wave * 32 + li;   // this lane's query
    const int ic = min(i, Tq - 1);
    const int ip = ic + q_pos0;          // its absolute position: the last key it sees
    const float slope = slopes[h], inv_scale = 1.f / scale_div;
    // workgroup-uniform: the positions of the 128 queries, the keys any of them sees, the blocks that hold those keys
    const int pmax = min(q0 + 127, Tq - 1) + q_pos0;
    const int jlo = max(0, q0 + q_pos0 - W + 1);
    const int blk_lo = jlo / KB, blk_hi = pmax / KB;
    const int c0 = ring > 0 ? jlo % ring : jlo;   // the column of key jlo; pmax - jlo < ring (host check), so one wrap at most
    auto col_of = [&](int j) {                    // the column of key j in [jlo, pmax]
        const int c = c0 + (j - jlo);
        return (ring > 0 && c >= ring) ? c - ring : c;
    };

    // ---- the query fragment stays in registers for the whole key loop ----
    float qf[DH / 2];
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) {
        const int d = 2 * s + lh;
        qf[s] = d < Dh ? qb[size_t(d) * Tq + ic] : 0.f;
    }

    f32x16 o[DVT];
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m = -INFINITY, l = 0.f;

    auto stage_v = [&](int blk, float *dst) {   // V[dv < Dh][64 keys of block blk] -> LDS, zeros outside [jlo, pmax] (stale columns are never read)
        for (int e = tid; e < DH * KB; e += 256) {
            const int dv = e / KB, jj = e - dv * KB, j = blk * KB + jj;
            dst[dv * VP + jj] = (dv < Dh && j >= jlo && j <= pmax) ? vb[size_t(dv) * krs + col_of(j)] : 0.f;
        }
    };
    stage_v(blk_lo, vs + (blk_lo & 1) * DH * VP);
    __syncthreads();

    for (int blk = blk_lo; blk <= blk_hi; ++blk) {
        const int j0 = blk * KB;
        float *vcur = vs + (blk & 1) * DH * VP;
        if (blk + 1 <= blk_hi) stage_v(blk + 1, vs + ((blk + 1) & 1) * DH * VP);   // next block streams in meanwhile

        // ---- S^T = K^T Q for this block: rows = keys, columns = queries ----
        f32x16 acc[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t2][r] = 0.f;
        int kcol[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) kcol[t2] = col_of(max(jlo, min(j0 + t2 * 32 + li, pmax)));
#pragma unroll 4
        for (int s = 0; s < DH / 2; ++s) {
            const int d = min(2 * s + lh, Dh - 1);
            float kf[2];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) kf[t2] = kb[size_t(d) * krs + kcol[t2]];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) acc[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[t2], qf[s], acc[t2], 0, 0, 0);
        }

        // ---- scale, one-sided ALiBi, window mask, online softmax (in-lane over the 32 registers + one shuffle) ----
        float bm = -INFINITY;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + t2 * 32 + acc_row(r, lh);
                float s = acc[t2][r] * inv_scale - float(ip - j) * slope;
                s = (j <= ip && j > ip - W) ? s : -INFINITY;   // a select: whatever the masked score was, it is gone
                acc[t2][r] = s;
                bm = fmaxf(bm, s);
            }
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        const float mn = fmaxf(m, bm);                    // -inf until the row has seen its first key
        const float ms = mn == -INFINITY ? 0.f : mn;      // never (-inf) - (-inf): a leading all-masked block is the identity
        const float alpha = expf(m - ms);                 // m = -inf: exp(-inf) = 0 (l = 0, o = 0 stay); a later all-masked block: exp(0) = 1
        float bl = 0.f;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pe = expf(acc[t2][r] - ms);   // masked: exp(-inf) = 0 exactly
                acc[t2][r] = pe;
                bl += pe;
            }
        bl += __shfl_xor(bl, 32);
        l = l * alpha + bl;
        m = mn;
#pragma unroll
        for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;

        // ---- O^T += V P^T : B operand = the probability registers ----
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int jj = t2 * 32 + acc_row(s, lh);
#pragma unroll
                for (int dt = 0; dt < DVT; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vcur[(dt * 32 + li) * VP + jj], acc[t2][s], o[dt], 0, 0, 0);
            }
        __syncthreads();   // the next block's V has been written by everyone; this block's is free
    }

    const float inv = 1.f / l;
    float *ob = out + (size_t(b) * HD + size_t(h) * Dh) * Tq;
    if (i < Tq) {
#pragma unroll
        for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dv = dt * 32 + acc_row(r, lh);
                if (dv < Dh) ob[size_t(dv) * Tq + i] = o[dt][r] * inv;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Backward of the full windowed self-attention (q_pos0 = 0, Tq = Tk = T, linear kv): stats / dq / dkv.
// TWIN CODE of attn_causal_bwd_stats / _dq / _dkv of attention_causal.hip (see the header).  q / kv and dq / dkv are reached
// through base pointers and batch strides (rows of pitch T), so qkv is read and dqkv written in place.  stats and dq walk the
// key blocks from the one that holds key max(0, i0 - W + 1) to the last one their 16 queries see; dkv walks the query blocks
// from j0 to min(T, j0 + 63 + W): the queries that see any of its 64 keys.  A masked (i, j) pair has P = dS = 0 exactly.
constexpr int AW_QB = 16;    // queries per block
constexpr int AW_KB = 64;    // keys per block
constexpr float AW_MASKED = -3.0e38f;   // the stats kernel's score of a masked key (a logit never comes near it)

// The logit of (query i, key j in the window), rounded the same way in all three kernels: the product feeds an explicit fmaf,
// so no contraction can differ between them (lse is built from these values; see attn_causal_bwd_logit).
static __device__ __forceinline__ float attn_window_bwd_logit(float s, float inv, int i, int j, float slope) {
    return fmaf(-float(i - j), slope, s * inv);
}

// one workgroup per (query block, head, item): lse and delta of its 16 queries, delta summed online next to l from dP values
// formed as the dq and dkv kernels form them.  A masked key carries the sentinel AW_MASKED.  The causal twin lets
// exp(sentinel - mn) = 0 do the masking, which holds once m is a real logit; here a row can meet a block it sees nothing of
// while m is still the sentinel, and exp(sentinel - sentinel) = 1 would count its 64 masked keys.  The probability of a masked
// key is therefore a select, 0 whatever mn is: such a block has bs = bd = 0 and alpha = exp(0) = 1, the exact identity on
// (m, l, dl).  For a visible key the arithmetic is the twin's.
__global__ __launch_bounds__(256) void attn_window_bwd_stats_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                    int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                    const float *__restrict__ dout, float *__restrict__ lse,
                                                                    float *__restrict__ delta, int H, int Dh, int T, int W,
                                                                    float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                 // [Dh][QB]
    float *Os = Qs + Dh * AW_QB;    // [Dh][QB]  dO
    float *Ks = Os + Dh * AW_QB;    // [Dh][KB]
    float *Vs = Ks + Dh * AW_KB;    // [Dh][KB]
    float *Ss = Vs + Dh * AW_KB;    // [QB][KB]
    float *Ds = Ss + AW_QB * AW_KB;  // [QB][KB]  dP
    __shared__ float red[AW_QB][16], redd[AW_QB][16];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, i0 = blockIdx.x * AW_QB;
    const int HD = H * Dh;
    const float *qg = q + size_t(b) * sq + size_t(h) * Dh * T, *kg = kv + size_t(b) * skv + size_t(h) * Dh * T, *vg = kg + size_t(HD) * T;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * T;
    const float slope = slopes[h], inv = 1.f / scale_div;
    for (int e = tid; e < Dh * AW_QB; e += 256) {
        const int d = e / AW_QB, qi = e - d * AW_QB, i = min(i0 + qi, T - 1);
        Qs[e] = qg[size_t(d) * T + i];
        Os[e] = dg[size_t(d) * T + i];
    }
    const int rq = tid / 16, rl = tid % 16;   // 16 threads per query row
    float m = AW_MASKED, l = 0.f, dl = 0.f;
    const int jend = min(i0 + AW_QB - 1, T - 1);                    // the last key any of the 16 queries sees (workgroup-uniform)
    const int jbeg = max(0, i0 - W + 1) / AW_KB * AW_KB;            // the block of the first key any of them sees
    for (int j0 = jbeg; j0 <= jend; j0 += AW_KB) {
        __syncthreads();
        for (int e = tid; e < Dh * AW_KB; e += 256) {
            const int d = e / AW_KB, j = e - d * AW_KB, jc = min(j0 + j, T - 1);
            Ks[e] = kg[size_t(d) * T + jc];
            Vs[e] = vg[size_t(d) * T + jc];
        }
        __syncthreads();
        for (int e = tid; e < AW_QB * AW_KB; e += 256) {
            const int qi = e / AW_KB, j = e - qi * AW_KB, i = min(i0 + qi, T - 1);
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AW_QB + qi], Ks[d * AW_KB + j], s);
                dp = fmaf(Os[d * AW_QB + qi], Vs[d * AW_KB + j], dp);
            }
            Ds[e] = dp;
            Ss[e] = (j0 + j <= i && j0 + j > i - W) ? attn_window_bwd_logit(s, inv, i, j0 + j, slope) : AW_MASKED;
        }
        __syncthreads();
        float bm = AW_MASKED;
        for (int j = rl; j < AW_KB; j += 16) bm = fmaxf(bm, Ss[rq * AW_KB + j]);
        red[rq][rl] = bm;
        __syncthreads();
        bm = red[rq][0];
        for (int k = 1; k < 16; ++k) bm = fmaxf(bm, red[rq][k]);
        const float mn = fmaxf(m, bm);
        float bs = 0.f, bd = 0.f;
        for (int j = rl; j < AW_KB; j += 16) {
            const float s = Ss[rq * AW_KB + j];
            const float p = s == AW_MASKED ? 0.f : expf(s - mn);   // a select: 0 for a masked key, also while mn is the sentinel
            bs += p;
            bd = fmaf(p, Ds[rq * AW_KB + j], bd);
        }
        __syncthreads();
        red[rq][rl] = bs;
        redd[rq][rl] = bd;
        __syncthreads();
        bs = bd = 0.f;
        for (int k = 0; k < 16; ++k) {
            bs += red[rq][k];
            bd += redd[rq][k];
        }
        const float alpha = expf(m - mn);   // a leading all-masked block: exp(0) = 1 on l = dl = 0; the first key: exp(-3e38 - mn) = 0
        l = l * alpha + bs;
        dl = dl * alpha + bd;
        m = mn;
    }
    if (rl == 0 && i0 + rq < T) {
        const size_t o = (size_t(b) * H + h) * T + i0 + rq;
        lse[o] = m + logf(l);
        delta[o] = dl / l;
    }
}

// one workgroup per (query block, head, item): dQ of its 16 queries, keys in blocks of 64 from the first to the last visible one
__global__ __launch_bounds__(256) void attn_window_bwd_dq_kernel(const float *__restrict__ q, const float *__restrict__ kv, int64_t sq,
                                                                 int64_t skv, const float *__restrict__ slopes,
                                                                 const float *__restrict__ dout, const float *__restrict__ lse,
                                                                 const float *__restrict__ delta, float *__restrict__ dq_out,
                                                                 int64_t sdq, int H, int Dh, int T, int W, float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                  // [Dh][QB]
    float *Os = Qs + Dh * AW_QB;     // [Dh][QB]  dO
    float *Ks = Os + Dh * AW_QB;     // [Dh][KB]
    float *Vs = Ks + Dh * AW_KB;     // [Dh][KB]
    float *Ss = Vs + Dh * AW_KB;     // [QB][KB]  dS / scale
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, i0 = blockIdx.x * AW_QB;
    const int HD = H * Dh;
    const float *qg = q + size_t(b) * sq + size_t(h) * Dh * T;
    const float *kg = kv + size_t(b) * skv + size_t(h) * Dh * T, *vg = kg + size_t(HD) * T;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * T;
    float *dqg = dq_out + size_t(b) * sdq + size_t(h) * Dh * T;
    const float slope = slopes[h], inv = 1.f / scale_div;
    const size_t so = (size_t(b) * H + h) * T;
    for (int e = tid; e < Dh * AW_QB; e += 256) {
        const int d = e / AW_QB, qi = e - d * AW_QB, i = min(i0 + qi, T - 1);
        Qs[e] = qg[size_t(d) * T + i];
        Os[e] = dg[size_t(d) * T + i];
    }
    constexpr int MAXA = 8;          // dQ elements per thread: Dh * 16 <= 128 * 16 = 8 * 256
    float dq[MAXA];
#pragma unroll
    for (int u = 0; u < MAXA; ++u) dq[u] = 0.f;
    const int jend = min(i0 + AW_QB - 1, T - 1);                    // workgroup-uniform
    const int jbeg = max(0, i0 - W + 1) / AW_KB * AW_KB;
    for (int j0 = jbeg; j0 <= jend; j0 += AW_KB) {
        __syncthreads();
        for (int e = tid; e < Dh * AW_KB; e += 256) {
            const int d = e / AW_KB, j = e - d * AW_KB, jc = min(j0 + j, T - 1);
            Ks[e] = kg[size_t(d) * T + jc];
            Vs[e] = vg[size_t(d) * T + jc];
        }
        __syncthreads();
        for (int e = tid; e < AW_QB * AW_KB; e += 256) {
            const int qi = e / AW_KB, j = e - qi * AW_KB, i = i0 + qi;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AW_QB + qi], Ks[d * AW_KB + j], s);
                dp = fmaf(Os[d * AW_QB + qi], Vs[d * AW_KB + j], dp);
            }
            float ds = 0.f;
            if (i < T && j0 + j <= i && j0 + j > i - W) {     // i - W < j <= i < T: a visible pair; every other one contributes exactly 0
                const float pn = expf(attn_window_bwd_logit(s, inv, i, j0 + j, slope) - lse[so + i]);
                ds = pn * (dp - delta[so + i]) * inv;
            }
            Ss[e] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXA; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * AW_QB) {
                const int d = e / AW_QB, qi = e - d * AW_QB;
                float a = dq[u];
                for (int j = 0; j < AW_KB; ++j) a = fmaf(Ss[qi * AW_KB + j], Ks[d * AW_KB + j], a);
                dq[u] = a;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXA; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * AW_QB) {
            const int d = e / AW_QB, qi = e - d * AW_QB;
            if (i0 + qi < T) dqg[size_t(d) * T + i0 + qi] = dq[u];
        }
    }
}

// one workgroup per (key block, head, item): dK and dV of its 64 keys, queries in blocks of 16 from the first one that sees
// key j0 (query block j0 / 16: 64 is a multiple of 16) to the last one that sees key j0 + 63, query j0 + 63 + W - 1
__global__ __launch_bounds__(256) void attn_window_bwd_dkv_kernel(const float *__restrict__ q, const float *__restrict__ kv, int64_t sq,
                                                                  int64_t skv, const float *__restrict__ slopes,
                                                                  const float *__restrict__ dout, const float *__restrict__ lse,
                                                                  const float *__restrict__ delta, float *__restrict__ dkv,
                                                                  int64_t sdkv, int H, int Dh, int T, int W, float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Ks = sm;                  // [Dh][KB]
    float *Vs = Ks + Dh * AW_KB;     // [Dh][KB]
    float *Qs = Vs + Dh * AW_KB;     // [Dh][QB]
    float *Os = Qs + Dh * AW_QB;     // [Dh][QB]
    float *Ps = Os + Dh * AW_QB;     // [QB][KB]
    float *Ss = Ps + AW_QB * AW_KB;  // [QB][KB]
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, j0 = blockIdx.x * AW_KB;
    const int HD = H * Dh;
    const float *qg = q + size_t(b) * sq + size_t(h) * Dh * T;
    const float *kg = kv + size_t(b) * skv + size_t(h) * Dh * T, *vg = kg + size_t(HD) * T;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * T;
    float *dkg = dkv + size_t(b) * sdkv + size_t(h) * Dh * T, *dvg = dkg + size_t(HD) * T;
    const float slope = slopes[h], inv = 1.f / scale_div;
    const size_t so = (size_t(b) * H + h) * T;
    for (int e = tid; e < Dh * AW_KB; e += 256) {
        const int d = e / AW_KB, j = e - d * AW_KB, jc = min(j0 + j, T - 1);
        Ks[e] = kg[size_t(d) * T + jc];
        Vs[e] = vg[size_t(d) * T + jc];
    }
    constexpr int MAXE = 32;         // dK / dV elements per thread: Dh * 64 <= 128 * 64 = 32 * 256
    float dk[MAXE], dv[MAXE];
#pragma unroll
    for (int u = 0; u < MAXE; ++u) dk[u] = dv[u] = 0.f;
    const int iend = min(T, j0 + AW_KB - 1 + W);   // W <= T (host): no overflow; queries from iend on see none of these keys
    for (int i0 = j0; i0 < iend; i0 += AW_QB) {    // queries before j0 see none of them either
        __syncthreads();
        for (int e = tid; e < Dh * AW_QB; e += 256) {
            const int d = e / AW_QB, qi = e - d * AW_QB, i = min(i0 + qi, T - 1);
            Qs[e] = qg[size_t(d) * T + i];
            Os[e] = (i0 + qi < T) ? dg[size_t(d) * T + i] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < AW_QB * AW_KB; e += 256) {
            const int qi = e / AW_KB, j = e - qi * AW_KB, i = i0 + qi;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AW_QB + qi], Ks[d * AW_KB + j], s);
                dp = fmaf(Os[d * AW_QB + qi], Vs[d * AW_KB + j], dp);
            }
            float pn = 0.f, ds = 0.f;
            if (i < T && j0 + j <= i && j0 + j > i - W) {
                pn = expf(attn_window_bwd_logit(s, inv, i, j0 + j, slope) - lse[so + i]);
                ds = pn * (dp - delta[so + i]) * inv;
            }
            Ps[e] = pn;
            Ss[e] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXE; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * AW_KB) {
                const int d = e / AW_KB, j = e - d * AW_KB;
                float ak = dk[u], av = dv[u];
#pragma unroll
                for (int qi = 0; qi < AW_QB; ++qi) {
                    ak = fmaf(Ss[qi * AW_KB + j], Qs[d * AW_QB + qi], ak);
                    av = fmaf(Ps[qi * AW_KB + j], Os[d * AW_QB + qi], av);
                }
                dk[u] = ak;
                dv[u] = av;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXE; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * AW_KB) {
            const int d = e / AW_KB, j = e - d * AW_KB;
            if (j0 + j < T) {
                dkg[size_t(d) * T + j0 + j] = dk[u];
                dvg[size_t(d) * T + j0 + j] = dv[u];
            }
        }
    }
}

// ------------------------------------------------------------------ host side: one pick feeds launch and name query
struct AttnWindowPick;
#define AGX_ATTN_WINDOW_ARGS                                                                                                        \
    const AttnWindowPick &k, const float *q, const float *kv, int64_t sq, int64_t skv, int krs, const float *slopes, float *out, \
        int H, int Dh, int Tq, int q_pos0, int W, int ring, float scale_div, hipStream_t st
struct AttnWindowRow { const char *name; int (*launch)(AGX_ATTN_WINDOW_ARGS); };
// empty: batch, heads or tq <= 0 -- the entry points return AGX_OK and launch nothing; code: a refusal (fail() was called)
struct AttnWindowPick { const AttnWindowRow *row; const char *bwd_name; dim3 grid; size_t lds; int lds_limit, code; bool empty; };

template <int DVT>
static int run_attention_window(AGX_ATTN_WINDOW_ARGS) {
    auto kern = attention_window_kernel<DVT>;
    static DeviceOnce once;
    if (int rc = prepare_kernel(reinterpret_cast<const void *>(kern), once, k.lds_limit, nullptr, "attention_window")) return rc;
    hipLaunchKernelGGL(kern, k.grid, dim3(256), k.lds, st, q, kv, sq, skv, krs, slopes, out, H, Dh, Tq, q_pos0, W, ring, scale_div);
    return check_launch("attention_window");
}

#define AGX_ATTN_ROW(DVT) {"attention_window<" #DVT ">", run_attention_window<DVT>}
static const AttnWindowRow kAttnWindowRows[3] = {AGX_ATTN_ROW(1), AGX_ATTN_ROW(2), AGX_ATTN_ROW(4)};   // [log2(DVT)]
#undef AGX_ATTN_ROW

static AttnWindowPick attn_window_pick(const char *op, int B, int H, int Dh, int Tq, int W) {
    AttnWindowPick k{};
    k.empty = B <= 0 || H <= 0 || Tq <= 0;
    if (Dh <= 0) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: bad shape head_dim=%d", op, Dh);
    else if (Dh > 128) k.code = fail(AGX_ERR_UNSUPPORTED, "%s: head_dim=%d > 128", op, Dh);
    else if (H > 65535 || B > 65535) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: grid too large", op);
    else if (W < 1) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: window=%d < 1", op, W);
    if (k.code || k.empty) return k;
    const int dvt = Dh <= 32 ? 1 : (Dh <= 64 ? 2 : 4), di = dvt / 2;   // 32-row tiles of the head dim; di = log2(dvt)
    k.row = &kAttnWindowRows[di];
    k.bwd_name = "attn_window_bwd_stats+attn_window_bwd_dq+attn_window_bwd_dkv";
    k.lds = size_t(2) * 32 * dvt * 65 * sizeof(float);                 // the double-buffered V block
    k.lds_limit = k.lds > 48 * 1024 ? 96 * 1024 : 0;
    k.grid = dim3(ceil_div(Tq, 128), H, B);
    return k;
}

// a batch stride must hold one item: the kernels index [b * stride + row * pitch + t]
static int check_window_strides(const char *op, int64_t have, int64_t need, const char *what) {
    return have >= need ? AGX_OK : fail(AGX_ERR_BAD_SHAPE, "%s: %s batch stride %lld < %lld", op, what, (long long)have, (long long)need);
}

static int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t r = a % b;
        a = b;
        b = r;
    }
    return a;
}

static int launch_attention_window_backward(const float *q, const float *kv, int64_t sq, int64_t skv, const float *slopes,
                                            const float *dout, float *dq, float *dkv, int64_t sdq, int64_t sdkv, float *workspace,
                                            int B, int H, int Dh, int T, int W, float scale_div, hipStream_t st) {
    float *lse = workspace, *delta = workspace + size_t(B) * H * T;
    const dim3 gq(ceil_div(T, AW_QB), H, B), gk(ceil_div(T, AW_KB), H, B);
    const size_t l_stats = size_t(2 * Dh * AW_QB + 2 * Dh * AW_KB + 2 * AW_QB * AW_KB) * sizeof(float);
    const size_t l_dq = size_t(2 * Dh * AW_QB + 2 * Dh * AW_KB + AW_QB * AW_KB) * sizeof(float);
    const size_t l_dkv = size_t(2 * Dh * AW_KB + 2 * Dh * AW_QB + 2 * AW_QB * AW_KB) * sizeof(float);
    static DeviceOnce once[3];
    {
        const void *ks[3] = {reinterpret_cast<const void *>(attn_window_bwd_stats_kernel),
                             reinterpret_cast<const void *>(attn_window_bwd_dq_kernel),
                             reinterpret_cast<const void *>(attn_window_bwd_dkv_kernel)};
        for (int i = 0; i < 3; ++i)
            if (int rc = prepare_kernel(ks[i], once[i], 96 * 1024, nullptr, "attention_window_backward")) return rc;   // head_dim 128: 90 KB
    }
    hipLaunchKernelGGL(attn_window_bwd_stats_kernel, gq, dim3(256), l_stats, st, q, kv, sq, skv, slopes, dout, lse, delta, H, Dh, T, W,
                       scale_div);
    hipLaunchKernelGGL(attn_window_bwd_dq_kernel, gq, dim3(256), l_dq, st, q, kv, sq, skv, slopes, dout, lse, delta, dq, sdq, H, Dh, T,
                       W, scale_div);
    hipLaunchKernelGGL(attn_window_bwd_dkv_kernel, gk, dim3(256), l_dkv, st, q, kv, sq, skv, slopes, dout, lse, delta, dkv, sdkv, H, Dh,
                       T, W, scale_div);
    return check_launch("attention_window_backward");
}

}  // namespace agx

extern "C" {

int agx_attention_alibi_window(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride, int64_t kv_row_stride,
                               const float *slopes, float *out, int32_t batch, int32_t heads, int32_t head_dim, int32_t tq,
                               int64_t q_pos0, int32_t window, int32_t kv_ring, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_window";
    const AttnWindowPick k = attn_window_pick(op, batch, heads, head_dim, tq, window);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (q_pos0 < 0) return fail(AGX_ERR_BAD_SHAPE, "%s: q_pos0=%lld < 0", op, (long long)q_pos0);
    if (q_pos0 > (int64_t(1) << 62)) return fail(AGX_ERR_BAD_SHAPE, "%s: q_pos0=%lld is beyond 2^62", op, (long long)q_pos0);
    if (kv_ring < 0) return fail(AGX_ERR_BAD_SHAPE, "%s: kv_ring=%d < 0", op, kv_ring);
    if (kv_ring == 0 && kv_row_stride < q_pos0 + tq)
        return fail(AGX_ERR_BAD_SHAPE, "%s: kv row stride %lld < q_pos0 + tq = %lld (linear kv)", op, (long long)kv_row_stride,
                    (long long)(q_pos0 + tq));
    const int64_t span = tq + std::min<int64_t>(window - 1, q_pos0);   // the keys the call reads: max(0, q_pos0 - window + 1) .. q_pos0 + tq - 1
    if (kv_ring > 0 && span > kv_ring)
        return fail(AGX_ERR_BAD_SHAPE, "%s: kv_ring=%d < tq + min(window - 1, q_pos0) = %lld", op, kv_ring, (long long)span);
    if (kv_ring > kv_row_stride) return fail(AGX_ERR_BAD_SHAPE, "%s: kv_ring=%d > kv row stride %lld", op, kv_ring, (long long)kv_row_stride);
    if (kv_row_stride > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: kv row stride %lld is beyond int32", op, (long long)kv_row_stride);
    if (!q || !kv || !slopes || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_window_strides(op, q_batch_stride, hd * tq, "q")) return rc;
    if (int rc = check_window_strides(op, kv_batch_stride, 2 * hd * kv_row_stride, "kv")) return rc;
    // No query sees further back than position 0: a window beyond the last position is that position + 1 (and fits int32 below).
    const int64_t w = std::min<int64_t>(window, q_pos0 + tq);
    // The kernel indexes in int32.  On a ring every position may be lowered by a multiple of lcm(64, ring): the 64-key block
    // alignment, the ring column and every p - j stay what they were.  The lowered q_pos0 stays >= w - 1, so that the floor
    // "no key before position 0" still bites nowhere it did not.
    int64_t pos = q_pos0;
    if (kv_ring > 0 && pos > w - 1) {
        const int64_t period = 64 / gcd64(64, kv_ring) * int64_t(kv_ring);
        pos -= (pos - (w - 1)) / period * period;
    }
    if (pos + tq + 128 > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: q_pos0 + tq is beyond int32", op);
    return k.row->launch(k, q, kv, q_batch_stride, kv_batch_stride, int(kv_row_stride), slopes, out, heads, head_dim, tq, int(pos),
                         int(w), kv_ring, scale_div, static_cast<hipStream_t>(stream));
}

size_t agx_attention_window_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t t) {
    if (batch <= 0 || heads <= 0 || t <= 0) return 0;
    return size_t(2) * batch * heads * t * sizeof(float);
}

int agx_attention_alibi_window_backward(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                        const float *slopes, const float *out, const float *dout, float *dq, float *dkv,
                                        int64_t dq_batch_stride, int64_t dkv_batch_stride, float *workspace, size_t workspace_bytes,
                                        int32_t batch, int32_t heads, int32_t head_dim, int32_t t, int32_t window, float scale_div,
                                        void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_window_backward";
    const AttnWindowPick k = attn_window_pick(op, batch, heads, head_dim, t, window);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (!q || !kv || !slopes || !out || !dout || !dq || !dkv || !workspace) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    if (workspace_bytes < agx_attention_window_backward_workspace_bytes(batch, heads, t))
        return fail(AGX_ERR_WORKSPACE, "%s: workspace too small", op);
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_window_strides(op, q_batch_stride, hd * t, "q")) return rc;
    if (int rc = check_window_strides(op, kv_batch_stride, 2 * hd * t, "kv")) return rc;
    if (int rc = check_window_strides(op, dq_batch_stride, hd * t, "dq")) return rc;
    if (int rc = check_window_strides(op, dkv_batch_stride, 2 * hd * t, "dkv")) return rc;
    return launch_attention_window_backward(q, kv, q_batch_stride, kv_batch_stride, slopes, dout, dq, dkv, dq_batch_stride,
                                            dkv_batch_stride, workspace, batch, heads, head_dim, t, std::min(window, t), scale_div,
                                            static_cast<hipStream_t>(stream));
}

int agx_attention_window_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t window, int32_t backward,
                                     char *buf, size_t buf_len) {
    using namespace agx;
    const AttnWindowPick k = attn_window_pick(backward ? "attention_alibi_window_backward" : "attention_alibi_window", batch, heads,
                                              head_dim, tq, window);
    if (k.code) return k.code;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "agx_attention_window_kernel_name: NULL buffer");
    snprintf(buf, buf_len, "%s", k.empty ? "none" : (backward ? k.bwd_name : k.row->name));
    return AGX_OK;
}

}  // extern "C"
