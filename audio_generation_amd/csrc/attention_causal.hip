// Causal self-attention with the one-sided ALiBi bias: a query at absolute position p sees the keys j <= p only.
//
//     out[b,h,:,i] = sum_j softmax_j( q_i . k_j / scale_div - slope_h (i + q_pos0 - j) ) v_j,    j in [0, min(i + q_pos0, Tk - 1)]
//
// Build-defined: the reference's Alibi (networks/transformers.py:7-93) is symmetric, -slope_h |i - j| over every key, and has
// no causal branch.  Full causal self-attention is q_pos0 = 0, Tq = Tk = T; a step on a key/value cache that already holds
// Tk - Tq frames is q_pos0 = Tk - Tq.
//
// Layouts (channel-major fp32):  q (B, H*Dh, Tq), rows of pitch Tq;  kv (B, 2*H*Dh, .), K rows first, then V rows, rows of
// pitch kv_row_stride >= Tk (a preallocated cache whose valid length is Tk);  out (B, H*Dh, Tq).  q and kv have their own base
// pointers and batch strides, so a (B, 3*H*Dh, T) qkv tensor is read in place.
//
// TWIN CODE: the forward is a copy of attention_cross_kernel<DVT> of attention_cross.hip and the three backward kernels are
// copies of attn_cross_bwd_stats / _dq / _dkv (same tiling, same arithmetic; the mask, the one-sided bias, the block bounds
// and the strides are what differs), kept apart so that the self-, cross- and dropout-attention kernels stay the code they
// were.  A fix to one belongs in the other too.
//
// Block skipping.  Keys come in blocks of 64.  A workgroup of 128 queries starting at q0 ends its key loop at the last block
// any of its queries can see, nblk = min(Tk - 1, q0 + 127 + q_pos0) / 64 + 1: a function of blockIdx alone, so the loop bound
// and the V prefetch of blk + 1 are workgroup-uniform and every thread meets every __syncthreads.  There is no finer skip:
// a wave-uniform branch around the MFMAs of a block that only the later waves of the workgroup see was measured and made no
// difference (B = 32, H = 8, Dh = 64: 92.4 against 93.4 us at T = 225, 1030 against 1034 us at T = 1125), so the loop body
// stays the straight-line code of its twin.
//
// Two hazards, and what is done about them:
//  * All-masked blocks.  A row can meet a block in which every key is masked (the other rows of its workgroup reach further).
//    Key 0 is visible to every query (q_pos0 >= 0), so after block 0 the running maximum m is finite; an all-masked block then
//    has bm = -inf, mn = max(m, bm) = m, alpha = exp(0) = 1, pe = exp(-inf) = 0: the identity on (m, l, o), exactly what the
//    block left out of the loop would be.  mn is never -inf, so (-inf) - (-inf) is never formed.
//  * Garbage in masked positions.  A masked probability is exactly 0, but 0 * NaN = NaN in the PV product.  V positions >= Tk
//    (the unwritten tail of a cache) are staged as zeros; K loads clamp the column into [0, Tk) and the masked score is
//    replaced by -inf with a select, whatever it was.  Nothing at or beyond column Tk of a kv row is read.
#include "mfma_tile.hpp"

namespace agx {

template <int DVT>
__global__ __launch_bounds__(256) void attention_causal_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                               int64_t sq, int64_t skv, int krs,
                                                               const float *__restrict__ slopes, float *__restrict__ out, int H,
                                                               int Dh, int Tq, int Tk, int q_pos0, float scale_div) {
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
    const int nblk = min(Tk - 1, q0 + 127 + q_pos0) / KB + 1;   // workgroup-uniform: the last block any of the 128 queries sees

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

    auto stage_v = [&](int blk, float *dst) {   // V[dv < Dh][64 keys of block blk] -> LDS, zeros outside (a cache's tail is never read)
        for (int e = tid; e < DH * KB; e += 256) {
            const int dv = e / KB, jj = e - dv * KB, j = blk * KB + jj;
            dst[dv * VP + jj] = (dv < Dh && j < Tk) ? vb[size_t(dv) * krs + j] : 0.f;
        }
    };
    stage_v(0, vs);
    __syncthreads();

    for (int blk = 0; blk < nblk; ++blk) {
        const int j0 = blk * KB;
        float *vcur = vs + (blk & 1) * DH * VP;
        if (blk + 1 < nblk) stage_v(blk + 1, vs + ((blk + 1) & 1) * DH * VP);   // next block streams in meanwhile

        // ---- S^T = K^T Q for this block: rows = keys, columns = queries ----
        f32x16 acc[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t2][r] = 0.f;
        int kcol[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) kcol[t2] = min(j0 + t2 * 32 + li, Tk - 1);
#pragma unroll 4
        for (int s = 0; s < DH / 2; ++s) {
            const int d = min(2 * s + lh, Dh - 1);
            float kf[2];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) kf[t2] = kb[size_t(d) * krs + kcol[t2]];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) acc[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[t2], qf[s], acc[t2], 0, 0, 0);
        }

        // ---- scale, one-sided ALiBi, causal mask, online softmax (in-lane over the 32 registers + one shuffle) ----
        float bm = -INFINITY;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + t2 * 32 + acc_row(r, lh);
                float s = acc[t2][r] * inv_scale - float(ip - j) * slope;
                s = (j <= ip && j < Tk) ? s : -INFINITY;   // a select: whatever the masked score was, it is gone
                acc[t2][r] = s;
                bm = fmaxf(bm, s);
            }
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        const float mn = fmaxf(m, bm);            // finite: block 0 holds key 0, which every query sees
        const float alpha = expf(m - mn);         // first block: exp(-inf) = 0; an all-masked block: exp(0) = 1
        float bl = 0.f;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pe = expf(acc[t2][r] - mn);   // masked: exp(-inf) = 0 exactly
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
// Backward of the full causal self-attention (q_pos0 = 0, Tq = Tk = T): stats / dq / dkv.
// TWIN CODE of attn_cross_bwd_stats / _dq / _dkv of attention_cross.hip (see the header).  q / kv and dq / dkv are reached
// through base pointers and batch strides (rows of pitch T), so qkv is read and dqkv written in place.  stats and dq stop at
// the last key block their 16 queries see, dkv starts at the first query block that sees its 64 keys; a masked (i, j) pair
// has P = dS = 0 exactly.
constexpr int AK_QB = 16;    // queries per block
constexpr int AK_KB = 64;    // keys per block

// The logit of (query i, key j <= i), rounded the same way in all three kernels: the product feeds an explicit fmaf, so no
// contraction can differ between them (lse is built from these values; see attn_cross_bwd_logit).
static __device__ __forceinline__ float attn_causal_bwd_logit(float s, float inv, int i, int j, float slope) {
    return fmaf(-float(i - j), slope, s * inv);
}

// one workgroup per (query block, head, item): lse and delta of its 16 queries, delta summed online next to l from dP values
// formed as the dq and dkv kernels form them.  A masked key carries the sentinel -3.0e38: block 0 holds key 0, which every
// query sees, so from block 0 on m is a real logit and exp(sentinel - mn) = 0 exactly, also in a block a row sees nothing of.
__global__ __launch_bounds__(256) void attn_causal_bwd_stats_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                    int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                    const float *__restrict__ dout, float *__restrict__ lse,
                                                                    float *__restrict__ delta, int H, int Dh, int T, float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                 // [Dh][QB]
    float *Os = Qs + Dh * AK_QB;    // [Dh][QB]  dO
    float *Ks = Os + Dh * AK_QB;    // [Dh][KB]
    float *Vs = Ks + Dh * AK_KB;    // [Dh][KB]
    float *Ss = Vs + Dh * AK_KB;    // [QB][KB]
    float *Ds = Ss + AK_QB * AK_KB;  // [QB][KB]  dP
    __shared__ float red[AK_QB][16], redd[AK_QB][16];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, i0 = blockIdx.x * AK_QB;
    const int HD = H * Dh;
    const float *qg = q + size_t(b) * sq + size_t(h) * Dh * T, *kg = kv + size_t(b) * skv + size_t(h) * Dh * T, *vg = kg + size_t(HD) * T;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * T;
    const float slope = slopes[h], inv = 1.f / scale_div;
    for (int e = tid; e < Dh * AK_QB; e += 256) {
        const int d = e / AK_QB, qi = e - d * AK_QB, i = min(i0 + qi, T - 1);
        Qs[e] = qg[size_t(d) * T + i];
        Os[e] = dg[size_t(d) * T + i];
    }
    const int rq = tid / 16, rl = tid % 16;   // 16 threads per query row
    float m = -3.0e38f, l = 0.f, dl = 0.f;
    const int jend = min(i0 + AK_QB - 1, T - 1);   // the last key any of the 16 queries sees (workgroup-uniform)
    for (int j0 = 0; j0 <= jend; j0 += AK_KB) {
        __syncthreads();
        for (int e = tid; e < Dh * AK_KB; e += 256) {
            const int d = e / AK_KB, j = e - d * AK_KB, jc = min(j0 + j, T - 1);
            Ks[e] = kg[size_t(d) * T + jc];
            Vs[e] = vg[size_t(d) * T + jc];
        }
        __syncthreads();
        for (int e = tid; e < AK_QB * AK_KB; e += 256) {
            const int qi = e / AK_KB, j = e - qi * AK_KB, i = min(i0 + qi, T - 1);
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AK_QB + qi], Ks[d * AK_KB + j], s);
                dp = fmaf(Os[d * AK_QB + qi], Vs[d * AK_KB + j], dp);
            }
            Ds[e] = dp;
            Ss[e] = (j0 + j <= i) ? attn_causal_bwd_logit(s, inv, i, j0 + j, slope) : -3.0e38f;
        }
        __syncthreads();
        float bm = -3.0e38f;
        for (int j = rl; j < AK_KB; j += 16) bm = fmaxf(bm, Ss[rq * AK_KB + j]);
        red[rq][rl] = bm;
        __syncthreads();
        bm = red[rq][0];
        for (int k = 1; k < 16; ++k) bm = fmaxf(bm, red[rq][k]);
        const float mn = fmaxf(m, bm);
        float bs = 0.f, bd = 0.f;
        for (int j = rl; j < AK_KB; j += 16) {
            const float p = expf(Ss[rq * AK_KB + j] - mn);   // 0 for a masked key
            bs += p;
            bd = fmaf(p, Ds[rq * AK_KB + j], bd);
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
        const float alpha = expf(m - mn);
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

// one workgroup per (query block, head, item): dQ of its 16 queries, keys in blocks of 64 up to the last visible one
__global__ __launch_bounds__(256) void attn_causal_bwd_dq_kernel(const float *__restrict__ q, const float *__restrict__ kv, int64_t sq,
                                                                 int64_t skv, const float *__restrict__ slopes,
                                                                 const float *__restrict__ dout, const float *__restrict__ lse,
                                                                 const float *__restrict__ delta, float *__restrict__ dq_out,
                                                                 int64_t sdq, int H, int Dh, int T, float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                  // [Dh][QB]
    float *Os = Qs + Dh * AK_QB;     // [Dh][QB]  dO
    float *Ks = Os + Dh * AK_QB;     // [Dh][KB]
    float *Vs = Ks + Dh * AK_KB;     // [Dh][KB]
    float *Ss = Vs + Dh * AK_KB;     // [QB][KB]  dS / scale
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, i0 = blockIdx.x * AK_QB;
    const int HD = H * Dh;
    const float *qg = q + size_t(b) * sq + size_t(h) * Dh * T;
    const float *kg = kv + size_t(b) * skv + size_t(h) * Dh * T, *vg = kg + size_t(HD) * T;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * T;
    float *dqg = dq_out + size_t(b) * sdq + size_t(h) * Dh * T;
    const float slope = slopes[h], inv = 1.f / scale_div;
    const size_t so = (size_t(b) * H + h) * T;
    for (int e = tid; e < Dh * AK_QB; e += 256) {
        const int d = e / AK_QB, qi = e - d * AK_QB, i = min(i0 + qi, T - 1);
        Qs[e] = qg[size_t(d) * T + i];
        Os[e] = dg[size_t(d) * T + i];
    }
    constexpr int MAXA = 8;          // dQ elements per thread: Dh * 16 <= 128 * 16 = 8 * 256
    float dq[MAXA];
#pragma unroll
    for (int u = 0; u < MAXA; ++u) dq[u] = 0.f;
    const int jend = min(i0 + AK_QB - 1, T - 1);   // workgroup-uniform
    for (int j0 = 0; j0 <= jend; j0 += AK_KB) {
        __syncthreads();
        for (int e = tid; e < Dh * AK_KB; e += 256) {
            const int d = e / AK_KB, j = e - d * AK_KB, jc = min(j0 + j, T - 1);
            Ks[e] = kg[size_t(d) * T + jc];
            Vs[e] = vg[size_t(d) * T + jc];
        }
        __syncthreads();
        for (int e = tid; e < AK_QB * AK_KB; e += 256) {
            const int qi = e / AK_KB, j = e - qi * AK_KB, i = i0 + qi;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AK_QB + qi], Ks[d * AK_KB + j], s);
                dp = fmaf(Os[d * AK_QB + qi], Vs[d * AK_KB + j], dp);
            }
            float ds = 0.f;
            if (i < T && j0 + j <= i) {     // j <= i < T: a visible pair; every other one contributes exactly 0
                const float pn = expf(attn_causal_bwd_logit(s, inv, i, j0 + j, slope) - lse[so + i]);
                ds = pn * (dp - delta[so + i]) * inv;
            }
            Ss[e] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXA; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * AK_QB) {
                const int d = e / AK_QB, qi = e - d * AK_QB;
                float a = dq[u];
                for (int j = 0; j < AK_KB; ++j) a = fmaf(Ss[qi * AK_KB + j], Ks[d * AK_KB + j], a);
                dq[u] = a;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXA; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * AK_QB) {
            const int d = e / AK_QB, qi = e - d * AK_QB;
            if (i0 + qi < T) dqg[size_t(d) * T + i0 + qi] = dq[u];
        }
    }
}

// one workgroup per (key block, head, item): dK and dV of its 64 keys, queries in blocks of 16 from the first one that sees
// key j0 (query block j0 / 16: 64 is a multiple of 16)
__global__ __launch_bounds__(256) void attn_causal_bwd_dkv_kernel(const float *__restrict__ q, const float *__restrict__ kv, int64_t sq,
                                                                  int64_t skv, const float *__restrict__ slopes,
                                                                  const float *__restrict__ dout, const float *__restrict__ lse,
                                                                  const float *__restrict__ delta, float *__restrict__ dkv,
                                                                  int64_t sdkv, int H, int Dh, int T, float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Ks = sm;                  // [Dh][KB]
    float *Vs = Ks + Dh * AK_KB;     // [Dh][KB]
    float *Qs = Vs + Dh * AK_KB;     // [Dh][QB]
    float *Os = Qs + Dh * AK_QB;     // [Dh][QB]
    float *Ps = Os + Dh * AK_QB;     // [QB][KB]
    float *Ss = Ps + AK_QB * AK_KB;  // [QB][KB]
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, j0 = blockIdx.x * AK_KB;
    const int HD = H * Dh;
    const float *qg = q + size_t(b) * sq + size_t(h) * Dh * T;
    const float *kg = kv + size_t(b) * skv + size_t(h) * Dh * T, *vg = kg + size_t(HD) * T;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * T;
    float *dkg = dkv + size_t(b) * sdkv + size_t(h) * Dh * T, *dvg = dkg + size_t(HD) * T;
    const float slope = slopes[h], inv = 1.f / scale_div;
    const size_t so = (size_t(b) * H + h) * T;
    for (int e = tid; e < Dh * AK_KB; e += 256) {
        const int d = e / AK_KB, j = e - d * AK_KB, jc = min(j0 + j, T - 1);
        Ks[e] = kg[size_t(d) * T + jc];
        Vs[e] = vg[size_t(d) * T + jc];
    }
    constexpr int MAXE = 32;         // dK / dV elements per thread: Dh * 64 <= 128 * 64 = 32 * 256
    float dk[MAXE], dv[MAXE];
#pragma unroll
    for (int u = 0; u < MAXE; ++u) dk[u] = dv[u] = 0.f;
    for (int i0 = j0; i0 < T; i0 += AK_QB) {   // queries before j0 see none of these keys
        __syncthreads();
        for (int e = tid; e < Dh * AK_QB; e += 256) {
            const int d = e / AK_QB, qi = e - d * AK_QB, i = min(i0 + qi, T - 1);
            Qs[e] = qg[size_t(d) * T + i];
            Os[e] = (i0 + qi < T) ? dg[size_t(d) * T + i] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < AK_QB * AK_KB; e += 256) {
            const int qi = e / AK_KB, j = e - qi * AK_KB, i = i0 + qi;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AK_QB + qi], Ks[d * AK_KB + j], s);
                dp = fmaf(Os[d * AK_QB + qi], Vs[d * AK_KB + j], dp);
            }
            float pn = 0.f, ds = 0.f;
            if (i < T && j0 + j <= i) {
                pn = expf(attn_causal_bwd_logit(s, inv, i, j0 + j, slope) - lse[so + i]);
                ds = pn * (dp - delta[so + i]) * inv;
            }
            Ps[e] = pn;
            Ss[e] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXE; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * AK_KB) {
                const int d = e / AK_KB, j = e - d * AK_KB;
                float ak = dk[u], av = dv[u];
#pragma unroll
                for (int qi = 0; qi < AK_QB; ++qi) {
                    ak = fmaf(Ss[qi * AK_KB + j], Qs[d * AK_QB + qi], ak);
                    av = fmaf(Ps[qi * AK_KB + j], Os[d * AK_QB + qi], av);
                }
                dk[u] = ak;
                dv[u] = av;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXE; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * AK_KB) {
            const int d = e / AK_KB, j = e - d * AK_KB;
            if (j0 + j < T) {
                dkg[size_t(d) * T + j0 + j] = dk[u];
                dvg[size_t(d) * T + j0 + j] = dv[u];
            }
        }
    }
}

// ------------------------------------------------------------------ host side: one pick feeds launch and name query
struct AttnCausalPick;
#define AGX_ATTN_CAUSAL_ARGS                                                                                                        \
    const AttnCausalPick &k, const float *q, const float *kv, int64_t sq, int64_t skv, int krs, const float *slopes, float *out, \
        int H, int Dh, int Tq, int Tk, int q_pos0, float scale_div, hipStream_t st
struct AttnCausalRow { const char *name; int (*launch)(AGX_ATTN_CAUSAL_ARGS); };
// empty: batch, heads, tq or tk <= 0 -- the entry points return AGX_OK and launch nothing; code: a refusal (fail() was called)
struct AttnCausalPick { const AttnCausalRow *row; const char *bwd_name; dim3 grid; size_t lds; int lds_limit, code; bool empty; };

template <int DVT>
static int run_attention_causal(AGX_ATTN_CAUSAL_ARGS) {
    auto kern = attention_causal_kernel<DVT>;
    static DeviceOnce once;
    if (int rc = prepare_kernel(reinterpret_cast<const void *>(kern), once, k.lds_limit, nullptr, "attention_causal")) return rc;
    hipLaunchKernelGGL(kern, k.grid, dim3(256), k.lds, st, q, kv, sq, skv, krs, slopes, out, H, Dh, Tq, Tk, q_pos0, scale_div);
    return check_launch("attention_causal");
}

#define AGX_ATTN_ROW(DVT) {"attention_causal<" #DVT ">", run_attention_causal<DVT>}
static const AttnCausalRow kAttnCausalRows[3] = {AGX_ATTN_ROW(1), AGX_ATTN_ROW(2), AGX_ATTN_ROW(4)};   // [log2(DVT)]
#undef AGX_ATTN_ROW

static AttnCausalPick attn_causal_pick(const char *op, int B, int H, int Dh, int Tq, int Tk) {
    AttnCausalPick k{};
    k.empty = B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0;
    if (Dh <= 0) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: bad shape head_dim=%d", op, Dh);
    else if (Dh > 128) k.code = fail(AGX_ERR_UNSUPPORTED, "%s: head_dim=%d > 128", op, Dh);
    else if (H > 65535 || B > 65535) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: grid too large", op);
    if (k.code || k.empty) return k;
    const int dvt = Dh <= 32 ? 1 : (Dh <= 64 ? 2 : 4), di = dvt / 2;   // 32-row tiles of the head dim; di = log2(dvt)
    k.row = &kAttnCausalRows[di];
    k.bwd_name = "attn_causal_bwd_stats+attn_causal_bwd_dq+attn_causal_bwd_dkv";
    k.lds = size_t(2) * 32 * dvt * 65 * sizeof(float);                 // the double-buffered V block
    k.lds_limit = k.lds > 48 * 1024 ? 96 * 1024 : 0;
    k.grid = dim3(ceil_div(Tq, 128), H, B);
    return k;
}

// a batch stride must hold one item: the kernels index [b * stride + row * pitch + t]
static int check_strides(const char *op, int64_t have, int64_t need, const char *what) {
    return have >= need ? AGX_OK : fail(AGX_ERR_BAD_SHAPE, "%s: %s batch stride %lld < %lld", op, what, (long long)have, (long long)need);
}

static int launch_attention_causal_backward(const float *q, const float *kv, int64_t sq, int64_t skv, const float *slopes,
                                            const float *dout, float *dq, float *dkv, int64_t sdq, int64_t sdkv, float *workspace,
                                            int B, int H, int Dh, int T, float scale_div, hipStream_t st) {
    float *lse = workspace, *delta = workspace + size_t(B) * H * T;
    const dim3 gq(ceil_div(T, AK_QB), H, B), gk(ceil_div(T, AK_KB), H, B);
    const size_t l_stats = size_t(2 * Dh * AK_QB + 2 * Dh * AK_KB + 2 * AK_QB * AK_KB) * sizeof(float);
    const size_t l_dq = size_t(2 * Dh * AK_QB + 2 * Dh * AK_KB + AK_QB * AK_KB) * sizeof(float);
    const size_t l_dkv = size_t(2 * Dh * AK_KB + 2 * Dh * AK_QB + 2 * AK_QB * AK_KB) * sizeof(float);
    static DeviceOnce once[3];
    {
        const void *ks[3] = {reinterpret_cast<const void *>(attn_causal_bwd_stats_kernel),
                             reinterpret_cast<const void *>(attn_causal_bwd_dq_kernel),
                             reinterpret_cast<const void *>(attn_causal_bwd_dkv_kernel)};
        for (int i = 0; i < 3; ++i)
            if (int rc = prepare_kernel(ks[i], once[i], 96 * 1024, nullptr, "attention_causal_backward")) return rc;   // head_dim 128: 90 KB
    }
    hipLaunchKernelGGL(attn_causal_bwd_stats_kernel, gq, dim3(256), l_stats, st, q, kv, sq, skv, slopes, dout, lse, delta, H, Dh, T,
                       scale_div);
    hipLaunchKernelGGL(attn_causal_bwd_dq_kernel, gq, dim3(256), l_dq, st, q, kv, sq, skv, slopes, dout, lse, delta, dq, sdq, H, Dh, T,
                       scale_div);
    hipLaunchKernelGGL(attn_causal_bwd_dkv_kernel, gk, dim3(256), l_dkv, st, q, kv, sq, skv, slopes, dout, lse, delta, dkv, sdkv, H, Dh,
                       T, scale_div);
    return check_launch("attention_causal_backward");
}

}  // namespace agx

extern "C" {

int agx_attention_alibi_causal(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride, int64_t kv_row_stride,
                               const float *slopes, float *out, int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk,
                               int32_t q_pos0, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_causal";
    const AttnCausalPick k = attn_causal_pick(op, batch, heads, head_dim, tq, tk);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (q_pos0 < 0) return fail(AGX_ERR_BAD_SHAPE, "%s: q_pos0=%d < 0", op, q_pos0);
    if (int64_t(q_pos0) + tq + 128 > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: q_pos0 + tq is beyond int32", op);
    if (kv_row_stride < tk) return fail(AGX_ERR_BAD_SHAPE, "%s: kv row stride %lld < tk=%d", op, (long long)kv_row_stride, tk);
    if (kv_row_stride > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: kv row stride %lld is beyond int32", op, (long long)kv_row_stride);
    if (!q || !kv || !slopes || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_strides(op, q_batch_stride, hd * tq, "q")) return rc;
    if (int rc = check_strides(op, kv_batch_stride, 2 * hd * kv_row_stride, "kv")) return rc;
    return k.row->launch(k, q, kv, q_batch_stride, kv_batch_stride, int(kv_row_stride), slopes, out, heads, head_dim, tq, tk, q_pos0,
                         scale_div, static_cast<hipStream_t>(stream));
}

size_t agx_attention_causal_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t t) {
    if (batch <= 0 || heads <= 0 || t <= 0) return 0;
    return size_t(2) * batch * heads * t * sizeof(float);
}

int agx_attention_alibi_causal_backward(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                        const float *slopes, const float *out, const float *dout, float *dq, float *dkv,
                                        int64_t dq_batch_stride, int64_t dkv_batch_stride, float *workspace, size_t workspace_bytes,
                                        int32_t batch, int32_t heads, int32_t head_dim, int32_t t, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_causal_backward";
    const AttnCausalPick k = attn_causal_pick(op, batch, heads, head_dim, t, t);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (!q || !kv || !slopes || !out || !dout || !dq || !dkv || !workspace) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    if (workspace_bytes < agx_attention_causal_backward_workspace_bytes(batch, heads, t))
        return fail(AGX_ERR_WORKSPACE, "%s: workspace too small", op);
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_strides(op, q_batch_stride, hd * t, "q")) return rc;
    if (int rc = check_strides(op, kv_batch_stride, 2 * hd * t, "kv")) return rc;
    if (int rc = check_strides(op, dq_batch_stride, hd * t, "dq")) return rc;
    if (int rc = check_strides(op, dkv_batch_stride, 2 * hd * t, "dkv")) return rc;
    return launch_attention_causal_backward(q, kv, q_batch_stride, kv_batch_stride, slopes, dout, dq, dkv, dq_batch_stride,
                                            dkv_batch_stride, workspace, batch, heads, head_dim, t, scale_div,
                                            static_cast<hipStream_t>(stream));
}

int agx_attention_causal_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, int32_t backward,
                                     char *buf, size_t buf_len) {
    using namespace agx;
    const AttnCausalPick k = attn_causal_pick(backward ? "attention_alibi_causal_backward" : "attention_alibi_causal", batch, heads,
                                              head_dim, tq, tk);
    if (k.code) return k.code;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "agx_attention_causal_kernel_name: NULL buffer");
    snprintf(buf, buf_len, "%s", k.empty ? "none" : (backward ? k.bwd_name : k.row->name));
    return AGX_OK;
}

}  // extern "C"
