// Ragged batches: ALiBi attention (self and cross) with a valid length per batch row for the queries and for the keys, and
// the elementwise tail mask of the transformer block.
//
//     ql = clamp(q_len[b], 0, Tq),  kl = clamp(k_len[b], 0, Tk)        (a NULL array: every row is full)
//     out[b,h,:,i] = sum_{j < kl} softmax_{j < kl}( q_i . k_j / scale_div - slope_h |i - j| ) v_j     for i < ql
//     out[b,h,:,i] = 0                                                   for ql <= i < Tq, and for every i when kl == 0
// Positions are absolute and the padding is on the right.  Nothing at or beyond a row's length reaches a result: q at
// i >= ql, K / V at j >= kl and dout at i >= ql may hold anything, NaN included (the contract of the key/value cache's tail).
// The lengths are read from device memory by every workgroup, so a captured graph replays with the lengths of the replay.
//
// Layouts are those of attention_dropout.hip: q and kv (K rows, then V rows) have their own base pointers and batch strides,
// so a (B, 3*H*Dh, T) qkv tensor is q = qkv, kv = qkv + H*Dh*T with both strides 3*H*Dh*T; dq and dkv likewise.
//
// TWIN CODE: the forward is attention_cross_kernel<DVT> (attention_cross.hip) with the batch strides and with ql / kl in
// the place of Tq / Tk wherever a position is compared or clamped (Tq and Tk stay the row pitches); the three backward
// kernels are attn_cross_bwd_stats / _dq / _dkv in the same way.  The arithmetic of every element -- the fmaf chains over d,
// attn_cross_bwd_logit's relative logit, now relative to key kl - 1 -- is that of the twins, so a row of length (ql, kl)
// computes bit for bit what the same kernel computes for that row cropped and run alone with NULL lengths.  Every load is
// clamped below its length (not merely into the tensor) and V / dO are staged as 0 beyond it: a masked value is never
// multiplied, because 0 x NaN is NaN in an MFMA and in an fmaf.  Separate templates, not a generalisation: the cross and
// self-attention kernels stay the code they were.  A fix to one belongs in the other too.
#include "mfma_tile.hpp"

namespace agx {

// the valid length of batch row b: clamp(len[b], 0, t); NULL: the full row
static __device__ __forceinline__ int ragged_len(const int32_t *len, int b, int t) { return len ? min(max(int(len[b]), 0), t) : t; }

template <int DVT>
__global__ __launch_bounds__(256) void attention_ragged_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                               int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                               const int32_t *__restrict__ q_len, const int32_t *__restrict__ k_len,
                                                               float *__restrict__ out, int H, int Dh, int Tq, int Tk,
                                                               float scale_div) {
    constexpr int KB = 64;         // keys per block (two 32-key accumulator tiles)
    constexpr int DH = 32 * DVT;   // head_dim rounded up to the tile
    constexpr int VP = KB + 1;     // LDS pitch of the V block
    extern __shared__ __attribute__((aligned(16))) float vs[];   // [2][DH][VP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int HD = H * Dh;
    const int ql = ragged_len(q_len, b, Tq), kl = ragged_len(k_len, b, Tk);
    float *ob = out + (size_t(b) * HD + size_t(h) * Dh) * Tq;
    const int wg0 = blockIdx.x * 128;                  // this workgroup's first query
    if (wg0 >= ql || kl == 0) {                        // workgroup-uniform, before the first barrier: nothing valid to compute
        for (int e = tid; e < Dh * 128; e += 256) {
            const int d = e >> 7, ii = wg0 + (e & 127);
            if (ii < Tq) ob[size_t(d) * Tq + ii] = 0.f;
        }
        return;
    }
    const float *qb = q + size_t(b) * sq + size_t(h) * Dh * Tq;
    const float *kb = kv + size_t(b) * skv + size_t(h) * Dh * Tk;
    const float *vb = kb + size_t(HD) * Tk;
    const int i = wg0 + wave * 32 + li;   // this lane's query
    const int ic = min(i, ql - 1);        // ql >= 1 here
    const float slope = slopes[h], inv_scale = 1.f / scale_div;
    const int nblk = (kl + KB - 1) / KB;

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

    auto stage_v = [&](int blk, float *dst) {   // V[dv < Dh][64 keys of block blk] -> LDS, zeros (never the stored value) outside
        for (int e = tid; e < DH * KB; e += 256) {
            const int dv = e / KB, jj = e - dv * KB, j = blk * KB + jj;
            dst[dv * VP + jj] = (dv < Dh && j < kl) ? vb[size_t(dv) * Tk + j] : 0.f;
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
        for (int t2 = 0; t2 < 2; ++t2) kcol[t2] = min(j0 + t2 * 32 + li, kl - 1);
#pragma unroll 4
        for (int s = 0; s < DH / 2; ++s) {
            const int d = min(2 * s + lh, Dh - 1);
            float kf[2];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) kf[t2] = kb[size_t(d) * Tk + kcol[t2]];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) acc[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[t2], qf[s], acc[t2], 0, 0, 0);
        }

        // ---- scale, ALiBi, online softmax (in-lane over the 32 registers + one shuffle) ----
        float bm = -INFINITY;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + t2 * 32 + acc_row(r, lh);
                float s = acc[t2][r] * inv_scale - fabsf(float(ic - j)) * slope;
                s = j < kl ? s : -INFINITY;
                acc[t2][r] = s;
                bm = fmaxf(bm, s);
            }
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        const float mn = fmaxf(m, bm);            // finite: every block holds at least one key < kl
        const float alpha = expf(m - mn);         // first block: exp(-inf) = 0
        float bl = 0.f;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pe = expf(acc[t2][r] - mn);
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

    const float inv = 1.f / l;    // kl >= 1 here: l >= 1
    if (i < Tq) {
        const bool valid = i < ql;
#pragma unroll
        for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dv = dt * 32 + acc_row(r, lh);
                if (dv < Dh) ob[size_t(dv) * Tq + i] = valid ? o[dt][r] * inv : 0.f;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Backward: stats / dq / dkv, twins of attn_cross_bwd_* (see the head of this file).
constexpr int AR_QB = 16;    // queries per block
constexpr int AR_KB = 64;    // keys per block

// attn_cross_bwd_logit with the row's last valid key kl - 1 in the place of Tk - 1
static __device__ __forceinline__ float attn_ragged_bwd_logit(float s, float inv, int i, int j, int kl, float slope) {
    return fmaf(-float(abs(i - j) - max(0, i - (kl - 1))), slope, s * inv);
}

// one workgroup per (query block, head, item): lse and delta of its 16 queries; 0 for a masked query and for a row without keys
__global__ __launch_bounds__(256) void attn_ragged_bwd_stats_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                    int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                    const int32_t *__restrict__ q_len, const int32_t *__restrict__ k_len,
                                                                    const float *__restrict__ dout, float *__restrict__ lse,
                                                                    float *__restrict__ delta, int H, int Dh, int Tq, int Tk,
                                                                    float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                 // [Dh][QB]
    float *Os = Qs + Dh * AR_QB;    // [Dh][QB]  dO
    float *Ks = Os + Dh * AR_QB;    // [Dh][KB]
    float *Vs = Ks + Dh * AR_KB;    // [Dh][KB]
    float *Ss = Vs + Dh * AR_KB;    // [QB][KB]
    float *Ds = Ss + AR_QB * AR_KB;  // [QB][KB]  dP
    __shared__ float red[AR_QB][16], redd[AR_QB][16];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, i0 = blockIdx.x * AR_QB;
    const int HD = H * Dh;
    const int ql = ragged_len(q_len, b, Tq), kl = ragged_len(k_len, b, Tk);
    const size_t so = (size_t(b) * H + h) * Tq;
    if (i0 >= ql || kl == 0) {      // workgroup-uniform, before the first barrier
        if (tid < AR_QB && i0 + tid < Tq) lse[so + i0 + tid] = delta[so + i0 + tid] = 0.f;
        return;
    }
    const float *qg = q + size_t(b) * sq + size_t(h) * Dh * Tq;
    const float *kg = kv + size_t(b) * skv + size_t(h) * Dh * Tk, *vg = kg + size_t(HD) * Tk;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * Tq;
    const float slope = slopes[h], inv = 1.f / scale_div;
    for (int e = tid; e < Dh * AR_QB; e += 256) {
        const int d = e / AR_QB, qi = e - d * AR_QB, i = min(i0 + qi, ql - 1);
        Qs[e] = qg[size_t(d) * Tq + i];
        Os[e] = dg[size_t(d) * Tq + i];
    }
    const int rq = tid / 16, rl = tid % 16;   // 16 threads per query row
    float m = -3.0e38f, l = 0.f, dl = 0.f;
    for (int j0 = 0; j0 < kl; j0 += AR_KB) {
        __syncthreads();
        for (int e = tid; e < Dh * AR_KB; e += 256) {
            const int d = e / AR_KB, j = e - d * AR_KB, jc = min(j0 + j, kl - 1);
            Ks[e] = kg[size_t(d) * Tk + jc];
            Vs[e] = vg[size_t(d) * Tk + jc];
        }
        __syncthreads();
        for (int e = tid; e < AR_QB * AR_KB; e += 256) {
            const int qi = e / AR_KB, j = e - qi * AR_KB;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AR_QB + qi], Ks[d * AR_KB + j], s);
                dp = fmaf(Os[d * AR_QB + qi], Vs[d * AR_KB + j], dp);
            }
            Ds[e] = dp;
            Ss[e] = (j0 + j < kl) ? attn_ragged_bwd_logit(s, inv, i0 + qi, j0 + j, kl, slope) : -3.0e38f;
        }
        __syncthreads();
        float bm = -3.0e38f;
        for (int j = rl; j < AR_KB; j += 16) bm = fmaxf(bm, Ss[rq * AR_KB + j]);
        red[rq][rl] = bm;
        __syncthreads();
        bm = red[rq][0];
        for (int k = 1; k < 16; ++k) bm = fmaxf(bm, red[rq][k]);
        const float mn = fmaxf(m, bm);
        float bs = 0.f, bd = 0.f;
        for (int j = rl; j < AR_KB; j += 16) {
            const float p = expf(Ss[rq * AR_KB + j] - mn);   // 0 for a masked key
            bs += p;
            bd = fmaf(p, Ds[rq * AR_KB + j], bd);
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
    if (rl == 0 && i0 + rq < Tq) {
        const bool valid = i0 + rq < ql;
        lse[so + i0 + rq] = valid ? m + logf(l) : 0.f;
        delta[so + i0 + rq] = valid ? dl / l : 0.f;
    }
}

// one workgroup per (query block, head, item): dQ of its 16 queries, keys in blocks of 64 up to kl
__global__ __launch_bounds__(256) void attn_ragged_bwd_dq_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                 int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                 const int32_t *__restrict__ q_len, const int32_t *__restrict__ k_len,
                                                                 const float *__restrict__ dout, const float *__restrict__ lse,
                                                                 const float *__restrict__ delta, float *__restrict__ dq_out, int64_t sdq,
                                                                 int H, int Dh, int Tq, int Tk, float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                  // [Dh][QB]
    float *Os = Qs + Dh * AR_QB;     // [Dh][QB]  dO
    float *Ks = Os + Dh * AR_QB;     // [Dh][KB]
    float *Vs = Ks + Dh * AR_KB;     // [Dh][KB]
    float *Ss = Vs + Dh * AR_KB;     // [QB][KB]  dS / scale
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, i0 = blockIdx.x * AR_QB;
    const int HD = H * Dh;
    const int ql = ragged_len(q_len, b, Tq), kl = ragged_len(k_len, b, Tk);
    float *dqg = dq_out + size_t(b) * sdq + size_t(h) * Dh * Tq;
    if (i0 >= ql || kl == 0) {       // workgroup-uniform, before the first barrier: this block's dQ is 0
        for (int e = tid; e < Dh * AR_QB; e += 256) {
            const int d = e / AR_QB, qi = e - d * AR_QB;
            if (i0 + qi < Tq) dqg[size_t(d) * Tq + i0 + qi] = 0.f;
        }
        return;
    }
    const float *qg = q + size_t(b) * sq + size_t(h) * Dh * Tq;
    const float *kg = kv + size_t(b) * skv + size_t(h) * Dh * Tk, *vg = kg + size_t(HD) * Tk;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * Tq;
    const float slope = slopes[h], inv = 1.f / scale_div;
    const size_t so = (size_t(b) * H + h) * Tq;
    for (int e = tid; e < Dh * AR_QB; e += 256) {
        const int d = e / AR_QB, qi = e - d * AR_QB, i = min(i0 + qi, ql - 1);
        Qs[e] = qg[size_t(d) * Tq + i];
        Os[e] = dg[size_t(d) * Tq + i];
    }
    constexpr int MAXA = 8;          // dQ elements per thread: Dh * 16 <= 128 * 16 = 8 * 256
    float dq[MAXA];
#pragma unroll
    for (int u = 0; u < MAXA; ++u) dq[u] = 0.f;
    for (int j0 = 0; j0 < kl; j0 += AR_KB) {
        __syncthreads();
        for (int e = tid; e < Dh * AR_KB; e += 256) {
            const int d = e / AR_KB, j = e - d * AR_KB, jc = min(j0 + j, kl - 1);
            Ks[e] = kg[size_t(d) * Tk + jc];
            Vs[e] = vg[size_t(d) * Tk + jc];
        }
        __syncthreads();
        for (int e = tid; e < AR_QB * AR_KB; e += 256) {
            const int qi = e / AR_KB, j = e - qi * AR_KB, i = i0 + qi;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AR_QB + qi], Ks[d * AR_KB + j], s);
                dp = fmaf(Os[d * AR_QB + qi], Vs[d * AR_KB + j], dp);
            }
            float ds = 0.f;
            if (i < ql && j0 + j < kl) {
                const float pn = expf(attn_ragged_bwd_logit(s, inv, i, j0 + j, kl, slope) - lse[so + i]);
                ds = pn * (dp - delta[so + i]) * inv;
            }
            Ss[e] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXA; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * AR_QB) {
                const int d = e / AR_QB, qi = e - d * AR_QB;
                float a = dq[u];
                for (int j = 0; j < AR_KB; ++j) a = fmaf(Ss[qi * AR_KB + j], Ks[d * AR_KB + j], a);
                dq[u] = a;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXA; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * AR_QB) {
            const int d = e / AR_QB, qi = e - d * AR_QB;
            if (i0 + qi < Tq) dqg[size_t(d) * Tq + i0 + qi] = i0 + qi < ql ? dq[u] : 0.f;
        }
    }
}

// one workgroup per (key block, head, item): dK and dV of its 64 keys, queries in blocks of 16 up to ql
__global__ __launch_bounds__(256) void attn_ragged_bwd_dkv_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                  int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                  const int32_t *__restrict__ q_len, const int32_t *__restrict__ k_len,
                                                                  const float *__restrict__ dout, const float *__restrict__ lse,
                                                                  const float *__restrict__ delta, float *__restrict__ dkv, int64_t sdkv,
                                                                  int H, int Dh, int Tq, int Tk, float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Ks = sm;                  // [Dh][KB]
    float *Vs = Ks + Dh * AR_KB;     // [Dh][KB]
    float *Qs = Vs + Dh * AR_KB;     // [Dh][QB]
    float *Os = Qs + Dh * AR_QB;     // [Dh][QB]
    float *Ps = Os + Dh * AR_QB;     // [QB][KB]
    float *Ss = Ps + AR_QB * AR_KB;  // [QB][KB]
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, j0 = blockIdx.x * AR_KB;
    const int HD = H * Dh;
    const int ql = ragged_len(q_len, b, Tq), kl = ragged_len(k_len, b, Tk);
    float *dkg = dkv + size_t(b) * sdkv + size_t(h) * Dh * Tk, *dvg = dkg + size_t(HD) * Tk;
    if (j0 >= kl || ql == 0) {       // workgroup-uniform, before the first barrier: this block's dK / dV are 0
        for (int e = tid; e < Dh * AR_KB; e += 256) {
            const int d = e / AR_KB, j = e - d * AR_KB;
            if (j0 + j < Tk) dkg[size_t(d) * Tk + j0 + j] = dvg[size_t(d) * Tk + j0 + j] = 0.f;
        }
        return;
    }
    const float *qg = q + size_t(b) * sq + size_t(h) * Dh * Tq;
    const float *kg = kv + size_t(b) * skv + size_t(h) * Dh * Tk, *vg = kg + size_t(HD) * Tk;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * Tq;
    const float slope = slopes[h], inv = 1.f / scale_div;
    const size_t so = (size_t(b) * H + h) * Tq;
    for (int e = tid; e < Dh * AR_KB; e += 256) {
        const int d = e / AR_KB, j = e - d * AR_KB, jc = min(j0 + j, kl - 1);
        Ks[e] = kg[size_t(d) * Tk + jc];
        Vs[e] = vg[size_t(d) * Tk + jc];
    }
    constexpr int MAXE = 32;         // dK / dV elements per thread: Dh * 64 <= 128 * 64 = 32 * 256
    float dk[MAXE], dv[MAXE];
#pragma unroll
    for (int u = 0; u < MAXE; ++u) dk[u] = dv[u] = 0.f;
    for (int i0 = 0; i0 < ql; i0 += AR_QB) {
        __syncthreads();
        for (int e = tid; e < Dh * AR_QB; e += 256) {
            const int d = e / AR_QB, qi = e - d * AR_QB, i = min(i0 + qi, ql - 1);
            Qs[e] = qg[size_t(d) * Tq + i];
            Os[e] = (i0 + qi < ql) ? dg[size_t(d) * Tq + i] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < AR_QB * AR_KB; e += 256) {
            const int qi = e / AR_KB, j = e - qi * AR_KB, i = i0 + qi;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AR_QB + qi], Ks[d * AR_KB + j], s);
                dp = fmaf(Os[d * AR_QB + qi], Vs[d * AR_KB + j], dp);
            }
            float pn = 0.f, ds = 0.f;
            if (i < ql && j0 + j < kl) {
                pn = expf(attn_ragged_bwd_logit(s, inv, i, j0 + j, kl, slope) - lse[so + i]);
                ds = pn * (dp - delta[so + i]) * inv;
            }
            Ps[e] = pn;
            Ss[e] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXE; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * AR_KB) {
                const int d = e / AR_KB, j = e - d * AR_KB;
                float ak = dk[u], av = dv[u];
#pragma unroll
                for (int qi = 0; qi < AR_QB; ++qi) {
                    ak = fmaf(Ss[qi * AR_KB + j], Qs[d * AR_QB + qi], ak);
                    av = fmaf(Ps[qi * AR_KB + j], Os[d * AR_QB + qi], av);
                }
                dk[u] = ak;
                dv[u] = av;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXE; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * AR_KB) {
            const int d = e / AR_KB, j = e - d * AR_KB;
            if (j0 + j < Tk) {
                const bool valid = j0 + j < kl;
                dkg[size_t(d) * Tk + j0 + j] = valid ? dk[u] : 0.f;
                dvg[size_t(d) * Tk + j0 + j] = valid ? dv[u] : 0.f;
            }
        }
    }
}

// out[b,c,i] = i < clamp(len[b], 0, T) ? x[b,c,i] : 0 over a contiguous (B, C, T) tensor: a select, so a NaN tail gives 0.
// A thread owns four consecutive elements of the flat tensor (one 16-byte access when both pointers allow it), reads all of
// them before it writes any: out may alias x.  x and out are deliberately not __restrict__.
__global__ __launch_bounds__(256) void mask_tail_kernel(const float *x, const int32_t *__restrict__ len, float *out, int64_t n, int C,
                                                        int T, int vec) {
    const int64_t e0 = (int64_t(blockIdx.x) * 256 + threadIdx.x) * 4;
    if (e0 >= n) return;
    int64_t row = e0 / T;            // b * C + c
    int i = int(e0 - row * T);
    int lim = ragged_len(len, int(row / C), T);
    const int cnt = int(min(int64_t(4), n - e0));
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec && cnt == 4) {
        const float4 w = *reinterpret_cast<const float4 *>(x + e0);
        v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
    } else {
        for (int u = 0; u < cnt; ++u) v[u] = x[e0 + u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u >= cnt) break;         // the tensor's last quartet: no row, and no length, beyond the end
        while (i >= T) {             // the quartet runs into the next row (T < 4: more than once)
            i -= T;
            ++row;
            lim = ragged_len(len, int(row / C), T);
        }
        v[u] = i < lim ? v[u] : 0.f;
        ++i;
    }
    if (vec && cnt == 4) {
        *reinterpret_cast<float4 *>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int u = 0; u < cnt; ++u) out[e0 + u] = v[u];
    }
}

// ------------------------------------------------------------------ host side: one pick and its rows
struct AttnRaggedPick;
#define AGX_ATTN_RAGGED_ARGS                                                                                                 \
    const AttnRaggedPick &k, const float *q, const float *kv, int64_t sq, int64_t skv, const float *slopes, const int32_t *q_len, \
        const int32_t *k_len, float *out, int H, int Dh, int Tq, int Tk, float scale_div, hipStream_t st
struct AttnRaggedRow { const char *name; int (*launch)(AGX_ATTN_RAGGED_ARGS); };
// empty: batch, heads, tq or tk <= 0 -- the entry points return AGX_OK and launch nothing; code: a refusal (fail() was called)
struct AttnRaggedPick { const AttnRaggedRow *row; const char *bwd_name; dim3 grid; size_t lds; int lds_limit, code; bool empty; };

template <int DVT>
static int run_attention_ragged(AGX_ATTN_RAGGED_ARGS) {
    auto kern = attention_ragged_kernel<DVT>;
    static DeviceOnce once;
    if (int rc = prepare_kernel(reinterpret_cast<const void *>(kern), once, k.lds_limit, nullptr, "attention_ragged")) return rc;
    hipLaunchKernelGGL(kern, k.grid, dim3(256), k.lds, st, q, kv, sq, skv, slopes, q_len, k_len, out, H, Dh, Tq, Tk, scale_div);
    return check_launch("attention_ragged");
}

#define AGX_ATTN_ROW(DVT) {"attention_ragged<" #DVT ">", run_attention_ragged<DVT>}
static const AttnRaggedRow kAttnRaggedRows[3] = {AGX_ATTN_ROW(1), AGX_ATTN_ROW(2), AGX_ATTN_ROW(4)};   // [log2(DVT)]
#undef AGX_ATTN_ROW

static AttnRaggedPick attn_ragged_pick(const char *op, int B, int H, int Dh, int Tq, int Tk) {
    AttnRaggedPick k{};
    k.empty = B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0;
    if (Dh <= 0) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: bad shape head_dim=%d", op, Dh);
    else if (Dh > 128) k.code = fail(AGX_ERR_UNSUPPORTED, "%s: head_dim=%d > 128", op, Dh);
    else if (H > 65535 || B > 65535) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: grid too large", op);
    if (k.code || k.empty) return k;
    const int dvt = Dh <= 32 ? 1 : (Dh <= 64 ? 2 : 4), di = dvt / 2;   // 32-row tiles of the head dim; di = log2(dvt)
    k.row = &kAttnRaggedRows[di];
    k.bwd_name = "attn_ragged_bwd_stats+attn_ragged_bwd_dq+attn_ragged_bwd_dkv";
    k.lds = size_t(2) * 32 * dvt * 65 * sizeof(float);                 // the double-buffered V block
    k.lds_limit = k.lds > 48 * 1024 ? 96 * 1024 : 0;
    k.grid = dim3(ceil_div(Tq, 128), H, B);
    return k;
}

// a batch stride must hold one item: the kernels index [b * stride + row * T + t]
static int ragged_stride(const char *op, int64_t have, int64_t need, const char *what) {
    return have >= need ? AGX_OK : fail(AGX_ERR_BAD_SHAPE, "%s: %s batch stride %lld < %lld", op, what, (long long)have, (long long)need);
}

static int launch_attention_ragged_backward(const float *q, const float *kv, int64_t sq, int64_t skv, const float *slopes,
                                            const int32_t *q_len, const int32_t *k_len, const float *dout, float *dq, float *dkv,
                                            int64_t sdq, int64_t sdkv, float *workspace, int B, int H, int Dh, int Tq, int Tk,
                                            float scale_div, hipStream_t st) {
    float *lse = workspace, *delta = workspace + size_t(B) * H * Tq;
    const dim3 gq(ceil_div(Tq, AR_QB), H, B), gk(ceil_div(Tk, AR_KB), H, B);
    const size_t l_stats = size_t(2 * Dh * AR_QB + 2 * Dh * AR_KB + 2 * AR_QB * AR_KB) * sizeof(float);
    const size_t l_dq = size_t(2 * Dh * AR_QB + 2 * Dh * AR_KB + AR_QB * AR_KB) * sizeof(float);
    const size_t l_dkv = size_t(2 * Dh * AR_KB + 2 * Dh * AR_QB + 2 * AR_QB * AR_KB) * sizeof(float);
    static DeviceOnce once[3];
    {
        const void *ks[3] = {reinterpret_cast<const void *>(attn_ragged_bwd_stats_kernel),
                             reinterpret_cast<const void *>(attn_ragged_bwd_dq_kernel),
                             reinterpret_cast<const void *>(attn_ragged_bwd_dkv_kernel)};
        for (int i = 0; i < 3; ++i)
            if (int rc = prepare_kernel(ks[i], once[i], 96 * 1024, nullptr, "attention_ragged_backward")) return rc;   // head_dim 128: 90 KB
    }
    hipLaunchKernelGGL(attn_ragged_bwd_stats_kernel, gq, dim3(256), l_stats, st, q, kv, sq, skv, slopes, q_len, k_len, dout, lse, delta,
                       H, Dh, Tq, Tk, scale_div);
    hipLaunchKernelGGL(attn_ragged_bwd_dq_kernel, gq, dim3(256), l_dq, st, q, kv, sq, skv, slopes, q_len, k_len, dout, lse, delta, dq, sdq,
                       H, Dh, Tq, Tk, scale_div);
    hipLaunchKernelGGL(attn_ragged_bwd_dkv_kernel, gk, dim3(256), l_dkv, st, q, kv, sq, skv, slopes, q_len, k_len, dout, lse, delta, dkv,
                       sdkv, H, Dh, Tq, Tk, scale_div);
    return check_launch("attention_ragged_backward");
}

}  // namespace agx

extern "C" {

int agx_attention_alibi_ragged(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride, const float *slopes,
                               const int32_t *q_len, const int32_t *k_len, float *out, int32_t batch, int32_t heads, int32_t head_dim,
                               int32_t tq, int32_t tk, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_ragged";
    const AttnRaggedPick k = attn_ragged_pick(op, batch, heads, head_dim, tq, tk);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = ragged_stride(op, q_batch_stride, hd * tq, "q")) return rc;
    if (int rc = ragged_stride(op, kv_batch_stride, 2 * hd * tk, "kv")) return rc;
    if (!q || !kv || !slopes || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);   // q_len / k_len: NULL = full
    return k.row->launch(k, q, kv, q_batch_stride, kv_batch_stride, slopes, q_len, k_len, out, heads, head_dim, tq, tk, scale_div,
                         static_cast<hipStream_t>(stream));
}

size_t agx_attention_ragged_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t tq) {
    if (batch <= 0 || heads <= 0 || tq <= 0) return 0;
    return size_t(2) * batch * heads * tq * sizeof(float);
}

int agx_attention_alibi_ragged_backward(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                        const float *slopes, const int32_t *q_len, const int32_t *k_len, const float *out,
                                        const float *dout, float *dq, float *dkv, int64_t dq_batch_stride, int64_t dkv_batch_stride,
                                        float *workspace, size_t workspace_bytes, int32_t batch, int32_t heads, int32_t head_dim,
                                        int32_t tq, int32_t tk, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_ragged_backward";
    const AttnRaggedPick k = attn_ragged_pick(op, batch, heads, head_dim, tq, tk);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = ragged_stride(op, q_batch_stride, hd * tq, "q")) return rc;
    if (int rc = ragged_stride(op, kv_batch_stride, 2 * hd * tk, "kv")) return rc;
    if (int rc = ragged_stride(op, dq_batch_stride, hd * tq, "dq")) return rc;
    if (int rc = ragged_stride(op, dkv_batch_stride, 2 * hd * tk, "dkv")) return rc;
    if (workspace_bytes < agx_attention_ragged_backward_workspace_bytes(batch, heads, tq))
        return fail(AGX_ERR_WORKSPACE, "%s: workspace too small", op);
    if (!q || !kv || !slopes || !out || !dout || !dq || !dkv || !workspace) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    return launch_attention_ragged_backward(q, kv, q_batch_stride, kv_batch_stride, slopes, q_len, k_len, dout, dq, dkv, dq_batch_stride,
                                            dkv_batch_stride, workspace, batch, heads, head_dim, tq, tk, scale_div,
                                            static_cast<hipStream_t>(stream));
}

int agx_attention_ragged_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, int32_t backward,
                                     char *buf, size_t buf_len) {
    using namespace agx;
    const AttnRaggedPick k = attn_ragged_pick(backward ? "attention_alibi_ragged_backward" : "attention_alibi_ragged", batch, heads,
                                              head_dim, tq, tk);
    if (k.code) return k.code;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "agx_attention_ragged_kernel_name: NULL buffer");
    snprintf(buf, buf_len, "%s", k.empty ? "none" : (backward ? k.bwd_name : k.row->name));
    return AGX_OK;
}

int agx_mask_tail(const float *x, const int32_t *len, float *out, int32_t batch, int32_t channels, int32_t t, void *stream) {
    using namespace agx;
    if (batch <= 0 || channels <= 0 || t <= 0) return AGX_OK;
    const int64_t n = int64_t(batch) * channels * t;
    const int64_t blocks = ceil_div64(ceil_div64(n, 4), 256);
    if (blocks > 0x7fffffff || int64_t(batch) * channels > 0x7fffffff)
        return fail(AGX_ERR_BAD_SHAPE, "mask_tail: (%d, %d, %d) is beyond the grid", batch, channels, t);
    if (!x || !out) return fail(AGX_ERR_NULL_POINTER, "mask_tail: NULL pointer");   // len: NULL = every row is full
    const int vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    hipLaunchKernelGGL(mask_tail_kernel, dim3(unsigned(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), x, len, out, n, channels, t,
                       vec);
    return check_launch("mask_tail");
}

}  // extern "C"
