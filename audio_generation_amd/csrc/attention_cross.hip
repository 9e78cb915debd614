// Cross-attention with the ALiBi bias: queries of one sequence (length Tq), keys and values of another (length Tk).
//
// networks/transformers.py:165-188 with `cross_attention`:  q = W_q LN(x), k = W_k y, v = W_v y,
//     out[b,h,:,i] = sum_j softmax_j( q_i . k_j / scale_div - slope_h |i - j| ) v_j,    j in [0, Tk)
// with i and j the absolute positions in their own sequences (Alibi._create_M :45-77 builds -slope_h |row - col| for both
// orders of the two context lengths; the formula is symmetric, so the reference's transposed (H, context_y, context_x) shape
// does not change a value).
//
// Layouts (channel-major fp32, as the self-attention block):  q (B, H*Dh, Tq);  kv (B, 2*H*Dh, Tk), K rows first, then V
// rows;  out (B, H*Dh, Tq).  q and kv have their own base pointers and their own batch strides.
//
// These are separate templates beside attention_flash.hip, not a generalisation of it: the self-attention kernels, their
// rows and their names stay exactly the code they were.  The forward is the online-softmax form of attention_flash<DVT,0>
// (64-key blocks, fp32-input MFMA for both contractions, V double-buffered through LDS, row statistics in-lane); the
// backward is the three deterministic kernels of agx_attention_alibi_backward_ex (row statistics over Tq, dQ per 16-query
// block over the key blocks up to Tk, dK / dV per 64-key block over the query blocks up to Tq; P recomputed from lse, no
// atomics).  Keys >= Tk are masked, queries >= Tq are not stored; every global index is clamped into its own sequence.
#include "mfma_tile.hpp"

namespace agx {

template <int DVT>
__global__ __launch_bounds__(256) void attention_cross_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                              const float *__restrict__ slopes, float *__restrict__ out,
                                                              int H, int Dh, int Tq, int Tk, float scale_div) {
    constexpr int KB = 64;         // keys per block (two 32-key accumulator tiles)
    constexpr int DH = 32 * DVT;   // head_dim rounded up to the tile
    constexpr int VP = KB + 1;     // LDS pitch of the V block
    extern __shared__ __attribute__((aligned(16))) float vs[];   // [2][DH][VP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int HD = H * Dh;
    const float *qb = q + (size_t(b) * HD + size_t(h) * Dh) * Tq;
    const float *kb = kv + (size_t(b) * 2 * HD + size_t(h) * Dh) * Tk;
    const float *vb = kb + size_t(HD) * Tk;
    const int i = blockIdx.x * 128 + wave * 32 + li;   // this lane's query
    const int ic = min(i, Tq - 1);
    const float slope = slopes[h], inv_scale = 1.f / scale_div;
    const int nblk = (Tk + KB - 1) / KB;

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

    auto stage_v = [&](int blk, float *dst) {   // V[dv < Dh][64 keys of block blk] -> LDS, zeros outside
        for (int e = tid; e < DH * KB; e += 256) {
            const int dv = e / KB, jj = e - dv * KB, j = blk * KB + jj;
            dst[dv * VP + jj] = (dv < Dh && j < Tk) ? vb[size_t(dv) * Tk + j] : 0.f;
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
                float s = acc[t2][r] * inv_scale - fabsf(float(ic - j)) * slope;   // == M[h, j, i] = M[h, i, j] of Alibi._create_M
                s = j < Tk ? s : -INFINITY;
                acc[t2][r] = s;
                bm = fmaxf(bm, s);
            }
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        const float mn = fmaxf(m, bm);            // finite: every block holds at least one key < Tk
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
// Backward: stats / dq / dkv as in attention_flash.hip, with the query side (q, out, dout, dq, lse, delta) indexed by
// Tq and the key side (kv, dkv) by Tk.
// TWIN CODE: these three kernels are copies of attn_bwd_stats / _dq / _dkv of attention_flash.hip (same tiling, same
// arithmetic, only the pointers and the two lengths are split), kept apart so that the self-attention kernels stay the code
// they were.  A fix to one belongs in the other too.  The forward above is the same kind of twin of attention_flash<DVT,0>.
constexpr int AC_QB = 16;    // queries per block
constexpr int AC_KB = 64;    // keys per block

// The logit of (query i, key j), rounded the same way in all three kernels: the product feeds an explicit fmaf, so no
// contraction can differ between them.  lse is built from these values, and P = exp(logit - lse) is exactly 1 on a row that one
// key holds alone; a logit near 100 rounded differently in two kernels would put 1e-5 of relative error into P instead.
// The bias is taken relative to the query's nearest key, max(0, i - (Tk - 1)) positions away: a constant of the row, which the
// softmax does not see, subtracted exactly.  A query far beyond the last key (Tq > Tk) with a steep slope would otherwise
// have all its logits near -slope (i - Tk), and lse = m + log l, rounded to an ulp of that magnitude, would lose log l.
// The workspace's lse is that of these relative logits.  (The self-attention twin has no such rows: i <= T - 1.)
static __device__ __forceinline__ float attn_cross_bwd_logit(float s, float inv, int i, int j, int Tk, float slope) {
    return fmaf(-float(abs(i - j) - max(0, i - (Tk - 1))), slope, s * inv);
}

// one workgroup per (query block, head, item): lse and delta of its 16 queries.  delta_i = sum_j P_ij dP_ij is summed online
// next to l, from dP values formed exactly as the dq and dkv kernels form them (the same fmaf chain over d), not taken as
// sum_d dO[d,i] O[d,i] from the forward's output: where one key holds all of a row's weight, dP_ij == delta_i must cancel
// to zero in dS = P (dP - delta), and two differently rounded dot products leave a residue that K / scale multiplies into dQ.
// (`out` stays in the signature for the callers; it is not read.)
__global__ __launch_bounds__(256) void attn_cross_bwd_stats_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                   const float *__restrict__ slopes, const float *__restrict__ out,
                                                                   const float *__restrict__ dout, float *__restrict__ lse,
                                                                   float *__restrict__ delta, int H, int Dh, int Tq, int Tk,
                                                                   float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                 // [Dh][QB]
    float *Os = Qs + Dh * AC_QB;    // [Dh][QB]  dO
    float *Ks = Os + Dh * AC_QB;    // [Dh][KB]
    float *Vs = Ks + Dh * AC_KB;    // [Dh][KB]
    float *Ss = Vs + Dh * AC_KB;    // [QB][KB]
    float *Ds = Ss + AC_QB * AC_KB;  // [QB][KB]  dP
    __shared__ float red[AC_QB][16], redd[AC_QB][16];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, i0 = blockIdx.x * AC_QB;
    const int HD = H * Dh;
    const float *qg = q + (size_t(b) * HD + h * Dh) * Tq, *kg = kv + (size_t(b) * 2 * HD + h * Dh) * Tk, *vg = kg + size_t(HD) * Tk;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * Tq;
    const float slope = slopes[h], inv = 1.f / scale_div;
    for (int e = tid; e < Dh * AC_QB; e += 256) {
        const int d = e / AC_QB, qi = e - d * AC_QB, i = min(i0 + qi, Tq - 1);
        Qs[e] = qg[size_t(d) * Tq + i];
        Os[e] = dg[size_t(d) * Tq + i];
    }
    const int rq = tid / 16, rl = tid % 16;   // 16 threads per query row
    float m = -3.0e38f, l = 0.f, dl = 0.f;
    for (int j0 = 0; j0 < Tk; j0 += AC_KB) {
        __syncthreads();
        for (int e = tid; e < Dh * AC_KB; e += 256) {
            const int d = e / AC_KB, j = e - d * AC_KB, jc = min(j0 + j, Tk - 1);
            Ks[e] = kg[size_t(d) * Tk + jc];
            Vs[e] = vg[size_t(d) * Tk + jc];
        }
        __syncthreads();
        for (int e = tid; e < AC_QB * AC_KB; e += 256) {
            const int qi = e / AC_KB, j = e - qi * AC_KB;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AC_QB + qi], Ks[d * AC_KB + j], s);
                dp = fmaf(Os[d * AC_QB + qi], Vs[d * AC_KB + j], dp);
            }
            Ds[e] = dp;
            Ss[e] = (j0 + j < Tk) ? attn_cross_bwd_logit(s, inv, i0 + qi, j0 + j, Tk, slope) : -3.0e38f;
        }
        __syncthreads();
        float bm = -3.0e38f;
        for (int j = rl; j < AC_KB; j += 16) bm = fmaxf(bm, Ss[rq * AC_KB + j]);
        red[rq][rl] = bm;
        __syncthreads();
        bm = red[rq][0];
        for (int k = 1; k < 16; ++k) bm = fmaxf(bm, red[rq][k]);
        const float mn = fmaxf(m, bm);
        float bs = 0.f, bd = 0.f;
        for (int j = rl; j < AC_KB; j += 16) {
            const float p = expf(Ss[rq * AC_KB + j] - mn);   // 0 for a padded key
            bs += p;
            bd = fmaf(p, Ds[rq * AC_KB + j], bd);
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
        const size_t o = (size_t(b) * H + h) * Tq + i0 + rq;
        lse[o] = m + logf(l);
        delta[o] = dl / l;
    }
}

// one workgroup per (query block, head, item): dQ of its 16 queries, keys in blocks of 64
__global__ __launch_bounds__(256) void attn_cross_bwd_dq_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                const float *__restrict__ slopes, const float *__restrict__ dout,
                                                                const float *__restrict__ lse, const float *__restrict__ delta,
                                                                float *__restrict__ dq_out, int H, int Dh, int Tq, int Tk,
                                                                float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                  // [Dh][QB]
    float *Os = Qs + Dh * AC_QB;     // [Dh][QB]  dO
    float *Ks = Os + Dh * AC_QB;     // [Dh][KB]
    float *Vs = Ks + Dh * AC_KB;     // [Dh][KB]
    float *Ss = Vs + Dh * AC_KB;     // [QB][KB]  dS / scale
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, i0 = blockIdx.x * AC_QB;
    const int HD = H * Dh;
    const float *qg = q + (size_t(b) * HD + h * Dh) * Tq;
    const float *kg = kv + (size_t(b) * 2 * HD + h * Dh) * Tk, *vg = kg + size_t(HD) * Tk;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * Tq;
    float *dqg = dq_out + (size_t(b) * HD + h * Dh) * Tq;
    const float slope = slopes[h], inv = 1.f / scale_div;
    const size_t so = (size_t(b) * H + h) * Tq;
    for (int e = tid; e < Dh * AC_QB; e += 256) {
        const int d = e / AC_QB, qi = e - d * AC_QB, i = min(i0 + qi, Tq - 1);
        Qs[e] = qg[size_t(d) * Tq + i];
        Os[e] = dg[size_t(d) * Tq + i];
    }
    constexpr int MAXA = 8;          // dQ elements per thread: Dh * 16 <= 128 * 16 = 8 * 256
    float dq[MAXA];
#pragma unroll
    for (int u = 0; u < MAXA; ++u) dq[u] = 0.f;
    for (int j0 = 0; j0 < Tk; j0 += AC_KB) {
        __syncthreads();
        for (int e = tid; e < Dh * AC_KB; e += 256) {
            const int d = e / AC_KB, j = e - d * AC_KB, jc = min(j0 + j, Tk - 1);
            Ks[e] = kg[size_t(d) * Tk + jc];
            Vs[e] = vg[size_t(d) * Tk + jc];
        }
        __syncthreads();
        for (int e = tid; e < AC_QB * AC_KB; e += 256) {
            const int qi = e / AC_KB, j = e - qi * AC_KB, i = i0 + qi;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AC_QB + qi], Ks[d * AC_KB + j], s);
                dp = fmaf(Os[d * AC_QB + qi], Vs[d * AC_KB + j], dp);
            }
            float ds = 0.f;
            if (i < Tq && j0 + j < Tk) {
                const float pn = expf(attn_cross_bwd_logit(s, inv, i, j0 + j, Tk, slope) - lse[so + i]);
                ds = pn * (dp - delta[so + i]) * inv;
            }
            Ss[e] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXA; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * AC_QB) {
                const int d = e / AC_QB, qi = e - d * AC_QB;
                float a = dq[u];
                for (int j = 0; j < AC_KB; ++j) a = fmaf(Ss[qi * AC_KB + j], Ks[d * AC_KB + j], a);
                dq[u] = a;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXA; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * AC_QB) {
            const int d = e / AC_QB, qi = e - d * AC_QB;
            if (i0 + qi < Tq) dqg[size_t(d) * Tq + i0 + qi] = dq[u];
        }
    }
}

// one workgroup per (key block, head, item): dK and dV of its 64 keys, queries in blocks of 16
__global__ __launch_bounds__(256) void attn_cross_bwd_dkv_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                 const float *__restrict__ slopes, const float *__restrict__ dout,
                                                                 const float *__restrict__ lse, const float *__restrict__ delta,
                                                                 float *__restrict__ dkv, int H, int Dh, int Tq, int Tk,
                                                                 float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Ks = sm;                  // [Dh][KB]
    float *Vs = Ks + Dh * AC_KB;     // [Dh][KB]
    float *Qs = Vs + Dh * AC_KB;     // [Dh][QB]
    float *Os = Qs + Dh * AC_QB;     // [Dh][QB]
    float *Ps = Os + Dh * AC_QB;     // [QB][KB]
    float *Ss = Ps + AC_QB * AC_KB;  // [QB][KB]
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z, j0 = blockIdx.x * AC_KB;
    const int HD = H * Dh;
    const float *qg = q + (size_t(b) * HD + h * Dh) * Tq;
    const float *kg = kv + (size_t(b) * 2 * HD + h * Dh) * Tk, *vg = kg + size_t(HD) * Tk;
    const float *dg = dout + (size_t(b) * HD + h * Dh) * Tq;
    float *dkg = dkv + (size_t(b) * 2 * HD + h * Dh) * Tk, *dvg = dkg + size_t(HD) * Tk;
    const float slope = slopes[h], inv = 1.f / scale_div;
    const size_t so = (size_t(b) * H + h) * Tq;
    for (int e = tid; e < Dh * AC_KB; e += 256) {
        const int d = e / AC_KB, j = e - d * AC_KB, jc = min(j0 + j, Tk - 1);
        Ks[e] = kg[size_t(d) * Tk + jc];
        Vs[e] = vg[size_t(d) * Tk + jc];
    }
    constexpr int MAXE = 32;         // dK / dV elements per thread: Dh * 64 <= 128 * 64 = 32 * 256
    float dk[MAXE], dv[MAXE];
#pragma unroll
    for (int u = 0; u < MAXE; ++u) dk[u] = dv[u] = 0.f;
    for (int i0 = 0; i0 < Tq; i0 += AC_QB) {
        __syncthreads();
        for (int e = tid; e < Dh * AC_QB; e += 256) {
            const int d = e / AC_QB, qi = e - d * AC_QB, i = min(i0 + qi, Tq - 1);
            Qs[e] = qg[size_t(d) * Tq + i];
            Os[e] = (i0 + qi < Tq) ? dg[size_t(d) * Tq + i] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < AC_QB * AC_KB; e += 256) {
            const int qi = e / AC_KB, j = e - qi * AC_KB, i = i0 + qi;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AC_QB + qi], Ks[d * AC_KB + j], s);
                dp = fmaf(Os[d * AC_QB + qi], Vs[d * AC_KB + j], dp);
            }
            float pn = 0.f, ds = 0.f;
            if (i < Tq && j0 + j < Tk) {
                pn = expf(attn_cross_bwd_logit(s, inv, i, j0 + j, Tk, slope) - lse[so + i]);
                ds = pn * (dp - delta[so + i]) * inv;
            }
            Ps[e] = pn;
            Ss[e] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXE; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * AC_KB) {
                const int d = e / AC_KB, j = e - d * AC_KB;
                float ak = dk[u], av = dv[u];
#pragma unroll
                for (int qi = 0; qi < AC_QB; ++qi) {
                    ak = fmaf(Ss[qi * AC_KB + j], Qs[d * AC_QB + qi], ak);
                    av = fmaf(Ps[qi * AC_KB + j], Os[d * AC_QB + qi], av);
                }
                dk[u] = ak;
                dv[u] = av;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXE; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * AC_KB) {
            const int d = e / AC_KB, j = e - d * AC_KB;
            if (j0 + j < Tk) {
                dkg[size_t(d) * Tk + j0 + j] = dk[u];
                dvg[size_t(d) * Tk + j0 + j] = dv[u];
            }
        }
    }
}

// ------------------------------------------------------------------ host side: cross-attention has its own pick and rows
struct AttnCrossPick;
#define AGX_ATTN_CROSS_ARGS \
    const AttnCrossPick &k, const float *q, const float *kv, const float *slopes, float *out, int H, int Dh, int Tq, int Tk, float scale_div, hipStream_t st
struct AttnCrossRow { const char *name; int (*launch)(AGX_ATTN_CROSS_ARGS); };
// empty: batch, heads, tq or tk <= 0 -- the entry points return AGX_OK and launch nothing; code: a refusal (fail() was called)
struct AttnCrossPick { const AttnCrossRow *row; const char *bwd_name; dim3 grid; size_t lds; int lds_limit, code; bool empty; };

template <int DVT>
static int run_attention_cross(AGX_ATTN_CROSS_ARGS) {
    auto kern = attention_cross_kernel<DVT>;
    static DeviceOnce once;
    if (int rc = prepare_kernel(reinterpret_cast<const void *>(kern), once, k.lds_limit, nullptr, "attention_cross")) return rc;
    hipLaunchKernelGGL(kern, k.grid, dim3(256), k.lds, st, q, kv, slopes, out, H, Dh, Tq, Tk, scale_div);
    return check_launch("attention_cross");
}

#define AGX_ATTN_ROW(DVT) {"attention_cross<" #DVT ">", run_attention_cross<DVT>}
static const AttnCrossRow kAttnCrossRows[3] = {AGX_ATTN_ROW(1), AGX_ATTN_ROW(2), AGX_ATTN_ROW(4)};   // [log2(DVT)]
#undef AGX_ATTN_ROW

static AttnCrossPick attn_cross_pick(const char *op, int B, int H, int Dh, int Tq, int Tk) {
    AttnCrossPick k{};
    k.empty = B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0;
    if (Dh <= 0) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: bad shape head_dim=%d", op, Dh);
    else if (Dh > 128) k.code = fail(AGX_ERR_UNSUPPORTED, "%s: head_dim=%d > 128", op, Dh);
    else if (H > 65535 || B > 65535) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: grid too large", op);
    if (k.code || k.empty) return k;
    const int dvt = Dh <= 32 ? 1 : (Dh <= 64 ? 2 : 4), di = dvt / 2;   // 32-row tiles of the head dim; di = log2(dvt)
    k.row = &kAttnCrossRows[di];
    k.bwd_name = "attn_cross_bwd_stats+attn_cross_bwd_dq+attn_cross_bwd_dkv";
    k.lds = size_t(2) * 32 * dvt * 65 * sizeof(float);                 // the double-buffered V block
    k.lds_limit = k.lds > 48 * 1024 ? 96 * 1024 : 0;
    k.grid = dim3(ceil_div(Tq, 128), H, B);
    return k;
}

static int launch_attention_cross_backward(const float *q, const float *kv, const float *slopes, const float *out, const float *dout,
                                           float *dq, float *dkv, float *workspace, int B, int H, int Dh, int Tq, int Tk,
                                           float scale_div, hipStream_t st) {
    float *lse = workspace, *delta = workspace + size_t(B) * H * Tq;
    const dim3 gq(ceil_div(Tq, AC_QB), H, B), gk(ceil_div(Tk, AC_KB), H, B);
    const size_t l_stats = size_t(2 * Dh * AC_QB + 2 * Dh * AC_KB + 2 * AC_QB * AC_KB) * sizeof(float);
    const size_t l_dq = size_t(2 * Dh * AC_QB + 2 * Dh * AC_KB + AC_QB * AC_KB) * sizeof(float);
    const size_t l_dkv = size_t(2 * Dh * AC_KB + 2 * Dh * AC_QB + 2 * AC_QB * AC_KB) * sizeof(float);
    static DeviceOnce once[3];
    {
        const void *ks[3] = {reinterpret_cast<const void *>(attn_cross_bwd_stats_kernel),
                             reinterpret_cast<const void *>(attn_cross_bwd_dq_kernel),
                             reinterpret_cast<const void *>(attn_cross_bwd_dkv_kernel)};
        for (int i = 0; i < 3; ++i)
            if (int rc = prepare_kernel(ks[i], once[i], 96 * 1024, nullptr, "attention_cross_backward")) return rc;   // head_dim 128: 90 KB
    }
    hipLaunchKernelGGL(attn_cross_bwd_stats_kernel, gq, dim3(256), l_stats, st, q, kv, slopes, out, dout, lse, delta, H, Dh, Tq, Tk,
                       scale_div);
    hipLaunchKernelGGL(attn_cross_bwd_dq_kernel, gq, dim3(256), l_dq, st, q, kv, slopes, dout, lse, delta, dq, H, Dh, Tq, Tk, scale_div);
    hipLaunchKernelGGL(attn_cross_bwd_dkv_kernel, gk, dim3(256), l_dkv, st, q, kv, slopes, dout, lse, delta, dkv, H, Dh, Tq, Tk,
                       scale_div);
    return check_launch("attention_cross_backward");
}

}  // namespace agx

extern "C" {

int agx_attention_alibi_cross(const float *q, const float *kv, const float *slopes, float *out, int32_t batch, int32_t heads,
                              int32_t head_dim, int32_t tq, int32_t tk, float scale_div, void *stream) {
    using namespace agx;
    const AttnCrossPick k = attn_cross_pick("attention_alibi_cross", batch, heads, head_dim, tq, tk);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (!q || !kv || !slopes || !out) return fail(AGX_ERR_NULL_POINTER, "attention_alibi_cross: NULL pointer");
    return k.row->launch(k, q, kv, slopes, out, heads, head_dim, tq, tk, scale_div, static_cast<hipStream_t>(stream));
}

size_t agx_attention_cross_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t tq) {
    if (batch <= 0 || heads <= 0 || tq <= 0) return 0;
    return size_t(2) * batch * heads * tq * sizeof(float);
}

int agx_attention_alibi_cross_backward(const float *q, const float *kv, const float *slopes, const float *out, const float *dout,
                                       float *dq, float *dkv, float *workspace, size_t workspace_bytes, int32_t batch,
                                       int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, float scale_div, void *stream) {
    using namespace agx;
    const AttnCrossPick k = attn_cross_pick("attention_alibi_cross_backward", batch, heads, head_dim, tq, tk);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (!q || !kv || !slopes || !out || !dout || !dq || !dkv || !workspace)
        return fail(AGX_ERR_NULL_POINTER, "attention_alibi_cross_backward: NULL pointer");
    if (workspace_bytes < agx_attention_cross_backward_workspace_bytes(batch, heads, tq))
        return fail(AGX_ERR_WORKSPACE, "attention_alibi_cross_backward: workspace too small");
    return launch_attention_cross_backward(q, kv, slopes, out, dout, dq, dkv, workspace, batch, heads, head_dim, tq, tk, scale_div,
                                           static_cast<hipStream_t>(stream));
}

int agx_attention_cross_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, int32_t backward,
                                    char *buf, size_t buf_len) {
    using namespace agx;
    const AttnCrossPick k = attn_cross_pick(backward ? "attention_alibi_cross_backward" : "attention_alibi_cross", batch, heads,
                                            head_dim, tq, tk);
    if (k.code) return k.code;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "agx_attention_cross_kernel_name: NULL buffer");
    snprintf(buf, buf_len, "%s", k.empty ? "none" : (backward ? k.bwd_name : k.row->name));
    return AGX_OK;
}

}  // extern "C"
