// Packed variable-length batches: symmetric ALiBi attention (self and cross) over sequences concatenated along the time
// axis, and the two layout kernels that move a right-padded (B, C, T) batch into the packed (C, N) form and back.
//
//     q0 = clamp(cu_q[s], 0, nq),  q1 = clamp(cu_q[s + 1], q0, nq),  ql = min(q1 - q0, max_q)      (cu_k / nk / max_k likewise)
//     out[h,:,q0 + i] = sum_{j < kl} softmax_{j < kl}( q_{q0+i} . k_{k0+j} / scale_div - slope_h |i - j| ) v_{k0+j}    for i < ql
//     out[h,:,q0 + i] = 0                                                 for i < ql when kl == 0
//     out[h,:,n]      = 0                                                 for n < clamp(cu_q[0]) and n >= clamp(cu_q[n_seq])
// Positions are relative to the sequence's own start.  Sequence s is blockIdx.z = s; blockIdx.z = n_seq is the slack: the
// columns no sequence owns.  The cu arrays are read from device memory by every workgroup, so a captured graph replays with
// the partition of the replay.  Memory safety does not depend on what they hold: every start and end is clamped into the
// tensor, an end to at least its start, a length to the host-known bound that sized the grid.  For arrays that break the
// contract (decreasing, a first entry that is not 0 -- the columns before it count as slack --, or a sequence longer than
// the bound) the values are unspecified and some columns may stay unwritten, but no access leaves the tensors.
//
// q has H*Dh rows of pitch sq >= nq; kv has K rows then V rows, 2*H*Dh of them, of pitch skv >= nk; out is contiguous
// (H*Dh, nq); dq / dkv have pitches of their own.
//
// TWIN CODE: the forward is attention_ragged_kernel<DVT> (attention_ragged.hip) with the base pointers advanced by the
// sequence's start, the row pitch decoupled from the length (sq / skv where the twin has Tq / Tk as a pitch, ql / kl where it
// compares or clamps a position) and blockIdx.z = sequence; the three backward kernels are attn_ragged_bwd_stats / _dq / _dkv
// in the same way.  Key and query blocks are aligned to the sequence's start, not to the absolute column, and the arithmetic
// of every element -- the fmaf chains over d, attn_ragged_bwd_logit -- is that of the twins, so sequence s computes bit for
// bit what agx_attention_alibi_ragged computes for that sequence cropped and run alone with NULL lengths.  A workgroup beyond
// its sequence's length returns before its first barrier and writes nothing: those columns belong to a neighbour.  Every load
// is clamped below the sequence's end (not merely into the tensor) and V / dO are staged as 0 beyond it: a masked value is
// never multiplied.  Separate templates, not a generalisation: the ragged kernels stay the code they were.  A fix to one
// belongs in the other too.
#include "mfma_tile.hpp"

namespace agx {

struct PackedSpan { int start, len; };

// sequence s of a cu array over n columns: start and end clamped into [0, n], the end to at least the start, the length to cap
static __device__ __forceinline__ PackedSpan packed_span(const int32_t *cu, int s, int n, int cap) {
    const int a = min(max(int(cu[s]), 0), n);
    const int b = min(max(int(cu[s + 1]), a), n);
    return {a, min(b - a, cap)};
}

// the slack of a cu array over n columns: [0, lo) and [hi, n)
static __device__ __forceinline__ void packed_slack(const int32_t *cu, int n_seq, int n, int &lo, int &hi) {
    lo = min(max(int(cu[0]), 0), n);
    hi = min(max(int(cu[n_seq]), 0), n);
}

// rows [0, rows) of pitch `pitch`, slack columns := 0; the workgroups (blockIdx.x of gridDim.x) share the columns
static __device__ __forceinline__ void packed_zero_slack(float *base, int64_t pitch, int rows, int lo, int hi, int n) {
    const int cols = lo + (n - hi);                     // slack columns: c < lo -> c, else hi + (c - lo)
    const int64_t total = int64_t(rows) * cols;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
        const int r = int(e / cols), c = int(e - int64_t(r) * cols);
        base[int64_t(r) * pitch + (c < lo ? c : hi + (c - lo))] = 0.f;
    }
}

template <int DVT>
__global__ __launch_bounds__(256) void attention_packed_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                               int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                               const int32_t *__restrict__ cu_q, const int32_t *__restrict__ cu_k,
                                                               float *__restrict__ out, int n_seq, int H, int Dh, int nq, int nk,
                                                               int max_q, int max_k, float scale_div) {
    constexpr int KB = 64;         // keys per block (two 32-key accumulator tiles)
    constexpr int DH = 32 * DVT;   // head_dim rounded up to the tile
    constexpr int VP = KB + 1;     // LDS pitch of the V block
    extern __shared__ __attribute__((aligned(16))) float vs[];   // [2][DH][VP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int h = blockIdx.y, sidx = blockIdx.z;
    const int HD = H * Dh;
    if (sidx == n_seq) {                               // the slack workgroups of this head: zeros, no barrier
        int lo, hi;
        packed_slack(cu_q, n_seq, nq, lo, hi);
        packed_zero_slack(out + size_t(h) * Dh * nq, nq, Dh, lo, hi, nq);
        return;
    }
    const PackedSpan qs = packed_span(cu_q, sidx, nq, max_q), ks = packed_span(cu_k, sidx, nk, max_k);
    const int ql = qs.len, kl = ks.len;
    float *ob = out + size_t(h) * Dh * nq + qs.start;
    const int wg0 = blockIdx.x * 128;                  // this workgroup's first query, relative to the sequence
    if (wg0 >= ql) return;                             // workgroup-uniform, before the first barrier: a neighbour's columns
    if (kl == 0) {                                     // a sequence without keys: its queries get 0
        for (int e = tid; e < Dh * 128; e += 256) {
            const int d = e >> 7, ii = wg0 + (e & 127);
            if (ii < ql) ob[size_t(d) * nq + ii] = 0.f;
        }
        return;
    }
    const float *qb = q + size_t(h) * Dh * sq + qs.start;
    const float *kb = kv + size_t(h) * Dh * skv + ks.start;
    const float *vb = kb + size_t(HD) * skv;
    const int i = wg0 + wave * 32 + li;   // this lane's query
    const int ic = min(i, ql - 1);        // ql >= 1 here
    const float slope = slopes[h], inv_scale = 1.f / scale_div;
    const int nblk = (kl + KB - 1) / KB;

    // ---- the query fragment stays in registers for the whole key loop ----
    float qf[DH / 2];
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) {
        const int d = 2 * s + lh;
        qf[s] = d < Dh ? qb[size_t(d) * sq + ic] : 0.f;
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
            dst[dv * VP + jj] = (dv < Dh && j < kl) ? vb[size_t(dv) * skv + j] : 0.f;
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
            for (int t2 = 0; t2 < 2; ++t2) kf[t2] = kb[size_t(d) * skv + kcol[t2]];
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
    if (i < ql) {                 // a column at or beyond ql belongs to a neighbour (or to the slack workgroups)
#pragma unroll
        for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dv = dt * 32 + acc_row(r, lh);
                if (dv < Dh) ob[size_t(dv) * nq + i] = o[dt][r] * inv;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Backward: stats / dq / dkv, twins of attn_ragged_bwd_* (see the head of this file).
constexpr int AP_QB = 16;    // queries per block
constexpr int AP_KB = 64;    // keys per block

// attn_ragged_bwd_logit: the relative logit, relative to the sequence's last key kl - 1
static __device__ __forceinline__ float attn_packed_bwd_logit(float s, float inv, int i, int j, int kl, float slope) {
    return fmaf(-float(abs(i - j) - max(0, i - (kl - 1))), slope, s * inv);
}

// one workgroup per (query block, head, sequence): lse and delta of its 16 queries; 0 for a sequence without keys and in slack
__global__ __launch_bounds__(256) void attn_packed_bwd_stats_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                    int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                    const int32_t *__restrict__ cu_q, const int32_t *__restrict__ cu_k,
                                                                    const float *__restrict__ dout, float *__restrict__ lse,
                                                                    float *__restrict__ delta, int n_seq, int H, int Dh, int nq, int nk,
                                                                    int max_q, int max_k, float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                 // [Dh][QB]
    float *Os = Qs + Dh * AP_QB;    // [Dh][QB]  dO
    float *Ks = Os + Dh * AP_QB;    // [Dh][KB]
    float *Vs = Ks + Dh * AP_KB;    // [Dh][KB]
    float *Ss = Vs + Dh * AP_KB;    // [QB][KB]
    float *Ds = Ss + AP_QB * AP_KB;  // [QB][KB]  dP
    __shared__ float red[AP_QB][16], redd[AP_QB][16];
    const int tid = threadIdx.x, h = blockIdx.y, sidx = blockIdx.z, i0 = blockIdx.x * AP_QB;
    const int HD = H * Dh;
    if (sidx == n_seq) {            // the slack of lse / delta: every float of the workspace is written
        int lo, hi;
        packed_slack(cu_q, n_seq, nq, lo, hi);
        packed_zero_slack(lse + size_t(h) * nq, nq, 1, lo, hi, nq);
        packed_zero_slack(delta + size_t(h) * nq, nq, 1, lo, hi, nq);
        return;
    }
    const PackedSpan qs = packed_span(cu_q, sidx, nq, max_q), ks = packed_span(cu_k, sidx, nk, max_k);
    const int ql = qs.len, kl = ks.len;
    const size_t so = size_t(h) * nq + qs.start;
    if (i0 >= ql) return;           // workgroup-uniform, before the first barrier: a neighbour's columns
    if (kl == 0) {
        if (tid < AP_QB && i0 + tid < ql) lse[so + i0 + tid] = delta[so + i0 + tid] = 0.f;
        return;
    }
    const float *qg = q + size_t(h) * Dh * sq + qs.start;
    const float *kg = kv + size_t(h) * Dh * skv + ks.start, *vg = kg + size_t(HD) * skv;
    const float *dg = dout + size_t(h) * Dh * nq + qs.start;
    const float slope = slopes[h], inv = 1.f / scale_div;
    for (int e = tid; e < Dh * AP_QB; e += 256) {
        const int d = e / AP_QB, qi = e - d * AP_QB, i = min(i0 + qi, ql - 1);
        Qs[e] = qg[size_t(d) * sq + i];
        Os[e] = dg[size_t(d) * nq + i];
    }
    const int rq = tid / 16, rl = tid % 16;   // 16 threads per query row
    float m = -3.0e38f, l = 0.f, dl = 0.f;
    for (int j0 = 0; j0 < kl; j0 += AP_KB) {
        __syncthreads();
        for (int e = tid; e < Dh * AP_KB; e += 256) {
            const int d = e / AP_KB, j = e - d * AP_KB, jc = min(j0 + j, kl - 1);
            Ks[e] = kg[size_t(d) * skv + jc];
            Vs[e] = vg[size_t(d) * skv + jc];
        }
        __syncthreads();
        for (int e = tid; e < AP_QB * AP_KB; e += 256) {
            const int qi = e / AP_KB, j = e - qi * AP_KB;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AP_QB + qi], Ks[d * AP_KB + j], s);
                dp = fmaf(Os[d * AP_QB + qi], Vs[d * AP_KB + j], dp);
            }
            Ds[e] = dp;
            Ss[e] = (j0 + j < kl) ? attn_packed_bwd_logit(s, inv, i0 + qi, j0 + j, kl, slope) : -3.0e38f;
        }
        __syncthreads();
        float bm = -3.0e38f;
        for (int j = rl; j < AP_KB; j += 16) bm = fmaxf(bm, Ss[rq * AP_KB + j]);
        red[rq][rl] = bm;
        __syncthreads();
        bm = red[rq][0];
        for (int k = 1; k < 16; ++k) bm = fmaxf(bm, red[rq][k]);
        const float mn = fmaxf(m, bm);
        float bs = 0.f, bd = 0.f;
        for (int j = rl; j < AP_KB; j += 16) {
            const float p = expf(Ss[rq * AP_KB + j] - mn);   // 0 for a masked key
            bs += p;
            bd = fmaf(p, Ds[rq * AP_KB + j], bd);
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
    if (rl == 0 && i0 + rq < ql) {
        lse[so + i0 + rq] = m + logf(l);
        delta[so + i0 + rq] = dl / l;
    }
}

// one workgroup per (query block, head, sequence): dQ of its 16 queries, keys in blocks of 64 up to kl
__global__ __launch_bounds__(256) void attn_packed_bwd_dq_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                 int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                 const int32_t *__restrict__ cu_q, const int32_t *__restrict__ cu_k,
                                                                 const float *__restrict__ dout, const float *__restrict__ lse,
                                                                 const float *__restrict__ delta, float *__restrict__ dq_out, int64_t sdq,
                                                                 int n_seq, int H, int Dh, int nq, int nk, int max_q, int max_k,
                                                                 float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                  // [Dh][QB]
    float *Os = Qs + Dh * AP_QB;     // [Dh][QB]  dO
    float *Ks = Os + Dh * AP_QB;     // [Dh][KB]
    float *Vs = Ks + Dh * AP_KB;     // [Dh][KB]
    float *Ss = Vs + Dh * AP_KB;     // [QB][KB]  dS / scale
    const int tid = threadIdx.x, h = blockIdx.y, sidx = blockIdx.z, i0 = blockIdx.x * AP_QB;
    const int HD = H * Dh;
    if (sidx == n_seq) {             // the slack columns of dQ: exactly 0
        int lo, hi;
        packed_slack(cu_q, n_seq, nq, lo, hi);
        packed_zero_slack(dq_out + size_t(h) * Dh * sdq, sdq, Dh, lo, hi, nq);
        return;
    }
    const PackedSpan qs = packed_span(cu_q, sidx, nq, max_q), ks = packed_span(cu_k, sidx, nk, max_k);
    const int ql = qs.len, kl = ks.len;
    float *dqg = dq_out + size_t(h) * Dh * sdq + qs.start;
    if (i0 >= ql) return;            // workgroup-uniform, before the first barrier: a neighbour's columns
    if (kl == 0) {                   // a sequence without keys: this block's dQ is 0
        for (int e = tid; e < Dh * AP_QB; e += 256) {
            const int d = e / AP_QB, qi = e - d * AP_QB;
            if (i0 + qi < ql) dqg[size_t(d) * sdq + i0 + qi] = 0.f;
        }
        return;
    }
    const float *qg = q + size_t(h) * Dh * sq + qs.start;
    const float *kg = kv + size_t(h) * Dh * skv + ks.start, *vg = kg + size_t(HD) * skv;
    const float *dg = dout + size_t(h) * Dh * nq + qs.start;
    const float slope = slopes[h], inv = 1.f / scale_div;
    const size_t so = size_t(h) * nq + qs.start;
    for (int e = tid; e < Dh * AP_QB; e += 256) {
        const int d = e / AP_QB, qi = e - d * AP_QB, i = min(i0 + qi, ql - 1);
        Qs[e] = qg[size_t(d) * sq + i];
        Os[e] = dg[size_t(d) * nq + i];
    }
    constexpr int MAXA = 8;          // dQ elements per thread: Dh * 16 <= 128 * 16 = 8 * 256
    float dq[MAXA];
#pragma unroll
    for (int u = 0; u < MAXA; ++u) dq[u] = 0.f;
    for (int j0 = 0; j0 < kl; j0 += AP_KB) {
        __syncthreads();
        for (int e = tid; e < Dh * AP_KB; e += 256) {
            const int d = e / AP_KB, j = e - d * AP_KB, jc = min(j0 + j, kl - 1);
            Ks[e] = kg[size_t(d) * skv + jc];
            Vs[e] = vg[size_t(d) * skv + jc];
        }
        __syncthreads();
        for (int e = tid; e < AP_QB * AP_KB; e += 256) {
            const int qi = e / AP_KB, j = e - qi * AP_KB, i = i0 + qi;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AP_QB + qi], Ks[d * AP_KB + j], s);
                dp = fmaf(Os[d * AP_QB + qi], Vs[d * AP_KB + j], dp);
            }
            float ds = 0.f;
            if (i < ql && j0 + j < kl) {
                const float pn = expf(attn_packed_bwd_logit(s, inv, i, j0 + j, kl, slope) - lse[so + i]);
                ds = pn * (dp - delta[so + i]) * inv;
            }
            Ss[e] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXA; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * AP_QB) {
                const int d = e / AP_QB, qi = e - d * AP_QB;
                float a = dq[u];
                for (int j = 0; j < AP_KB; ++j) a = fmaf(Ss[qi * AP_KB + j], Ks[d * AP_KB + j], a);
                dq[u] = a;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXA; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * AP_QB) {
            const int d = e / AP_QB, qi = e - d * AP_QB;
            if (i0 + qi < ql) dqg[size_t(d) * sdq + i0 + qi] = dq[u];
        }
    }
}

// one workgroup per (key block, head, sequence): dK and dV of its 64 keys, queries in blocks of 16 up to ql
__global__ __launch_bounds__(256) void attn_packed_bwd_dkv_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                  int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                  const int32_t *__restrict__ cu_q, const int32_t *__restrict__ cu_k,
                                                                  const float *__restrict__ dout, const float *__restrict__ lse,
                                                                  const float *__restrict__ delta, float *__restrict__ dkv, int64_t sdkv,
                                                                  int n_seq, int H, int Dh, int nq, int nk, int max_q, int max_k,
                                                                  float scale_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Ks = sm;                  // [Dh][KB]
    float *Vs = Ks + Dh * AP_KB;     // [Dh][KB]
    float *Qs = Vs + Dh * AP_KB;     // [Dh][QB]
    float *Os = Qs + Dh * AP_QB;     // [Dh][QB]
    float *Ps = Os + Dh * AP_QB;     // [QB][KB]
    float *Ss = Ps + AP_QB * AP_KB;  // [QB][KB]
    const int tid = threadIdx.x, h = blockIdx.y, sidx = blockIdx.z, j0 = blockIdx.x * AP_KB;
    const int HD = H * Dh;
    if (sidx == n_seq) {             // the slack columns of dK and dV: exactly 0
        int lo, hi;
        packed_slack(cu_k, n_seq, nk, lo, hi);
        packed_zero_slack(dkv + size_t(h) * Dh * sdkv, sdkv, Dh, lo, hi, nk);
        packed_zero_slack(dkv + (size_t(HD) + size_t(h) * Dh) * sdkv, sdkv, Dh, lo, hi, nk);
        return;
    }
    const PackedSpan qs = packed_span(cu_q, sidx, nq, max_q), ks = packed_span(cu_k, sidx, nk, max_k);
    const int ql = qs.len, kl = ks.len;
    float *dkg = dkv + size_t(h) * Dh * sdkv + ks.start, *dvg = dkg + size_t(HD) * sdkv;
    if (j0 >= kl) return;            // workgroup-uniform, before the first barrier: a neighbour's columns
    if (ql == 0) {                   // a sequence without queries: this block's dK / dV are 0
        for (int e = tid; e < Dh * AP_KB; e += 256) {
            const int d = e / AP_KB, j = e - d * AP_KB;
            if (j0 + j < kl) dkg[size_t(d) * sdkv + j0 + j] = dvg[size_t(d) * sdkv + j0 + j] = 0.f;
        }
        return;
    }
    const float *qg = q + size_t(h) * Dh * sq + qs.start;
    const float *kg = kv + size_t(h) * Dh * skv + ks.start, *vg = kg + size_t(HD) * skv;
    const float *dg = dout + size_t(h) * Dh * nq + qs.start;
    const float slope = slopes[h], inv = 1.f / scale_div;
    const size_t so = size_t(h) * nq + qs.start;
    for (int e = tid; e < Dh * AP_KB; e += 256) {
        const int d = e / AP_KB, j = e - d * AP_KB, jc = min(j0 + j, kl - 1);
        Ks[e] = kg[size_t(d) * skv + jc];
        Vs[e] = vg[size_t(d) * skv + jc];
    }
    constexpr int MAXE = 32;         // dK / dV elements per thread: Dh * 64 <= 128 * 64 = 32 * 256
    float dk[MAXE], dv[MAXE];
#pragma unroll
    for (int u = 0; u < MAXE; ++u) dk[u] = dv[u] = 0.f;
    for (int i0 = 0; i0 < ql; i0 += AP_QB) {
        __syncthreads();
        for (int e = tid; e < Dh * AP_QB; e += 256) {
            const int d = e / AP_QB, qi = e - d * AP_QB, i = min(i0 + qi, ql - 1);
            Qs[e] = qg[size_t(d) * sq + i];
            Os[e] = (i0 + qi < ql) ? dg[size_t(d) * nq + i] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < AP_QB * AP_KB; e += 256) {
            const int qi = e / AP_KB, j = e - qi * AP_KB, i = i0 + qi;
            float s = 0.f, dp = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s = fmaf(Qs[d * AP_QB + qi], Ks[d * AP_KB + j], s);
                dp = fmaf(Os[d * AP_QB + qi], Vs[d * AP_KB + j], dp);
            }
            float pn = 0.f, ds = 0.f;
            if (i < ql && j0 + j < kl) {
                pn = expf(attn_packed_bwd_logit(s, inv, i, j0 + j, kl, slope) - lse[so + i]);
                ds = pn * (dp - delta[so + i]) * inv;
            }
            Ps[e] = pn;
            Ss[e] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXE; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * AP_KB) {
                const int d = e / AP_KB, j = e - d * AP_KB;
                float ak = dk[u], av = dv[u];
#pragma unroll
                for (int qi = 0; qi < AP_QB; ++qi) {
                    ak = fmaf(Ss[qi * AP_KB + j], Qs[d * AP_QB + qi], ak);
                    av = fmaf(Ps[qi * AP_KB + j], Os[d * AP_QB + qi], av);
                }
                dk[u] = ak;
                dv[u] = av;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXE; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * AP_KB) {
            const int d = e / AP_KB, j = e - d * AP_KB;
            if (j0 + j < kl) {
                dkg[size_t(d) * sdkv + j0 + j] = dk[u];
                dvg[size_t(d) * sdkv + j0 + j] = dv[u];
            }
        }
    }
}

// ------------------------------------------------------------------ layout kernels
constexpr int PR_CH = 8;     // channels per thread

// out[c, n] = x[b, c, n - start_b] where sequence b owns column n and n - start_b < t; 0 where no sequence does.  One thread
// per packed column and PR_CH channels: it finds its sequence by bisection over cu (the index stays in [0, n_seq] whatever
// the array holds), checks the ownership it found, then walks its channels.
__global__ __launch_bounds__(256) void pack_rows_kernel(const float *__restrict__ x, const int32_t *__restrict__ cu,
                                                        float *__restrict__ out, int B, int C, int T, int N) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    int lo = 0, hi = B;              // the last b in [0, B) with clamp(cu[b]) <= n, if any
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (min(max(int(cu[mid]), 0), N) <= n) lo = mid; else hi = mid;
    }
    const PackedSpan sp = packed_span(cu, lo, N, T);
    const int i = n - sp.start;
    const bool own = i >= 0 && i < sp.len;
    const int c0 = blockIdx.y * PR_CH;
    const float *xb = x + (size_t(lo) * C + c0) * T + (own ? i : 0);
#pragma unroll
    for (int u = 0; u < PR_CH; ++u)
        if (c0 + u < C) out[size_t(c0 + u) * N + n] = own ? xb[size_t(u) * T] : 0.f;
}

// out[b, c, i] = i < len_b ? xp[c, start_b + i] : 0: a select on the index, the padded positions read nothing
__global__ __launch_bounds__(256) void unpack_rows_kernel(const float *__restrict__ xp, const int32_t *__restrict__ cu,
                                                          float *__restrict__ out, int B, int C, int T, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
    if (i >= T) return;
    const PackedSpan sp = packed_span(cu, b, N, T);
    const bool own = i < sp.len;
    const int c0 = blockIdx.y * PR_CH;
    const float *src = xp + size_t(c0) * N + sp.start + (own ? i : 0);
    float *dst = out + (size_t(b) * C + c0) * T + i;
#pragma unroll
    for (int u = 0; u < PR_CH; ++u)
        if (c0 + u < C) dst[size_t(u) * T] = own ? src[size_t(u) * N] : 0.f;
}

// ------------------------------------------------------------------ host side: one pick and its rows
struct AttnPackedPick;
#define AGX_ATTN_PACKED_ARGS                                                                                                 \
    const AttnPackedPick &k, const float *q, const float *kv, int64_t sq, int64_t skv, const float *slopes, const int32_t *cu_q, \
        const int32_t *cu_k, float *out, int n_seq, int H, int Dh, int nq, int nk, int max_q, int max_k, float scale_div,       \
        hipStream_t st
struct AttnPackedRow { const char *name; int (*launch)(AGX_ATTN_PACKED_ARGS); };
// empty: n_seq, heads, nq or nk <= 0 -- the entry points return AGX_OK and launch nothing; code: a refusal (fail() was called)
struct AttnPackedPick { const AttnPackedRow *row; const char *bwd_name; dim3 grid; size_t lds; int lds_limit, code; bool empty; };

template <int DVT>
static int run_attention_packed(AGX_ATTN_PACKED_ARGS) {
    auto kern = attention_packed_kernel<DVT>;
    static DeviceOnce once;
    if (int rc = prepare_kernel(reinterpret_cast<const void *>(kern), once, k.lds_limit, nullptr, "attention_packed")) return rc;
    hipLaunchKernelGGL(kern, k.grid, dim3(256), k.lds, st, q, kv, sq, skv, slopes, cu_q, cu_k, out, n_seq, H, Dh, nq, nk, max_q, max_k,
                       scale_div);
    return check_launch("attention_packed");
}

#define AGX_ATTN_ROW(DVT) {"attention_packed<" #DVT ">", run_attention_packed<DVT>}
static const AttnPackedRow kAttnPackedRows[3] = {AGX_ATTN_ROW(1), AGX_ATTN_ROW(2), AGX_ATTN_ROW(4)};   // [log2(DVT)]
#undef AGX_ATTN_ROW

// the grid's x extent for sequences of up to `bound` positions in blocks of `block`: at least one, for the slack workgroups
static int packed_blocks(int bound, int block) { return bound > 0 ? ceil_div(bound, block) : 1; }

static AttnPackedPick attn_packed_pick(const char *op, int n_seq, int H, int Dh, int nq, int nk, int max_q, int max_k) {
    AttnPackedPick k{};
    k.empty = n_seq <= 0 || H <= 0 || nq <= 0 || nk <= 0;
    if (Dh <= 0) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: bad shape head_dim=%d", op, Dh);
    else if (Dh > 128) k.code = fail(AGX_ERR_UNSUPPORTED, "%s: head_dim=%d > 128", op, Dh);
    else if (max_q < 0 || max_k < 0) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: max_q=%d, max_k=%d: a bound is >= 0", op, max_q, max_k);
    else if (H > 65535 || n_seq >= 65535) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: grid too large", op);
    if (k.code || k.empty) return k;
    const int dvt = Dh <= 32 ? 1 : (Dh <= 64 ? 2 : 4), di = dvt / 2;   // 32-row tiles of the head dim; di = log2(dvt)
    k.row = &kAttnPackedRows[di];
    k.bwd_name = "attn_packed_bwd_stats+attn_packed_bwd_dq+attn_packed_bwd_dkv";
    k.lds = size_t(2) * 32 * dvt * 65 * sizeof(float);                 // the double-buffered V block
    k.lds_limit = k.lds > 48 * 1024 ? 96 * 1024 : 0;
    k.grid = dim3(packed_blocks(min(max_q, nq), 128), H, n_seq + 1);   // z = n_seq: the slack workgroups
    return k;
}

// a row pitch must hold the row: the kernels index [row * pitch + column]
static int packed_stride(const char *op, int64_t have, int64_t need, const char *what) {
    return have >= need ? AGX_OK : fail(AGX_ERR_BAD_SHAPE, "%s: %s row stride %lld < %lld", op, what, (long long)have, (long long)need);
}

static int launch_attention_packed_backward(const float *q, const float *kv, int64_t sq, int64_t skv, const float *slopes,
                                            const int32_t *cu_q, const int32_t *cu_k, const float *dout, float *dq, float *dkv,
                                            int64_t sdq, int64_t sdkv, float *workspace, int n_seq, int H, int Dh, int nq, int nk,
                                            int max_q, int max_k, float scale_div, hipStream_t st) {
    float *lse = workspace, *delta = workspace + size_t(H) * nq;
    const dim3 gq(packed_blocks(min(max_q, nq), AP_QB), H, n_seq + 1), gk(packed_blocks(min(max_k, nk), AP_KB), H, n_seq + 1);
    const size_t l_stats = size_t(2 * Dh * AP_QB + 2 * Dh * AP_KB + 2 * AP_QB * AP_KB) * sizeof(float);
    const size_t l_dq = size_t(2 * Dh * AP_QB + 2 * Dh * AP_KB + AP_QB * AP_KB) * sizeof(float);
    const size_t l_dkv = size_t(2 * Dh * AP_KB + 2 * Dh * AP_QB + 2 * AP_QB * AP_KB) * sizeof(float);
    static DeviceOnce once[3];
    {
        const void *ks[3] = {reinterpret_cast<const void *>(attn_packed_bwd_stats_kernel),
                             reinterpret_cast<const void *>(attn_packed_bwd_dq_kernel),
                             reinterpret_cast<const void *>(attn_packed_bwd_dkv_kernel)};
        for (int i = 0; i < 3; ++i)
            if (int rc = prepare_kernel(ks[i], once[i], 96 * 1024, nullptr, "attention_packed_backward")) return rc;   // head_dim 128: 90 KB
    }
    hipLaunchKernelGGL(attn_packed_bwd_stats_kernel, gq, dim3(256), l_stats, st, q, kv, sq, skv, slopes, cu_q, cu_k, dout, lse, delta,
                       n_seq, H, Dh, nq, nk, max_q, max_k, scale_div);
    hipLaunchKernelGGL(attn_packed_bwd_dq_kernel, gq, dim3(256), l_dq, st, q, kv, sq, skv, slopes, cu_q, cu_k, dout, lse, delta, dq, sdq,
                       n_seq, H, Dh, nq, nk, max_q, max_k, scale_div);
    hipLaunchKernelGGL(attn_packed_bwd_dkv_kernel, gk, dim3(256), l_dkv, st, q, kv, sq, skv, slopes, cu_q, cu_k, dout, lse, delta, dkv,
                       sdkv, n_seq, H, Dh, nq, nk, max_q, max_k, scale_div);
    return check_launch("attention_packed_backward");
}

// the shapes both layout kernels accept; *empty: no output element exists, nothing to launch (out_n: the output is the packed
// tensor; the padded one exists with n == 0 too and is then all padding)
static int pack_rows_check(const char *op, int B, int C, int T, int N, bool out_n, bool *empty) {
    *empty = B <= 0 || C <= 0 || T <= 0 || (out_n ? N <= 0 : N < 0);
    if (*empty) return AGX_OK;
    if (B >= 65535 || ceil_div(C, PR_CH) > 65535) return fail(AGX_ERR_BAD_SHAPE, "%s: (%d, %d, %d) is beyond the grid", op, B, C, T);
    return AGX_OK;
}

}  // namespace agx

extern "C" {

int agx_attention_alibi_packed(const float *q, const float *kv, int64_t q_row_stride, int64_t kv_row_stride, const float *slopes,
                               const int32_t *cu_q, const int32_t *cu_k, float *out, int32_t n_seq, int32_t heads, int32_t head_dim,
                               int32_t nq, int32_t nk, int32_t max_q, int32_t max_k, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_packed";
    const AttnPackedPick k = attn_packed_pick(op, n_seq, heads, head_dim, nq, nk, max_q, max_k);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (int rc = packed_stride(op, q_row_stride, nq, "q")) return rc;
    if (int rc = packed_stride(op, kv_row_stride, nk, "kv")) return rc;
    if (!q || !kv || !slopes || !cu_q || !cu_k || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    return k.row->launch(k, q, kv, q_row_stride, kv_row_stride, slopes, cu_q, cu_k, out, n_seq, heads, head_dim, nq, nk, max_q, max_k,
                         scale_div, static_cast<hipStream_t>(stream));
}

size_t agx_attention_packed_backward_workspace_bytes(int32_t heads, int32_t nq) {
    if (heads <= 0 || nq <= 0) return 0;
    return size_t(2) * heads * nq * sizeof(float);
}

int agx_attention_alibi_packed_backward(const float *q, const float *kv, int64_t q_row_stride, int64_t kv_row_stride,
                                        const float *slopes, const int32_t *cu_q, const int32_t *cu_k, const float *out,
                                        const float *dout, float *dq, float *dkv, int64_t dq_row_stride, int64_t dkv_row_stride,
                                        float *workspace, size_t workspace_bytes, int32_t n_seq, int32_t heads, int32_t head_dim,
                                        int32_t nq, int32_t nk, int32_t max_q, int32_t max_k, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_packed_backward";
    const AttnPackedPick k = attn_packed_pick(op, n_seq, heads, head_dim, nq, nk, max_q, max_k);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (int rc = packed_stride(op, q_row_stride, nq, "q")) return rc;
    if (int rc = packed_stride(op, kv_row_stride, nk, "kv")) return rc;
    if (int rc = packed_stride(op, dq_row_stride, nq, "dq")) return rc;
    if (int rc = packed_stride(op, dkv_row_stride, nk, "dkv")) return rc;
    if (workspace_bytes < agx_attention_packed_backward_workspace_bytes(heads, nq))
        return fail(AGX_ERR_WORKSPACE, "%s: workspace too small", op);
    (void)out;   // not read: P is recomputed from the row statistics
    if (!q || !kv || !slopes || !cu_q || !cu_k || !dout || !dq || !dkv || !workspace) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    return launch_attention_packed_backward(q, kv, q_row_stride, kv_row_stride, slopes, cu_q, cu_k, dout, dq, dkv, dq_row_stride,
                                            dkv_row_stride, workspace, n_seq, heads, head_dim, nq, nk, max_q, max_k, scale_div,
                                            static_cast<hipStream_t>(stream));
}

int agx_attention_packed_kernel_name(int32_t n_seq, int32_t heads, int32_t head_dim, int32_t nq, int32_t nk, int32_t max_q,
                                     int32_t max_k, int32_t backward, char *buf, size_t buf_len) {
    using namespace agx;
    const AttnPackedPick k = attn_packed_pick(backward ? "attention_alibi_packed_backward" : "attention_alibi_packed", n_seq, heads,
                                              head_dim, nq, nk, max_q, max_k);
    if (k.code) return k.code;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "agx_attention_packed_kernel_name: NULL buffer");
    snprintf(buf, buf_len, "%s", k.empty ? "none" : (backward ? k.bwd_name : k.row->name));
    return AGX_OK;
}

int agx_pack_rows(const float *x, const int32_t *cu, float *out, int32_t batch, int32_t channels, int32_t t, int32_t n, void *stream) {
    using namespace agx;
    bool empty;
    if (int rc = pack_rows_check("pack_rows", batch, channels, t, n, true, &empty)) return rc;
    if (empty) return AGX_OK;
    if (!x || !cu || !out) return fail(AGX_ERR_NULL_POINTER, "pack_rows: NULL pointer");
    hipLaunchKernelGGL(pack_rows_kernel, dim3(ceil_div(n, 256), ceil_div(channels, PR_CH)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       cu, out, batch, channels, t, n);
    return check_launch("pack_rows");
}

int agx_unpack_rows(const float *xp, const int32_t *cu, float *out, int32_t batch, int32_t channels, int32_t t, int32_t n, void *stream) {
    using namespace agx;
    bool empty;
    if (int rc = pack_rows_check("unpack_rows", batch, channels, t, n, false, &empty)) return rc;
    if (empty) return AGX_OK;
    if ((!xp && n > 0) || !cu || !out) return fail(AGX_ERR_NULL_POINTER, "unpack_rows: NULL pointer");   // n == 0: xp is never read
    hipLaunchKernelGGL(unpack_rows_kernel, dim3(ceil_div(t, 256), ceil_div(channels, PR_CH), batch), dim3(256), 0,
                       static_cast<hipStream_t>(stream), xp, cu, out, batch, channels, t, n);
    return check_launch("unpack_rows");
}

}  // extern "C"
