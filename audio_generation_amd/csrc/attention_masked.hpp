// Masked ALiBi attention: the one forward body and the one backward trio behind the cross, causal, window, stream, ragged and
// packed families (attention_{cross,causal,window,stream,ragged,packed}.hip), the dropout family (attention_dropout.hip: the cross
// view behind batch strides, with a dropout policy) and the self-attention split backward (attention_flash.hip: the cross view on
// the packed qkv layout), and the host scaffolding they share.
// (One kernel is not an instance: the ragged forward, which measured slower as one; attention_ragged.hip says why.  The
// self-attention forwards of attention_flash.hip / attention.hip, with their bf16 variants, are their own code.)
//
// Each family's file holds its __global__ kernels -- a few lines that build a View and call a body -- and its C entry points.
// A View says what the families really differ in and nothing else:
//   * AttnView: the rows of this workgroup's (item, head) -- base pointers of Q, K, V, dO and their pitches, of whatever
//     integer type the family's kernel arguments have -- and where its lse / delta start;
//   * a mask it inherits from (SymMask, CausalMask, WindowMask below): the valid lengths ql / kl, the columns the workgroup
//     owns (q_end / k_end), the workgroup-uniform block bounds, the clamp and column of a K gather and of a V load, which V
//     positions are staged as zero, the visibility predicate, the bias, the backward's logit, and the arithmetic traits.
// The bodies are __forceinline__ templates: a family's kernel is the body with its View's answers folded in, so where two
// families computed differently before they were folded (the traits), they still do.  DESIGN.md 4.5 has the table of Views
// against traits and the device-code comparison with the hand-copied kernels.
//
// What every family does about masked values, written once:
//   * A masked probability is exactly 0, but 0 * NaN = NaN in an MFMA and in an fmaf, and a masked position may hold anything
//     (a cache's unwritten tail, a stale ring column, the padding of a ragged row).  So V is staged as zeros wherever
//     v_live() says no, dO of a query >= ql is staged as zero in dK / dV, every K / Q load is clamped to a position that holds
//     what it should (k_col(), min(., ql - 1)), and a masked score is replaced with a select, whatever it was.
//   * Every loop bound is a function of blockIdx and kernel arguments (or of one workgroup-uniform load), so every thread
//     meets every __syncthreads; an early exit happens before the first barrier.
#pragma once

#include <algorithm>
#include <tuple>

#include "mfma_tile.hpp"

namespace agx {

constexpr int kAttnQB = 16;              // backward: queries per block
constexpr int kAttnKB = 64;              // keys per block, forward and backward
// The backward's score of a masked key: a finite sentinel no logit comes near (the forward uses -INFINITY: its row maximum
// lives in registers next to a select; the stats kernel reduces through LDS and fmaxf and keeps every value finite).
constexpr float kAttnMasked = -3.0e38f;

// ------------------------------------------------------------------------------------------------------------ the masks
// Symmetric bias -slope |i - j|, keys [0, kl), queries [0, ql): cross (ql = Tq, kl = Tk), ragged (the row's lengths) and
// packed (the sequence's lengths).  EXIT: the lengths come from device memory, so a workgroup may have nothing to compute.
template <bool EXIT>
struct SymMask {
    // A workgroup with no valid query (its first is >= ql) or a row without keys zero-fills the columns it owns, [.., q_end) /
    // [.., k_end), and returns before the first barrier.  Ragged owns the whole padded row (q_end = Tq); packed owns its
    // sequence only (q_end = ql: beyond it the columns are a neighbour's, and nothing is written).
    static constexpr bool kEarlyExit = EXIT;
    // Every key block holds a key < kl, so after the first block the running maximum is finite and exp(-inf - mn) = 0 masks.
    static constexpr bool kGuardMs = false, kSelectMasked = false;
    static constexpr bool kRoundBothProducts = false;   // see attn_score
    int ql, kl, q_end, k_end;
    // forward: blocks [blk_begin, blk_end) of 64 keys for the 128 queries from q0; p = qpos(clamped query)
    __device__ __forceinline__ int blk_begin(int) const { return 0; }
    __device__ __forceinline__ int blk_end(int) const { return (kl + kAttnKB - 1) / kAttnKB; }
    __device__ __forceinline__ int qpos(int ic) const { return ic; }
    __device__ __forceinline__ bool v_live(int j) const { return j < kl; }
    __device__ __forceinline__ int v_col(int j) const { return j; }
    __device__ __forceinline__ int k_col(int j) const { return min(j, kl - 1); }
    __device__ __forceinline__ bool visible(int, int j) const { return j < kl; }
    __device__ __forceinline__ float bias(int p, int j) const { return fabsf(float(p - j)); }   // == M[h, i, j] of Alibi._create_M
    // backward: key blocks [key_begin, key_end) of the 16 queries from i0, query blocks [query_begin, query_end) of the 64 keys from j0
    __device__ __forceinline__ int stats_row(int i) const { return i; }
    __device__ __forceinline__ int key_begin(int) const { return 0; }
    __device__ __forceinline__ int key_end(int) const { return kl; }
    __device__ __forceinline__ int query_begin(int) const { return 0; }
    __device__ __forceinline__ int query_end(int) const { return ql; }
    // The bias is taken relative to the query's nearest key, max(0, i - (kl - 1)) positions away: a constant of the row, which
    // the softmax does not see, subtracted exactly.  A query far beyond the last key (ql > kl) with a steep slope would otherwise
    // have all its logits near -slope (i - kl), and lse = m + log l, rounded to an ulp of that magnitude, would lose log l.
    // The workspace's lse is that of these relative logits.
    __device__ __forceinline__ float logit(float s, float inv, int i, int j, float slope) const {
        return fmaf(-float(abs(i - j) - max(0, i - (kl - 1))), slope, s * inv);
    }
};

// One-sided bias -slope (p - j), keys j <= p = i + q_pos0 and j < kl: causal.  The backward is the full self-attention,
// q_pos0 = 0 and ql = kl = T, where j <= i < T already implies j < kl: CACHE = false leaves that test out of its inner loops.
template <bool CACHE>
struct CausalMask {
    static constexpr bool kEarlyExit = false;
    // Key 0 is visible to every query (q_pos0 >= 0), so after block 0 the running maximum is finite; a later all-masked block
    // has bm = -inf, mn = m, alpha = exp(0) = 1, pe = exp(-inf) = 0: the identity on (m, l, o), and (-inf) - (-inf) is never
    // formed.  The stats kernel's exp(sentinel - mn) = 0 holds for the same reason.
    static constexpr bool kGuardMs = false, kSelectMasked = false;
    static constexpr bool kRoundBothProducts = true;   // see attn_score
    int ql, kl, q_end, k_end, q_pos0;
    // the key loop ends at the last block any of the workgroup's queries sees; there is no finer skip (a wave-uniform branch
    // around the MFMAs of a block only the later waves see was measured and made no difference)
    __device__ __forceinline__ int blk_begin(int) const { return 0; }
    __device__ __forceinline__ int blk_end(int q0) const { return min(kl - 1, q0 + 127 + q_pos0) / kAttnKB + 1; }
    __device__ __forceinline__ int qpos(int ic) const { return ic + q_pos0; }
    __device__ __forceinline__ bool v_live(int j) const { return j < kl; }
    __device__ __forceinline__ int v_col(int j) const { return j; }
    __device__ __forceinline__ int k_col(int j) const { return min(j, kl - 1); }
    __device__ __forceinline__ bool visible(int p, int j) const { return j <= p && (!CACHE || j < kl); }
    __device__ __forceinline__ float bias(int p, int j) const { return float(p - j); }
    __device__ __forceinline__ int stats_row(int i) const { return min(i, ql - 1); }
    __device__ __forceinline__ int key_begin(int) const { return 0; }
    __device__ __forceinline__ int key_end(int i0) const { return min(i0 + kAttnQB, kl); }
    __device__ __forceinline__ int query_begin(int j0) const { return j0; }   // queries before j0 see none of these keys
    __device__ __forceinline__ int query_end(int) const { return ql; }
    __device__ __forceinline__ float logit(float s, float inv, int i, int j, float slope) const { return fmaf(-float(i - j), slope, s * inv); }
};

// One-sided bias, the last W keys only: j in (p - W, p].  The forward (window: LINEAR allowed, ring = 0; stream: the ring is
// mandatory) reads key j from column j mod ring; place() sets the workgroup's range.  The backward is the full linear
// self-attention, ql = kl = T.
template <bool LINEAR>
struct WindowMask {
    static constexpr bool kEarlyExit = false;
    // Leading all-masked blocks: a row can meet a block in which every key is masked BEFORE it has seen any key (T = 130,
    // W = 3: query 127 sees keys 125..127, block 0 is empty for it), and m = -inf, bm = -inf would form (-inf) - (-inf) = NaN.
    // kGuardMs: the forward's exponentials are taken against ms = (mn == -inf ? 0 : mn); for such a block alpha = 0 scales
    // l = 0 and o = 0 to themselves, every pe = 0, m stays -inf: the exact identity.  Once a row has seen a key, ms = mn.
    // kSelectMasked: the stats kernel's m is then still the sentinel and exp(sentinel - sentinel) = 1 would count 64 masked
    // keys, so the probability of a masked key is a select, 0 whatever mn is.
    static constexpr bool kGuardMs = true, kSelectMasked = true;
    static constexpr bool kRoundBothProducts = true;   // see attn_score
    int ql, kl, q_end, k_end, q_pos0, W;
    int ring, jlo, pmax, c0;   // forward: the keys [jlo, pmax] any of the 128 queries sees, and the column of key jlo
    // Blocks are aligned to absolute positions (block = j / 64), so what a query adds up, and in which order, does not depend on
    // the chunk that delivered it.  pmax - jlo < ring (host check): one wrap at most, no division in the loop.
    __device__ __forceinline__ void place(int q0, int Tq) {
        pmax = min(q0 + 127, Tq - 1) + q_pos0;
        jlo = max(0, q0 + q_pos0 - W + 1);
        c0 = (!LINEAR || ring > 0) ? jlo % ring : jlo;
    }
    __device__ __forceinline__ int col_of(int j) const {   // the column of key j in [jlo, pmax]
        const int c = c0 + (j - jlo);
        return ((!LINEAR || ring > 0) && c >= ring) ? c - ring : c;
    }
    __device__ __forceinline__ int blk_begin(int) const { return jlo / kAttnKB; }
    __device__ __forceinline__ int blk_end(int) const { return pmax / kAttnKB + 1; }
    __device__ __forceinline__ int qpos(int ic) const { return ic + q_pos0; }
    // Stale ring columns: outside [jlo, pmax] a column holds an older frame or unwritten memory.  Inside it every column is a
    // frame of this stream, finite, and a masked one meets p = 0.
    __device__ __forceinline__ bool v_live(int j) const { return j >= jlo && j <= pmax; }
    __device__ __forceinline__ int v_col(int j) const { return col_of(j); }
    __device__ __forceinline__ int k_col(int j) const { return col_of(max(jlo, min(j, pmax))); }
    __device__ __forceinline__ bool visible(int p, int j) const { return j <= p && j > p - W; }
    __device__ __forceinline__ float bias(int p, int j) const { return float(p - j); }
    __device__ __forceinline__ int stats_row(int i) const { return min(i, ql - 1); }
    __device__ __forceinline__ int key_begin(int i0) const { return max(0, i0 - W + 1) / kAttnKB * kAttnKB; }
    __device__ __forceinline__ int key_end(int i0) const { return min(i0 + kAttnQB, kl); }
    __device__ __forceinline__ int query_begin(int j0) const { return j0; }
    __device__ __forceinline__ int query_end(int j0) const { return min(ql, j0 + kAttnKB - 1 + W); }   // W <= T (host): no overflow
    __device__ __forceinline__ float logit(float s, float inv, int i, int j, float slope) const { return fmaf(-float(i - j), slope, s * inv); }
};

// The pitches have the integer types of the family's kernel arguments (int, or int64_t for the packed layout).  The bodies copy
// them into locals before their loops: read through the struct, the dQ kernels took 66 VGPRs instead of 64 (7 waves per SIMD
// instead of 8) for the same instructions in another order.
template <class Mask, class PQ = int, class PK = int, class PD = int>
struct AttnView : Mask {
    const float *qg, *kg, *vg, *dg;   // Q, K, V and (backward) dO rows of this (item, head)
    PQ pq;                            // their pitches; pd is that of out and dout
    PK pk;
    PD pd;
    size_t so;                        // backward: where this (item, head)'s lse / delta start
};

// The view of the window family (attention_window.hip forward and backward, attention_stream.hip): q rows of pitch Tq behind a
// batch stride, kv rows of pitch krs behind another, the queries at positions q_pos0 .. q_pos0 + Tq - 1.  dout: the backward's
// (NULL in a forward view, which has no dO rows).  A forward wrapper calls place() on the result; the backward reads no column.
template <bool LINEAR>
static __device__ __forceinline__ AttnView<WindowMask<LINEAR>> window_view(const float *q, const float *kv, int64_t sq, int64_t skv,
                                                                           int krs, const float *dout, int h, int b, int H, int Dh,
                                                                           int Tq, int q_pos0, int W, int ring) {
    const int HD = H * Dh;
    AttnView<WindowMask<LINEAR>> v{};
    v.ql = v.q_end = v.kl = v.k_end = Tq;
    v.q_pos0 = q_pos0;
    v.W = W;
    v.ring = ring;
    v.qg = q + size_t(b) * sq + size_t(h) * Dh * Tq;
    v.kg = kv + size_t(b) * skv + size_t(h) * Dh * krs;
    v.vg = v.kg + size_t(HD) * krs;
    if (dout) v.dg = dout + (size_t(b) * HD + h * Dh) * Tq;
    v.pq = v.pd = Tq;
    v.pk = krs;
    v.so = (size_t(b) * H + h) * Tq;
    return v;
}

// The forward's biased score a * inv - b * slope (a: the MFMA's dot product, b: the mask's bias).  The one-sided families round
// both products and subtract (EXACT2: their compiler had packed the two multiplies before it looked for an fma, for all 32
// scores of a lane); the symmetric families leave the contraction to the compiler, as their source always did, and get an fma
// for most of a lane's scores.  Which it is changes the last bit of a score whenever scale_div is no power of two, and a cached
// step must reproduce the full run's bits, so the one-sided form is written down here instead of being left to a heuristic.
template <bool EXACT2>
static __device__ __forceinline__ float attn_score(float a, float inv, float b, float slope) {
    if constexpr (EXACT2) {
#pragma clang fp contract(off)
        const float x = a * inv, y = b * slope;
        return x - y;
    } else {
        return a * inv - b * slope;
    }
}

// Dropout on the probabilities is a policy of the bodies.  kDrop = false: no factor exists, and every line that would use one is
// compiled out, so a family without dropout pays nothing for it.  A policy with kDrop = true (PhiloxDrop, attention_dropout.hip) answers
//   live()              whether any pair is dropped at all (p > 0), a runtime test around the forward's hook;
//   quartet(jq, i, f)   the factors (1 / (1 - p) or 0) of keys 4 jq .. 4 jq + 3 of query i, when live();
//   factors(jq, i, f)   the same, or the scale for all four when not live() -- what the backward multiplies by either way.
// The softmax statistics (m, l, lse) never see a factor: P is the softmax, P~ = f o P meets V and dO only.
struct NoDrop {
    static constexpr bool kDrop = false;
};

// --------------------------------------------------------------------------------------------------------- the forward
// 128 queries per workgroup (one per lane of each wave's two halves), keys in blocks of 64: the query fragment in registers,
// S^T = K^T Q and O^T += V P^T on the fp32-input MFMA, V double-buffered through LDS at pitch 65, the row statistics in-lane.
// og: the out rows of this (item, head), pitch pd.  Dynamic LDS: 2 * 32 * DVT * 65 floats.
template <int DVT, class View, class Drop = NoDrop>
__device__ __forceinline__ void attn_fwd_body(const View &v, float *og, const float *slopes, int h, int Dh,
                                              float scale_div, const Drop &drop = Drop{}) {
    constexpr int KB = kAttnKB;    // keys per block (two 32-key accumulator tiles)
    constexpr int DH = 32 * DVT;   // head_dim rounded up to the tile
    constexpr int VP = KB + 1;     // LDS pitch of the V block
    extern __shared__ __attribute__((aligned(16))) float vs[];   // [2][DH][VP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto pq = v.pq;   // the pitches as locals (see AttnView)
    const auto pk = v.pk;
    const auto pd = v.pd;
    const Drop dr = drop;   // ... and the policy's fields
    const int li = lane & 31, lh = lane >> 5;
    const int q0 = blockIdx.x * 128;                   // this workgroup's first query
    if constexpr (View::kEarlyExit) {
        if (q0 >= v.ql || v.kl == 0) {                 // workgroup-uniform, before the first barrier: nothing valid to compute
            if (q0 < v.q_end)
                for (int e = tid; e < Dh * 128; e += 256) {
                    const int d = e >> 7, ii = q0 + (e & 127);
                    if (ii < v.q_end) og[size_t(d) * pd + ii] = 0.f;
                }
            return;
        }
    }
    const int i = q0 + wave * 32 + li;   // this lane's query
    const int ic = min(i, v.ql - 1);
    const int ip = v.qpos(ic);           // its position: what the bias and the mask are taken from
    const float slope = slopes[h], inv_scale = 1.f / scale_div;
    const int blk_lo = v.blk_begin(q0), blk_end = v.blk_end(q0);   // workgroup-uniform

    // ---- the query fragment stays in registers for the whole key loop ----
    float qf[DH / 2];
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) {
        const int d = 2 * s + lh;
        qf[s] = d < Dh ? v.qg[size_t(d) * pq + ic] : 0.f;
    }

    f32x16 o[DVT];
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m = -INFINITY, l = 0.f;

    auto stage_v = [&](int blk, float *dst) {   // V[dv < Dh][64 keys of block blk] -> LDS, zeros (never the stored value) where not live
        for (int e = tid; e < DH * KB; e += 256) {
            const int dv = e / KB, jj = e - dv * KB, j = blk * KB + jj;
            dst[dv * VP + jj] = (dv < Dh && v.v_live(j)) ? v.vg[size_t(dv) * pk + v.v_col(j)] : 0.f;
        }
    };
    stage_v(blk_lo, vs + (blk_lo & 1) * DH * VP);
    __syncthreads();

    for (int blk = blk_lo; blk < blk_end; ++blk) {
        const int j0 = blk * KB;
        float *vcur = vs + (blk & 1) * DH * VP;
        if (blk + 1 < blk_end) stage_v(blk + 1, vs + ((blk + 1) & 1) * DH * VP);   // next block streams in meanwhile

        // ---- S^T = K^T Q for this block: rows = keys, columns = queries ----
        f32x16 acc[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t2][r] = 0.f;
        int kcol[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) kcol[t2] = v.k_col(j0 + t2 * 32 + li);
#pragma unroll 4
        for (int s = 0; s < DH / 2; ++s) {
            const int d = min(2 * s + lh, Dh - 1);
            float kf[2];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) kf[t2] = v.kg[size_t(d) * pk + kcol[t2]];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) acc[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[t2], qf[s], acc[t2], 0, 0, 0);
        }

        // ---- scale, ALiBi, mask, online softmax (in-lane over the 32 registers + one shuffle) ----
        float bm = -INFINITY;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + t2 * 32 + acc_row(r, lh);
                float s = attn_score<View::kRoundBothProducts>(acc[t2][r], inv_scale, v.bias(ip, j), slope);
                s = v.visible(ip, j) ? s : -INFINITY;   // a select: whatever the masked score was, it is gone
                acc[t2][r] = s;
                bm = fmaxf(bm, s);
            }
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        const float mn = fmaxf(m, bm);
        float ms = mn;
        if constexpr (View::kGuardMs) ms = mn == -INFINITY ? 0.f : mn;
        const float alpha = expf(m - ms);         // first block: exp(-inf) = 0; an all-masked block after a key: exp(0) = 1
        float bl = 0.f;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pe = expf(acc[t2][r] - ms);   // masked: exp(-inf) = 0 exactly
                acc[t2][r] = pe;
                bl += pe;                                 // m and l come from the UNMASKED exponentials: P is the softmax
            }
        bl += __shfl_xor(bl, 32);
        l = l * alpha + bl;
        m = mn;
#pragma unroll
        for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;

        // ---- dropout: registers 4 g .. 4 g + 3 of a lane are the aligned key quartet j0 + 32 t2 + 8 g + 4 lh (acc_row) ----
        if constexpr (Drop::kDrop) {
            if (dr.live()) {
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        float f[4];
                        dr.quartet(uint32_t(j0 + t2 * 32 + 8 * g + 4 * lh) >> 2, uint32_t(i), f);   // i: the unclamped query
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[t2][4 * g + u] *= f[u];
                    }
            }
        }

        // ---- O^T += V P~^T : B operand = the (masked) probability registers ----
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

    const float inv = 1.f / l;    // every valid query sees a key: l > 0
    if (i < v.q_end) {
        const bool valid = i < v.ql;
#pragma unroll
        for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dv = dt * 32 + acc_row(r, lh);
                if (dv < Dh) og[size_t(dv) * pd + i] = valid ? o[dt][r] * inv : 0.f;
            }
    }
}

// ------------------------------------------------------------------------------------------------------- the backward
// Three deterministic kernels, 16 queries x 64 keys per tile through LDS, P recomputed from lse, no atomics.  The logit of a
// pair is rounded the same way in all three: the product feeds an explicit fmaf (View::logit), so no contraction can differ
// between them.  lse is built from these values, and P = exp(logit - lse) is exactly 1 on a row that one key holds alone; a
// logit near 100 rounded differently in two kernels would put 1e-5 of relative error into P instead.

// The pair pass of all three, over the 16 x 64 tile: thread tid owns query qi = tid / 16 and the aligned keys jb .. jb + 3,
// jb = 4 (tid % 16) -- Q / dO read once per four pairs, 16-byte reads of Ks / Vs, lse_i / delta_i loaded once, and one Philox call
// where there is dropout.  s[u] = q_i . k_j and dp[u] = dO_i . v_j, each the fmaf chain over d; under dropout dp takes the pair's
// factor f[u], one multiply on top (dP = f o (dO V^T)), and f is written; without, neither exists.  jq: the quartet
// (j0 + jb) / 4; i: the unclamped query.  (An ownership of four scattered elements, tid + 256 k, gives every pair the same value
// in the same LDS slot with 10 registers fewer, an occupancy step of the stats and dq kernels, and 1.6 times the time:
// DESIGN.md 4.5.)
template <class Drop>
static __device__ __forceinline__ void attn_bwd_pair_dots(const float *Qs, const float *Os, const float *Ks, const float *Vs, int Dh,
                                                          int qi, int jb, const Drop &dr, uint32_t jq, uint32_t i, float (&s)[4],
                                                          float (&dp)[4], float (&f)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = dp[u] = 0.f;
    for (int d = 0; d < Dh; ++d) {
        const float qv = Qs[d * kAttnQB + qi], ov = Os[d * kAttnQB + qi];
        const f32x4 k4 = *reinterpret_cast<const f32x4 *>(Ks + d * kAttnKB + jb);
        const f32x4 v4 = *reinterpret_cast<const f32x4 *>(Vs + d * kAttnKB + jb);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s[u] = fmaf(qv, k4[u], s[u]);
            dp[u] = fmaf(ov, v4[u], dp[u]);
        }
    }
    if constexpr (Drop::kDrop) {
        dr.factors(jq, i, f);
#pragma unroll
        for (int u = 0; u < 4; ++u) dp[u] *= f[u];
    }
}

// One workgroup per (query block, head, item): lse and delta of its 16 queries; 0 for a query >= ql it owns.  delta_i =
// sum_j P_ij dP_ij is summed online next to l, from dP values formed exactly as the dq and dkv kernels form them (the same fmaf
// chain over d), not taken as sum_d dO[d,i] O[d,i] from the forward's output: where one key holds all of a row's weight,
// dP_ij == delta_i must cancel to zero in dS = P (dP - delta), and two differently rounded dot products leave a residue that
// K / scale multiplies into dQ.  Dynamic LDS: 2 Dh 16 + 2 Dh 64 + 2 * 16 * 64 floats.
template <class View, class Drop = NoDrop>
__device__ __forceinline__ void attn_bwd_stats_body(const View &v, const float *slopes, int h, float *lse,
                                                    float *delta, int Dh, float scale_div, const Drop &drop = Drop{}) {
    constexpr int QB = kAttnQB, KB = kAttnKB;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                 // [Dh][QB]
    float *Os = Qs + Dh * QB;       // [Dh][QB]  dO
    float *Ks = Os + Dh * QB;       // [Dh][KB]
    float *Vs = Ks + Dh * KB;       // [Dh][KB]
    float *Ss = Vs + Dh * KB;       // [QB][KB]
    float *Ds = Ss + QB * KB;       // [QB][KB]  dP
    __shared__ float red[QB][16], redd[QB][16];
    const int tid = threadIdx.x, i0 = blockIdx.x * QB;
    const auto pq = v.pq;   // the pitches as locals (see AttnView)
    const auto pk = v.pk;
    const auto pd = v.pd;
    const Drop dr = drop;   // ... and the policy's fields
    if constexpr (View::kEarlyExit) {
        if (i0 >= v.ql || v.kl == 0) {      // workgroup-uniform, before the first barrier
            if (tid < QB && i0 + tid < v.q_end) lse[v.so + i0 + tid] = delta[v.so + i0 + tid] = 0.f;
            return;
        }
    }
    const float slope = slopes[h], inv = 1.f / scale_div;
    for (int e = tid; e < Dh * QB; e += 256) {
        const int d = e / QB, qi = e - d * QB, i = min(i0 + qi, v.ql - 1);
        Qs[e] = v.qg[size_t(d) * pq + i];
        Os[e] = v.dg[size_t(d) * pd + i];
    }
    const int rq = tid / 16, rl = tid % 16;   // 16 threads per query row; the pair pass: query rq, keys 4 rl .. 4 rl + 3
    float m = kAttnMasked, l = 0.f, dl = 0.f;
    const int jbeg = v.key_begin(i0), jend = v.key_end(i0);   // workgroup-uniform
    for (int j0 = jbeg; j0 < jend; j0 += KB) {
        __syncthreads();
        for (int e = tid; e < Dh * KB; e += 256) {
            const int d = e / KB, j = e - d * KB, jc = min(j0 + j, v.kl - 1);
            Ks[e] = v.kg[size_t(d) * pk + jc];
            Vs[e] = v.vg[size_t(d) * pk + jc];
        }
        __syncthreads();
        {
            const int jb = 4 * rl, i = v.stats_row(i0 + rq);
            float s[4], dp[4], f[4];
            attn_bwd_pair_dots(Qs, Os, Ks, Vs, Dh, rq, jb, dr, uint32_t(j0 + jb) >> 2, uint32_t(i0 + rq), s, dp, f);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = rq * KB + jb + u, j = j0 + jb + u;
                Ds[e] = dp[u];
                Ss[e] = v.visible(i, j) ? v.logit(s[u], inv, i, j, slope) : kAttnMasked;
            }
        }
        __syncthreads();
        float bm = kAttnMasked;
        for (int j = rl; j < KB; j += 16) bm = fmaxf(bm, Ss[rq * KB + j]);
        red[rq][rl] = bm;
        __syncthreads();
        bm = red[rq][0];
        for (int k = 1; k < 16; ++k) bm = fmaxf(bm, red[rq][k]);
        const float mn = fmaxf(m, bm);
        float bs = 0.f, bd = 0.f;
        for (int j = rl; j < KB; j += 16) {
            const float s = Ss[rq * KB + j];
            float p = expf(s - mn);                                         // 0 for a masked key once m is a real logit
            if constexpr (View::kSelectMasked) p = s == kAttnMasked ? 0.f : p;   // ... and also while mn is the sentinel
            bs += p;
            bd = fmaf(p, Ds[rq * KB + j], bd);
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
    if (rl == 0 && i0 + rq < v.q_end) {
        const bool valid = i0 + rq < v.ql;
        lse[v.so + i0 + rq] = valid ? m + logf(l) : 0.f;
        delta[v.so + i0 + rq] = valid ? dl / l : 0.f;
    }
}

// One workgroup per (query block, head, item): dQ of its 16 queries, keys in blocks of 64 over [key_begin, key_end).
// dqg: the dQ rows of this (item, head), pitch pdq.  Dynamic LDS: 2 Dh 16 + 2 Dh 64 + 16 * 64 floats.
template <class View, class Pitch, class Drop = NoDrop>
__device__ __forceinline__ void attn_bwd_dq_body(const View &v, const float *slopes, int h, const float *lse,
                                                 const float *delta, float *dqg, Pitch pdq, int Dh,
                                                 float scale_div, const Drop &drop = Drop{}) {
    constexpr int QB = kAttnQB, KB = kAttnKB;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Qs = sm;                  // [Dh][QB]
    float *Os = Qs + Dh * QB;        // [Dh][QB]  dO
    float *Ks = Os + Dh * QB;        // [Dh][KB]
    float *Vs = Ks + Dh * KB;        // [Dh][KB]
    float *Ss = Vs + Dh * KB;        // [QB][KB]  dS / scale
    const int tid = threadIdx.x, i0 = blockIdx.x * QB;
    const auto pq = v.pq;   // the pitches as locals (see AttnView)
    const auto pk = v.pk;
    const auto pd = v.pd;
    const Drop dr = drop;   // ... and the policy's fields
    if constexpr (View::kEarlyExit) {
        if (i0 >= v.ql || v.kl == 0) {       // workgroup-uniform, before the first barrier: this block's dQ is 0
            if (i0 < v.q_end)
                for (int e = tid; e < Dh * QB; e += 256) {
                    const int d = e / QB, qi = e - d * QB;
                    if (i0 + qi < v.q_end) dqg[size_t(d) * pdq + i0 + qi] = 0.f;
                }
            return;
        }
    }
    const float slope = slopes[h], inv = 1.f / scale_div;
    for (int e = tid; e < Dh * QB; e += 256) {
        const int d = e / QB, qi = e - d * QB, i = min(i0 + qi, v.ql - 1);
        Qs[e] = v.qg[size_t(d) * pq + i];
        Os[e] = v.dg[size_t(d) * pd + i];
    }
    const int rq = tid / 16, jb = 4 * (tid % 16), iq = i0 + rq;   // the pair pass: query iq, keys j0 + jb .. + 3
    float lse_i = 0.f, delta_i = 0.f;
    if (iq < v.ql) {
        lse_i = lse[v.so + iq];
        delta_i = delta[v.so + iq];
    }
    constexpr int MAXA = 8;          // dQ elements per thread: Dh * 16 <= 128 * 16 = 8 * 256
    float dq[MAXA];
#pragma unroll
    for (int u = 0; u < MAXA; ++u) dq[u] = 0.f;
    const int jbeg = v.key_begin(i0), jend = v.key_end(i0);   // workgroup-uniform
    for (int j0 = jbeg; j0 < jend; j0 += KB) {
        __syncthreads();
        for (int e = tid; e < Dh * KB; e += 256) {
            const int d = e / KB, j = e - d * KB, jc = min(j0 + j, v.kl - 1);
            Ks[e] = v.kg[size_t(d) * pk + jc];
            Vs[e] = v.vg[size_t(d) * pk + jc];
        }
        __syncthreads();
        {
            float s[4], dp[4], f[4];
            attn_bwd_pair_dots(Qs, Os, Ks, Vs, Dh, rq, jb, dr, uint32_t(j0 + jb) >> 2, uint32_t(iq), s, dp, f);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + jb + u;
                float ds = 0.f;
                if (iq < v.ql && v.visible(iq, j)) {     // a visible pair; every other one contributes exactly 0
                    const float pn = expf(v.logit(s[u], inv, iq, j, slope) - lse_i);
                    ds = pn * (dp[u] - delta_i) * inv;
                }
                Ss[rq * KB + jb + u] = ds;
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXA; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * QB) {
                const int d = e / QB, qi = e - d * QB;
                float a = dq[u];
                for (int j = 0; j < KB; ++j) a = fmaf(Ss[qi * KB + j], Ks[d * KB + j], a);
                dq[u] = a;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXA; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * QB) {
            const int d = e / QB, qi = e - d * QB;
            if (i0 + qi < v.q_end) dqg[size_t(d) * pdq + i0 + qi] = i0 + qi < v.ql ? dq[u] : 0.f;
        }
    }
}

// One workgroup per (key block, head, item): dK and dV of its 64 keys, queries in blocks of 16 over [query_begin, query_end).
// dkg / dvg: the dK and dV rows of this (item, head), pitch pdk.  Dynamic LDS: 2 Dh 64 + 2 Dh 16 + 2 * 16 * 64 floats.
template <class View, class Pitch, class Drop = NoDrop>
__device__ __forceinline__ void attn_bwd_dkv_body(const View &v, const float *slopes, int h, const float *lse,
                                                  const float *delta, float *dkg, float *dvg,
                                                  Pitch pdk, int Dh, float scale_div, const Drop &drop = Drop{}) {
    constexpr int QB = kAttnQB, KB = kAttnKB;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Ks = sm;                  // [Dh][KB]
    float *Vs = Ks + Dh * KB;        // [Dh][KB]
    float *Qs = Vs + Dh * KB;        // [Dh][QB]
    float *Os = Qs + Dh * QB;        // [Dh][QB]
    float *Ps = Os + Dh * QB;        // [QB][KB]  P, under dropout P~ = f o P
    float *Ss = Ps + QB * KB;        // [QB][KB]  dS / scale
    const int tid = threadIdx.x, j0 = blockIdx.x * KB;
    const auto pq = v.pq;   // the pitches as locals (see AttnView)
    const auto pk = v.pk;
    const auto pd = v.pd;
    const Drop dr = drop;   // ... and the policy's fields
    if constexpr (View::kEarlyExit) {
        if (j0 >= v.kl || v.ql == 0) {       // workgroup-uniform, before the first barrier: this block's dK / dV are 0
            if (j0 < v.k_end)
                for (int e = tid; e < Dh * KB; e += 256) {
                    const int d = e / KB, j = e - d * KB;
                    if (j0 + j < v.k_end) dkg[size_t(d) * pdk + j0 + j] = dvg[size_t(d) * pdk + j0 + j] = 0.f;
                }
            return;
        }
    }
    const float slope = slopes[h], inv = 1.f / scale_div;
    for (int e = tid; e < Dh * KB; e += 256) {
        const int d = e / KB, j = e - d * KB, jc = min(j0 + j, v.kl - 1);
        Ks[e] = v.kg[size_t(d) * pk + jc];
        Vs[e] = v.vg[size_t(d) * pk + jc];
    }
    const int rq = tid / 16, jb = 4 * (tid % 16);   // the pair pass: query i0 + rq, keys j0 + jb .. + 3
    constexpr int MAXE = 32;         // dK / dV elements per thread: Dh * 64 <= 128 * 64 = 32 * 256
    float dk[MAXE], dv[MAXE];
#pragma unroll
    for (int u = 0; u < MAXE; ++u) dk[u] = dv[u] = 0.f;
    const int ibeg = v.query_begin(j0), iend = v.query_end(j0);   // workgroup-uniform
    for (int i0 = ibeg; i0 < iend; i0 += QB) {
        __syncthreads();
        for (int e = tid; e < Dh * QB; e += 256) {
            const int d = e / QB, qi = e - d * QB, i = min(i0 + qi, v.ql - 1);
            Qs[e] = v.qg[size_t(d) * pq + i];
            Os[e] = (i0 + qi < v.ql) ? v.dg[size_t(d) * pd + i] : 0.f;   // a masked query's dO is never multiplied
        }
        __syncthreads();
        {
            const int iq = i0 + rq;
            float s[4], dp[4], f[4];
            attn_bwd_pair_dots(Qs, Os, Ks, Vs, Dh, rq, jb, dr, uint32_t(j0 + jb) >> 2, uint32_t(iq), s, dp, f);
            float lse_i = 0.f, delta_i = 0.f;
            if (iq < v.ql) {
                lse_i = lse[v.so + iq];
                delta_i = delta[v.so + iq];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + jb + u;
                float pm = 0.f, ds = 0.f;
                if (iq < v.ql && v.visible(iq, j)) {
                    const float pn = expf(v.logit(s[u], inv, iq, j, slope) - lse_i);
                    ds = pn * (dp[u] - delta_i) * inv;
                    pm = pn;
                    if constexpr (Drop::kDrop) pm = pn * f[u];
                }
                Ps[rq * KB + jb + u] = pm;
                Ss[rq * KB + jb + u] = ds;
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAXE; ++u) {
            const int e = tid + u * 256;
            if (e < Dh * KB) {
                const int d = e / KB, j = e - d * KB;
                float ak = dk[u], av = dv[u];
#pragma unroll
                for (int qi = 0; qi < QB; ++qi) {
                    ak = fmaf(Ss[qi * KB + j], Qs[d * QB + qi], ak);
                    av = fmaf(Ps[qi * KB + j], Os[d * QB + qi], av);
                }
                dk[u] = ak;
                dv[u] = av;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MAXE; ++u) {
        const int e = tid + u * 256;
        if (e < Dh * KB) {
            const int d = e / KB, j = e - d * KB;
            if (j0 + j < v.k_end) {
                const bool valid = j0 + j < v.kl;
                dkg[size_t(d) * pdk + j0 + j] = valid ? dk[u] : 0.f;
                dvg[size_t(d) * pdk + j0 + j] = valid ? dv[u] : 0.f;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
// One pick feeds launch and name query.  A family's forward kernels for DVT = 1, 2, 4 sit in a table of three rows.
template <class Kern>
struct MaskedRow { const char *name; Kern kern; DeviceOnce once; };
#define AGX_MASKED_ROWS(family)                                                                                    \
    {{"attention_" #family "<1>", attention_##family##_kernel<1>}, {"attention_" #family "<2>", attention_##family##_kernel<2>}, \
     {"attention_" #family "<4>", attention_##family##_kernel<4>}}   // [log2(DVT)]
// empty: an extent <= 0 -- the entry points return AGX_OK and launch nothing; code: a refusal (fail() was called); di: the row
struct MaskedPick { int di; dim3 grid; size_t lds; int lds_limit, code; bool empty; };

// the head_dim refusals, first in every family; 0 or the code of the refusal
static int masked_head_dim(const char *op, int Dh) {
    if (Dh <= 0) return fail(AGX_ERR_BAD_SHAPE, "%s: bad shape head_dim=%d", op, Dh);
    if (Dh > 128) return fail(AGX_ERR_UNSUPPORTED, "%s: head_dim=%d > 128", op, Dh);
    return 0;
}

// code: what masked_head_dim and the family's own checks ahead of the grid refusal said
static MaskedPick masked_pick(const char *op, bool empty, int code, int Dh, int gx, int gy, int gz) {
    MaskedPick k{};
    k.empty = empty;
    k.code = code;
    if (!k.code && (gy > 65535 || gz > 65535)) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: grid too large", op);
    if (k.code || k.empty) return k;
    const int dvt = Dh <= 32 ? 1 : (Dh <= 64 ? 2 : 4);                 // 32-row tiles of the head dim
    k.di = dvt / 2;                                                    // log2(dvt)
    k.lds = size_t(2) * 32 * dvt * 65 * sizeof(float);                 // the double-buffered V block
    k.lds_limit = k.lds > 48 * 1024 ? 96 * 1024 : 0;
    k.grid = dim3(gx, gy, gz);
    return k;
}

// the pick of the window family (attention_window.hip, attention_stream.hip): the window refusal comes after the grid's
static MaskedPick masked_window_pick(const char *op, int B, int H, int Dh, int Tq, int W) {
    MaskedPick k = masked_pick(op, B <= 0 || H <= 0 || Tq <= 0, masked_head_dim(op, Dh), Dh, ceil_div(Tq, 128), H, B);
    if (!k.code && W < 1) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: window=%d < 1", op, W);
    return k;
}

template <class Kern, class... A>
static int masked_launch(MaskedRow<Kern> &row, const MaskedPick &k, const char *what, hipStream_t st, A... a) {
    if (int rc = prepare_kernel(reinterpret_cast<const void *>(row.kern), row.once, k.lds_limit, nullptr, what)) return rc;
    hipLaunchKernelGGL(row.kern, k.grid, dim3(256), k.lds, st, a...);
    return check_launch(what);
}

// the answer of every agx_attention_*_kernel_name
static int masked_name(const MaskedPick &k, const char *query, const char *name, char *buf, size_t buf_len) {
    if (k.code) return k.code;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "%s: NULL buffer", query);
    snprintf(buf, buf_len, "%s", k.empty ? "none" : name);
    return AGX_OK;
}

// a stride (kind: "batch", or "row" for the packed layout) must hold what the kernels index through it
static int check_strides(const char *op, int64_t have, int64_t need, const char *what, const char *kind = "batch") {
    return have >= need ? AGX_OK
                        : fail(AGX_ERR_BAD_SHAPE, "%s: %s %s stride %lld < %lld", op, what, kind, (long long)have, (long long)need);
}

static int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t r = a % b;
        a = b;
        b = r;
    }
    return a;
}

// The backward's three launches: stats and dq on the query-block grid gq, dkv on the key-block grid gk.  args_* are tuples of
// each kernel's arguments; the dynamic LDS is the bodies' (head_dim 128: 90 KB, so the limit is raised for all three).
template <class KS, class KQ, class KK, class TS, class TQ, class TK>
static int masked_launch_backward(const char *what, DeviceOnce (&once)[3], KS stats, KQ dq, KK dkv, dim3 gq, dim3 gk, int Dh,
                                  hipStream_t st, const TS &args_stats, const TQ &args_dq, const TK &args_dkv) {
    const size_t tile = size_t(kAttnQB) * kAttnKB, rows = size_t(2) * Dh * (kAttnQB + kAttnKB);
    const void *ks[3] = {reinterpret_cast<const void *>(stats), reinterpret_cast<const void *>(dq), reinterpret_cast<const void *>(dkv)};
    for (int i = 0; i < 3; ++i)
        if (int rc = prepare_kernel(ks[i], once[i], 96 * 1024, nullptr, what)) return rc;
    std::apply([&](auto... a) { hipLaunchKernelGGL(stats, gq, dim3(256), (rows + 2 * tile) * sizeof(float), st, a...); }, args_stats);
    std::apply([&](auto... a) { hipLaunchKernelGGL(dq, gq, dim3(256), (rows + tile) * sizeof(float), st, a...); }, args_dq);
    std::apply([&](auto... a) { hipLaunchKernelGGL(dkv, gk, dim3(256), (rows + 2 * tile) * sizeof(float), st, a...); }, args_dkv);
    return check_launch(what);
}

}  // namespace agx
