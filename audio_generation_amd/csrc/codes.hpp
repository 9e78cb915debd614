// What the code path shares (rvq.hip, rvq_step.hip, prior.hip, entropy.hip): the per-stage size table and the host loop that fills
// it, the per-row clamp of a count, and the one order of a stage's codes with the workgroup minimum over it.
#pragma once

#include "common.hpp"

namespace agx {

// sizes of the stages of a launch, by value in the kernel arguments: n[q] = K where the caller gave no sizes
struct StageSizes { int n[64]; };

// The 64-stage limit, the fill and the range refusal of every entry point that takes `sizes` (null: every stage has k codes).
inline int stage_sizes(const char *what, const int32_t *sizes, int q_total, int k, StageSizes *sz) {
    if (q_total > 64) return fail(AGX_ERR_UNSUPPORTED, "%s: at most 64 stages (Q=%d)", what, q_total);
    for (int q = 0; q < 64; ++q) sz->n[q] = k;
    for (int q = 0; q < q_total && sizes; ++q) {
        if (sizes[q] < 1 || sizes[q] > k) return fail(AGX_ERR_BAD_SHAPE, "%s: stage %d has %d codes (K=%d)", what, q, sizes[q], k);
        sz->n[q] = sizes[q];
    }
    return AGX_OK;
}

// clamp(c, 0, hi): what a row takes of `hi` frames or stages when it asks for c (include/agx.h "Per-row frame counts", "Per-row
// stage counts")
__device__ __forceinline__ int count_clamp(int64_t c, int hi) { return c < 0 ? 0 : (c > hi ? hi : int(c)); }
// ... of row b of a per-row tensor; a null pointer is the plain entry point: every row takes all `hi`
__device__ __forceinline__ int row_clamp(const int64_t *v, int b, int hi) { return v ? count_clamp(v[b], hi) : hi; }

// THE order of the codes of a stage: include/agx.h "Code prior" step 2, "the codes are ordered by (l_c descending, c ascending);
// the comparisons are exact (-0 == +0)", and a NaN counts as -inf.  Ascending keys are that order.  The sampler sorts by it and the
// entropy tables take "the lowest argmax a of the binary32 logits" ("Entropy coding" step 3) as its least key: one function, so the
// code a greedy sampler draws is the code that takes the table's spare frequency.
__device__ __forceinline__ unsigned long long code_key(float l, int k) {
    if (l != l) l = -1.0f / 0.0f;
    if (l == 0.f) l = 0.f;
    unsigned u = __float_as_uint(l);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);      // ascending in l
    return ((unsigned long long)(~u) << 32) | unsigned(k);
}
__device__ __forceinline__ float code_key_logit(unsigned long long key) {
    unsigned u = ~unsigned(key >> 32);
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}

// The least key of a 256-thread workgroup, in every thread, in two steps around the caller's one store:
//     best = wave_min_key(best);  if (lane == 0) slots[wave] = best;  best = block_min_key(best, slots);
// (the store stays with the kernel: inside a helper the compiler guards it with one more scalar instruction)
__device__ __forceinline__ unsigned long long wave_min_key(unsigned long long best) {     // a butterfly: every lane has the result
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o < best ? o : best;
    }
    return best;
}
__device__ __forceinline__ unsigned long long block_min_key(unsigned long long best, const unsigned long long *slots /* LDS, 4 */) {
    __syncthreads();
    for (int w = 0; w < 4; ++w) best = slots[w] < best ? slots[w] : best;
    return best;
}

}  // namespace agx
