// RVQ streaming step: the quantiser of a streaming chunk -- 1 .. AGX_RVQ_STEP_MAX_N frames per row, per-row
// counts -- as the full DEFINING search (oracle/rvq_exact.c) spread over the chip, and the packets it speaks.
//
// Encode: one launch per stage plus one output launch.  rvq_step_search_kernel, grid (frames, ceil(K / 64)), one wave per
// workgroup: workgroup (f, j) searches codewords 64 j .. 64 j + 63 of the stage for frame f, ONE summation chain per lane
// (a (codeword, frame) pair walked in d order: binary64, one subtract, one multiply, one add per term, never fused), and writes its
// (distance, index) minimum -- the lowest index on equal distance -- as partial j of the frame.  The next launch combines the
// partials in its prologue, in index order (a fixed order: deterministic, no atomics), and forms r_q = fl32(r_{q-1} - c); the
// workgroups j = 0 also store the code and r_q for the launches behind them.  No workgroup ever waits for another: the only
// ordering is the launch boundary.  A workgroup whose frame lies behind its row's count leaves after reading the count.
// rvq_step_output_kernel, one workgroup per row, combines the last stage and writes index, zq and the row's packet.
//
// Decode: rvq_step_decode_kernel, one workgroup per frame: the frame's codes out of the row's packet, then the stage-order sum.
//
// Per-row stage counts: every kernel reads q_b = clamp(stages[b], 0, Q) through row_clamp, beside the frame count
// (NULL: Q, the plain entry points).  Stage q of row b is searched, stored, packed and summed only when q < q_b; the row's packet is
// dense over its own q_b.  rvq_packets_restage_kernel, one workgroup per row, re-packs a row to fewer stages: a bit gather.
#include "codes.hpp"

// the whole file is the defining arithmetic or plain sums: nothing here may be fused
#pragma clang fp contract(off)

namespace agx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int STEP_CW = 64;       // codewords per search workgroup: one per lane of its single wave
constexpr int STEP_NO_CODE = 0x7fffffff;

// workspace: [pd: 2 x F x NB double | res: 2 x F x D float | pi: 2 x F x NB int32 | codes: F x Q int32], each part 8-byte aligned
struct RvqStepWs {
    size_t pd, res, pi, codes, total;
};
__host__ __device__ inline size_t step_align8(size_t v) { return (v + 7) & ~size_t(7); }
__host__ __device__ inline RvqStepWs rvq_step_ws(int64_t F, int D, int K, int Q) {
    const size_t nb = size_t((K + STEP_CW - 1) / STEP_CW);
    RvqStepWs w;
    w.pd = 0;
    w.res = w.pd + 2 * size_t(F) * nb * sizeof(double);
    w.pi = w.res + step_align8(2 * size_t(F) * size_t(D) * sizeof(float));
    w.codes = w.pi + step_align8(2 * size_t(F) * nb * sizeof(int32_t));
    w.total = w.codes + step_align8(size_t(F) * size_t(Q) * sizeof(int32_t));
    return w;
}

// (distance, index) minimum over the wave, the lowest index on equal distance: a butterfly, every lane ends with the result
__device__ __forceinline__ void step_wave_min(double &best, int &arg) {
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oa = __shfl_xor(arg, off);
        if (ob < best || (ob == best && oa < arg)) best = ob, arg = oa;
    }
}

// The code of one (frame, stage) from its nb partials, by one whole wave: lane L takes partials L, L + 64, .. in ascending order
// (codeword blocks ascend with the partial's number, so the first of equal distances has the lowest index), then the butterfly.
// A frame whose distances are all NaN has no minimum; it gets code 0 (unspecified by the contract, but in bounds).
__device__ __forceinline__ int step_combine(const double *__restrict__ pd, const int32_t *__restrict__ pi, int nb, int kq, int lane) {
    double best = 1.0 / 0.0;
    int arg = STEP_NO_CODE;
    for (int j = lane; j < nb; j += 64) {
        const double d = pd[j];
        const int a = pi[j];
        if (d < best || (d == best && a < arg)) best = d, arg = a;
    }
    step_wave_min(best, arg);
    return arg >= 0 && arg < kq ? arg : 0;
}

// 16 terms of a chain: acc + sq_0 + .. + sq_15 in that order, the squares formed before the additions start (step_dist_lane)
__device__ __forceinline__ double step_chain16(double acc, const float *__restrict__ r16 /* LDS */, const f32x4 *cv) {
    f32x4 rv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) rv[j] = *reinterpret_cast<const f32x4 *>(r16 + 4 * j);
    double sq[16];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double diff = double(rv[j][e]) - double(cv[j][e]);
            sq[4 * j + e] = diff * diff;
        }
#pragma unroll
    for (int e = 0; e < 16; ++e) acc = acc + sq[e];
    return acc;
}

// this lane's chain: the defining distance of the frame's residual (LDS, the same row for all lanes) to one codeword
__device__ __forceinline__ double step_dist_lane(const float *__restrict__ r_row, const float *__restrict__ c, int D) {
    double acc = 0.0;
    int d = 0;
    if ((D & 3) == 0) {   // codeword rows are 16-byte aligned
        // A lone wave has nothing else to issue, so the loop is laid out for it.  Sub-blocks of 16 dims run in two phases: the 16
        // squares first -- independent convert / subtract / multiply strings -- then the 16 dependent additions of the chain; and
        // the codeword is read a block of 64 dims ahead, under the current block's chain.  Together 150 -> 111 us for eight stages
        // of D = 512 (not measured apart).  The order of the additions is untouched.
        if (D >= 64) {
            f32x4 cur[16], nxt[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) cur[j] = *reinterpret_cast<const f32x4 *>(c + 4 * j);
            for (; d + 64 <= D; d += 64) {
                const float *cn = c + (d + 128 <= D ? d + 64 : d);     // the last block loads itself again: no branch, in bounds
#pragma unroll
                for (int j = 0; j < 16; ++j) nxt[j] = *reinterpret_cast<const f32x4 *>(cn + 4 * j);
#pragma unroll
                for (int g = 0; g < 4; ++g) acc = step_chain16(acc, r_row + d + 16 * g, cur + 4 * g);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    asm volatile("" : "+v"(nxt[j]));     // opaque: keeps the look-ahead from being folded back into a load at its use
                    cur[j] = nxt[j];
                }
            }
        }
        for (; d + 16 <= D; d += 16) {
            f32x4 cv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) cv[j] = *reinterpret_cast<const f32x4 *>(c + d + 4 * j);
            acc = step_chain16(acc, r_row + d, cv);
        }
    }
    for (; d < D; ++d) {
        const double diff = double(r_row[d]) - double(c[d]);
        const double sq = diff * diff;
        acc = acc + sq;
    }
    return acc;
}

struct RvqStepArgs {
    const float *z;
    int64_t z_sb, z_st, z_sd;
    const float *cb;          // (Q_total, K, D)
    const int64_t *counts;    // (B,) or null
    const int64_t *stages;    // (B,) or null
    int n, D, K, Q;
    unsigned char *ws;
    RvqStepWs map;
    int64_t F;
    StageSizes sizes;
};

// stage q of the search: grid (F, ceil(K / 64)), 64 threads, D floats of dynamic LDS
__global__ __launch_bounds__(64) void rvq_step_search_kernel(RvqStepArgs a, int q) {
    extern __shared__ __align__(16) float step_r[];
    const int lane = threadIdx.x;
    const int64_t f = blockIdx.x;
    const int j = blockIdx.y;
    const int b = int(f / a.n), t = int(f % a.n);
    if (t >= row_clamp(a.counts, b, a.n)) return;       // a dead frame: nothing of it is loaded
    if (q >= row_clamp(a.stages, b, a.Q)) return;       // a stage the row does not send: likewise, and the row's last partials stay
    const int kq = a.sizes.n[q];
    if (j * STEP_CW >= kq) return;                      // a short stage: no codeword here, and no partial is read for this block
    const int nb_max = (a.K + STEP_CW - 1) / STEP_CW;
    double *pd = reinterpret_cast<double *>(a.ws + a.map.pd);
    int32_t *pi = reinterpret_cast<int32_t *>(a.ws + a.map.pi);
    float *res = reinterpret_cast<float *>(a.ws + a.map.res);
    int32_t *codes = reinterpret_cast<int32_t *>(a.ws + a.map.codes);
    const size_t slot = size_t(q & 1) * size_t(a.F) + size_t(f), prev_slot = size_t((q & 1) ^ 1) * size_t(a.F) + size_t(f);

    // prologue: r_q of this frame into LDS
    const float *zf = a.z + b * a.z_sb + t * a.z_st;
    if (q == 0) {
        for (int d = lane; d < a.D; d += 64) step_r[d] = zf[d * a.z_sd];
    } else {
        const int kp = a.sizes.n[q - 1];
        const int code = step_combine(pd + prev_slot * nb_max, pi + prev_slot * nb_max, (kp + STEP_CW - 1) / STEP_CW, kp, lane);
        const float *c = a.cb + (size_t(q - 1) * a.K + size_t(code)) * a.D;
        const float *prev = q == 1 ? zf : res + prev_slot * a.D;
        const int64_t prev_sd = q == 1 ? a.z_sd : 1;
        float *mine = res + slot * a.D;
        for (int d = lane; d < a.D; d += 64) {
            const float r = prev[d * prev_sd] - c[d];
            step_r[d] = r;
            if (j == 0) mine[d] = r;
        }
        if (j == 0 && lane == 0) codes[size_t(f) * a.Q + (q - 1)] = code;
    }
    __syncthreads();

    const int k = j * STEP_CW + lane;
    const int row = k < kq ? k : kq - 1;
    double best = step_dist_lane(step_r, a.cb + (size_t(q) * a.K + size_t(row)) * a.D, a.D);
    int arg = k;
    if (k >= kq || !(best == best)) best = 1.0 / 0.0, arg = STEP_NO_CODE;   // no codeword, or NaN: never the minimum
    step_wave_min(best, arg);
    if (lane == 0) {
        pd[slot * nb_max + j] = best;
        pi[slot * nb_max + j] = arg;
    }
}

struct RvqStepOutArgs {
    const float *cb;
    const int64_t *counts;
    const int64_t *stages;
    int n, D, K, Q, bits;
    float *zq;
    int64_t q_sb, q_st, q_sd;
    int64_t *index;            // (B, n, Q)
    unsigned char *packets;    // (B, P) or null
    int P;
    const unsigned char *ws;
    RvqStepWs map;
    int64_t F;
    StageSizes sizes;
};

// byte i of a row's packet: the dense little-endian packing of `n_codes` codes of `bits` bits; code_at(e) is code e of the row,
// no wider than `bits`, and is asked only for the codes whose bits the byte holds
template <class CodeAt>
__device__ __forceinline__ unsigned step_packet_byte(CodeAt code_at, int n_codes, int bits, int i) {
    const int lo = 8 * i;
    unsigned v = 0;
    for (int e = lo / bits; e < n_codes && e * bits < lo + 8; ++e) {
        const unsigned code = code_at(e);
        const int shift = e * bits - lo;
        v |= shift >= 0 ? code << shift : code >> -shift;
    }
    return v & 0xffu;
}

// one workgroup per row: grid (B), 256 threads, n Q ints of dynamic LDS.  The row's codes lie in LDS dense over its own q_b
// stages, as its packet holds them; its last live stage q_b - 1 is combined here, from the slot that stage's launch wrote.
__global__ __launch_bounds__(256) void rvq_step_output_kernel(RvqStepOutArgs a) {
    extern __shared__ __align__(16) int step_codes[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cnt = row_clamp(a.counts, b, a.n);
    const int qb = row_clamp(a.stages, b, a.Q);
    if (qb > 0) {
        const int nb_max = (a.K + STEP_CW - 1) / STEP_CW;
        const double *pd = reinterpret_cast<const double *>(a.ws + a.map.pd);
        const int32_t *pi = reinterpret_cast<const int32_t *>(a.ws + a.map.pi);
        const int32_t *codes = reinterpret_cast<const int32_t *>(a.ws + a.map.codes);
        const int kl = a.sizes.n[qb - 1];
        for (int t = wave; t < cnt; t += 4) {              // live frames only: nothing of a dead frame's workspace is read
            const int64_t f = int64_t(b) * a.n + t;
            const size_t slot = size_t((qb - 1) & 1) * size_t(a.F) + size_t(f);
            const int last = step_combine(pd + slot * nb_max, pi + slot * nb_max, (kl + STEP_CW - 1) / STEP_CW, kl, lane);
            for (int q = lane; q < qb; q += 64) {
                const int code = q == qb - 1 ? last : codes[size_t(f) * a.Q + q];
                step_codes[t * qb + q] = code >= 0 && code < a.sizes.n[q] ? code : 0;   // (in bounds whatever the workspace held)
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < a.n * a.Q; e += 256) {
        const int t = e / a.Q, q = e % a.Q;
        a.index[size_t(b) * a.n * a.Q + e] = t < cnt && q < qb ? int64_t(step_codes[t * qb + q]) : int64_t(-1);
    }
    if (a.zq) {
        for (int e = tid; e < a.n * a.D; e += 256) {
            const int t = e / a.D, d = e % a.D;
            float acc = 0.f;
            if (t < cnt)
                for (int q = 0; q < qb; ++q) acc = acc + a.cb[(size_t(q) * a.K + size_t(step_codes[t * qb + q])) * a.D + d];
            a.zq[b * a.q_sb + t * a.q_st + d * a.q_sd] = acc;
        }
    }
    if (a.packets) {
        const int live_bytes = (cnt * qb * a.bits + 7) / 8;
        const unsigned mask = (1u << a.bits) - 1u;
        auto code_at = [&](int e) { return unsigned(step_codes[e]) & mask; };
        for (int i = tid; i < a.P; i += 256)
            a.packets[size_t(b) * a.P + i] = i < live_bytes ? (unsigned char)step_packet_byte(code_at, cnt * qb, a.bits, i) : (unsigned char)0;
    }
}

// the `bits`-bit code that starts at bit `bit0` of a packet row; reads the bytes that hold it and no other
__device__ __forceinline__ unsigned step_read_code(const unsigned char *__restrict__ row, int bit0, int bits) {
    unsigned v = 0;
    for (int o = bit0 >> 3, s = 0; o <= (bit0 + bits - 1) >> 3; ++o, s += 8) v |= unsigned(row[o]) << s;
    return (v >> (bit0 & 7)) & ((1u << bits) - 1u);
}

struct RvqStepDecArgs {
    const unsigned char *packets;   // (B, P)
    int P, bits;
    const float *cb;
    const int64_t *counts;
    const int64_t *stages;
    int n, D, K, Q;
    float *zq;
    int64_t q_sb, q_st, q_sd;
    int64_t *index;                 // (B, n, Q) or null
    StageSizes sizes;
};

// one workgroup per frame: grid (B n), 256 threads
__global__ __launch_bounds__(256) void rvq_step_decode_kernel(RvqStepDecArgs a) {
    __shared__ int codes[64];
    const int64_t f = blockIdx.x;
    const int b = int(f / a.n), t = int(f % a.n), tid = threadIdx.x;
    const int cnt = row_clamp(a.counts, b, a.n);
    const int qb = row_clamp(a.stages, b, a.Q);
    const bool live = t < cnt;
    if (tid < a.Q) {
        int code = -1;
        if (live && tid < qb)                              // bits of a live code lie inside the row's first ceil(c_b q_b bits / 8) bytes
            code = int(step_read_code(a.packets + size_t(b) * a.P, (t * qb + tid) * a.bits, a.bits));
        codes[tid] = code;
        if (a.index) a.index[size_t(f) * a.Q + tid] = int64_t(code);
    }
    __syncthreads();
    for (int d = tid; d < a.D; d += 256) {
        float acc = 0.f;
        if (live)
            for (int q = 0; q < qb; ++q) {
                const int code = codes[q];
                if (code < a.sizes.n[q]) acc = acc + a.cb[(size_t(q) * a.K + size_t(code)) * a.D + d];   // a code past the stage adds and reads nothing
            }
        a.zq[b * a.q_sb + t * a.q_st + d * a.q_sd] = acc;
    }
}

struct RvqRestageArgs {
    const unsigned char *in;        // (B, P)
    const int64_t *stages_in;       // (B,) or null: Q
    const int64_t *stages_to;       // (B,)
    const int64_t *counts;          // (B,) or null
    int n, Q, bits, P;
    unsigned char *out;             // (B, P), no byte shared with `in`
    int64_t *stages_out;            // (B,) or null
};

// one workgroup per row: grid (B), 256 threads.  Output byte i collects the codes whose bits it holds -- code e of the output is
// stage e % q_out of frame e / q_out, which the input holds at bit ((e / q_out) q_in + e % q_out) bits.  q_out <= q_in and the frame
// lies below the count, so every bit read lies inside the row's first ceil(c_b q_in bits / 8) input bytes.
__global__ __launch_bounds__(256) void rvq_packets_restage_kernel(RvqRestageArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cnt = row_clamp(a.counts, b, a.n);
    const int q_in = row_clamp(a.stages_in, b, a.Q);
    const int q_to = row_clamp(a.stages_to, b, a.Q);
    const int q_out = q_to < q_in ? q_to : q_in;
    if (tid == 0 && a.stages_out) a.stages_out[b] = int64_t(q_out);
    const unsigned char *row = a.in + size_t(b) * a.P;
    const int n_codes = cnt * q_out;
    const int live_bytes = (n_codes * a.bits + 7) / 8;
    auto code_at = [&](int e) { return step_read_code(row, ((e / q_out) * q_in + e % q_out) * a.bits, a.bits); };
    for (int i = tid; i < a.P; i += 256)
        a.out[size_t(b) * a.P + i] = (unsigned char)(i < live_bytes ? step_packet_byte(code_at, n_codes, a.bits, i) : 0u);
}

// the shape checks both entry points share; `what` names the entry point.  Fills sz.
static int rvq_step_shape(const char *what, const int32_t *sizes, int32_t batch, int32_t n, int32_t dim, int32_t k, int32_t q_total,
                          int32_t q_used, int32_t bits, StageSizes *sz) {
    if (batch <= 0 || n <= 0 || dim <= 0 || k <= 0 || q_total <= 0 || q_used < 0 || q_used > q_total)
        return fail(AGX_ERR_BAD_SHAPE, "%s: bad shape B=%d n=%d D=%d K=%d Q=%d q_used=%d", what, batch, n, dim, k, q_total, q_used);
    if (bits < 1 || bits > 16) return fail(AGX_ERR_BAD_SHAPE, "%s: bits=%d outside 1 .. 16", what, bits);
    if (n > AGX_RVQ_STEP_MAX_N)
        return fail(AGX_ERR_UNSUPPORTED, "%s: a step takes at most %d frames per row, got n=%d (agx_rvq_forward is the kernel for long chunks)",
                    what, AGX_RVQ_STEP_MAX_N, n);
    if (q_total > 64) return fail(AGX_ERR_UNSUPPORTED, "%s: at most 64 stages (Q=%d)", what, q_total);   // ahead of the limits below, as ever
    if (dim > 8192 || k > 65536) return fail(AGX_ERR_UNSUPPORTED, "%s: D=%d (at most 8192) or K=%d (at most 65536) is too large", what, dim, k);
    if (int64_t(batch) * n > 0x7fffffff) return fail(AGX_ERR_UNSUPPORTED, "%s: B n = %lld frames exceed 2^31 - 1", what, (long long)batch * n);
    return stage_sizes(what, sizes, q_total, k, sz);
}

// the encode entry points: `stages` null is every stage for every row
static int rvq_step_encode_any(const char *what, const float *z, int64_t z_sb, int64_t z_st, int64_t z_sd, const float *codebooks,
                               const int32_t *sizes, const int64_t *counts, const int64_t *stages, int32_t batch, int32_t n, int32_t dim,
                               int32_t k, int32_t q_total, int32_t q_used, int32_t bits, float *zq, int64_t q_sb, int64_t q_st,
                               int64_t q_sd, int64_t *index, uint8_t *packets, void *workspace, size_t workspace_bytes, void *stream) {
    StageSizes sz;
    if (int rc = rvq_step_shape(what, sizes, batch, n, dim, k, q_total, q_used, bits, &sz)) return rc;
    for (int q = 0; q < q_used && packets; ++q)
        if (sz.n[q] > (1 << bits))
            return fail(AGX_ERR_UNSUPPORTED, "%s: stage %d has %d codewords, a packet of %d-bit codes cannot hold them", what, q, sz.n[q], bits);
    if (!z || !codebooks || (q_used > 0 && !index)) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", what);
    const size_t need = agx_rvq_step_workspace_bytes(batch, n, dim, k, q_used);
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(AGX_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace_bytes, need);
    if (need > 0 && (reinterpret_cast<uintptr_t>(workspace) & 7)) return fail(AGX_ERR_BAD_SHAPE, "%s: the workspace is not 8-byte aligned", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t F = int64_t(batch) * n;
    const RvqStepWs map = rvq_step_ws(F, dim, k, q_used > 0 ? q_used : 1);
    if (q_used > 0) {
        RvqStepArgs a{z, z_sb, z_st, z_sd, codebooks, counts, stages, n, dim, k, q_used, static_cast<unsigned char *>(workspace), map, F, sz};
        const dim3 grid((unsigned)F, (unsigned)ceil_div(k, STEP_CW));
        for (int q = 0; q < q_used; ++q)
            hipLaunchKernelGGL(rvq_step_search_kernel, grid, dim3(64), size_t(dim) * sizeof(float), st, a, q);
    }
    if (zq || packets || q_used > 0) {
        const int P = int((int64_t(n) * q_used * bits + 7) / 8);
        RvqStepOutArgs o{codebooks, counts, stages, n, dim, k, q_used, bits, zq, q_sb, q_st, q_sd, index, packets, P,
                         static_cast<const unsigned char *>(workspace), map, F, sz};
        hipLaunchKernelGGL(rvq_step_output_kernel, dim3((unsigned)batch), dim3(256), size_t(n) * (q_used > 0 ? q_used : 1) * sizeof(int), st, o);
    }
    return check_launch(what);
}

static int rvq_step_decode_any(const char *what, const uint8_t *packets, int32_t bits, const float *codebooks, const int32_t *sizes,
                               const int64_t *counts, const int64_t *stages, int32_t batch, int32_t n, int32_t dim, int32_t k,
                               int32_t q_total, int32_t q_used, float *zq, int64_t q_sb, int64_t q_st, int64_t q_sd, int64_t *index,
                               void *stream) {
    StageSizes sz;
    if (int rc = rvq_step_shape(what, sizes, batch, n, dim, k, q_total, q_used, bits, &sz)) return rc;
    if (!codebooks || !zq || (q_used > 0 && !packets)) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", what);
    const int P = int((int64_t(n) * q_used * bits + 7) / 8);
    RvqStepDecArgs a{packets, P, bits, codebooks, counts, stages, n, dim, k, q_used, zq, q_sb, q_st, q_sd, index, sz};
    hipLaunchKernelGGL(rvq_step_decode_kernel, dim3((unsigned)(int64_t(batch) * n)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return check_launch(what);
}

}  // namespace agx

extern "C" {

int64_t agx_rvq_step_packet_bytes(int32_t n, int32_t q_used, int32_t bits) {
    if (n < 1 || n > AGX_RVQ_STEP_MAX_N || q_used < 0 || q_used > 64 || bits < 1 || bits > 16) return AGX_ERR_BAD_SHAPE;
    return (int64_t(n) * q_used * bits + 7) / 8;
}

size_t agx_rvq_step_workspace_bytes(int32_t batch, int32_t n, int32_t dim, int32_t k, int32_t q_used) {
    if (batch <= 0 || n <= 0 || dim <= 0 || k <= 0 || q_used <= 0) return 0;
    return agx::rvq_step_ws(int64_t(batch) * n, dim, k, q_used).total;
}

int agx_rvq_step_encode(const float *z, int64_t z_sb, int64_t z_st, int64_t z_sd, const float *codebooks, const int32_t *sizes,
                        const int64_t *counts, int32_t batch, int32_t n, int32_t dim, int32_t k, int32_t q_total, int32_t q_used,
                        int32_t bits, float *zq, int64_t q_sb, int64_t q_st, int64_t q_sd, int64_t *index, uint8_t *packets,
                        void *workspace, size_t workspace_bytes, void *stream) {
    return agx::rvq_step_encode_any("rvq_step_encode", z, z_sb, z_st, z_sd, codebooks, sizes, counts, nullptr, batch, n, dim, k, q_total,
                                    q_used, bits, zq, q_sb, q_st, q_sd, index, packets, workspace, workspace_bytes, stream);
}

int agx_rvq_step_encode_staged(const float *z, int64_t z_sb, int64_t z_st, int64_t z_sd, const float *codebooks, const int32_t *sizes,
                               const int64_t *counts, const int64_t *stages, int32_t batch, int32_t n, int32_t dim, int32_t k,
                               int32_t q_total, int32_t q_used, int32_t bits, float *zq, int64_t q_sb, int64_t q_st, int64_t q_sd,
                               int64_t *index, uint8_t *packets, void *workspace, size_t workspace_bytes, void *stream) {
    return agx::rvq_step_encode_any("rvq_step_encode_staged", z, z_sb, z_st, z_sd, codebooks, sizes, counts, stages, batch, n, dim, k,
                                    q_total, q_used, bits, zq, q_sb, q_st, q_sd, index, packets, workspace, workspace_bytes, stream);
}

int agx_rvq_step_decode(const uint8_t *packets, int32_t bits, const float *codebooks, const int32_t *sizes, const int64_t *counts,
                        int32_t batch, int32_t n, int32_t dim, int32_t k, int32_t q_total, int32_t q_used, float *zq, int64_t q_sb,
                        int64_t q_st, int64_t q_sd, int64_t *index, void *stream) {
    return agx::rvq_step_decode_any("rvq_step_decode", packets, bits, codebooks, sizes, counts, nullptr, batch, n, dim, k, q_total, q_used,
                                    zq, q_sb, q_st, q_sd, index, stream);
}

int agx_rvq_step_decode_staged(const uint8_t *packets, int32_t bits, const float *codebooks, const int32_t *sizes, const int64_t *counts,
                               const int64_t *stages, int32_t batch, int32_t n, int32_t dim, int32_t k, int32_t q_total, int32_t q_used,
                               float *zq, int64_t q_sb, int64_t q_st, int64_t q_sd, int64_t *index, void *stream) {
    return agx::rvq_step_decode_any("rvq_step_decode_staged", packets, bits, codebooks, sizes, counts, stages, batch, n, dim, k, q_total,
                                    q_used, zq, q_sb, q_st, q_sd, index, stream);
}

int agx_rvq_packets_restage(const uint8_t *in, const int64_t *stages_in, const int64_t *stages_to, const int64_t *counts, int32_t batch,
                            int32_t n, int32_t q_used, int32_t bits, uint8_t *out, int64_t *stages_out, void *stream) {
    using namespace agx;
    if (batch <= 0 || n <= 0 || n > AGX_RVQ_STEP_MAX_N || q_used < 0 || q_used > 64 || bits < 1 || bits > 16)
        return fail(AGX_ERR_BAD_SHAPE, "rvq_packets_restage: bad shape B=%d n=%d q_used=%d bits=%d (n at most %d, q_used at most 64, bits 1 .. 16)",
                    batch, n, q_used, bits, AGX_RVQ_STEP_MAX_N);
    const int P = int((int64_t(n) * q_used * bits + 7) / 8);
    if (!stages_to || (P > 0 && (!in || !out))) return fail(AGX_ERR_NULL_POINTER, "rvq_packets_restage: NULL pointer");
    const size_t total = size_t(batch) * size_t(P);
    if (P > 0 && in < out + total && out < in + total)
        return fail(AGX_ERR_BAD_SHAPE, "rvq_packets_restage: in and out overlap (a byte is gathered from bits other bytes' threads write)");
    RvqRestageArgs a{in, stages_in, stages_to, counts, n, q_used, bits, P, out, stages_out};
    hipLaunchKernelGGL(rvq_packets_restage_kernel, dim3((unsigned)batch), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("rvq_packets_restage");
}

}  // extern "C"
