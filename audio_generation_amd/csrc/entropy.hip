// Entropy coding: the code prior's logits as the probability model of a byte-wise rANS coder for the stream packets.
//
//   logits -> tables.  cum_kernel: one workgroup per (b, i, q), a sibling of sample_kernel.  The contract (include/agx.h "Entropy
//                      coding") turns the logits of a stage into integer frequencies that sum to M = 2^16 exactly, every code of
//                      the stage at least 1: the maximum and the sum of exp(l - l_max) are workgroup reductions in binary64, the
//                      floor of every share is taken per code, the lowest argmax takes the rest, and the exclusive scan of the
//                      frequencies runs in LDS.  Every decision is a binary64 value; the integers that follow are exact.
//   tables -> bytes.   rans_encode_kernel: one wave per row.  The lanes gather the (start, f) pair of every live code of the hop
//                      into LDS; one lane runs the byte-wise rANS chain over them, last symbol first, and pushes its bytes into
//                      LDS; the wave writes the reversed bytes and the zero tail of the row.
//   bytes -> codes.    rans_decode_kernel: one wave per row, frame by frame.  The state x is the same in every lane; the search of
//                      the k + 1 sorted entries of a table is two rounds of compare + ballot (64 samples, then the entries between
//                      two of them); lane 0 writes.  The state and the read cursor live in device memory between calls.
#include "codes.hpp"

// defining arithmetic: nothing here may be fused
#pragma clang fp contract(off)

namespace agx {

constexpr int RANS_M = 1 << AGX_RANS_SCALE_BITS;
constexpr uint32_t RANS_L = AGX_RANS_L;
constexpr int CUM_MAX_K = AGX_CODES_CUM_MAX_K;
constexpr int CUM_PER = CUM_MAX_K / 256;           // codes per thread of the scan
constexpr uint32_t RANS_SKIP = 0xffffffffu;        // a gathered pair that is not coded: start 65535 with f 65536 cannot be a pair

// ------------------------------------------------------------------------------------------------------------------ tables
struct CumArgs {
    const float *logits;              // (B, Q K, n)
    const int64_t *counts, *stages;   // or null
    int32_t *cum;                     // (B, n_cum, Q, K + 1)
    int n, Q, K, n_cum, i_cum;
    StageSizes sizes;
};

// grid (B n Q), 256 threads
__global__ __launch_bounds__(256) void cum_kernel(CumArgs a) {
    __shared__ __attribute__((aligned(16))) int freq[CUM_MAX_K];
    __shared__ int table[CUM_MAX_K + 1];
    __shared__ unsigned long long wbest[4];
    __shared__ double wsum[4];
    __shared__ int wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x % a.Q;
    const int64_t f_in = blockIdx.x / a.Q;
    const int b = int(f_in / a.n), i = int(f_in % a.n);
    const int cnt = row_clamp(a.counts, b, a.n), qb = row_clamp(a.stages, b, a.Q);
    int32_t *out = a.cum + ((size_t(b) * a.n_cum + size_t(a.i_cum + i)) * a.Q + q) * size_t(a.K + 1);
    if (!(i < cnt && q < qb)) {                              // a dead entry: exact 0, its logits are not read
        for (int c = tid; c <= a.K; c += 256) out[c] = 0;
        return;
    }
    const int size = a.sizes.n[q];
    const float *col = a.logits + (size_t(b) * a.Q * a.K + size_t(q) * a.K) * a.n + i;
    // lanes along k at stride n: thread t holds the codes t + 256 u
    float l[CUM_PER];
    unsigned long long best = ~0ull;
#pragma unroll
    for (int u = 0; u < CUM_PER; ++u) {
        const int c = tid + 256 * u;
        l[u] = c < size ? col[size_t(c) * a.n] : 0.f;
        if (c < size) {
            const unsigned long long key = code_key(l[u], c);
            best = key < best ? key : best;
        }
    }
    best = wave_min_key(best);
    if (lane == 0) wbest[wave] = best;
    best = block_min_key(best, wbest);
    const int arg = int(unsigned(best));                     // the lowest argmax of the binary32 logits
    const double lmax = double(col[size_t(arg) * a.n]);
    double e[CUM_PER], part = 0.0;
#pragma unroll
    for (int u = 0; u < CUM_PER; ++u) {
        e[u] = tid + 256 * u < size ? exp(double(l[u]) - lmax) : 0.0;
        part = part + e[u];
    }
    for (int off = 32; off > 0; off >>= 1) part = part + __shfl_xor(part, off);
    if (lane == 0) wsum[wave] = part;
    __syncthreads();
    const double S = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    const double room = double(RANS_M - size);
    int mine = 0;
#pragma unroll
    for (int u = 0; u < CUM_PER; ++u) {
        const int c = tid + 256 * u;
        int f = 0;
        if (c < size) {
            double r = room * e[u] / S;
            if (!(r >= 0.0)) r = 0.0;                        // NaN or infinite logits: unspecified shares, but a table all the same
            if (r > room) r = room;
            f = 1 + int(floor(r));
        }
        freq[c] = f;
        mine += f;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane == 0) wtot[wave] = mine;
    __syncthreads();
    if (tid == 0) {                                          // the argmax takes the rest: the frequencies sum to M exactly
        freq[arg] += RANS_M - (wtot[0] + wtot[1] + wtot[2] + wtot[3]);   // with its sign: f_arg >= M / size >= 32 keeps it positive
    }
    __syncthreads();
    // exclusive scan: CUM_PER consecutive frequencies per thread, the threads' totals over the wave, the waves' over LDS
    const int4 lo = *reinterpret_cast<const int4 *>(&freq[tid * CUM_PER]), hi = *reinterpret_cast<const int4 *>(&freq[tid * CUM_PER + 4]);
    const int v[CUM_PER] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    int run = 0;
#pragma unroll
    for (int u = 0; u < CUM_PER; ++u) run += v[u];
    int incl = run;
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wtot[wave] = incl;                       // its last reader passed the barrier above
    __syncthreads();
    int base = incl - run;
    for (int w = 0; w < wave; ++w) base += wtot[w];
#pragma unroll
    for (int u = 0; u < CUM_PER; ++u) {
        base += v[u];
        table[tid * CUM_PER + u + 1] = base;                 // cum[c + 1]: M from c = size - 1 on, the frequencies behind it are 0
    }
    if (tid == 0) table[0] = 0;
    __syncthreads();
    for (int c = tid; c <= a.K; c += 256) out[c] = table[c];
}

// ------------------------------------------------------------------------------------------------------------------ encode
struct EncodeArgs {
    const int32_t *cum;               // (B, n, Q, K + 1)
    const int64_t *codes;             // (B, n, Q)
    const int64_t *counts, *stages;   // or null
    uint8_t *packets;                 // (B, P), P = 2 n Q + 4
    int64_t *nbytes, *status;         // (B,)
    int n, Q, K;
    StageSizes sizes;
};

// grid (B), 64 threads; dynamic LDS: the packet's length (16 bytes), n Q gathered pairs (uint32), then 2 n Q + 4 bytes
__global__ __launch_bounds__(64) void rans_encode_kernel(EncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t enc_lds[];
    const int lane = threadIdx.x, b = blockIdx.x;
    const int N = a.n * a.Q, P = 2 * N + 4;
    uint32_t *sym = enc_lds + 4;
    uint8_t *buf = reinterpret_cast<uint8_t *>(sym + N);
    const int cnt = row_clamp(a.counts, b, a.n), qb = row_clamp(a.stages, b, a.Q);
    bool bad = false;
    for (int e = lane; e < N; e += 64) {
        const int i = e / a.Q, q = e % a.Q;
        uint32_t pair = RANS_SKIP;
        if (i < cnt && q < qb) {
            const int64_t code = a.codes[size_t(b) * N + e];
            bool coded = false;
            if (code >= 0 && code < a.sizes.n[q]) {
                const int32_t *t = a.cum + (size_t(b) * N + e) * size_t(a.K + 1) + code;
                const int start = t[0], f = t[1] - t[0];
                if (start >= 0 && f >= 1 && start + f <= RANS_M) {       // anything else is not a table of agx_codes_cum
                    pair = uint32_t(start) | (uint32_t(f - 1) << 16);
                    coded = true;
                }
            }
            bad |= !coded;                                   // sticky: a lane takes the entries e, e + 64, ..
        }
        sym[e] = pair;
    }
    const bool any_bad = __ballot(bad) != 0ull;
    __syncthreads();
    if (lane == 0) {
        uint32_t x = RANS_L;
        int len = 0, coded = 0;
        for (int e = N - 1; e >= 0; --e) {
            const uint32_t pair = sym[e];
            if (pair == RANS_SKIP) continue;
            const uint32_t start = pair & 0xffffu, f = (pair >> 16) + 1u;
            const unsigned long long x_max = (unsigned long long)((RANS_L >> AGX_RANS_SCALE_BITS) << 8) * f;
            for (int push = 0; push < 2 && x >= x_max; ++push) {         // x < 2^31 and x_max >= 2^15: two bytes at the most
                buf[len++] = uint8_t(x & 255u);
                x >>= 8;
            }
            x = ((x / f) << AGX_RANS_SCALE_BITS) + (x % f) + start;
            ++coded;
        }
        if (coded) {
            for (int j = 0; j < 4; ++j) buf[len++] = uint8_t((x >> (8 * j)) & 255u);
        }
        enc_lds[0] = uint32_t(len);
        a.nbytes[b] = len;
        a.status[b] = any_bad ? 1 : 0;
    }
    __syncthreads();
    // the packet is the pushed bytes reversed, zeros behind it: single bytes up to the first 4-byte boundary, then words
    const int len = int(enc_lds[0]);
    uint8_t *row = a.packets + size_t(b) * P;
    int lead = int((4 - (reinterpret_cast<uintptr_t>(row) & 3)) & 3);
    lead = lead < P ? lead : P;
    const int words = (P - lead) / 4, tail0 = lead + 4 * words;
    auto byte_at = [&](int t) -> uint32_t { return t < len ? uint32_t(buf[len - 1 - t]) : 0u; };
    for (int t = lane; t < lead; t += 64) row[t] = uint8_t(byte_at(t));
    for (int w = lane; w < words; w += 64) {
        const int t = lead + 4 * w;
        *reinterpret_cast<uint32_t *>(row + t) = byte_at(t) | (byte_at(t + 1) << 8) | (byte_at(t + 2) << 16) | (byte_at(t + 3) << 24);
    }
    for (int t = tail0 + lane; t < P; t += 64) row[t] = uint8_t(byte_at(t));
}

// ------------------------------------------------------------------------------------------------------------------ decode
struct DecodeArgs {
    const int32_t *cum;               // (B, hop, Q, K + 1)
    const uint8_t *packets;           // (B, P)
    const int64_t *nbytes;            // (B,)
    const int64_t *counts, *stages;   // or null
    int64_t *state;                   // (B, 2): x, cursor
    int64_t *codes;                   // (B, n, Q)
    int64_t *carry;                   // (B, Q) or null
    int64_t *status;                  // (B,)
    int hop, i0, n, Q, K, P;
    StageSizes sizes;
};

// grid (B), 64 threads.  x, the cursor and the status are the same in every lane; lane 0 writes.
__global__ __launch_bounds__(64) void rans_decode_kernel(DecodeArgs a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int cnt = row_clamp(a.counts, b, a.hop), qb = row_clamp(a.stages, b, a.Q);
    int64_t *codes = a.codes + size_t(b) * a.n * a.Q;
    for (int e = lane; e < a.n * a.Q; e += 64)
        if (!(a.i0 + e / a.Q < cnt && e % a.Q < qb)) codes[e] = -1;
    if (cnt == 0 || qb == 0) {                               // nothing was coded for this row: only its -1s (and a clean status)
        if (lane == 0 && a.i0 == 0) a.status[b] = 0;
        if (a.carry && a.i0 < cnt)                           // frames without a stage: the sampler's carry of such a frame
            for (int q = lane; q < a.Q; q += 64) a.carry[size_t(b) * a.Q + q] = -1;
        return;
    }
    const uint8_t *row = a.packets + size_t(b) * a.P;
    const int64_t nb64 = a.nbytes[b];
    const int nb = nb64 < 0 ? 0 : (nb64 > a.P ? a.P : int(nb64));        // no read at or behind it, nor behind the row
    uint32_t x, st;
    int cur;
    auto next_byte = [&]() -> uint32_t {
        uint32_t v = 0u;
        if (cur < nb) v = row[cur];
        else st |= 2u;
        if (cur < 0x7fffffff) ++cur;
        return v;
    };
    if (a.i0 == 0) {
        st = 0u, cur = 0, x = 0u;
        for (int j = 0; j < 4; ++j) x = (x << 8) | next_byte();
    } else {
        const int64_t c64 = a.state[size_t(b) * 2 + 1];
        x = uint32_t(uint64_t(a.state[size_t(b) * 2]));
        cur = c64 < 0 ? 0 : (c64 > 0x7fffffff ? 0x7fffffff : int(c64));
        st = uint32_t(uint64_t(a.status[b]));
    }
    const int i_end = a.i0 + a.n < cnt ? a.i0 + a.n : cnt;
    for (int i = a.i0; i < i_end; ++i) {
        for (int q = 0; q < qb; ++q) {
            const int size = a.sizes.n[q];
            const int32_t *t = a.cum + ((size_t(b) * a.hop + i) * a.Q + q) * size_t(a.K + 1);
            const int slot = int(x & 0xffffu);
            // the code is the count of the entries 1 .. size - 1 that are <= slot: 64 samples, then the entries between two of them
            const int step = (size + 63) / 64;
            const int c1 = (lane + 1) * step;
            const int blk = __popcll(__ballot(c1 < size && t[c1] <= slot)) * step;
            const int c2 = blk + 1 + lane;
            const int code = blk + __popcll(__ballot(lane < step - 1 && c2 < size && t[c2] <= slot));
            const uint32_t start = uint32_t(t[code]), f = uint32_t(t[code + 1]) - start;
            x = f * (x >> AGX_RANS_SCALE_BITS) + uint32_t(slot) - start;
            for (int pull = 0; pull < 2 && x < RANS_L; ++pull) x = (x << 8) | next_byte();   // a coder's state needs two at the most
            if (x < RANS_L) st |= 4u;                        // not a state of the coder: the packet or the tables are not the sender's
            if (lane == 0) {
                codes[size_t(i - a.i0) * a.Q + q] = code;
                if (a.carry && i == i_end - 1) a.carry[size_t(b) * a.Q + q] = code;
            }
        }
        if (a.carry && i == i_end - 1)                       // the last frame of the row this call decodes: what the next step embeds
            for (int q = qb + lane; q < a.Q; q += 64) a.carry[size_t(b) * a.Q + q] = -1;
    }
    if (a.i0 < cnt && cnt <= a.i0 + a.n && !(x == RANS_L && cur == nb64)) st |= 4u;     // the call reached the row's end
    if (lane == 0) {
        a.state[size_t(b) * 2] = int64_t(x);
        a.state[size_t(b) * 2 + 1] = cur;
        a.status[b] = int64_t(st);
    }
}

// stage_sizes with this file's limit on K between its two refusals
static int entropy_sizes(const char *what, const int32_t *sizes, int n_q, int k, StageSizes *sz) {
    if (n_q <= 64 && k > CUM_MAX_K)
        return fail(AGX_ERR_UNSUPPORTED, "%s: K=%d exceeds %d codes per stage (the frequencies and the table of a stage live in LDS)", what, k,
                    CUM_MAX_K);
    return stage_sizes(what, sizes, n_q, k, sz);
}

}  // namespace agx

extern "C" {

int agx_codes_cum(const float *logits, const int32_t *sizes, const int64_t *counts, const int64_t *stages, int32_t *cum, int32_t batch,
                  int32_t n, int32_t n_q, int32_t k, int32_t n_cum, int32_t i_cum, void *stream) {
    using namespace agx;
    if (batch <= 0 || n <= 0 || n_q <= 0 || k <= 0) return fail(AGX_ERR_BAD_SHAPE, "codes_cum: bad shape B=%d n=%d Q=%d K=%d", batch, n, n_q, k);
    StageSizes sz;
    if (int rc = entropy_sizes("codes_cum", sizes, n_q, k, &sz)) return rc;
    if (i_cum < 0 || n_cum < n || i_cum > n_cum - n)
        return fail(AGX_ERR_BAD_SHAPE, "codes_cum: frames %d .. %d do not lie in a table buffer of %d frames", i_cum, i_cum + n - 1, n_cum);
    if (int64_t(batch) * n * n_q > 0x7fffffff)
        return fail(AGX_ERR_UNSUPPORTED, "codes_cum: B n Q = %lld tables exceed 2^31 - 1", (long long)batch * n * n_q);
    if (!logits || !cum) return fail(AGX_ERR_NULL_POINTER, "codes_cum: NULL pointer");
    CumArgs a{logits, counts, stages, cum, n, n_q, k, n_cum, i_cum, sz};
    hipLaunchKernelGGL(cum_kernel, dim3(unsigned(batch * n * n_q)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("codes_cum");
}

static int rans_shape(const char *what, const int32_t *sizes, int32_t batch, int32_t n, int32_t n_q, int32_t k, agx::StageSizes *sz) {
    using namespace agx;
    if (batch <= 0 || n <= 0 || n_q <= 0 || k <= 0) return fail(AGX_ERR_BAD_SHAPE, "%s: bad shape B=%d n=%d Q=%d K=%d", what, batch, n, n_q, k);
    if (int rc = entropy_sizes(what, sizes, n_q, k, sz)) return rc;
    if (int64_t(n) * n_q > AGX_RANS_MAX_SYMBOLS)
        return fail(AGX_ERR_UNSUPPORTED, "%s: n Q = %lld symbols per row exceed %d (a row's pairs and bytes live in LDS)", what,
                    (long long)n * n_q, AGX_RANS_MAX_SYMBOLS);
    return AGX_OK;
}

int agx_codes_rans_encode(const int32_t *cum, const int64_t *codes, const int32_t *sizes, const int64_t *counts, const int64_t *stages,
                          uint8_t *packets, int64_t *nbytes, int64_t *status, int32_t batch, int32_t n, int32_t n_q, int32_t k,
                          void *stream) {
    using namespace agx;
    StageSizes sz;
    if (int rc = rans_shape("codes_rans_encode", sizes, batch, n, n_q, k, &sz)) return rc;
    if (!cum || !codes || !packets || !nbytes || !status) return fail(AGX_ERR_NULL_POINTER, "codes_rans_encode: NULL pointer");
    const int N = n * n_q;
    const size_t lds = 16 + size_t(N) * 4 + size_t((2 * N + 4 + 15) & ~15);
    EncodeArgs a{cum, codes, counts, stages, packets, nbytes, status, n, n_q, k, sz};
    hipLaunchKernelGGL(rans_encode_kernel, dim3(unsigned(batch)), dim3(64), lds, static_cast<hipStream_t>(stream), a);
    return check_launch("codes_rans_encode");
}

int agx_codes_rans_decode(const int32_t *cum, const uint8_t *packets, const int64_t *nbytes, const int32_t *sizes, const int64_t *counts,
                          const int64_t *stages, int64_t *state, int64_t *codes, int64_t *carry, int64_t *status, int32_t batch,
                          int32_t hop, int32_t i0, int32_t n, int32_t n_q, int32_t k, int32_t p, void *stream) {
    using namespace agx;
    StageSizes sz;
    if (int rc = rans_shape("codes_rans_decode", sizes, batch, hop, n_q, k, &sz)) return rc;
    if (n <= 0 || i0 < 0 || i0 > hop - n)
        return fail(AGX_ERR_BAD_SHAPE, "codes_rans_decode: frames %d .. %d do not lie in a hop of %d frames", i0, i0 + n - 1, hop);
    if (p <= 0) return fail(AGX_ERR_BAD_SHAPE, "codes_rans_decode: packet rows of %d bytes", p);
    if (!cum || !packets || !nbytes || !state || !codes || !status) return fail(AGX_ERR_NULL_POINTER, "codes_rans_decode: NULL pointer");
    DecodeArgs a{cum, packets, nbytes, counts, stages, state, codes, carry, status, hop, i0, n, n_q, k, p, sz};
    hipLaunchKernelGGL(rans_decode_kernel, dim3(unsigned(batch)), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("codes_rans_decode");
}

}  // extern "C"
