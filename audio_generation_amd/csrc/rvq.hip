// Residual vector quantiser for gfx950: one launch for all residual stages.
//
// Stands in for the external `som_quantizer.ResidualQuantizer` the reference
// calls at networks/vae.py:315-318 (source absent from the reference tree; the
// arithmetic reproduced bit-for-bit is the one fixed in oracle/rvq_exact.c).
//
// One workgroup (8 waves) owns 32 frames for the whole stage loop.  The fp32 residual tile R[frame][d] (frame-major) and
// the two bf16 planes of the centred residual live in LDS, so latents are read once and x_q / indices written once
// (x_q is rebuilt at the end from the chosen codewords, added in stage order).  Per stage:
//   A. scores s[k] = |c'_k|^2 - 2 r'.c'_k for all K codewords on the bf16 matrix pipe (three products of two bf16 pieces
//      per operand; rows = codewords streamed from the stage image in L2 -- the phase is bound by the CU's L2 port: 2 MB per
//      stage and workgroup --, columns = the 32 frames read from the planes), per-frame minimum by in-lane min over the
//      accumulator registers + one lane shuffle + an 8-entry LDS exchange;
//   B. every codeword whose score is within the error margin of the minimum (kernel header of the error unit: what is proved, what is modelled) is a candidate; a frame with one
//      candidate is decided, the rest are decided by the defining binary64 distance (sequential, unfused): squares by all
//      lanes, the d-ordered sums of up to 16 pairs side by side, one lane each;
//   C. r -= c, index written, squared residual accumulated, and the next stage's r' = fl(r - mu) split into the planes.
#include "codes.hpp"

namespace agx {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 rvq_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int FT = 32;    // frames per workgroup
constexpr int NWV = 8;    // waves per workgroup (2 per SIMD: one computes while the other waits on L2)
constexpr int NT = 64 * NWV;
constexpr int RS = 33;    // LDS row stride of R / O (conflict-free in both access patterns)
constexpr int CAND = 8;   // candidate slots per frame

__host__ __device__ inline int rvq_dp(int dim) { return (dim + 15) & ~15; }  // D rounded up to the 16-deep k block of the bf16 MFMA
// stage image, all on CENTRED codewords c' = fl(c - mu), mu = the stage's mean codeword:
//   CbH[Dp/16][plane 2][lane half 2][K][8] bf16 -- c' = h + m + (error <= 2^-16 |c'_d|), the A operand of
//   v_mfma_f32_32x32x16_bf16 as it stands: lane (code, half) reads its 8 dims 16 kq + 8 half + (0..7) of one plane with one
//   16-byte load; same number of bytes as an fp32 image -- | c2 = |c'|^2 (K) | cn = |c'| (K) | cmax2 + pad(3) | mu (Dp)
// Distances are translation invariant, and scoring |c'|^2 - 2 r'.c' with r' = fl(r - mu) keeps the fp32
// error bound proportional to the SPREAD of the data instead of its offset from the origin: without the
// centring, latents that share a large common component (any encoder with a bias) put most codewords
// inside the error margin of the minimum.
__host__ __device__ inline int64_t rvq_stage_floats(int k, int dim) {
    return int64_t(rvq_dp(dim)) * k + 2 * int64_t(k) + 4 + rvq_dp(dim);
}

// ------------------------------------------------------------------------- pack
// Stages may have fewer than K codewords (the reference takes one codebook size per quantizer, vae.py:233): rows
// kq .. K-1 of such a stage are padding -- excluded from the mean and from cmax2, |c'|^2 = +inf (never a candidate),
// zero in the score image; the stage's count rides in the image's tail for the kernel's full-search fallback.

// mu[d] = mean_k c[k][d].  One wave per dimension d: lane L adds codewords L, L + 64, ... in order, the 64 partial sums are
// combined by a fixed shuffle tree (deterministic).  (Round 2: one THREAD per d walking all K rows with a stride of D
// floats -- 384 us per repack at 8 x 1024 x 512.)
__global__ __launch_bounds__(256) void rvq_mean_kernel(const float *__restrict__ cb, int k, int dim,
                                                       float *__restrict__ packed, StageSizes sizes) {
    const int q = blockIdx.y;
    const int kq = sizes.n[q];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dp = rvq_dp(dim);
    float *mu = packed + q * rvq_stage_floats(k, dim) + size_t(dp) * k + 2 * size_t(k) + 4;
    // 4 waves x 16 dims per block: lane = (codeword phase c0 = lane / 16, dim d0 + lane % 16) so that a wave's loads are
    // 64-byte row segments; each lane walks codewords c0, c0 + 4, ... and the four phases are combined at the end
    const int d = blockIdx.x * 64 + wave * 16 + (lane & 15);
    const int c0 = lane >> 4;
    float acc = 0.f;
    if (d < dim)
        for (int c = c0; c < kq; c += 4) acc += cb[(size_t(q) * k + c) * dim + d];
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    if (d < dp && c0 == 0) mu[d] = d < dim ? acc / float(kq) : 0.f;
}

__global__ __launch_bounds__(256) void rvq_pack_kernel(const float *__restrict__ cb, int n_q, int k,
                                                       int dim, float *__restrict__ packed, StageSizes sizes) {
    const int q = blockIdx.y;
    const bool pad = blockIdx.x * 256 + threadIdx.x >= sizes.n[q];
    const int code = blockIdx.x * 256 + threadIdx.x;
    float *img = packed + q * rvq_stage_floats(k, dim);
    if (code >= k) return;
    const float *row = cb + (size_t(q) * k + code) * dim;
    const int dp = rvq_dp(dim);
    const float *mu = img + size_t(dp) * k + 2 * size_t(k) + 4;
    float acc = 0.f;
    __bf16 *imgb = reinterpret_cast<__bf16 *>(img);
    for (int d = 0; d < dp; ++d) {
        const float v = (d < dim && !pad) ? row[d] - mu[d] : 0.f;
        const __bf16 h = (__bf16)v;
        const __bf16 m = (__bf16)(v - (float)h);
        const size_t base = ((size_t(d >> 4) * 4 + ((d >> 3) & 1)) * k + code) * 8 + (d & 7);   // plane 0 (h), lane half (d/8)%2
        imgb[base] = h;
        imgb[base + size_t(2) * k * 8] = m;                                                      // plane 1 (m)
        acc = fmaf(v, v, acc);
    }
    img[size_t(dp) * k + code] = pad ? INFINITY : acc;
    img[size_t(dp) * k + k + code] = pad ? 0.f : sqrtf(acc);
}

__global__ __launch_bounds__(256) void rvq_cmax_kernel(int k, int dim, float *__restrict__ packed, StageSizes sizes) {
    float *img = packed + blockIdx.x * rvq_stage_floats(k, dim);
    const float *c2 = img + size_t(rvq_dp(dim)) * k;
    const int kq = sizes.n[blockIdx.x];
    float m = 0.f;
    for (int i = threadIdx.x; i < kq; i += 256) m = fmaxf(m, c2[i]);
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float *tail = img + size_t(rvq_dp(dim)) * k + 2 * size_t(k);
        tail[0] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
        tail[1] = __int_as_float(kq);      // codewords of this stage (an integer's bits)
        tail[2] = tail[3] = 0.f;
    }
}

// ------------------------------------------------------------------------ forward
struct RvqArgs {
    const float *x;
    int64_t x_sb, x_st, x_sd;
    const float *cb;      // (Q,K,D)
    const float *packed;  // stage images
    int B, T, D, K, Q;
    float *xq;
    int64_t q_sb, q_st, q_sd;
    int64_t *index;  // (B*T, Q)
    double *sq_err;  // (Q) [unused by the kernel since the partials moved to `part`]
    double *part;    // (workgroups, Q) squared error of each workgroup's 32 frames per stage
    // PROBE BUILD ONLY (-DAGX_RVQ_PROBE, tools/rvq_stamps.py build): the product build fixes acc_scale = 1 and compiles no stamp.
    float acc_scale; // 1; probe knob b3_dbg = 7: 4 (widens the accumulation term of the score error bound), 8: 0 (NOT rigorous:
                     // timing only), 9: -1 (the stage's "squared error" output carries the largest candidate count)
    unsigned long long *stamps;   // agx_rvq_debug_stamps: [workgroup][16] s_memtime at the phase boundaries of stage stamp_q
    int stamp_q;
};
#ifdef AGX_RVQ_PROBE
// thread 0 of every workgroup: kernel-level slots (0, 1, 15) and the phase boundaries of ONE stage (a null pointer costs a scalar branch)
#define RVQ_STAMP(slot, cond)                                                                                      \
    do {                                                                                                           \
        if (a.stamps != nullptr && tid == 0 && (cond)) a.stamps[size_t(blockIdx.x) * 16 + (slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#define RVQ_ACC_SCALE(a) fabsf((a).acc_scale)
#define RVQ_DIAG(a) ((a).acc_scale < 0.f)
#else
#define RVQ_STAMP(slot, cond) do { } while (0)
#define RVQ_ACC_SCALE(a) 1.f
#define RVQ_DIAG(a) false
#endif

// LDS map (byte offsets).  R is FRAME-major (a frame's residual is one contiguous row: the update, the centring / split and the
// binary64 distances walk it with 16-byte accesses); the score GEMM reads its B operand from the two bf16 PLANES
//   PL[piece 2][Dp / 8][frame][8 bf16]      r' = fl(r - mu) = h + m + O(2^-16 r'),
// written ONCE per stage by the update phase (round 3, first form: every wave re-read R, centred and split its B fragments
// itself -- 16 x redundant, ~50 vector instructions per 6 MFMAs).  The plane region is dead between a stage's score passes and
// its update: the binary64 distances use it for their squares.  x_q is not accumulated in LDS any more: it is rebuilt at the end
// from the chosen codewords, added in stage order (the same fp32 sums).
struct RvqLds {
    int R, PL, wmin, rn2, sqf, mus, cnt, state, best, ccode, cscore, cdist, work, flags, hist, tails, total;
};
constexpr int SQ_PAIRS = 16;   // (frame, candidate) pairs whose squares fit the plane region at a time: 128 Dp / (8 Dp)
constexpr int PROW = (FT + 1) * 16;   // bytes per 8-dim group of a plane: 32 frames x 16 B + 16 B, so that the update's writes (lane = group)
                                      // land 4 banks apart (4-way instead of 64-way conflicts); the GEMM's reads stay contiguous
__host__ __device__ inline int rvq_pad64(int n) { return (n + 63) & ~63; }
__host__ __device__ inline int rvq_rsf(int Dp) { return Dp + 4; }   // floats per row of R (rows stay 16-byte aligned, 4 banks apart)
__host__ __device__ inline RvqLds rvq_lds_map(int Dp, int K, int Q, bool tail) {
    RvqLds m;
    int o = 0;
    m.R = o;      o += FT * rvq_rsf(Dp) * 4;
    m.PL = o;     o += 2 * (Dp / 8) * PROW;      // >= SQ_PAIRS x Dp doubles
    m.cdist = o;  o += FT * CAND * 8;            // (8-byte aligned: everything above is a multiple of 16)
    m.wmin = o;   o += 2 * NWV * FT * 4;      // one buffer per score-pass parity
    m.rn2 = o;    o += FT * 4;
    m.sqf = o;    o += FT * 4;
    m.mus = o;    o += 2 * rvq_pad64(Dp) * 4;   // two buffers: the next stage's mean streams in (LDS-DMA) during the search
    m.cnt = o;    o += FT * 4;
    m.state = o;  o += FT * 4;
    m.best = o;   o += FT * 4;
    m.ccode = o;  o += FT * CAND * 4;
    m.cscore = o; o += FT * CAND * 4;
    m.work = o;   o += FT * CAND * 4;
    m.flags = o;  o += 16;
    m.hist = o;   o += Q * FT * 4;
    m.tails = o;  o += tail ? 2 * rvq_pad64(2 * K) * 4 : 0;   // two buffers, as mus
    m.total = o;
    return m;
}

// sum over the 64 lanes, the same value in every lane: four DPP steps inside the 16-lane rows (quad swaps, half-row and row mirrors
// -- no LDS crossbar), then the four row sums through v_readlane.  (Six ds_bpermute rounds per sum before: 2.9 k cycles for the
// eight sums of an update phase.)
#define RVQ_DPP(x, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (x)), (ctrl), 0xf, 0xf, true))
__device__ __forceinline__ float rvq_wave_sum(float v) {
    v += RVQ_DPP(v, 0xB1);    // quad_perm [1,0,3,2]
    v += RVQ_DPP(v, 0x4E);    // quad_perm [2,3,0,1]
    v += RVQ_DPP(v, 0x141);   // row_half_mirror
    v += RVQ_DPP(v, 0x140);   // row_mirror
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return (r0 + r1) + (r2 + r3);
}

// ---------------------------------------------------------------- exact distance
// The DEFINING arithmetic (oracle/rvq_exact.c): binary64, d ascending, one subtract + one multiply + one add per term, never fused.
#pragma clang fp contract(off)
// squares of one (frame, codeword) pair in the DEFINING arithmetic (binary64, never fused), all lanes in parallel: lane L forms
// dims 8 L .. 8 L + 7 (+ 512 per round) and leaves them in sq[d]; dims >= D give +0.0.
__device__ __forceinline__ void rvq_pair_squares(double *__restrict__ sq, const float *__restrict__ r_row,
                                                 const float *__restrict__ c, int D, int Dp, int lane) {
    for (int d0 = 8 * lane; d0 < Dp; d0 += 512) {
        const f32x4 r0 = *reinterpret_cast<const f32x4 *>(r_row + d0), r1 = *reinterpret_cast<const f32x4 *>(r_row + d0 + 4);
        float cv[8];
        if ((D & 3) == 0) {   // rows are 16-byte aligned
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            const f32x4 c0 = d0 < D ? *reinterpret_cast<const f32x4 *>(c + d0) : z;
            const f32x4 c1 = d0 + 4 < D ? *reinterpret_cast<const f32x4 *>(c + d0 + 4) : z;
#pragma unroll
            for (int e = 0; e < 4; ++e) cv[e] = c0[e], cv[4 + e] = c1[e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) cv[e] = d0 + e < D ? c[d0 + e] : 0.f;
        }
        double s[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const double diff = double(e < 4 ? r0[e] : r1[e - 4]) - double(cv[e]);
            s[e] = diff * diff;
        }
        typedef double f64x2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            f64x2 v = {s[e], s[e + 1]};
            *reinterpret_cast<f64x2 *>(sq + d0 + e) = v;
        }
    }
}
// ... and their sum in d order, ONE lane per pair: acc = (..((0 + sq_0) + sq_1) + ..) + sq_{D-1}
__device__ __forceinline__ double rvq_chain_sum(const double *__restrict__ sq, int D) {
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    double acc = 0.0;
    int d = 0;
    for (; d + 16 <= D; d += 16) {
        f64x2 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const f64x2 *>(sq + d + 2 * j);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc = acc + v[j][0];
            acc = acc + v[j][1];
        }
    }
    for (; d < D; ++d) acc = acc + sq[d];
    return acc;
}
// The full defining search of one frame (candidate overflow), ONE codeword per lane: every lane walks its codeword's row in d
// order -- the defining arithmetic and its summation order per codeword, 64 codewords side by side (the wave-wide evaluation above
// hands the running sum from lane to lane: 21 k cycles per distance, 1.5 ms per overflowing frame at K = 1024).  Returns this
// lane's distance; the caller takes the minimum (lowest index on ties).
__device__ __forceinline__ double rvq_dist_lane(const float *__restrict__ r_row /* LDS, the same for all lanes */,
                                                const float *__restrict__ c /* this lane's codeword */, int D) {
    double acc = 0.0;
    int d = 0;
    if ((D & 3) == 0) {
        for (; d + 16 <= D; d += 16) {
            f32x4 cv[4], rv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) cv[j] = *reinterpret_cast<const f32x4 *>(c + d + 4 * j);
#pragma unroll
            for (int j = 0; j < 4; ++j) rv[j] = *reinterpret_cast<const f32x4 *>(r_row + d + 4 * j);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double diff = double(rv[j][e]) - double(cv[j][e]);
                    const double sq = diff * diff;
                    acc = acc + sq;
                }
        }
    }
    for (; d < D; ++d) {
        const double diff = double(r_row[d]) - double(c[d]);
        const double sq = diff * diff;
        acc = acc + sq;
    }
    return acc;
}
#pragma clang fp contract(fast)

// One text, two kernels: rvq_forward_body.hpp holds the statements of the forward kernel and is compiled twice, as
// rvq_forward_kernel (STAGED = false) and as rvq_forward_staged_kernel (a stage count per batch row,
// q_f = clamp(stages[b], 0, Q) for the frames of row b).  The search runs all Q stages for every frame either way -- it is
// greedy, a stage's choice does not depend on later stages -- and the staged kernel differs at its three STAGED sites only: the
// index write (-1 at a dead stage), the frame's share of the stage's part[] (0 at a dead stage) and the stage bound of the x_q
// rebuild (q_f).  Every one of them is executed by the wave that owns the frame (frames w, w + NWV, ...), so q_f lives in that
// wave's scalar registers: the LDS map, and with it the TAIL_LDS choice and the 160 KB refusal, is the same for both kernels.
// (A textual include, not the __forceinline__ template body of attention_masked.hpp: inlined from a callee, the unstaged kernel
// comes out with another schedule and register allocation; compiled in place it keeps its machine code byte for byte.)
template <int MT, bool TAIL_LDS>   // TAIL_LDS: the stage's |c'|^2 and |c'| tables are copied to LDS (they fit beside R / the planes)
__global__ __launch_bounds__(NT) void rvq_forward_kernel(RvqArgs a) {
    constexpr bool STAGED = false;
    const int64_t *const stages = nullptr;
#include "rvq_forward_body.hpp"
}
template <int MT, bool TAIL_LDS>
__global__ __launch_bounds__(NT) void rvq_forward_staged_kernel(RvqArgs a, const int64_t *__restrict__ stages) {
    constexpr bool STAGED = true;
#include "rvq_forward_body.hpp"
}

// ------------------------------------------------------------------------ verify mode (debug knob rvq_verify)
// The DEFINING search of every (frame, stage) next to the fast path's answer: one wave per frame, a codeword per lane
// (rvq_dist_lane: binary64, d ascending, never fused -- oracle/rvq_exact.c), the minimum with the lowest index on ties, compared
// with index[frame][stage]; the residual then follows the FAST path's choice (r <- r - c[index], binary32), so every stage is
// checked on exactly the residual the fast path searched.  Counters (g_rvq_verify): [0] codes that differ, [1] frames with at
// least one, [2] codes checked.  ~30 G binary64 terms on the bench workload: tens of milliseconds, a debug tool.
__device__ unsigned long long g_rvq_verify[4];
__global__ __launch_bounds__(256) void rvq_verify_kernel(const float *__restrict__ x, int64_t x_sb, int64_t x_st, int64_t x_sd,
                                                         const float *__restrict__ cb, const float *__restrict__ packed, int64_t N,
                                                         int T, int D, int K, int Q, const int64_t *__restrict__ index) {
    extern __shared__ __align__(16) float vr[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t f = int64_t(blockIdx.x) * 4 + wave;
    if (f >= N) return;       // (no workgroup barrier below: a wave only touches its own row)
    float *r = vr + size_t(wave) * (D + 4);
    const float *xf = x + (f / T) * x_sb + (f % T) * x_st;
    for (int d = lane; d < D; d += 64) r[d] = xf[d * x_sd];
    const int Dp = rvq_dp(D);
    int bad = 0;
    for (int q = 0; q < Q; ++q) {
        const float *cbq = cb + size_t(q) * K * D;
        const int kq_bits = __float_as_int(packed[q * rvq_stage_floats(K, D) + size_t(Dp) * K + 2 * size_t(K) + 1]);
        const int Kq = kq_bits > 0 && kq_bits <= K ? kq_bits : K;
        double best = 1.0 / 0.0;
        int arg = 0x7fffffff;
        for (int c0 = 0; c0 < Kq; c0 += 64) {
            const int c = c0 + lane;
            const double dc = rvq_dist_lane(r, cbq + size_t(min(c, Kq - 1)) * D, D);
            if (c < Kq && dc < best) best = dc, arg = c;       // ascending c per lane: a tie keeps the lower index
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double ob = __shfl_xor(best, off);
            const int oa = __shfl_xor(arg, off);
            if (ob < best || (ob == best && oa < arg)) best = ob, arg = oa;
        }
        const int64_t got = index[f * Q + q];
        if (got != int64_t(arg)) ++bad;
        const float *cs = cbq + size_t(got >= 0 && got < Kq ? got : 0) * D;
        for (int d = lane; d < D; d += 64) r[d] = r[d] - cs[d];
    }
    if (lane == 0) {
        if (bad) {
            atomicAdd(&g_rvq_verify[0], (unsigned long long)bad);
            atomicAdd(&g_rvq_verify[1], 1ull);
        }
        atomicAdd(&g_rvq_verify[2], (unsigned long long)Q);
    }
}

static size_t rvq_lds_bytes(int dim, int k, int q, bool *tail_in_lds) {
    const int Dp = rvq_dp(dim);
    const size_t with = size_t(rvq_lds_map(Dp, k, q, true).total);
    const bool fits = with <= 160 * 1024;
    if (tail_in_lds) *tail_in_lds = fits;
    return fits ? with : size_t(rvq_lds_map(Dp, k, q, false).total);
}

// ------------------------------------------------------------------------ dequantize
__global__ __launch_bounds__(256) void rvq_dequant_kernel(const float *__restrict__ cb,
                                                          const int64_t *__restrict__ idx, int64_t n,
                                                          int k, int dim, float *__restrict__ out,
                                                          int64_t o_sn, int64_t o_sd, int accumulate) {
    const int64_t row = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    int64_t i = idx[row];
    i = i < 0 ? 0 : (i >= k ? k - 1 : i);
    const float *c = cb + i * dim;
    float *o = out + row * o_sn;
    for (int d = threadIdx.x & 63; d < dim; d += 64) {
        const float v = c[d];
        o[d * o_sd] = accumulate ? o[d * o_sd] + v : v;
    }
}

// sq_err[q] = sum over workgroups of part[wg][q] (pairwise per lane, then a fixed shuffle tree); commit = sum_q sq_err[q] * inv
__global__ __launch_bounds__(64) void rvq_sqerr_kernel(const double *__restrict__ part, int nwg, int Q, double *__restrict__ sq_err,
                                                       float *__restrict__ commit, double inv_numel) {
    const int lane = threadIdx.x;
    double total = 0.0;
    for (int q = 0; q < Q; ++q) {
        double s = 0.0;
        for (int w = lane; w < nwg; w += 64) s += part[size_t(w) * Q + q];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) sq_err[q] = s;
        total += s;
    }
    if (lane == 0 && commit) *commit = float(total * inv_numel);
}

}  // namespace agx

namespace agx {

// Assignment statistics of the EMA codebook update (quantizer.py:_ema_update): for stage q and code k
//     stats[q][k][0] = #{n : index[n][q] = k},   stats[q][k][1 + d] = sum over those n of r_q[n][d]
// with r_q[n] = frames[n] - c_0[index[n][0]] - ... - c_{q-1}[index[n][q-1]] (fp32, subtracted in stage order: the residual
// the search saw).  Two launches, no atomics, so the update is reproducible run to run (torch's index_add_ on the
// device is not):
//   rvq_residuals_kernel   R[q][n][:] for every stage (workspace, Q N D floats)
//   rvq_ema_stats_kernel   one workgroup per (code, stage): ordered compaction of the matching frames (ballot + prefix),
//                          wave w adds rows w, w+4, ... of the list in list order, the four partial sums are added in
//                          wave order.
constexpr int EMA_LIST = 1024;

__global__ __launch_bounds__(256) void rvq_residuals_kernel(const float *__restrict__ frames, const float *__restrict__ cb,
                                                            const int64_t *__restrict__ index, float *__restrict__ R,
                                                            int n, int dim, int K, int Q) {
    const int64_t total = int64_t(n) * dim;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
        const int f = int(e / dim), d = int(e - int64_t(f) * dim);
        float r = frames[e];
        for (int q = 0; q < Q; ++q) {
            R[int64_t(q) * total + e] = r;
            const int64_t c = index[int64_t(f) * Q + q];
            if (c >= 0 && c < K) r -= cb[(int64_t(q) * K + c) * dim + d];
        }
    }
}

// The row sum both per-code kernels share: the calling workgroup (256 threads) adds the rows Rq[f][:] of the frames f with
// index[f][q] == k, in list order as described above, and leaves the four wave sums in part[wave][0 .. dim).  Returns the
// number of such frames (uniform); the caller may read `part` right away.  A code that owns more than EMA_LIST - 256
// frames drains its list every time the next block of 256 might not fit.
template <bool VEC>
__device__ __forceinline__ int rvq_code_row_sum(const float *__restrict__ Rq, const int64_t *__restrict__ index, int n,
                                                int dim, int Q, int q, int k, float (*part)[1024]) {
    constexpr int NA = VEC ? 4 : 16;          // accumulators per lane: dim <= 1024
    __shared__ int list[EMA_LIST];
    __shared__ int wave_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    f32x4 av[VEC ? NA : 1];
    float as[VEC ? 1 : NA];
#pragma unroll
    for (int u = 0; u < (VEC ? NA : 1); ++u) av[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < (VEC ? 1 : NA); ++u) as[u] = 0.f;
    int held = 0, total = 0;
    auto drain = [&]() {
#pragma unroll 4
        for (int e = wave; e < held; e += 4) {
            const float *row = Rq + int64_t(list[e]) * dim;
            if (VEC) {
#pragma unroll
                for (int u = 0; u < NA; ++u) {
                    const int c = 4 * (lane + 64 * u);
                    if (c < dim) av[u] += *reinterpret_cast<const f32x4 *>(row + c);
                }
            } else {
#pragma unroll
                for (int u = 0; u < NA; ++u) {
                    const int d = lane + 64 * u;
                    if (d < dim) as[u] += row[d];
                }
            }
        }
    };
    for (int base = 0; base < n; base += 256) {
        const int f = base + tid;
        const bool hit = f < n && index[size_t(f) * Q + q] == k;
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = held;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        if (hit) list[off + __popcll(m & ((1ull << lane) - 1ull))] = f;
        const int add = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        held += add;
        total += add;
        __syncthreads();
        if (held > EMA_LIST - 256) {   // uniform: the next block of 256 might not fit
            drain();
            held = 0;
            __syncthreads();
        }
    }
    drain();
    if (VEC) {
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            const int c = 4 * (lane + 64 * u);
            if (c < dim)
#pragma unroll
                for (int i = 0; i < 4; ++i) part[wave][c + i] = av[u][i];
        }
    } else {
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            const int d = lane + 64 * u;
            if (d < dim) part[wave][d] = as[u];
        }
    }
    __syncthreads();
    return total;
}

template <bool VEC>
__global__ __launch_bounds__(256) void rvq_ema_stats_kernel(const float *__restrict__ R, const int64_t *__restrict__ index,
                                                            float *__restrict__ stats, int n, int dim, int K, int Q) {
    __shared__ float part[4][1024];
    const int k = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int total = rvq_code_row_sum<VEC>(R + int64_t(q) * n * dim, index, n, dim, Q, q, k, part);
    float *o = stats + (size_t(q) * K + k) * (dim + 1);
    if (tid == 0) o[0] = float(total);
    for (int d = tid; d < dim; d += 256) o[1 + d] = ((part[0][d] + part[1][d]) + part[2][d]) + part[3][d];
}

// Backward of the training call (agx_rvq_backward).  Everything is elementwise in d, so a workgroup owns a tile of
// BW_TF frames x BW_TD dims:
//   rvq_bwd_dx_kernel        x and g_xq tiles -> LDS with the lanes along whichever axis the tensor is contiguous in
//                            ((B, D, T) tensors: frames; (B, T, D): dims), then lanes along d (codeword rows and the S_q rows
//                            are D-contiguous): the residual chain r_1 .. r_Q in registers, walked back into the suffix sums
//                            S_q (-> workspace [q][n][D], when the codebook gradient is wanted) and dx = g + a S_0 -> LDS ->
//                            global, again along dx's own contiguous axis.
//   rvq_bwd_codebook_kernel  the ordered row sum of the EMA statistics over S_q, times -a; stages >= Q are zero-filled.
constexpr int BW_TF = 64, BW_TD = 64, BW_RS = BW_TD + 1;

struct RvqBwdArgs {
    const float *x;
    int64_t x_sb, x_st, x_sd;
    const float *g;            // NULL: zero
    int64_t g_sb, g_st, g_sd;
    float *dx;
    int64_t d_sb, d_st, d_sd;
    const float *cb;
    const int64_t *index;
    const float *g_commit;     // device scalar, NULL: zero
    float *S;                  // NULL: not wanted
    int n, t, dim, K, Q;
    float scale;               // 2 / (N D)
};

// One text, two kernels (as the forward): rvq_bwd_dx_body.hpp is rvq_bwd_dx_kernel (STAGED = false) and
// rvq_bwd_dx_staged_kernel, whose residual chain and suffix sums of frame (b, t) run over its
// q_f = clamp(stages[b], 0, Q) live stages only -- the rows S_q of its dead stages are not written, and the codebook kernel
// never selects them (the staged forward's index is -1 there).
template <int QMAX>   // Q <= QMAX residuals per element live in registers
__global__ __launch_bounds__(256) void rvq_bwd_dx_kernel(RvqBwdArgs a) {
    constexpr bool STAGED = false;
    const int64_t *const stages = nullptr;
#include "rvq_bwd_dx_body.hpp"
}
template <int QMAX>
__global__ __launch_bounds__(256) void rvq_bwd_dx_staged_kernel(RvqBwdArgs a, const int64_t *__restrict__ stages) {
    constexpr bool STAGED = true;
#include "rvq_bwd_dx_body.hpp"
}

template <bool VEC>
__global__ __launch_bounds__(256) void rvq_bwd_codebook_kernel(const float *__restrict__ S, const int64_t *__restrict__ index,
                                                               const float *__restrict__ g_commit, float scale,
                                                               float *__restrict__ dcb, int n, int dim, int K, int Q) {
    __shared__ float part[4][1024];
    const int k = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    float *o = dcb + (size_t(q) * K + k) * dim;
    if (q >= Q) {   // a stage this call did not run (uniform)
        for (int d = tid; d < dim; d += 256) o[d] = 0.f;
        return;
    }
    const int total = rvq_code_row_sum<VEC>(S + int64_t(q) * n * dim, index, n, dim, Q, q, k, part);
    // a code no frame chose gets +0 whatever g_commit holds: the padding rows of a short stage stay zero under Adam
    const float na = (g_commit && total > 0) ? -(*g_commit * scale) : 0.f;
    for (int d = tid; d < dim; d += 256)
        o[d] = total > 0 ? na * (((part[0][d] + part[1][d]) + part[2][d]) + part[3][d]) : 0.f;
}

}  // namespace agx

extern "C" {

int64_t agx_rvq_packed_floats(int32_t n_q, int32_t k, int32_t dim) {
    if (n_q <= 0 || k <= 0 || dim <= 0) return AGX_ERR_BAD_SHAPE;
    return int64_t(n_q) * agx::rvq_stage_floats(k, dim);
}

int agx_rvq_pack_sized(const float *codebooks, const int32_t *sizes, int32_t n_q, int32_t k, int32_t dim, float *packed,
                       void *stream) {
    using namespace agx;
    if (n_q <= 0 || k <= 0 || dim <= 0) return fail(AGX_ERR_BAD_SHAPE, "rvq_pack: bad shape Q=%d K=%d D=%d", n_q, k, dim);
    if (!codebooks || !packed) return fail(AGX_ERR_NULL_POINTER, "rvq_pack: NULL pointer");
    StageSizes sz;
    if (int rc = stage_sizes("rvq_pack", sizes, n_q, k, &sz)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(rvq_mean_kernel, dim3(ceil_div(rvq_dp(dim), 64), n_q), dim3(256), 0, st, codebooks, k, dim, packed, sz);
    hipLaunchKernelGGL(rvq_pack_kernel, dim3(ceil_div(k, 256), n_q), dim3(256), 0, st, codebooks, n_q, k, dim, packed, sz);
    hipLaunchKernelGGL(rvq_cmax_kernel, dim3(n_q), dim3(256), 0, st, k, dim, packed, sz);
    return check_launch("agx_rvq_pack");
}

int agx_rvq_pack(const float *codebooks, int32_t n_q, int32_t k, int32_t dim, float *packed, void *stream) {
    return agx_rvq_pack_sized(codebooks, nullptr, n_q, k, dim, packed, stream);
}

size_t agx_rvq_workspace_bytes(int32_t batch, int32_t t, int32_t, int32_t, int32_t q_used) {
    if (batch <= 0 || t <= 0 || q_used <= 0) return 0;
    return size_t(agx::ceil_div64(int64_t(batch) * t, agx::FT)) * q_used * sizeof(double);
}

// diagnostic: device buffer of (workgroups x 16) 64-bit stamps the next rvq_forward launches fill (NULL switches it off).
// PROBE BUILD ONLY (-DAGX_RVQ_PROBE; `tools/rvq_stamps.py build` writes lib/libagx_rvq_probe.so): the product library keeps no
// raw pointer between calls and refuses.
#ifdef AGX_RVQ_PROBE
static unsigned long long *g_rvq_stamps = nullptr;
static int g_rvq_stamp_q = 0;
int agx_rvq_debug_stamps(void *device_buffer, int32_t stage) {
    g_rvq_stamps = static_cast<unsigned long long *>(device_buffer);
    g_rvq_stamp_q = stage;
    return AGX_OK;
}
#else
int agx_rvq_debug_stamps(void *, int32_t) {
    return agx::fail(AGX_ERR_UNSUPPORTED, "agx_rvq_debug_stamps: probe build only (tools/rvq_stamps.py build)");
}
#endif

// Verify mode (knob rvq_verify = 1): the counters of the checker kernel, in the code object (nothing is allocated).
int agx_rvq_verify_counts(int64_t *out3, int32_t reset) {
    unsigned long long h[4] = {0, 0, 0, 0};
    if (out3) {
        hipError_t e = hipMemcpyFromSymbol(h, HIP_SYMBOL(agx::g_rvq_verify), sizeof(h), 0, hipMemcpyDeviceToHost);   // synchronises
        if (e != hipSuccess) return agx::fail(AGX_ERR_LAUNCH, "agx_rvq_verify_counts: %s", hipGetErrorString(e));
        for (int i = 0; i < 3; ++i) out3[i] = int64_t(h[i]);
    }
    if (reset) {
        const unsigned long long z[4] = {0, 0, 0, 0};
        hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(agx::g_rvq_verify), z, sizeof(z), 0, hipMemcpyHostToDevice);
        if (e != hipSuccess) return agx::fail(AGX_ERR_LAUNCH, "agx_rvq_verify_counts: %s", hipGetErrorString(e));
    }
    return AGX_OK;
}

int agx_rvq_forward(const float *x, int64_t x_sb, int64_t x_st, int64_t x_sd, const float *codebooks,
                    const float *packed, int32_t batch, int32_t t, int32_t dim, int32_t k, int32_t q_used,
                    float *xq, int64_t q_sb, int64_t q_st, int64_t q_sd, int64_t *index, double *sq_err,
                    void *workspace, size_t workspace_bytes, void *stream) {
    return agx_rvq_forward_ex(x, x_sb, x_st, x_sd, codebooks, packed, batch, t, dim, k, q_used, xq, q_sb, q_st, q_sd, index,
                              sq_err, nullptr, workspace, workspace_bytes, stream);
}

int agx_rvq_forward_ex(const float *x, int64_t x_sb, int64_t x_st, int64_t x_sd, const float *codebooks,
                       const float *packed, int32_t batch, int32_t t, int32_t dim, int32_t k, int32_t q_used,
                       float *xq, int64_t q_sb, int64_t q_st, int64_t q_sd, int64_t *index, double *sq_err,
                       float *commit_loss, void *workspace, size_t workspace_bytes, void *stream) {
    return agx_rvq_forward_staged(x, x_sb, x_st, x_sd, codebooks, packed, batch, t, dim, k, q_used, xq, q_sb, q_st, q_sd, index,
                                  nullptr, sq_err, commit_loss, workspace, workspace_bytes, stream);
}

// `stages` NULL: the unstaged kernel, exactly agx_rvq_forward_ex.  Same checks and the same two launches (search,
// rvq_sqerr_kernel) either way: the stage counts are device data the host never reads.
int agx_rvq_forward_staged(const float *x, int64_t x_sb, int64_t x_st, int64_t x_sd, const float *codebooks,
                           const float *packed, int32_t batch, int32_t t, int32_t dim, int32_t k, int32_t q_used,
                           float *xq, int64_t q_sb, int64_t q_st, int64_t q_sd, int64_t *index, const int64_t *stages,
                           double *sq_err, float *commit_loss, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace agx;
    if (q_used > 0 && (!workspace || workspace_bytes < agx_rvq_workspace_bytes(batch, t, dim, k, q_used)))
        return fail(AGX_ERR_WORKSPACE, "rvq_forward: workspace too small (%zu < %zu)", workspace_bytes,
                    agx_rvq_workspace_bytes(batch, t, dim, k, q_used));
    if (batch <= 0 || t <= 0 || dim <= 0 || k <= 0 || q_used < 0)
        return fail(AGX_ERR_BAD_SHAPE, "rvq_forward: bad shape B=%d T=%d D=%d K=%d Q=%d", batch, t, dim, k, q_used);
    if (!x || !codebooks || !packed || !xq || (q_used > 0 && (!index || !sq_err)))
        return fail(AGX_ERR_NULL_POINTER, "rvq_forward: NULL pointer");
    bool tail_lds = false;
    const size_t lds = rvq_lds_bytes(dim, k, q_used, &tail_lds);
    if (lds > 160 * 1024) return fail(AGX_ERR_UNSUPPORTED, "rvq_forward: D=%d needs %zu B of LDS", dim, lds);
    RvqArgs a{x, x_sb, x_st, x_sd, codebooks, packed, batch, t, dim, k, q_used, xq, q_sb, q_st, q_sd, index, sq_err,
              static_cast<double *>(workspace),
#ifdef AGX_RVQ_PROBE
              tuning().b3_dbg == 7 ? 4.f : (tuning().b3_dbg == 8 ? 0.f : (tuning().b3_dbg == 9 ? -1.f : 1.f)), g_rvq_stamps, g_rvq_stamp_q};
#else
              1.f, nullptr, 0};
#endif
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n = int64_t(batch) * t;
    dim3 grid((unsigned)ceil_div64(n, FT)), block(NT);
    auto launch = [&](auto kern, auto staged_kern) -> int {
        hipError_t e = hipFuncSetAttribute(stages ? reinterpret_cast<const void *>(staged_kern) : reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return fail(AGX_ERR_LAUNCH, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        if (stages)
            hipLaunchKernelGGL(staged_kern, grid, block, lds, st, a, stages);
        else
            hipLaunchKernelGGL(kern, grid, block, lds, st, a);
        if (q_used > 0)   // per-stage sums and the commit loss, in a fixed order: deterministic, no atomics, no host arithmetic
            hipLaunchKernelGGL(rvq_sqerr_kernel, dim3(1), dim3(64), 0, st, a.part, int(grid.x), q_used, sq_err, commit_loss,
                               1.0 / (double(batch) * t * dim));
        // DEBUG: the full defining search of every (frame, stage) beside the fast path (not on a staged call: the checker follows
        // the index, which is -1 at dead stages)
        if (tuning().rvq_verify && q_used > 0 && !stages) {
            const size_t vlds = size_t(4) * (size_t(dim) + 4) * sizeof(float);
            if (vlds > 64 * 1024) return fail(AGX_ERR_UNSUPPORTED, "rvq_verify: D=%d too large for the checker", dim);
            hipLaunchKernelGGL(rvq_verify_kernel, dim3((unsigned)ceil_div64(n, 4)), dim3(256), vlds, st, x, x_sb, x_st, x_sd,
                               codebooks, packed, n, t, dim, k, q_used, index);
        }
        return check_launch("rvq_forward");
    };
    // codewords per pass = 8 waves x MT x 32.  MT = 4 (one pass for K = 1024) spills at the 256-VGPR cap
    // of 2 waves/SIMD (measured again with the operand ring: 903 us against 807), so K > 512 runs as passes of
    // 512 codewords with the running-bound candidate rule.
    if (k > 256)
        return tail_lds ? launch(rvq_forward_kernel<2, true>, rvq_forward_staged_kernel<2, true>)
                        : launch(rvq_forward_kernel<2, false>, rvq_forward_staged_kernel<2, false>);
    return tail_lds ? launch(rvq_forward_kernel<1, true>, rvq_forward_staged_kernel<1, true>)
                    : launch(rvq_forward_kernel<1, false>, rvq_forward_staged_kernel<1, false>);
}

int agx_rvq_dequantize(const float *codebook, const int64_t *idx, int64_t n, int32_t k, int32_t dim,
                       float *out, int64_t o_sn, int64_t o_sd, int32_t accumulate, void *stream) {
    using namespace agx;
    if (n <= 0 || k <= 0 || dim <= 0) return fail(AGX_ERR_BAD_SHAPE, "rvq_dequantize: bad shape");
    if (!codebook || !idx || !out) return fail(AGX_ERR_NULL_POINTER, "rvq_dequantize: NULL pointer");
    hipLaunchKernelGGL(rvq_dequant_kernel, dim3((unsigned)ceil_div64(n, 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), codebook, idx, n, k, dim, out, o_sn, o_sd, accumulate);
    return check_launch("rvq_dequantize");
}

size_t agx_rvq_ema_workspace_bytes(int64_t n_frames, int32_t dim, int32_t q_used) {
    if (n_frames <= 0 || dim <= 0 || q_used <= 0) return 0;
    return size_t(n_frames) * dim * q_used * sizeof(float);
}

int agx_rvq_ema_stats(const float *frames, const float *codebooks, const int64_t *index, float *stats, int64_t n_frames,
                      int32_t dim, int32_t k, int32_t q_used, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace agx;
    if (n_frames <= 0 || n_frames > INT32_MAX || dim <= 0 || k <= 0 || q_used <= 0 || q_used > 65535)
        return fail(AGX_ERR_BAD_SHAPE, "rvq_ema_stats: bad shape N=%lld D=%d K=%d Q=%d", (long long)n_frames, dim, k, q_used);
    if (dim > 1024) return fail(AGX_ERR_UNSUPPORTED, "rvq_ema_stats: D=%d > 1024", dim);
    if (!frames || !codebooks || !index || !stats || !workspace) return fail(AGX_ERR_NULL_POINTER, "rvq_ema_stats: NULL pointer");
    if (workspace_bytes < agx_rvq_ema_workspace_bytes(n_frames, dim, q_used))
        return fail(AGX_ERR_WORKSPACE, "rvq_ema_stats: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *R = static_cast<float *>(workspace);
    const int64_t total = n_frames * dim;
    hipLaunchKernelGGL(rvq_residuals_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(total, 256), 16384)), dim3(256), 0, st,
                       frames, codebooks, index, R, int(n_frames), dim, k, q_used);
    if (dim % 4 == 0)
        hipLaunchKernelGGL(rvq_ema_stats_kernel<true>, dim3(k, q_used), dim3(256), 0, st, R, index, stats, int(n_frames), dim, k,
                           q_used);
    else
        hipLaunchKernelGGL(rvq_ema_stats_kernel<false>, dim3(k, q_used), dim3(256), 0, st, R, index, stats, int(n_frames), dim,
                           k, q_used);
    return check_launch("rvq_ema_stats");
}

size_t agx_rvq_backward_workspace_bytes(int64_t n_frames, int32_t dim, int32_t q_used) {
    if (n_frames <= 0 || dim <= 0 || q_used <= 0) return 0;
    return size_t(n_frames) * dim * q_used * sizeof(float);
}

int agx_rvq_backward(const float *x, int64_t x_sb, int64_t x_st, int64_t x_sd, const float *codebooks, const int64_t *index,
                     const float *g_xq, int64_t g_sb, int64_t g_st, int64_t g_sd, const float *g_commit,
                     int32_t batch, int32_t t, int32_t dim, int32_t k, int32_t n_q, int32_t q_used,
                     float *dx, int64_t d_sb, int64_t d_st, int64_t d_sd, float *dcodebooks,
                     void *workspace, size_t workspace_bytes, void *stream) {
    return agx_rvq_backward_staged(x, x_sb, x_st, x_sd, codebooks, index, nullptr, g_xq, g_sb, g_st, g_sd, g_commit, batch, t, dim,
                                   k, n_q, q_used, dx, d_sb, d_st, d_sd, dcodebooks, workspace, workspace_bytes, stream);
}

// `stages` NULL: the unstaged dx kernel, exactly agx_rvq_backward.  The codebook kernel is the same launch either way.
int agx_rvq_backward_staged(const float *x, int64_t x_sb, int64_t x_st, int64_t x_sd, const float *codebooks,
                            const int64_t *index, const int64_t *stages, const float *g_xq, int64_t g_sb, int64_t g_st,
                            int64_t g_sd, const float *g_commit, int32_t batch, int32_t t, int32_t dim, int32_t k, int32_t n_q,
                            int32_t q_used, float *dx, int64_t d_sb, int64_t d_st, int64_t d_sd, float *dcodebooks,
                            void *workspace, size_t workspace_bytes, void *stream) {
    using namespace agx;
    const int64_t n = int64_t(batch) * t;
    if (batch <= 0 || t <= 0 || dim <= 0 || k <= 0 || n_q <= 0 || q_used < 0 || q_used > n_q || n > INT32_MAX)
        return fail(AGX_ERR_BAD_SHAPE, "rvq_backward: bad shape B=%d T=%d D=%d K=%d n_q=%d q_used=%d", batch, t, dim, k, n_q, q_used);
    if (dim > 1024) return fail(AGX_ERR_UNSUPPORTED, "rvq_backward: D=%d > 1024", dim);
    if (n_q > 64) return fail(AGX_ERR_UNSUPPORTED, "rvq_backward: at most 64 stages (n_q=%d)", n_q);
    const bool want_dc = dcodebooks != nullptr && q_used > 0;   // the S_q are kept only for the codebook kernel
    if (!x || !dx || (q_used > 0 && (!codebooks || !index)) || (want_dc && !workspace))
        return fail(AGX_ERR_NULL_POINTER, "rvq_backward: NULL pointer");
    if (want_dc && workspace_bytes < agx_rvq_backward_workspace_bytes(n, dim, q_used))
        return fail(AGX_ERR_WORKSPACE, "rvq_backward: workspace too small (%zu < %zu)", workspace_bytes,
                    agx_rvq_backward_workspace_bytes(n, dim, q_used));
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *S = want_dc ? static_cast<float *>(workspace) : nullptr;
    const float scale = float(2.0 / (double(n) * dim));
    RvqBwdArgs a{x, x_sb, x_st, x_sd, g_xq, g_sb, g_st, g_sd, dx, d_sb, d_st, d_sd, codebooks, index, g_commit, S,
                 int(n), t, dim, k, q_used, scale};
    const dim3 grid((unsigned)ceil_div64(n, BW_TF), (unsigned)ceil_div(dim, BW_TD));
    if (stages) {
        if (q_used <= 16)
            hipLaunchKernelGGL(rvq_bwd_dx_staged_kernel<16>, grid, dim3(256), 0, st, a, stages);
        else
            hipLaunchKernelGGL(rvq_bwd_dx_staged_kernel<64>, grid, dim3(256), 0, st, a, stages);
    } else if (q_used <= 16)
        hipLaunchKernelGGL(rvq_bwd_dx_kernel<16>, grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(rvq_bwd_dx_kernel<64>, grid, dim3(256), 0, st, a);
    if (dcodebooks) {
        if (dim % 4 == 0)
            hipLaunchKernelGGL(rvq_bwd_codebook_kernel<true>, dim3(k, n_q), dim3(256), 0, st, S, index, g_commit, scale,
                               dcodebooks, int(n), dim, k, q_used);
        else
            hipLaunchKernelGGL(rvq_bwd_codebook_kernel<false>, dim3(k, n_q), dim3(256), 0, st, S, index, g_commit, scale,
                               dcodebooks, int(n), dim, k, q_used);
    }
    return check_launch("rvq_backward");
}

}  // extern "C"
