// Code prior: the three operations that turn the cached Transformer into a model over the quantiser's codes.
//
//   codes -> input.   codes_embed_kernel: a gather-sum of one table row per stage, in stage order from 0, written channel-major.
//                     One launch for all stages; a workgroup takes 16 frames x 64 channels, gathers the row pieces with the
//                     channels across the lanes and turns the tile through LDS so that the stores run along the frames.
//   its backward.     Store-and-sum without atomics: embed_rows_kernel stores dout once as (F, D) rows, embed_index_kernel the
//                     index as int32 [Q][F] (frames behind a row's count and indices outside the table as -1); embed_sum_kernel
//                     gives destination (q, r) to one workgroup, which walks the stage's indices in frame order (a ballot over 64
//                     frames at a time) and adds the matching rows one after the other: ONE chain per output element, in frame
//                     order -- a fixed tree, bitwise reproducible.  A row nobody chose ends as the 0 it started as.
//   logits -> loss.   ce_forward_kernel: a workgroup takes 64 entries (b, t, q), lanes along t, so the reads strided by T coalesce;
//                     its four waves share the K axis, each an online max / sum over a quarter of k < sizes[q], merged in wave
//                     order.  Workgroup sums on a fixed LDS tree, then ce_finish_kernel over the workgroups' partials in a fixed
//                     order: two stages, no atomics.  ce_backward_kernel: the same map, a quarter of the channels per wave.
//   logits -> codes.  sample_kernel: one workgroup per (b, i, q).  The contract (include/agx.h "Code prior") orders the codes
//                     by (logit descending, k ascending) -- a bitonic sort of 64-bit keys in LDS --, takes the prefix sums of
//                     exp((l - l_max) / tau) in that order in binary64 (a workgroup scan), cuts at top_k / top_p and inverts the
//                     distribution at a Philox draw.  Every decision is a comparison of binary64 values.
#include "codes.hpp"
#include "philox.hpp"

// gather-sums and defining arithmetic: nothing here may be fused
#pragma clang fp contract(off)

namespace agx {

// ---------------------------------------------------------------------------------------------------------------- embed
constexpr int EMB_TI = 16;   // frames per tile
constexpr int EMB_DC = 64;   // channels per tile: one per lane

struct EmbedArgs {
    const float *tables;      // (Q, R, D)
    const int64_t *index;     // (B, n, Q)
    const int64_t *counts;    // (B,) or null
    float *out;               // (B, D, n)
    int n, Q, R, D, tiles_n;
};

// grid (B * tiles_n, ceil(D / 64)), 256 threads
__global__ __launch_bounds__(256) void codes_embed_kernel(EmbedArgs a) {
    __shared__ float tile[EMB_TI][EMB_DC + 1];
    __shared__ int rows[EMB_TI][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / a.tiles_n, i0 = (blockIdx.x % a.tiles_n) * EMB_TI, d0 = blockIdx.y * EMB_DC;
    const int cnt = row_clamp(a.counts, b, a.n);
    for (int e = tid; e < EMB_TI * a.Q; e += 256) {
        const int fi = e / a.Q, q = e % a.Q, i = i0 + fi;
        int r = -1;
        if (i < cnt) {                                     // cnt <= n: nothing behind the row's count or the tensor is read
            const int64_t x = a.index[(size_t(b) * a.n + i) * a.Q + q];
            if (x >= 0 && x < a.R) r = int(x);
        }
        rows[fi][q] = r;
    }
    __syncthreads();
    const int d = d0 + lane;
    for (int fi = wave; fi < EMB_TI; fi += 4) {
        float acc = 0.f;
        if (d < a.D)
            for (int q = 0; q < a.Q; ++q) {
                const int r = rows[fi][q];
                if (r >= 0) acc = acc + a.tables[(size_t(q) * a.R + size_t(r)) * a.D + d];
            }
        tile[fi][lane] = acc;
    }
    __syncthreads();
    for (int e = tid; e < EMB_TI * EMB_DC; e += 256) {
        const int fi = e % EMB_TI, dd = e / EMB_TI, i = i0 + fi, dc = d0 + dd;
        if (i < a.n && dc < a.D) a.out[(size_t(b) * a.D + dc) * a.n + i] = tile[fi][dd];
    }
}

// workspace of the backward: [rows: F x D float | idx: Q x F int32], the second part 8-byte aligned
struct EmbedBwdWs { size_t rows, idx, total; };
__host__ __device__ inline EmbedBwdWs embed_bwd_ws(int64_t F, int D, int Q) {
    EmbedBwdWs w;
    w.rows = 0;
    w.idx = (size_t(F) * size_t(D) * sizeof(float) + 7) & ~size_t(7);
    w.total = w.idx + ((size_t(F) * size_t(Q) * sizeof(int32_t) + 7) & ~size_t(7));
    return w;
}

// dout (B, D, n) -> rows (B n, D): grid (ceil(n / 32), ceil(D / 32), B), 256 threads
__global__ __launch_bounds__(256) void embed_rows_kernel(const float *__restrict__ dout, float *__restrict__ rows, int n, int D) {
    __shared__ float tile[32][33];
    const int tid = threadIdx.x, i0 = blockIdx.x * 32, d0 = blockIdx.y * 32, b = blockIdx.z;
    for (int e = tid; e < 1024; e += 256) {
        const int ii = e & 31, dd = e >> 5;
        if (i0 + ii < n && d0 + dd < D) tile[dd][ii] = dout[(size_t(b) * D + d0 + dd) * n + i0 + ii];
    }
    __syncthreads();
    for (int e = tid; e < 1024; e += 256) {
        const int dd = e & 31, ii = e >> 5;
        if (i0 + ii < n && d0 + dd < D) rows[(size_t(b) * n + i0 + ii) * D + d0 + dd] = tile[dd][ii];
    }
}

// index (B, n, Q) -> idx (Q, F) int32, -1 for what contributes nothing: one thread per (frame, stage)
__global__ __launch_bounds__(256) void embed_index_kernel(const int64_t *__restrict__ index, const int64_t *__restrict__ counts,
                                                          int32_t *__restrict__ idx, int64_t F, int n, int Q, int R) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= F * Q) return;
    const int64_t f = e / Q;
    const int q = int(e % Q), b = int(f / n), i = int(f % n);
    const int64_t x = index[e];
    idx[size_t(q) * size_t(F) + size_t(f)] = i < row_clamp(counts, b, n) && x >= 0 && x < R ? int32_t(x) : int32_t(-1);
}

// destination (q, r): grid (R, Q), 256 threads; thread t owns channels t + 256 j.  Every wave walks the same frames.
__global__ __launch_bounds__(256) void embed_sum_kernel(const float *__restrict__ rows, const int32_t *__restrict__ idx,
                                                        float *__restrict__ dtables, int64_t F, int R, int D) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int r = blockIdx.x, q = blockIdx.y;
    const int32_t *ix = idx + size_t(q) * size_t(F);
    float *dst = dtables + (size_t(q) * R + size_t(r)) * D;
    for (int dbase = 0; dbase < D; dbase += 1024) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int64_t f0 = 0; f0 < F; f0 += 64) {
            const int64_t f = f0 + lane;
            const int32_t v = f < F ? ix[f] : -1;
            unsigned long long m = __ballot(v == r);
            while (m) {                                    // the matching frames of these 64, in ascending order
                const int g0 = __ffsll((long long)m) - 1;
                m &= m - 1;
                const float *row0 = rows + size_t(f0 + g0) * D + dbase;
                if (m) {                                   // two rows in flight; the additions keep the frame order
                    const int g1 = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const float *row1 = rows + size_t(f0 + g1) * D + dbase;
                    float v0[4], v1[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int d = tid + 256 * j;
                        v0[j] = dbase + d < D ? row0[d] : 0.f;
                        v1[j] = dbase + d < D ? row1[d] : 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = (acc[j] + v0[j]) + v1[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int d = tid + 256 * j;
                        if (dbase + d < D) acc[j] = acc[j] + row0[d];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = dbase + tid + 256 * j;
            if (d < D) dst[d] = acc[j];
        }
    }
}

// -------------------------------------------------------------------------------------------------------- cross-entropy
struct CeArgs {
    const float *logits;      // (B, Q K, T)
    const int64_t *target;    // (B, T, Q)
    int64_t E;                // B T Q
    int T, Q, K;
    StageSizes sizes;
};

// entry e of the thread map: t fastest, then q, then b
__device__ __forceinline__ void ce_entry(const CeArgs &a, int64_t e, int &b, int &t, int &q) {
    t = int(e % a.T);
    const int64_t r = e / a.T;
    q = int(r % a.Q);
    b = int(r / a.Q);
}

// one step of the online logsumexp: the running maximum m and the sum s of exp(l - m) take the logit x
__device__ __forceinline__ void ce_take(float x, float &m, float &s) {
    if (x > m) {
        s = (m == -1.0f / 0.0f ? 0.f : s * expf(m - x)) + 1.f;
        m = x;
    } else if (x == x && m != -1.0f / 0.0f) {
        s = s + expf(x - m);
    } else if (x != x) {
        s = x;                                            // a NaN logit makes the loss NaN: visible, not hidden
    }
}

// The online logsumexp of l_k0 .. l_{k1-1} (stride T) in index order, into (m, s).  Eight loads are issued before their eight
// steps, so a thread keeps eight rows of the strided column in flight; the order of the steps is that of the plain loop.
__device__ __forceinline__ void ce_lse_part(const float *__restrict__ l, int k0, int k1, int64_t stride, float &m, float &s) {
    m = -1.0f / 0.0f, s = 0.f;
    int k = k0;
    for (; k + 8 <= k1; k += 8) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = l[(k + j) * stride];
#pragma unroll
        for (int j = 0; j < 8; ++j) ce_take(x[j], m, s);
    }
    for (; k < k1; ++k) ce_take(l[k * stride], m, s);
}

constexpr int CE_SPLIT = 4;      // waves of a workgroup that share the K axis of its 64 entries
constexpr int CE_ENTRIES = 64;   // entries per workgroup: one per lane

// grid ceil(E / 64), 256 threads: lane = entry, wave w takes the w-th quarter of k < sizes[q]; the four (m, s) pairs meet in
// LDS and are merged in wave order (a fixed order).  part[blockIdx] = this workgroup's sum of nll, pcnt[blockIdx] = its live entries.
__global__ __launch_bounds__(256) void ce_forward_kernel(CeArgs a, float *__restrict__ nll, float *__restrict__ lse,
                                                         double *__restrict__ part, int64_t *__restrict__ pcnt) {
    __shared__ float pm[CE_SPLIT][CE_ENTRIES], ps[CE_SPLIT][CE_ENTRIES];
    __shared__ double ssum[CE_ENTRIES];
    __shared__ int scnt[CE_ENTRIES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t e = int64_t(blockIdx.x) * CE_ENTRIES + lane;
    int b = 0, t = 0, q = 0, size = 0;
    int64_t y = -1;
    size_t at = 0;
    const float *col = a.logits;
    bool live = false;
    if (e < a.E) {
        ce_entry(a, e, b, t, q);
        at = (size_t(b) * a.T + t) * a.Q + q;
        y = a.target[at];
        size = a.sizes.n[q];
        live = y >= 0 && y < size;
        col = a.logits + (size_t(b) * a.Q * a.K + size_t(q) * a.K) * a.T + t;
    }
    float m = -1.0f / 0.0f, s = 0.f;
    if (live) {
        const int chunk = (size + CE_SPLIT - 1) / CE_SPLIT, k0 = wave * chunk, k1 = k0 + chunk < size ? k0 + chunk : size;
        ce_lse_part(col, k0 < size ? k0 : size, k1, a.T, m, s);
    }
    pm[wave][lane] = m;
    ps[wave][lane] = s;
    __syncthreads();
    if (wave == 0) {
        float mine = 0.f, l = 0.f;
        if (live) {
            for (int w = 1; w < CE_SPLIT; ++w) {           // (m, s) takes the part of wave w: both sums scaled to the larger maximum
                const float m2 = pm[w][lane], s2 = ps[w][lane];
                if (s2 != s2) {
                    s = s2;
                } else if (m2 != -1.0f / 0.0f) {
                    const float big = m2 > m ? m2 : m;
                    s = (m == -1.0f / 0.0f ? 0.f : s * expf(m - big)) + s2 * expf(m2 - big);
                    m = big;
                }
            }
            l = m + logf(s);
            mine = l - col[y * int64_t(a.T)];
        }
        if (e < a.E) {
            nll[at] = mine;
            lse[at] = l;
        }
        ssum[lane] = double(mine);
        scnt[lane] = live ? 1 : 0;
    }
    __syncthreads();
    for (int off = CE_ENTRIES / 2; off > 0; off >>= 1) {
        if (tid < off) {
            ssum[tid] = ssum[tid] + ssum[tid + off];
            scnt[tid] += scnt[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[blockIdx.x] = ssum[0];
        pcnt[blockIdx.x] = scnt[0];
    }
}

// one workgroup: thread t sums partials t, t + 256, .. in ascending order, then the same tree
__global__ __launch_bounds__(256) void ce_finish_kernel(const double *__restrict__ part, const int64_t *__restrict__ pcnt, int nparts,
                                                        float *__restrict__ loss, int64_t *__restrict__ n_live) {
    __shared__ double ssum[256];
    __shared__ long long scnt[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    long long c = 0;
    for (int j = tid; j < nparts; j += 256) {
        s = s + part[j];
        c += pcnt[j];
    }
    ssum[tid] = s;
    scnt[tid] = c;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            ssum[tid] = ssum[tid] + ssum[tid + off];
            scnt[tid] += scnt[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        *n_live = scnt[0];
        *loss = scnt[0] > 0 ? float(ssum[0] / double(scnt[0])) : 0.f;
    }
}

// the thread map of the forward, wave w writing the w-th quarter of the K channels of (b, q) at frame t: every channel is written,
// k >= sizes[q] and dead entries as exact 0
__global__ __launch_bounds__(256) void ce_backward_kernel(CeArgs a, const float *__restrict__ lse, const int64_t *__restrict__ n_live,
                                                          const float *__restrict__ g, float *__restrict__ dlogits) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t e = int64_t(blockIdx.x) * CE_ENTRIES + lane;
    if (e >= a.E) return;
    int b, t, q;
    ce_entry(a, e, b, t, q);
    const size_t at = (size_t(b) * a.T + t) * a.Q + q;
    const int64_t y = a.target[at];
    const int size = a.sizes.n[q];
    const int64_t live_n = *n_live;
    const size_t col = (size_t(b) * a.Q * a.K + size_t(q) * a.K) * a.T + t;
    const int chunk = (a.K + CE_SPLIT - 1) / CE_SPLIT, k1 = (wave + 1) * chunk < a.K ? (wave + 1) * chunk : a.K;
    int k = wave * chunk;
    if (y >= 0 && y < size && live_n > 0) {
        const float coef = *g / float(live_n), l = lse[at];
        const int ke = k1 < size ? k1 : size;              // the live channels of this quarter end here
        for (; k + 4 <= ke; k += 4) {                      // four loads in flight, as in the forward
            float x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = a.logits[col + size_t(k + j) * a.T];
#pragma unroll
            for (int j = 0; j < 4; ++j) dlogits[col + size_t(k + j) * a.T] = coef * (expf(x[j] - l) - (k + j == y ? 1.f : 0.f));
        }
        for (; k < ke; ++k) {
            const float p = expf(a.logits[col + size_t(k) * a.T] - l);
            dlogits[col + size_t(k) * a.T] = coef * (p - (k == y ? 1.f : 0.f));
        }
    }
    for (; k < k1; ++k) dlogits[col + size_t(k) * a.T] = 0.f;
}

// --------------------------------------------------------------------------------------------------------------- sample
constexpr int SAMPLE_MAX_K = AGX_CODES_SAMPLE_MAX_K;
constexpr int SAMPLE_PER = SAMPLE_MAX_K / 256;     // elements per thread of the scan

struct SampleArgs {
    const float *logits;        // (B, Q K, n)
    const int64_t *seeds, *frame0;
    const float *temperature;
    const int64_t *top_k;
    const float *top_p;
    const int64_t *counts, *stages;   // or null
    int64_t *carry;             // (B, Q) or null
    int64_t *codes;             // (B, n, Q)
    int n, Q, K;
    StageSizes sizes;
};

// sum over the workgroup of one int per thread (integers: any order gives the same sum)
__device__ __forceinline__ int sample_block_sum(int v, int *slot) {
    __syncthreads();
    if (threadIdx.x == 0) *slot = 0;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) atomicAdd(slot, v);
    __syncthreads();
    return *slot;
}

// grid (B n Q), 256 threads
__global__ __launch_bounds__(256) void sample_kernel(SampleArgs a) {
    __shared__ unsigned long long key[SAMPLE_MAX_K];
    __shared__ double cum[SAMPLE_MAX_K];
    __shared__ double wsum[4];
    __shared__ int slot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x % a.Q;
    const int64_t f_in = blockIdx.x / a.Q;
    const int b = int(f_in / a.n), i = int(f_in % a.n);
    const int cnt = row_clamp(a.counts, b, a.n), qb = row_clamp(a.stages, b, a.Q);
    const bool live = i < cnt && q < qb;
    int64_t *code_out = a.codes + (size_t(b) * a.n + i) * a.Q + q;
    int64_t *carry_out = a.carry && i == cnt - 1 ? a.carry + size_t(b) * a.Q + q : nullptr;
    if (!live) {
        if (tid == 0) {
            *code_out = -1;
            if (carry_out) *carry_out = -1;
        }
        return;
    }
    const int size = a.sizes.n[q];
    const float *col = a.logits + (size_t(b) * a.Q * a.K + size_t(q) * a.K) * a.n + i;
    const float tau_f = a.temperature[b];
    int P = 2;
    while (P < size) P <<= 1;
    for (int k = tid; k < P; k += 256) key[k] = k < size ? code_key(col[size_t(k) * a.n], k) : ~0ull;
    __syncthreads();
    int code;
    if (!(tau_f > 0.f)) {
        // greedy: the least key, by every thread over its own stride, then over the workgroup through LDS
        unsigned long long best = ~0ull;
        for (int k = tid; k < P; k += 256) best = key[k] < best ? key[k] : best;
        unsigned long long *wbest = reinterpret_cast<unsigned long long *>(cum);
        best = wave_min_key(best);
        if (lane == 0) wbest[wave] = best;
        best = block_min_key(best, wbest);
        code = int(unsigned(best));
    } else {
        // (l descending, k ascending): bitonic sort of the P keys
        for (int k2 = 2; k2 <= P; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < P / 2; t += 256) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
                    const unsigned long long x = key[lo], y = key[hi];
                    if ((x > y) == ((lo & k2) == 0)) key[lo] = y, key[hi] = x;
                }
                __syncthreads();
            }
        const int64_t tk = a.top_k[b];
        const int kept0 = tk > 0 && tk < size ? int(tk) : size;
        const double tau = double(tau_f);
        const double zmax = double(code_key_logit(key[0])) / tau;
        // prefix sums of e_j = exp(z_j - z_max) over the first kept0 codes of the order: SAMPLE_PER consecutive per thread,
        // then the threads' totals over the wave and the waves' over LDS
        double e[SAMPLE_PER], run = 0.0;
#pragma unroll
        for (int u = 0; u < SAMPLE_PER; ++u) {
            const int j = tid * SAMPLE_PER + u;
            double v = 0.0;
            if (j < kept0) {
                const double z = double(code_key_logit(key[j])) / tau;
                v = z == zmax ? 1.0 : exp(z - zmax);
            }
            run = run + v;
            e[u] = run;
        }
        double incl = run;
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_up(incl, off);
            if (lane >= off) incl = incl + o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        double base = incl - run;
        for (int w = 0; w < wave; ++w) base = base + wsum[w];
#pragma unroll
        for (int u = 0; u < SAMPLE_PER; ++u) cum[tid * SAMPLE_PER + u] = base + e[u];
        __syncthreads();
        const double c_all = cum[kept0 - 1];
        int kept = kept0;
        const double tp = double(a.top_p[b]);
        if (tp < 1.0) {
            // the shortest prefix with C_j / C_all >= top_p: C ascends, so its length is 1 + the count of C_j / C_all < top_p
            int below = 0;
            for (int j = tid; j < kept0; j += 256) below += cum[j] / c_all < tp ? 1 : 0;
            below = sample_block_sum(below, &slot);
            kept = below + 1 < kept0 ? below + 1 : kept0;
        }
        const double c_kept = cum[kept - 1];
        const int64_t f = a.frame0[b] + i;
        const uint64_t seed = uint64_t(a.seeds[b]);
        uint32_t w[4];
        philox4x32_10(uint32_t(uint64_t(f)), uint32_t(uint64_t(f) >> 32), uint32_t(q), AGX_CODES_SAMPLE_STREAM, uint32_t(seed),
                      uint32_t(seed >> 32), w);
        const double thr = ((double(w[0]) + 0.5) * (1.0 / 4294967296.0)) * c_kept;
        // the first j of the kept prefix with C_j >= u C_kept: the count of C_j < u C_kept, and never past the prefix
        int before = 0;
        for (int j = tid; j < kept; j += 256) before += cum[j] < thr ? 1 : 0;
        before = sample_block_sum(before, &slot);
        const int j = before < kept ? before : kept - 1;
        code = int(unsigned(key[j]));
    }
    if (code < 0 || code >= size) code = 0;               // NaN logits, NaN settings: unspecified, but in bounds
    if (tid == 0) {
        *code_out = code;
        if (carry_out) *carry_out = code;
    }
}

}  // namespace agx

extern "C" {

int agx_codes_embed(const float *tables, const int64_t *index, const int64_t *counts, float *out, int32_t batch, int32_t n, int32_t n_q,
                    int32_t rows, int32_t dim, void *stream) {
    using namespace agx;
    if (batch <= 0 || n <= 0 || n_q <= 0 || rows <= 0 || dim <= 0)
        return fail(AGX_ERR_BAD_SHAPE, "codes_embed: bad shape B=%d n=%d Q=%d R=%d D=%d", batch, n, n_q, rows, dim);
    if (n_q > 64) return fail(AGX_ERR_UNSUPPORTED, "codes_embed: at most 64 stages (Q=%d)", n_q);
    const int tiles_n = ceil_div(n, EMB_TI);
    if (int64_t(batch) * tiles_n > 0x7fffffff || ceil_div(dim, EMB_DC) > 65535)
        return fail(AGX_ERR_UNSUPPORTED, "codes_embed: B ceil(n / 16) = %lld exceeds 2^31 - 1 or D = %d exceeds 64 * 65535",
                    (long long)batch * tiles_n, dim);
    if (!tables || !index || !out) return fail(AGX_ERR_NULL_POINTER, "codes_embed: NULL pointer");
    EmbedArgs a{tables, index, counts, out, n, n_q, rows, dim, tiles_n};
    hipLaunchKernelGGL(codes_embed_kernel, dim3(unsigned(batch * tiles_n), unsigned(ceil_div(dim, EMB_DC))), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return check_launch("codes_embed");
}

size_t agx_codes_embed_backward_workspace_bytes(int32_t batch, int32_t n, int32_t n_q, int32_t dim) {
    if (batch <= 0 || n <= 0 || n_q <= 0 || dim <= 0) return 0;
    return agx::embed_bwd_ws(int64_t(batch) * n, dim, n_q).total;
}

int agx_codes_embed_backward(const float *dout, const int64_t *index, const int64_t *counts, float *dtables, int32_t batch, int32_t n,
                             int32_t n_q, int32_t rows, int32_t dim, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace agx;
    if (batch <= 0 || n <= 0 || n_q <= 0 || rows <= 0 || dim <= 0)
        return fail(AGX_ERR_BAD_SHAPE, "codes_embed_backward: bad shape B=%d n=%d Q=%d R=%d D=%d", batch, n, n_q, rows, dim);
    if (n_q > 64) return fail(AGX_ERR_UNSUPPORTED, "codes_embed_backward: at most 64 stages (Q=%d)", n_q);
    const int64_t F = int64_t(batch) * n;
    if (F > 0x7fffffff || F * n_q > (int64_t(1) << 38) || batch > 65535 || ceil_div(dim, 32) > 65535)
        return fail(AGX_ERR_UNSUPPORTED, "codes_embed_backward: B n = %lld frames exceed 2^31 - 1 (or B > 65535, D > 32 * 65535)", (long long)F);
    if (!dout || !index || !dtables) return fail(AGX_ERR_NULL_POINTER, "codes_embed_backward: NULL pointer");
    const EmbedBwdWs map = embed_bwd_ws(F, dim, n_q);
    if (!workspace || workspace_bytes < map.total)
        return fail(AGX_ERR_WORKSPACE, "codes_embed_backward: workspace too small (%zu < %zu)", workspace_bytes, map.total);
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(AGX_ERR_BAD_SHAPE, "codes_embed_backward: the workspace is not 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *rws = reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + map.rows);
    int32_t *idx = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(workspace) + map.idx);
    hipLaunchKernelGGL(embed_rows_kernel, dim3(unsigned(ceil_div(n, 32)), unsigned(ceil_div(dim, 32)), unsigned(batch)), dim3(256), 0, st,
                       dout, rws, n, dim);
    hipLaunchKernelGGL(embed_index_kernel, dim3(unsigned(ceil_div64(F * n_q, 256))), dim3(256), 0, st, index, counts, idx, F, n, n_q, rows);
    hipLaunchKernelGGL(embed_sum_kernel, dim3(unsigned(rows), unsigned(n_q)), dim3(256), 0, st, rws, idx, dtables, F, rows, dim);
    return check_launch("codes_embed_backward");
}

static int ce_shape(const char *what, const int32_t *sizes, int32_t batch, int32_t t, int32_t n_q, int32_t k, agx::StageSizes *sz) {
    using namespace agx;
    if (batch <= 0 || t <= 0 || n_q <= 0 || k <= 0) return fail(AGX_ERR_BAD_SHAPE, "%s: bad shape B=%d T=%d Q=%d K=%d", what, batch, t, n_q, k);
    if (int rc = stage_sizes(what, sizes, n_q, k, sz)) return rc;
    if (int64_t(batch) * t * n_q > (int64_t(1) << 36))
        return fail(AGX_ERR_UNSUPPORTED, "%s: B T Q = %lld entries exceed 2^36", what, (long long)batch * t * n_q);
    return AGX_OK;
}

size_t agx_codes_cross_entropy_workspace_bytes(int32_t batch, int32_t t, int32_t n_q) {
    if (batch <= 0 || t <= 0 || n_q <= 0) return 0;
    return size_t(agx::ceil_div64(int64_t(batch) * t * n_q, agx::CE_ENTRIES)) * 16;
}

int agx_codes_cross_entropy(const float *logits, const int64_t *target, const int32_t *sizes, int32_t batch, int32_t t, int32_t n_q,
                            int32_t k, float *nll, float *lse, float *loss, int64_t *n_live, void *workspace, size_t workspace_bytes,
                            void *stream) {
    using namespace agx;
    StageSizes sz;
    if (int rc = ce_shape("codes_cross_entropy", sizes, batch, t, n_q, k, &sz)) return rc;
    if (!logits || !target || !nll || !lse || !loss || !n_live) return fail(AGX_ERR_NULL_POINTER, "codes_cross_entropy: NULL pointer");
    const int64_t E = int64_t(batch) * t * n_q, nparts = ceil_div64(E, CE_ENTRIES);
    if (!workspace || workspace_bytes < size_t(nparts) * 16)
        return fail(AGX_ERR_WORKSPACE, "codes_cross_entropy: workspace too small (%zu < %zu)", workspace_bytes, size_t(nparts) * 16);
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(AGX_ERR_BAD_SHAPE, "codes_cross_entropy: the workspace is not 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *part = static_cast<double *>(workspace);
    int64_t *pcnt = reinterpret_cast<int64_t *>(part + nparts);
    CeArgs a{logits, target, E, t, n_q, k, sz};
    hipLaunchKernelGGL(ce_forward_kernel, dim3(unsigned(nparts)), dim3(256), 0, st, a, nll, lse, part, pcnt);
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(256), 0, st, part, pcnt, int(nparts), loss, n_live);
    return check_launch("codes_cross_entropy");
}

int agx_codes_cross_entropy_backward(const float *logits, const int64_t *target, const int32_t *sizes, const float *lse,
                                     const int64_t *n_live, const float *g, int32_t batch, int32_t t, int32_t n_q, int32_t k,
                                     float *dlogits, void *stream) {
    using namespace agx;
    StageSizes sz;
    if (int rc = ce_shape("codes_cross_entropy_backward", sizes, batch, t, n_q, k, &sz)) return rc;
    if (!logits || !target || !lse || !n_live || !g || !dlogits) return fail(AGX_ERR_NULL_POINTER, "codes_cross_entropy_backward: NULL pointer");
    const int64_t E = int64_t(batch) * t * n_q;
    CeArgs a{logits, target, E, t, n_q, k, sz};
    hipLaunchKernelGGL(ce_backward_kernel, dim3(unsigned(ceil_div64(E, CE_ENTRIES))), dim3(256), 0, static_cast<hipStream_t>(stream), a, lse,
                       n_live, g, dlogits);
    return check_launch("codes_cross_entropy_backward");
}

int agx_codes_sample(const float *logits, const int32_t *sizes, const int64_t *seeds, const int64_t *frame0, const float *temperature,
                     const int64_t *top_k, const float *top_p, const int64_t *counts, const int64_t *stages, int64_t *carry,
                     int64_t *codes, int32_t batch, int32_t n, int32_t n_q, int32_t k, void *stream) {
    using namespace agx;
    if (batch <= 0 || n <= 0 || n_q <= 0 || k <= 0) return fail(AGX_ERR_BAD_SHAPE, "codes_sample: bad shape B=%d n=%d Q=%d K=%d", batch, n, n_q, k);
    if (k > AGX_CODES_SAMPLE_MAX_K)
        return fail(AGX_ERR_UNSUPPORTED, "codes_sample: K=%d exceeds %d codes per stage (the order and the prefix sums of a stage live in LDS)",
                    k, AGX_CODES_SAMPLE_MAX_K);
    StageSizes sz;
    if (int rc = stage_sizes("codes_sample", sizes, n_q, k, &sz)) return rc;
    if (int64_t(batch) * n * n_q > 0x7fffffff)
        return fail(AGX_ERR_UNSUPPORTED, "codes_sample: B n Q = %lld rows exceed 2^31 - 1", (long long)batch * n * n_q);
    if (!logits || !seeds || !frame0 || !temperature || !top_k || !top_p || !codes) return fail(AGX_ERR_NULL_POINTER, "codes_sample: NULL pointer");
    SampleArgs a{logits, seeds, frame0, temperature, top_k, top_p, counts, stages, carry, codes, n, n_q, k, sz};
    hipLaunchKernelGGL(sample_kernel, dim3(unsigned(batch * n * n_q)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("codes_sample");
}

}  // extern "C"
