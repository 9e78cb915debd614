// The convolution module of a Conformer block (networks/transformers.py:281-335): GLU, depthwise "same" convolution, BatchNorm
// and SiLU, forward and backward, and the stand-alone SiLU of its feed-forward halves.  fp32, channel-major contiguous
// (B, C, T), no atomics; every sum has one fixed order that depends on the shape alone.  With left = (K - 1) / 2:
//
//   g[b, c, t]  = u[b, c, t] * sigmoid(u[b, C + c, t])                  sigmoid(v) = 1 / (1 + expf(-v)), as agx_sigmoid_gate
//   z[b, c, t]  = bias[c] + sum_k w[c, k] g[b, c, t + k - left]         zeros outside [0, T); fma chain in increasing k from bias
//   a           = training ? ((z - mean) * rstd) * gamma + beta : z * scale + shift        rstd = 1 / sqrtf(var + eps)
//   y           = a * sigmoid(a)                                        scale = gamma * rstd, shift = beta - mean * scale
//
// g is never written to memory: the forward and the backward stage it in LDS from u, with its K - 1 halo.  An element is indexed,
// never addressed: the arithmetic and the order of every sum do not depend on how an operand is aligned.
//
// The causal form (agx.h: left = K - 1) is the same kernels with the other halo width, and it streams: hist (B, C, K - 1) holds the
// post-GLU values of the K - 1 frames before a call -- the one place g is written -- and the step kernel (7) and the history
// update (8) rewrite it in place.  Chunked calls are bit for bit the single call: an output's fma chain sees the same K operands.
#include "rowwise.hpp"

namespace {

using namespace agx;

constexpr int kTile = 1024;                       // output positions of a row one workgroup of the conv kernels takes
constexpr int kMaxK = AGX_CONFORMER_MAX_K;        // taps; the LDS images hold kTile + kMaxK - 1 floats

// Per-channel constants of the normalisation.
struct Norm {
    float mean, rstd, gamma, beta, scale, shift;
    int training;
};

__device__ inline Norm norm_of(const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean,
                               const float *__restrict__ var, float eps, int c, int training) {
    Norm n;
    n.mean = mean[c];
    n.rstd = 1.f / sqrtf(var[c] + eps);
    n.gamma = gamma[c];
    n.beta = beta[c];
    n.scale = n.gamma * n.rstd;
    n.shift = fmaf(-n.mean, n.scale, n.beta);
    n.training = training;
    return n;
}

__device__ inline float zhat_of(float z, const Norm &n) { return (z - n.mean) * n.rstd; }
__device__ inline float act_of(float z, const Norm &n) { return n.training ? fmaf(zhat_of(z, n), n.gamma, n.beta) : fmaf(z, n.scale, n.shift); }

// g of the positions [first, first + span) of row (b, c) into LDS, zeros outside [0, T).  HIST: before 0 the row's history
// instead, hr[t] with hr the end of its K - 1 floats -- the g of the frame t < 0 of an earlier call.
template <bool HIST>
__device__ inline void stage_glu(const float *__restrict__ ua, const float *__restrict__ ug, const float *__restrict__ hr, float *sg,
                                 int first, int span, int T) {
    for (int i = threadIdx.x; i < span; i += 256) {
        const int t = first + i;
        if (HIST && t < 0) sg[i] = hr[t];
        else sg[i] = (t >= 0 && t < T) ? ua[t] * sigmoidf(ug[t]) : 0.f;
    }
}

// Kernel 1.  One workgroup per (row, tile of kTile positions): g of the tile and its K - 1 halo goes to LDS, thread j takes the
// positions j, j + 256, ... of the tile.  EVAL: the normalisation on the running statistics and the SiLU are applied and only y is
// written.  CAUSAL: left = K - 1 instead of (K - 1) / 2, and the halo before 0 comes from hist (B, C, K - 1) where it is given.
template <bool EVAL, bool CAUSAL>
__global__ __launch_bounds__(256) void glu_dwconv_kernel(const float *__restrict__ u, const float *__restrict__ w,
                                                         const float *__restrict__ bias, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, const float *__restrict__ mean,
                                                         const float *__restrict__ var, float eps, const float *__restrict__ hist,
                                                         float *__restrict__ out, int C, int T, int K, int tiles) {
    __shared__ float sg[kTile + kMaxK - 1];
    const int64_t row = int64_t(blockIdx.x) / tiles;
    const int t0 = int(int64_t(blockIdx.x) - row * tiles) * kTile;
    const int b = int(row / C), c = int(row - int64_t(b) * C);
    const int n = T - t0 < kTile ? T - t0 : kTile, left = CAUSAL ? K - 1 : (K - 1) / 2;
    const float *ua = u + (int64_t(b) * 2 * C + c) * T, *ug = ua + int64_t(C) * T;
    if (CAUSAL && hist) stage_glu<true>(ua, ug, hist + (row + 1) * (K - 1), sg, t0 - left, n + K - 1, T);
    else stage_glu<false>(ua, ug, nullptr, sg, t0 - left, n + K - 1, T);
    __syncthreads();
    const float *wc = w + int64_t(c) * K;
    const float bc = bias[c];
    Norm nm{};
    if (EVAL) nm = norm_of(gamma, beta, mean, var, eps, c, 0);
    float *os = out + row * T + t0;
    for (int i = threadIdx.x; i < n; i += 256) {
        float z = bc;
        for (int k = 0; k < K; ++k) z = fmaf(wc[k], sg[i + k], z);
        os[i] = EVAL ? siluf(act_of(z, nm)) : z;
    }
}

// Kernel 2, stage 1.  One workgroup per (row, segment of kRedSeg floats): the segment's mean (sum / n, the sum in the order of
// block_sum over walkers that add their elements j, j + 256, ... in increasing order) and M2 = sum (z - mean)^2 about that
// mean, from the values held in registers: two passes, one read.
__global__ __launch_bounds__(256) void bn_stats_kernel(const float *__restrict__ z, float *__restrict__ partial, int T, int segs) {
    __shared__ float red[4];
    const int64_t row = int64_t(blockIdx.x) / segs;
    const int s0 = int(int64_t(blockIdx.x) - row * segs) * kRedSeg;
    const int n = T - s0 < kRedSeg ? T - s0 : kRedSeg;
    const float *zs = z + row * T + s0;
    float v[kRedSeg / 256], acc = 0.f;
#pragma unroll
    for (int j = 0; j < kRedSeg / 256; ++j) {
        const int i = threadIdx.x + 256 * j;
        v[j] = i < n ? zs[i] : 0.f;
        acc += v[j];
    }
    const float m = block_sum(acc, red) / float(n);
    acc = 0.f;
#pragma unroll
    for (int j = 0; j < kRedSeg / 256; ++j) {
        const float d = v[j] - m;
        if (threadIdx.x + 256 * j < n) acc = fmaf(d, d, acc);
    }
    const float m2 = block_sum(acc, red);
    if (threadIdx.x == 0) {
        partial[2 * int64_t(blockIdx.x)] = m;
        partial[2 * int64_t(blockIdx.x) + 1] = m2;
    }
}

// (n, mean, M2) of the union of two disjoint sets (Chan et al.); an empty side leaves the other as it is.
struct Moments {
    float n, mean, m2;
};
__device__ inline Moments merge(const Moments &a, const Moments &b) {
    if (b.n == 0.f) return a;
    if (a.n == 0.f) return b;
    Moments r;
    r.n = a.n + b.n;
    const float d = b.mean - a.mean, f = b.n / r.n;
    r.mean = fmaf(d, f, a.mean);
    r.m2 = (a.m2 + b.m2) + (d * d) * (a.n * f);
    return r;
}

// Kernel 2, stage 2.  One wavefront per channel.  The channel's partials are numbered p = b * segs + seg; lane l merges
// p = l, l + 64, ... in increasing order, then the lanes merge in a halving tree, the lower lane on the left.  Lane 0 writes the
// batch mean and the biased variance, and updates the running statistics with the unbiased one.
__global__ __launch_bounds__(64) void bn_stats_finish_kernel(const float *__restrict__ partial, float *__restrict__ mean,
                                                             float *__restrict__ var, float *running_mean, float *running_var,
                                                             int64_t *batches, float momentum, int C, int T, int segs,
                                                             int64_t count) {
    const int c = blockIdx.x, lane = threadIdx.x;
    Moments acc{0.f, 0.f, 0.f};
    for (int64_t p = lane; p < count; p += kWave) {
        const int64_t b = p / segs;
        const int seg = int(p - b * segs);
        const int64_t at = 2 * ((b * C + c) * segs + seg);
        const int n = T - seg * kRedSeg < kRedSeg ? T - seg * kRedSeg : kRedSeg;
        acc = merge(acc, Moments{float(n), partial[at], partial[at + 1]});
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        Moments other{__shfl_xor(acc.n, o, kWave), __shfl_xor(acc.mean, o, kWave), __shfl_xor(acc.m2, o, kWave)};
        acc = (lane & o) == 0 ? merge(acc, other) : merge(other, acc);
    }
    if (lane == 0) {
        mean[c] = acc.mean;
        var[c] = acc.m2 / acc.n;
        if (running_mean) running_mean[c] = fmaf(momentum, acc.mean - running_mean[c], running_mean[c]);
        if (running_var) running_var[c] = fmaf(momentum, acc.m2 / (acc.n - 1.f) - running_var[c], running_var[c]);
        if (batches && c == 0) *batches += 1;
    }
}

// Kernel 3 and the last stage of kernel 4, on the row walk (rowwise.hpp).  BWD == false: out = silu(a(z)).  BWD == true
// (training): out = dz = gamma rstd (da - sum da / N - zhat sum (da zhat) / N), d = dy, sums[2 c], sums[2 c + 1] the channel's two
// sums.  out may alias z (forward) or d (backward).
template <bool BWD>
__global__ __launch_bounds__(256) void bn_silu_walk_kernel(const float *z, const float *d, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, const float *__restrict__ mean,
                                                           const float *__restrict__ var, const float *__restrict__ sums, float eps,
                                                           float inv_count, float *out, int C, int64_t len, int64_t segs,
                                                           int64_t items, int training, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t item = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (item >= items) return;
    const int64_t row = item / segs, s0 = (item - row * segs) * kSeg;
    const int n = int(len - s0 < kSeg ? len - s0 : kSeg);
    const int c = int(row % C);
    const Norm nm = norm_of(gamma, beta, mean, var, eps, c, training);
    const float k1 = BWD ? sums[2 * c] * inv_count : 0.f, k2 = BWD ? sums[2 * c + 1] * inv_count : 0.f;
    const float *zs = z + row * len + s0, *ds = BWD ? d + row * len + s0 : nullptr;
    float *os = out + row * len + s0;
    row_walk<2, BWD>(row_split(zs, n, vec), zs, ds, os, n, lane, [&](float zv, float dv) {
        const float a = act_of(zv, nm);
        if (!BWD) return siluf(a);
        const float da = dv * silu_gradf(a);
        return nm.scale * fmaf(-zhat_of(zv, nm), k2, da - k1);
    });
}

// Kernel 4, stage 1.  One workgroup per (row, segment of kRedSeg floats): da = dy silu'(a), the partial sums of da and of
// da zhat (walker j takes the elements j, j + 256, ... in increasing order; block_sum), and with frozen statistics
// (training == 0) dz = da scale in the same pass.  dz may be NULL, or alias dy.
__global__ __launch_bounds__(256) void bn_silu_bwd_reduce_kernel(const float *dy, const float *__restrict__ z,
                                                                 const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                 const float *__restrict__ mean, const float *__restrict__ var,
                                                                 float eps, float *dz, float *__restrict__ partial, int C, int T,
                                                                 int segs, int training) {
    __shared__ float red[4];
    const int64_t row = int64_t(blockIdx.x) / segs;
    const int s0 = int(int64_t(blockIdx.x) - row * segs) * kRedSeg;
    const int n = T - s0 < kRedSeg ? T - s0 : kRedSeg;
    const Norm nm = norm_of(gamma, beta, mean, var, eps, int(row % C), training);
    const float *zs = z + row * T + s0, *ds = dy + row * T + s0;
    float *os = (dz && !training) ? dz + row * T + s0 : nullptr;
    float sb = 0.f, sgm = 0.f;
#pragma unroll 4
    for (int i = threadIdx.x; i < n; i += 256) {
        const float zv = zs[i];
        const float da = ds[i] * silu_gradf(act_of(zv, nm));
        if (os) os[i] = da * nm.scale;
        sb += da;
        sgm = fmaf(da, zhat_of(zv, nm), sgm);
    }
    sb = block_sum(sb, red);
    sgm = block_sum(sgm, red);
    if (threadIdx.x == 0) {
        partial[2 * int64_t(blockIdx.x)] = sb;
        partial[2 * int64_t(blockIdx.x) + 1] = sgm;
    }
}

// Kernel 4, stage 2.  One wavefront per channel: the channel finish order of channel_sum (rowwise.hpp), written out because both
// slots are added in one pass over p.  sums (2 C floats behind the partials) is what the training apply stage reads.
__global__ __launch_bounds__(64) void bn_silu_bwd_finish_kernel(const float *__restrict__ partial, float *__restrict__ sums,
                                                                float *__restrict__ dgamma, float *__restrict__ dbeta, int C,
                                                                int segs, int64_t count) {
    const int c = blockIdx.x;
    float sb = 0.f, sgm = 0.f;
    for (int64_t p = threadIdx.x; p < count; p += kWave) {
        const int64_t b = p / segs;
        const int64_t at = 2 * ((b * C + c) * segs + (p - b * segs));
        sb += partial[at];
        sgm += partial[at + 1];
    }
    sb = wave_sum(sb);
    sgm = wave_sum(sgm);
    if (threadIdx.x == 0) {
        sums[2 * c] = sb;
        sums[2 * c + 1] = sgm;
        if (dbeta) dbeta[c] = sb;
        if (dgamma) dgamma[c] = sgm;
    }
}

// Kernel 5, stage 1.  One workgroup per (row, tile of kTile positions).  g with its halo and dz with the mirrored halo go to LDS;
// thread j takes the positions j, j + 256, ... of the tile:
//   dg[t] = sum_k w[c, k] dz[t + left - k]   (fma chain in increasing k from 0)      du_a = dg s      du_gate = (dg a) (s (1 - s))
// PARAMS: the tile's share of dw[c, k] = sum_t dz[t] g[t + k - left] for every k, and of dbias[c] = sum_t dz[t] (slot K): walker
// sums in increasing t (fma), added in the workgroup order (rowwise.hpp), every slot behind the one barrier.
template <bool PARAMS, bool CAUSAL>
__global__ __launch_bounds__(256) void glu_dwconv_bwd_kernel(const float *__restrict__ dz, const float *__restrict__ u,
                                                             const float *__restrict__ w, float *__restrict__ du,
                                                             float *__restrict__ partial, int C, int T, int K, int tiles) {
    __shared__ float sg[kTile + kMaxK - 1], sd[kTile + kMaxK - 1];
    __shared__ float red[(kMaxK + 1) * 4];
    const int64_t row = int64_t(blockIdx.x) / tiles;
    const int t0 = int(int64_t(blockIdx.x) - row * tiles) * kTile;
    const int b = int(row / C), c = int(row - int64_t(b) * C);
    const int n = T - t0 < kTile ? T - t0 : kTile, left = CAUSAL ? K - 1 : (K - 1) / 2, right = K - 1 - left;
    const float *ua = u + (int64_t(b) * 2 * C + c) * T, *ug = ua + int64_t(C) * T, *dzr = dz + row * T;
    if (PARAMS) stage_glu<false>(ua, ug, nullptr, sg, t0 - left, n + K - 1, T);
    for (int i = threadIdx.x; i < n + K - 1; i += 256) {
        const int t = t0 - right + i;
        sd[i] = (t >= 0 && t < T) ? dzr[t] : 0.f;
    }
    __syncthreads();
    const float *wc = w + int64_t(c) * K;
    if (du) {
        float *da = du + (int64_t(b) * 2 * C + c) * T, *dgt = da + int64_t(C) * T;
        for (int i = threadIdx.x; i < n; i += 256) {
            float dg = 0.f;
            for (int k = 0; k < K; ++k) dg = fmaf(wc[k], sd[i + K - 1 - k], dg);
            const float a = ua[t0 + i], s = sigmoidf(ug[t0 + i]);
            da[t0 + i] = dg * s;
            dgt[t0 + i] = (dg * a) * (s * (1.f - s));
        }
    }
    if (PARAMS) {
        const int wv = threadIdx.x >> 6;
        for (int k = 0; k <= K; ++k) {
            float acc = 0.f;
            if (k < K) {
                for (int i = threadIdx.x; i < n; i += 256) acc = fmaf(sd[i + right], sg[i + k], acc);
            } else {
                for (int i = threadIdx.x; i < n; i += 256) acc += sd[i + right];
            }
            acc = wave_sum(acc);
            if ((threadIdx.x & 63) == 0) red[4 * k + wv] = acc;
        }
        __syncthreads();
        if (int(threadIdx.x) <= K) {
            const float *r = red + 4 * threadIdx.x;      // groups_sum (rowwise.hpp) written out: a call reorders the loop set-up
            partial[int64_t(blockIdx.x) * (K + 1) + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
        }
    }
}

// Kernel 5, stage 2.  One wavefront per channel, slot by slot: the channel finish order of channel_sum (rowwise.hpp) with tiles
// for segments, written out because a call moves the loop-invariant index arithmetic.
__global__ __launch_bounds__(64) void glu_dwconv_bwd_finish_kernel(const float *__restrict__ partial, float *__restrict__ dw,
                                                                   float *__restrict__ dbias, int C, int K, int tiles,
                                                                   int64_t count) {
    const int c = blockIdx.x;
    for (int k = 0; k <= K; ++k) {
        float acc = 0.f;
        for (int64_t p = threadIdx.x; p < count; p += kWave) {
            const int64_t b = p / tiles;
            acc += partial[((b * C + c) * tiles + (p - b * tiles)) * (K + 1) + k];
        }
        acc = wave_sum(acc);
        if (threadIdx.x == 0) {
            if (k < K) dw[int64_t(c) * K + k] = acc;
            else dbias[c] = acc;
        }
    }
}

// Kernel 6.  out = silu(x), or with d: out = d silu'(x).  out may alias x or d.
template <bool BWD>
__global__ __launch_bounds__(256) void silu_kernel(const float *x, const float *d, float *out, int64_t n, int vec) {
    int64_t i, stride, n4;
    flat_walk(n, vec, i, stride, n4);
    auto one = [](float xv, float dv) { return BWD ? dv * silu_gradf(xv) : siluf(xv); };
    for (int64_t q = i; q < n4; q += stride) {
        float4 v = reinterpret_cast<const float4 *>(x)[q];
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (BWD) g = reinterpret_cast<const float4 *>(d)[q];
        v.x = one(v.x, g.x);
        v.y = one(v.y, g.y);
        v.z = one(v.z, g.z);
        v.w = one(v.w, g.w);
        reinterpret_cast<float4 *>(out)[q] = v;
    }
    for (int64_t e = 4 * n4 + i; e < n; e += stride) out[e] = one(x[e], BWD ? d[e] : 0.f);
}

// i / d for 0 <= i < 2^15 and a quotient below 2^9, inv = 1.f / float(d), 1 <= d <= 64: the product is within 2^9 2^-22 of
// (i + 0.5) / d, which is at least 0.5 / 64 from an integer.  An integer division costs a latency-bound step a tenth of its time.
__device__ inline int quot(int i, float inv) { return int((float(i) + 0.5f) * inv); }

// Kernel 7, the streaming step: n <= kMaxStep new frames of every row, packed by output.  A workgroup owns R whole rows
// row0 .. row0 + R - 1 (R n <= 256) and keeps per row, in LDS, the image [hist (K - 1) | g of the chunk (n)] at an odd stride and
// the row's K taps at an odd stride: the three fills walk hist, u and w in address order, and with odd strides the 32 lanes of an
// LDS access group fall on 32 banks at n == 1, where neighbouring lanes are neighbouring rows.  After the one barrier thread e
// takes the output (row0 + e / n, e % n) -- the fma chain of kernel 1 on the same values, then the eval normalisation and SiLU --
// and the image's last K - 1 floats go back to hist.  rows = B C < 2^31: row arithmetic is 32-bit.  Every read of hist is before the barrier, every write behind it, and no
// other workgroup touches these rows.
//
// CNT, the counted form: batch entry b takes its first cnt = clamp(counts[b], 0, n) frames.  A workgroup holds rows of several
// batch entries, so the count is per thread and nobody returns early.  Outputs at t >= cnt are exact 0 (a select); the new history
// is the image's K - 1 floats from cnt on, the last K - 1 values of [hist | first cnt chunk values], and is not written at all
// where cnt == 0.  An output t < cnt and the new history read image columns below H + cnt only: what u holds past the count (NaN
// included) reaches neither.  The uncounted instance compiles the count out.
template <bool CNT>
__global__ __launch_bounds__(256) void glu_dwconv_step_kernel(const float *__restrict__ u, const float *__restrict__ w,
                                                              const float *__restrict__ bias, const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, const float *__restrict__ mean,
                                                              const float *__restrict__ var, float eps, float *hist,
                                                              float *__restrict__ out, const int64_t *__restrict__ counts, int C, int n,
                                                              int K, int R, int rows, float inv_n, float inv_h, float inv_k) {
    auto count_of = [&](unsigned row) {      // the frames the row's batch entry takes
        const int64_t cb = counts[row / unsigned(C)];
        return int(cb < 0 ? 0 : cb > n ? n : cb);
    };
    extern __shared__ float step_lds[];
    const int H = K - 1, stride = (H + n) | 1, wstride = K | 1;
    float *img = step_lds, *sw = step_lds + R * stride;
    const int row0 = int(blockIdx.x) * R;
    const int nr = rows - row0 < R ? rows - row0 : R;
    // this thread's output (R n <= 256: one each) and its channel's constants: their loads are in flight with the fills
    const int e = threadIdx.x;
    const bool mine = e < nr * n;
    int r = 0, t = 0, c = 0, cnt = n;
    float bc = 0.f;
    Norm nm{};
    if (mine) {
        r = quot(e, inv_n);
        t = e - r * n;
        const unsigned row = unsigned(row0 + r), b = row / unsigned(C);
        c = int(row - b * unsigned(C));
        if (CNT) cnt = count_of(row);
        bc = bias[c];
        nm = norm_of(gamma, beta, mean, var, eps, c, 0);
        const float *ua = u + (int64_t(b) * 2 * C + c) * n;
        img[r * stride + H + t] = ua[t] * sigmoidf(ua[int64_t(C) * n + t]);
    }
    // the walks of the history start at the third wavefront and the one of the taps at the second: where a workgroup holds few rows
    // (a small batch) the outputs, the taps and the history are the work of different wavefronts, side by side
    for (int i = (threadIdx.x + 128) & 255; i < nr * H; i += 256) {
        const int ri = quot(i, inv_h);
        img[ri * stride + (i - ri * H)] = hist[int64_t(row0) * H + i];
    }
    for (int i = (threadIdx.x + 192) & 255; i < nr * K; i += 256) {
        const int ri = quot(i, inv_k);
        sw[ri * wstride + (i - ri * K)] = w[int64_t(unsigned(row0 + ri) % unsigned(C)) * K + (i - ri * K)];
    }
    __syncthreads();
    for (int i = (threadIdx.x + 128) & 255; i < nr * H; i += 256) {
        const int ri = quot(i, inv_h);
        const int ci = CNT ? count_of(unsigned(row0 + ri)) : n;
        if (CNT && ci == 0) continue;
        hist[int64_t(row0) * H + i] = img[ri * stride + ci + (i - ri * H)];
    }
    if (mine) {
        const float *wc = sw + r * wstride, *sg = img + r * stride + t;
        float z = bc;
        for (int k = 0; k < K; ++k) z = fmaf(wc[k], sg[k], z);
        const float y = siluf(act_of(z, nm));
        out[int64_t(row0) * n + e] = CNT && t >= cnt ? 0.f : y;
    }
}

// Kernel 8.  hist <- the last K - 1 values of [hist | g of a chunk of T frames], K >= 2.  A workgroup owns R whole rows,
// R (K - 1) <= 256: thread e holds element (row0 + e / (K - 1), j = e % (K - 1)) of the new history in a register -- g[j + T - (K - 1)]
// from u, or where that frame lies before the chunk the old hist[j + T] -- then the barrier, then the write.
__global__ __launch_bounds__(256) void glu_hist_update_kernel(const float *__restrict__ u, float *hist, int C, int T, int K, int R,
                                                              int rows, float inv_h) {
    const int H = K - 1, e = threadIdx.x;
    const int row0 = int(blockIdx.x) * R;
    const int nr = rows - row0 < R ? rows - row0 : R;
    const bool mine = e < nr * H;
    float v = 0.f;
    if (mine) {
        const int r = quot(e, inv_h), t = e - r * H + T - H;
        const unsigned row = unsigned(row0 + r), b = row / unsigned(C);
        const float *ua = u + (int64_t(b) * 2 * C + (row - b * unsigned(C))) * T;
        v = t >= 0 ? ua[t] * sigmoidf(ua[int64_t(C) * T + t]) : hist[int64_t(row0) * H + e + T];
    }
    __syncthreads();
    if (mine) hist[int64_t(row0) * H + e] = v;
}

// The shape of every op but the two SiLU ones: rows and the workgroup counts of the three passes over them.
struct Shape {
    int64_t rows, tiles;            // rows = B C; conv tiles per row
    int64_t segs, red;              // reducing pass: segments per row, workgroups = (row, segment) partials
    int64_t wsegs, items, walk;     // row walk: segments per row, wavefront items, workgroups
};
enum ShapeFault { kShapeOk, kShapeDims, kShapeTaps, kShapeGrid };
// The computation.  The conv tiles are the finest of the three divisions of a row: within their grid, so are the other two.
inline ShapeFault shape_fault(int32_t B, int32_t C, int32_t T, int32_t K, Shape &s) {
    if (B <= 0 || C <= 0 || T <= 0) return kShapeDims;
    if (K < 1 || K > kMaxK) return kShapeTaps;
    s.rows = int64_t(B) * C;
    s.tiles = ceil_div64(T, kTile);
    if (s.tiles > kMaxGrid / s.rows) return kShapeGrid;
    s.red = reduce_blocks(s.rows, T, s.segs);
    s.walk = walk_blocks(s.rows, T, s.wsegs, s.items);
    return kShapeOk;
}
// ... and its refusals.  AGX_OK: s is valid.
inline int shape_of(const char *op, int32_t B, int32_t C, int32_t T, int32_t K, Shape &s) {
    switch (shape_fault(B, C, T, K, s)) {
    case kShapeDims: return fail(AGX_ERR_BAD_SHAPE, "%s: (B, C, T) = (%d, %d, %d)", op, B, C, T);
    case kShapeTaps: return fail(AGX_ERR_BAD_SHAPE, "%s: K = %d is outside [1, %d]", op, K, kMaxK);
    case kShapeGrid: return fail(AGX_ERR_BAD_SHAPE, "%s: (%d, %d, %d) exceeds the grid", op, B, C, T);
    default: return AGX_OK;
    }
}

}  // namespace

namespace {

// The "same" and the causal forward: the one tile kernel with its left halo width and, causal only, the history.
int glu_dwconv_forward(const char *op, const float *u, const float *w, const float *bias, const float *gamma, const float *beta,
                       const float *mean, const float *var, float eps, const float *hist, float *out, int32_t B, int32_t C, int32_t T,
                       int32_t K, bool causal, void *stream) {
    Shape s;
    if (const int rc = shape_of(op, B, C, T, K, s); rc != AGX_OK) return rc;
    if (!u || !w || !bias || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    const bool eval = gamma || beta || mean || var;
    if (eval && !(gamma && beta && mean && var))
        return fail(AGX_ERR_NULL_POINTER, "%s: gamma, beta, mean and var come together or not at all", op);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(unsigned(s.rows * s.tiles));
    auto kernel = eval ? (causal ? glu_dwconv_kernel<true, true> : glu_dwconv_kernel<true, false>)
                       : (causal ? glu_dwconv_kernel<false, true> : glu_dwconv_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, u, w, bias, gamma, beta, mean, var, eps, hist, out, C, T, K, int(s.tiles));
    return check_launch(op);
}

}  // namespace

int agx_glu_dwconv_forward(const float *u, const float *w, const float *bias, const float *gamma, const float *beta,
                           const float *mean, const float *var, float eps, float *out, int32_t B, int32_t C, int32_t T, int32_t K,
                           void *stream) {
    return glu_dwconv_forward("agx_glu_dwconv_forward", u, w, bias, gamma, beta, mean, var, eps, nullptr, out, B, C, T, K, false, stream);
}

int agx_glu_dwconv_causal_forward(const float *u, const float *w, const float *bias, const float *gamma, const float *beta,
                                  const float *mean, const float *var, float eps, const float *hist, float *out, int32_t B, int32_t C,
                                  int32_t T, int32_t K, void *stream) {
    return glu_dwconv_forward("agx_glu_dwconv_causal_forward", u, w, bias, gamma, beta, mean, var, eps, hist, out, B, C, T, K, true,
                              stream);
}

size_t agx_bn_stats_workspace_bytes(int32_t B, int32_t C, int32_t T) {
    Shape s;
    if (shape_fault(B, C, T, 1, s)) return 0;
    return size_t(2 * s.red) * sizeof(float);
}

int agx_bn_stats(const float *z, float *mean, float *var, float *running_mean, float *running_var, int64_t *num_batches_tracked,
                 float momentum, void *workspace, size_t workspace_bytes, int32_t B, int32_t C, int32_t T, void *stream) {
    Shape s;
    if (const int rc = shape_of("bn_stats", B, C, T, 1, s); rc != AGX_OK) return rc;
    if (int64_t(B) * T < 2)
        return fail(AGX_ERR_BAD_SHAPE, "bn_stats: B * T = %lld: batch statistics need more than one value per channel", (long long)B * T);
    if (!z || !mean || !var) return fail(AGX_ERR_NULL_POINTER, "bn_stats: NULL pointer");
    const size_t need = agx_bn_stats_workspace_bytes(B, C, T);
    if (!workspace || workspace_bytes < need)
        return fail(AGX_ERR_WORKSPACE, "bn_stats: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *partial = static_cast<float *>(workspace);
    hipLaunchKernelGGL(bn_stats_kernel, dim3(unsigned(s.red)), dim3(256), 0, st, z, partial, T, int(s.segs));
    if (const int rc = check_launch("agx_bn_stats"); rc != AGX_OK) return rc;
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(unsigned(C)), dim3(64), 0, st, static_cast<const float *>(partial), mean, var,
                       running_mean, running_var, num_batches_tracked, momentum, C, T, int(s.segs),
                       int64_t(B) * s.segs);
    return check_launch("agx_bn_stats");
}

int agx_bn_silu_forward(const float *z, const float *gamma, const float *beta, const float *mean, const float *var, float eps,
                        int32_t training, float *y, int32_t B, int32_t C, int32_t T, void *stream) {
    Shape s;
    if (const int rc = shape_of("bn_silu_forward", B, C, T, 1, s); rc != AGX_OK) return rc;
    if (!z || !gamma || !beta || !mean || !var || !y) return fail(AGX_ERR_NULL_POINTER, "bn_silu_forward: NULL pointer");
    hipLaunchKernelGGL(bn_silu_walk_kernel<false>, dim3(unsigned(s.walk)), dim3(256), 0, static_cast<hipStream_t>(stream), z,
                       static_cast<const float *>(nullptr), gamma, beta, mean, var, static_cast<const float *>(nullptr), eps, 0.f, y, C,
                       int64_t(T), s.wsegs, s.items, training != 0, int(same_phase16({z, y})));
    return check_launch("agx_bn_silu_forward");
}

size_t agx_bn_silu_backward_workspace_bytes(int32_t B, int32_t C, int32_t T) {
    Shape s;
    if (shape_fault(B, C, T, 1, s)) return 0;
    return size_t(2 * s.red + 2 * int64_t(C)) * sizeof(float);
}

int agx_bn_silu_backward(const float *dy, const float *z, const float *gamma, const float *beta, const float *mean, const float *var,
                         float eps, int32_t training, float *dz, float *dgamma, float *dbeta, void *workspace,
                         size_t workspace_bytes, int32_t B, int32_t C, int32_t T, void *stream) {
    Shape s;
    if (const int rc = shape_of("bn_silu_backward", B, C, T, 1, s); rc != AGX_OK) return rc;
    if (!dz && !dgamma && !dbeta) return AGX_OK;
    if (!dy || !z || !gamma || !beta || !mean || !var) return fail(AGX_ERR_NULL_POINTER, "bn_silu_backward: NULL pointer");
    const size_t need = agx_bn_silu_backward_workspace_bytes(B, C, T);
    if (!workspace || workspace_bytes < need)
        return fail(AGX_ERR_WORKSPACE, "bn_silu_backward: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *partial = static_cast<float *>(workspace), *sums = partial + 2 * s.red;
    hipLaunchKernelGGL(bn_silu_bwd_reduce_kernel, dim3(unsigned(s.red)), dim3(256), 0, st, dy, z, gamma, beta, mean, var, eps,
                       dz, partial, C, T, int(s.segs), training != 0);
    if (const int rc = check_launch("agx_bn_silu_backward"); rc != AGX_OK) return rc;
    hipLaunchKernelGGL(bn_silu_bwd_finish_kernel, dim3(unsigned(C)), dim3(64), 0, st, static_cast<const float *>(partial), sums, dgamma,
                       dbeta, C, int(s.segs), int64_t(B) * s.segs);
    if (const int rc = check_launch("agx_bn_silu_backward"); rc != AGX_OK || !training || !dz) return rc;
    hipLaunchKernelGGL(bn_silu_walk_kernel<true>, dim3(unsigned(s.walk)), dim3(256), 0, st, z, dy, gamma, beta, mean, var,
                       static_cast<const float *>(sums), eps, 1.f / (float(B) * float(T)), dz, C, int64_t(T), s.wsegs, s.items, 1,
                       int(same_phase16({z, dy, dz})));
    return check_launch("agx_bn_silu_backward");
}

size_t agx_glu_dwconv_backward_workspace_bytes(int32_t B, int32_t C, int32_t T, int32_t K) {
    Shape s;
    if (shape_fault(B, C, T, K, s)) return 0;
    return size_t(s.rows * s.tiles * (K + 1)) * sizeof(float);
}

namespace {

int glu_dwconv_backward(const char *op, const float *dz, const float *u, const float *w, float *du, float *dw, float *dbias,
                        void *workspace, size_t workspace_bytes, int32_t B, int32_t C, int32_t T, int32_t K, bool causal, void *stream) {
    Shape s;
    if (const int rc = shape_of(op, B, C, T, K, s); rc != AGX_OK) return rc;
    if (!du && !dw && !dbias) return AGX_OK;
    if ((dw == nullptr) != (dbias == nullptr)) return fail(AGX_ERR_NULL_POINTER, "%s: dw and dbias come together or not at all", op);
    if (!dz || !u || !w) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(unsigned(s.rows * s.tiles));
    if (!dw) {
        auto kernel = causal ? glu_dwconv_bwd_kernel<false, true> : glu_dwconv_bwd_kernel<false, false>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, dz, u, w, du, static_cast<float *>(nullptr), C, T, K, int(s.tiles));
        return check_launch(op);
    }
    const size_t need = agx_glu_dwconv_backward_workspace_bytes(B, C, T, K);
    if (!workspace || workspace_bytes < need) return fail(AGX_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", op, workspace_bytes, need);
    float *partial = static_cast<float *>(workspace);
    auto kernel = causal ? glu_dwconv_bwd_kernel<true, true> : glu_dwconv_bwd_kernel<true, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, dz, u, w, du, partial, C, T, K, int(s.tiles));
    if (const int rc = check_launch(op); rc != AGX_OK) return rc;
    hipLaunchKernelGGL(glu_dwconv_bwd_finish_kernel, dim3(unsigned(C)), dim3(64), 0, st, static_cast<const float *>(partial), dw, dbias,
                       C, K, int(s.tiles), int64_t(B) * s.tiles);
    return check_launch(op);
}

// Rows a workgroup of the step kernel owns: as many as fill its 256 threads with outputs, within kStepFloats of LDS -- and no
// more than leave kStepGrid workgroups: a step is bound by the latency of one workgroup's fills, not by bytes, so a small batch
// is spread over the compute units before it is packed.  A function of the shape alone.
constexpr int kMaxStep = AGX_CONFORMER_MAX_STEP;
constexpr int kStepFloats = 12288;
constexpr int kStepGrid = 1024;
inline int step_rows(int64_t rows, int n, int K) {
    const int per_row = ((K - 1 + n) | 1) + (K | 1);
    int64_t r = 256 / n;                                     // >= 4
    if (r > kStepFloats / per_row) r = kStepFloats / per_row;       // >= 64: per_row <= 127 + 65
    if (r > ceil_div64(rows, kStepGrid)) r = ceil_div64(rows, kStepGrid);
    return int(r);
}

}  // namespace

int agx_glu_dwconv_backward(const float *dz, const float *u, const float *w, float *du, float *dw, float *dbias, void *workspace,
                            size_t workspace_bytes, int32_t B, int32_t C, int32_t T, int32_t K, void *stream) {
    return glu_dwconv_backward("agx_glu_dwconv_backward", dz, u, w, du, dw, dbias, workspace, workspace_bytes, B, C, T, K, false, stream);
}

size_t agx_glu_dwconv_causal_backward_workspace_bytes(int32_t B, int32_t C, int32_t T, int32_t K) {
    return agx_glu_dwconv_backward_workspace_bytes(B, C, T, K);
}

int agx_glu_dwconv_causal_backward(const float *dz, const float *u, const float *w, float *du, float *dw, float *dbias, void *workspace,
                                   size_t workspace_bytes, int32_t B, int32_t C, int32_t T, int32_t K, void *stream) {
    return glu_dwconv_backward("agx_glu_dwconv_causal_backward", dz, u, w, du, dw, dbias, workspace, workspace_bytes, B, C, T, K, true,
                               stream);
}

static int glu_dwconv_step(const char *op, const float *u, const float *w, const float *bias, const float *gamma, const float *beta,
                           const float *mean, const float *var, float eps, float *hist, float *out, const int64_t *counts, int32_t B,
                           int32_t C, int32_t n, int32_t K, void *stream) {
    if (B <= 0 || C <= 0) return fail(AGX_ERR_BAD_SHAPE, "%s: (B, C) = (%d, %d)", op, B, C);
    if (n < 1 || n > kMaxStep) return fail(AGX_ERR_BAD_SHAPE, "%s: n = %d is outside [1, %d]", op, n, kMaxStep);
    if (K < 1 || K > kMaxK) return fail(AGX_ERR_BAD_SHAPE, "%s: K = %d is outside [1, %d]", op, K, kMaxK);
    const int64_t rows = int64_t(B) * C;
    if (rows > kMaxGrid) return fail(AGX_ERR_BAD_SHAPE, "%s: (%d, %d, %d) exceeds the grid", op, B, C, n);
    const int R = step_rows(rows, n, K);
    if (!u || !w || !bias || !gamma || !beta || !mean || !var || !out || (K > 1 && !hist))
        return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer (the step is the eval form: every statistic, and hist for K > 1)", op);
    const size_t lds = size_t(R) * (((K - 1 + n) | 1) + (K | 1)) * sizeof(float);
    const dim3 grid(unsigned(ceil_div64(rows, R)));
    const float inv_n = 1.f / float(n), inv_h = K > 1 ? 1.f / float(K - 1) : 0.f, inv_k = 1.f / float(K);
    if (counts)
        hipLaunchKernelGGL(glu_dwconv_step_kernel<true>, grid, dim3(256), lds, static_cast<hipStream_t>(stream), u, w, bias, gamma, beta,
                           mean, var, eps, hist, out, counts, C, n, K, R, int(rows), inv_n, inv_h, inv_k);
    else
        hipLaunchKernelGGL(glu_dwconv_step_kernel<false>, grid, dim3(256), lds, static_cast<hipStream_t>(stream), u, w, bias, gamma, beta,
                           mean, var, eps, hist, out, counts, C, n, K, R, int(rows), inv_n, inv_h, inv_k);
    return check_launch(op);
}

int agx_glu_dwconv_step(const float *u, const float *w, const float *bias, const float *gamma, const float *beta, const float *mean,
                        const float *var, float eps, float *hist, float *out, int32_t B, int32_t C, int32_t n, int32_t K, void *stream) {
    return glu_dwconv_step("glu_dwconv_step", u, w, bias, gamma, beta, mean, var, eps, hist, out, nullptr, B, C, n, K, stream);
}

int agx_glu_dwconv_step_counted(const float *u, const float *w, const float *bias, const float *gamma, const float *beta,
                                const float *mean, const float *var, float eps, float *hist, float *out, const int64_t *counts, int32_t B,
                                int32_t C, int32_t n, int32_t K, void *stream) {
    if (!counts) return fail(AGX_ERR_NULL_POINTER, "glu_dwconv_step_counted: NULL counts");
    return glu_dwconv_step("glu_dwconv_step_counted", u, w, bias, gamma, beta, mean, var, eps, hist, out, counts, B, C, n, K, stream);
}

int agx_glu_hist_update(const float *u, float *hist, int32_t B, int32_t C, int32_t T, int32_t K, void *stream) {
    Shape s;
    if (const int rc = shape_of("glu_hist_update", B, C, T, K, s); rc != AGX_OK) return rc;
    if (K == 1) return AGX_OK;
    if (!u || !hist) return fail(AGX_ERR_NULL_POINTER, "glu_hist_update: NULL pointer");
    const int R = 256 / (K - 1);                              // >= 4
    hipLaunchKernelGGL(glu_hist_update_kernel, dim3(unsigned(ceil_div64(s.rows, R))), dim3(256), 0, static_cast<hipStream_t>(stream), u,
                       hist, C, T, K, R, int(s.rows), 1.f / float(K - 1));
    return check_launch("agx_glu_hist_update");
}

int agx_silu(const float *x, float *out, int64_t n, void *stream) {
    if (n <= 0) return AGX_OK;
    if (!x || !out) return fail(AGX_ERR_NULL_POINTER, "silu: NULL pointer");
    hipLaunchKernelGGL(silu_kernel<false>, dim3(flat_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       static_cast<const float *>(nullptr), out, n, int(all_aligned16({x, out})));
    return check_launch("agx_silu");
}

int agx_silu_backward(const float *x, const float *dout, float *dx, int64_t n, void *stream) {
    if (n <= 0) return AGX_OK;
    if (!x || !dout || !dx) return fail(AGX_ERR_NULL_POINTER, "silu_backward: NULL pointer");
    hipLaunchKernelGGL(silu_kernel<true>, dim3(flat_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x, dout, dx, n,
                       int(all_aligned16({x, dout, dx})));
    return check_launch("agx_silu_backward");
}
