// Snake activations (networks/utils.py:44-105): Snek and SnekReLU, forward and backward.  fp32, no atomics; the sum behind
// dalpha has one fixed order that depends on (rows, channels, n) alone.  x is rows = B * C contiguous rows of n floats, the
// channel of a row is row % channels, and channels == 1 is one alpha for every row.
//
//   inv = 1 / (alpha[c] + eps)   (once per row)       theta = alpha[c] * x        (s, c) = sincosf(theta)
//   out = (relu ? max(x, 0) : x) + inv * s^2
//   dx  = dout * ((relu ? x >= 0 : 1) + alpha[c] * inv * 2 s c)
//   dalpha[c] = sum dout * inv * (x * 2 s c - inv * s^2)
//
// The sine is OCML's sincosf: one range reduction per element, sin^2 = s * s and sin 2 theta = 2 * (s * c) from its two
// results.  Its large-argument path has no data-dependent loop, so Inf and NaN cost what a large finite argument costs.
#include "common.hpp"

namespace {

using agx::ceil_div64;
using agx::check_launch;
using agx::fail;

constexpr int kWave = 64;
constexpr int kSeg = 1024;          // floats of a row one wavefront of the element-wise walk takes: 4 rounds of 64 lanes x 16 bytes
constexpr int kRedSeg = 2048;       // floats of a row one workgroup of the reducing backward takes: 8 per thread
constexpr int64_t kMaxGrid = 2147483647;

// Sum over the 64 lanes; lane 0 holds the halving tree ((p0 + p32) + (p16 + p48)) + ... of the lanes' values.
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

struct Row {
    float a, inv, ainv;     // alpha, 1 / (alpha + eps), alpha * inv
    int relu;
};

__device__ inline Row row_of(const float *__restrict__ alpha, int64_t row, int channels, int variant, float eps) {
    Row r;
    r.a = alpha[row % channels];
    r.inv = 1.f / (r.a + eps);
    r.ainv = r.a * r.inv;
    r.relu = variant;
    return r;
}

// Every fused multiply-add is written out, and nothing else has the shape a * b + c: the bits of out and dx do not depend on
// which kernel evaluates them.
__device__ inline float snake_fwd_one(float x, const Row &r) {
    float s, c;
    sincosf(r.a * x, &s, &c);
    return fmaf(r.inv, s * s, r.relu ? fmaxf(x, 0.f) : x);
}

// dx / dout of one element; with TERM the element's share of dalpha / dout as well.
template <bool TERM>
__device__ inline float snake_bwd_one(float x, const Row &r, float &term) {
    float s, c;
    sincosf(r.a * x, &s, &c);
    const float sin2 = 2.f * (s * c);
    if (TERM) term = r.inv * fmaf(x, sin2, -(r.inv * (s * s)));
    return fmaf(r.ainv, sin2, (r.relu && !(x >= 0.f)) ? 0.f : 1.f);
}

// The walk of film_apply_kernel<CT>: one wavefront takes kSeg floats of a row, scalar up to the first 16-byte boundary, float4
// to the last whole quadruple, scalar tail.  BWD == false: out = snake(x).  BWD == true: out = dx, d = dout (frozen alphas).
// out may alias x (forward) or d (backward): an element is read by the lane that writes it, before it writes.
template <bool BWD>
__global__ __launch_bounds__(256) void snake_walk_kernel(const float *x, const float *d, const float *__restrict__ alpha, float *out,
                                                         int channels, int64_t len, int64_t segs, int64_t items, int variant,
                                                         float eps, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t item = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (item >= items) return;
    const int64_t row = item / segs, s0 = (item - row * segs) * kSeg;
    const int n = int(len - s0 < kSeg ? len - s0 : kSeg);
    const Row r = row_of(alpha, row, channels, variant, eps);
    const float *xs = x + row * len + s0, *ds = BWD ? d + row * len + s0 : nullptr;
    float *os = out + row * len + s0;
    int head = vec ? int((4 - ((reinterpret_cast<uintptr_t>(xs) >> 2) & 3)) & 3) : n;
    head = head < n ? head : n;
    const int nvec = (n - head) / 4, tail0 = head + 4 * nvec;
    float unused;
    auto one = [&](float xv, float dv) { return BWD ? dv * snake_bwd_one<false>(xv, r, unused) : snake_fwd_one(xv, r); };
    for (int i = lane; i < head; i += kWave) os[i] = one(xs[i], BWD ? ds[i] : 0.f);      // all of it where vec == 0
#pragma unroll 2
    for (int q = lane; q < nvec; q += kWave) {
        float4 v = *reinterpret_cast<const float4 *>(xs + head + 4 * q);
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (BWD) g = *reinterpret_cast<const float4 *>(ds + head + 4 * q);
        v.x = one(v.x, g.x);
        v.y = one(v.y, g.y);
        v.z = one(v.z, g.z);
        v.w = one(v.w, g.w);
        *reinterpret_cast<float4 *>(os + head + 4 * q) = v;
    }
    if (tail0 + lane < n) os[tail0 + lane] = one(xs[tail0 + lane], BWD ? ds[tail0 + lane] : 0.f);
}

// Stage 1 of dalpha, with dx in the same pass: one workgroup per (row, segment of kRedSeg floats).  Walker j of 256 takes the
// segment's elements j, j + 256, ... in increasing order (fma of dout and the element's term); the walkers of a group of 64 are
// added in the halving tree of wave_sum, the groups as (g0 + g1) + (g2 + g3).  The walk is by index, never by address: the
// order does not depend on how the operands are aligned.  dx may be NULL, or alias dout.
__global__ __launch_bounds__(256) void snake_bwd_reduce_kernel(const float *__restrict__ x, const float *__restrict__ alpha,
                                                               const float *dout, float *dx, float *__restrict__ partial,
                                                               int channels, int64_t len, int64_t segs, int variant, float eps) {
    __shared__ float red[4];
    const int64_t row = int64_t(blockIdx.x) / segs, s0 = (int64_t(blockIdx.x) - row * segs) * kRedSeg;
    const int n = int(len - s0 < kRedSeg ? len - s0 : kRedSeg);
    const Row r = row_of(alpha, row, channels, variant, eps);
    const float *xs = x + row * len + s0, *ds = dout + row * len + s0;
    float *os = dx ? dx + row * len + s0 : nullptr;
    float acc = 0.f;
#pragma unroll 4
    for (int i = threadIdx.x; i < n; i += 256) {
        const float dv = ds[i];
        float term;
        const float g = snake_bwd_one<true>(xs[i], r, term);
        if (os) os[i] = dv * g;
        acc = fmaf(dv, term, acc);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Stage 2: one wavefront per channel.  The channel's partials are numbered p = b * segs + seg over its rows b * channels + c;
// lane l adds p = l, l + 64, ... in increasing order, then the halving tree.
__global__ __launch_bounds__(64) void snake_bwd_finish_kernel(const float *__restrict__ partial, float *__restrict__ dalpha,
                                                              int channels, int64_t segs, int64_t count) {
    const int c = blockIdx.x;
    float acc = 0.f;
    for (int64_t p = threadIdx.x; p < count; p += kWave) {
        const int64_t b = p / segs;
        acc += partial[(b * channels + c) * segs + (p - b * segs)];
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) dalpha[c] = acc;
}

// AGX_OK with go == false: nothing to do.  Otherwise the shape is valid.
inline int snake_shape(const char *op, int64_t rows, int32_t channels, int64_t n, int32_t variant, bool &go) {
    go = false;
    if (variant != AGX_SNAKE_PLAIN && variant != AGX_SNAKE_RELU)
        return fail(AGX_ERR_BAD_SHAPE, "%s: variant = %d is neither AGX_SNAKE_PLAIN nor AGX_SNAKE_RELU", op, variant);
    if (channels <= 0) return fail(AGX_ERR_BAD_SHAPE, "%s: channels = %d", op, channels);
    if (rows <= 0 || n <= 0) return AGX_OK;
    if (rows % channels != 0)
        return fail(AGX_ERR_BAD_SHAPE, "%s: rows = %lld is no multiple of channels = %d", op, (long long)rows, channels);
    go = true;
    return AGX_OK;
}

// Workgroups of the element-wise walk, or -1 beyond the grid.
inline int64_t walk_blocks(int64_t rows, int64_t n, int64_t &segs, int64_t &items) {
    segs = ceil_div64(n, kSeg);
    if (segs > kMaxGrid * 4 / rows) return -1;
    items = rows * segs;
    return ceil_div64(items, 4);
}

// Workgroups of the reducing backward = floats of its workspace, or -1 beyond the grid.
inline int64_t reduce_blocks(int64_t rows, int64_t n, int64_t &segs) {
    segs = ceil_div64(n, kRedSeg);
    return segs > kMaxGrid / rows ? -1 : rows * segs;
}

}  // namespace

int agx_snake_forward(const float *x, const float *alpha, float *out, int64_t rows, int32_t channels, int64_t n, int32_t variant,
                      float eps, void *stream) {
    bool go;
    if (const int rc = snake_shape("snake_forward", rows, channels, n, variant, go); rc != AGX_OK || !go) return rc;
    if (!x || !alpha || !out) return fail(AGX_ERR_NULL_POINTER, "snake_forward: NULL pointer");
    int64_t segs, items;
    const int64_t blocks = walk_blocks(rows, n, segs, items);
    if (blocks < 0) return fail(AGX_ERR_BAD_SHAPE, "snake_forward: (%lld, %lld) exceeds the grid", (long long)rows, (long long)n);
    const int vec = ((reinterpret_cast<uintptr_t>(x) ^ reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    hipLaunchKernelGGL(snake_walk_kernel<false>, dim3(unsigned(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       static_cast<const float *>(nullptr), alpha, out, channels, n, segs, items, variant, eps, vec);
    return check_launch("agx_snake_forward");
}

size_t agx_snake_backward_workspace_bytes(int64_t rows, int32_t channels, int64_t n) {
    if (rows <= 0 || n <= 0 || channels <= 0 || rows % channels != 0) return 0;
    int64_t segs;
    const int64_t blocks = reduce_blocks(rows, n, segs);
    return blocks < 0 ? 0 : size_t(blocks) * sizeof(float);
}

int agx_snake_backward(const float *x, const float *alpha, const float *dout, float *dx, float *dalpha, void *workspace,
                       size_t workspace_bytes, int64_t rows, int32_t channels, int64_t n, int32_t variant, float eps,
                       void *stream) {
    bool go;
    if (const int rc = snake_shape("snake_backward", rows, channels, n, variant, go); rc != AGX_OK || !go) return rc;
    if (!dx && !dalpha) return AGX_OK;
    if (!x || !alpha || !dout) return fail(AGX_ERR_NULL_POINTER, "snake_backward: NULL pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!dalpha) {       // frozen alphas: the element-wise walk, no workspace, no reduction
        int64_t segs, items;
        const int64_t blocks = walk_blocks(rows, n, segs, items);
        if (blocks < 0) return fail(AGX_ERR_BAD_SHAPE, "snake_backward: (%lld, %lld) exceeds the grid", (long long)rows, (long long)n);
        const uintptr_t px = reinterpret_cast<uintptr_t>(x), pd = reinterpret_cast<uintptr_t>(dout), po = reinterpret_cast<uintptr_t>(dx);
        const int vec = (((px ^ pd) | (px ^ po)) & 15) == 0;
        hipLaunchKernelGGL(snake_walk_kernel<true>, dim3(unsigned(blocks)), dim3(256), 0, st, x, dout, alpha, dx, channels, n, segs,
                           items, variant, eps, vec);
        return check_launch("agx_snake_backward");
    }
    int64_t segs;
    const int64_t blocks = reduce_blocks(rows, n, segs);
    if (blocks < 0) return fail(AGX_ERR_BAD_SHAPE, "snake_backward: (%lld, %lld) exceeds the grid", (long long)rows, (long long)n);
    if (!workspace || workspace_bytes < size_t(blocks) * sizeof(float))
        return fail(AGX_ERR_WORKSPACE, "snake_backward: workspace of %zu bytes, %zu needed", workspace_bytes, size_t(blocks) * sizeof(float));
    float *partial = static_cast<float *>(workspace);
    hipLaunchKernelGGL(snake_bwd_reduce_kernel, dim3(unsigned(blocks)), dim3(256), 0, st, x, alpha, dout, dx, partial, channels, n, segs,
                       variant, eps);
    if (const int rc = check_launch("agx_snake_backward"); rc != AGX_OK) return rc;
    hipLaunchKernelGGL(snake_bwd_finish_kernel, dim3(unsigned(channels)), dim3(64), 0, st, static_cast<const float *>(partial), dalpha,
                       channels, segs, (rows / channels) * segs);
    return check_launch("agx_snake_backward");
}
