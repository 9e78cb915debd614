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
#include "rowwise.hpp"

namespace {

using namespace agx;

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

// The row walk (rowwise.hpp).  BWD == false: out = snake(x).  BWD == true: out = dx, d = dout (frozen alphas).  out may alias x
// (forward) or d (backward).
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
    float unused;
    row_walk<2, BWD>(row_split(xs, n, vec), xs, ds, os, n, lane,
                     [&](float xv, float dv) { return BWD ? dv * snake_bwd_one<false>(xv, r, unused) : snake_fwd_one(xv, r); });
}

// Stage 1 of dalpha, with dx in the same pass: one workgroup per (row, segment of kRedSeg floats).  Walker j of 256 takes the
// segment's elements j, j + 256, ... in increasing order (fma of dout and the element's term); the walkers are added in the
// workgroup order (rowwise.hpp).  The walk is by index, never by address: the order does not depend on how the operands are
// aligned.  dx may be NULL, or alias dout.
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
    if (threadIdx.x == 0) partial[blockIdx.x] = groups_sum(red);
}

// Stage 2: one wavefront per channel, the channel finish order (rowwise.hpp) over its rows b * channels + c.
__global__ __launch_bounds__(64) void snake_bwd_finish_kernel(const float *__restrict__ partial, float *__restrict__ dalpha,
                                                              int channels, int64_t segs, int64_t count) {
    const int c = blockIdx.x;
    const float acc = channel_sum(partial, c, channels, segs, 1, 0, count);
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

}  // namespace

int agx_snake_forward(const float *x, const float *alpha, float *out, int64_t rows, int32_t channels, int64_t n, int32_t variant,
                      float eps, void *stream) {
    bool go;
    if (const int rc = snake_shape("snake_forward", rows, channels, n, variant, go); rc != AGX_OK || !go) return rc;
    if (!x || !alpha || !out) return fail(AGX_ERR_NULL_POINTER, "snake_forward: NULL pointer");
    int64_t segs, items;
    const int64_t blocks = walk_blocks(rows, n, segs, items);
    if (blocks < 0) return fail(AGX_ERR_BAD_SHAPE, "snake_forward: (%lld, %lld) exceeds the grid", (long long)rows, (long long)n);
    const int vec = same_phase16({x, out});
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
        const int vec = same_phase16({x, dout, dx});
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
