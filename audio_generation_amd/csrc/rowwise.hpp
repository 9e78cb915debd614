// The machinery of the HBM-bound "one value per channel, one pass over the row" kernels (conditioning.hip, snake.hip,
// conformer.hip, the small kernels of disc.hip, the parameter sums of wavelet.hip): the fixed orders of their sums, their two
// walks, and the host arithmetic of their grids.  Each is defined here once; the order of a sum is a contract tests hold bit for
// bit, so a kernel that needs one calls it, or says why it cannot.
#pragma once

#include "common.hpp"

#include <initializer_list>

namespace agx {

constexpr int kWave = 64;
constexpr int kSeg = 1024;          // floats of a row one wavefront of the row walk takes: 4 rounds of 64 lanes x 16 bytes
constexpr int kRedSeg = 2048;       // floats of a row one workgroup of a reducing pass takes: 8 per thread
constexpr int64_t kMaxGrid = 2147483647;

__device__ inline float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }
__device__ inline float siluf(float a) { return a * sigmoidf(a); }
// d silu / da = s (1 + a (1 - s)); s == 0 (a <= -89) gives exactly 0 and s == 1 (a >= 17) exactly 1
__device__ inline float silu_gradf(float a) {
    const float s = sigmoidf(a);
    return s * fmaf(a, 1.f - s, 1.f);
}

// ------------------------------------------------------------------ the orders
// Wave order.  Sum over the 64 lanes; lane 0 holds the halving tree ((p0 + p32) + (p16 + p48)) + ... of the lanes' values.
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// Workgroup order.  Sum over the 256 threads of a workgroup, the same value in every thread: the wave order per group of 64,
// the groups as (g0 + g1) + (g2 + g3).  red holds 4 floats.  The leading barrier keeps a call from overwriting red while a
// wavefront still reads the result of the call before it: back-to-back calls share red.
__device__ inline float block_sum(float v, float *red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);      // wave_sum, written out
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// The second half of the workgroup order, for a kernel that places its own barrier or puts several sums behind one: each group's
// lane 0 has left its wave_sum at r[group]; after the barrier this adds the four.
__device__ inline float groups_sum(const float *r) { return (r[0] + r[1]) + (r[2] + r[3]); }

// Channel finish order, one wavefront per channel c of C.  A first stage left S floats per (row, segment) at
// partial[((b C + c) segs + seg) S + k]; the channel's partials of slot k are numbered p = b * segs + seg, lane l adds
// p = l, l + 64, ... below count in increasing order, then the wave order: lane 0 returns the sum.
__device__ inline float channel_sum(const float *__restrict__ partial, int c, int C, int64_t segs, int S, int k, int64_t count) {
    float acc = 0.f;
    for (int64_t p = threadIdx.x; p < count; p += kWave) {
        const int64_t b = p / segs;
        acc += partial[((b * C + c) * segs + (p - b * segs)) * S + k];
    }
    return wave_sum(acc);
}

// ------------------------------------------------------------------ the walks
// Row walk.  One wavefront takes the n <= kSeg floats of a row segment at xs: scalar up to the first 16-byte boundary (head
// floats), float4 to the last whole quadruple (nvec of them), scalar from tail0 on.  vec == 0 (the operands differ in their
// address mod 16): all of it is head.
struct RowSplit {
    int head, nvec, tail0;
};
__device__ inline RowSplit row_split(const float *xs, int n, int vec) {
    int head = vec ? int((4 - ((reinterpret_cast<uintptr_t>(xs) >> 2) & 3)) & 3) : n;
    head = head < n ? head : n;
    const int nvec = (n - head) / 4;
    return {head, nvec, head + 4 * nvec};
}

// os[i] = one(xs[i], ds[i]) over the segment split as s (TWO == false: ds is not read, one's second argument is 0).  os may
// alias xs or ds: an element is read by the lane that writes it, before it writes.
template <int UNROLL, bool TWO, class F>
__device__ inline void row_walk(const RowSplit &s, const float *xs, const float *ds, float *os, int n, int lane, F one) {
    for (int i = lane; i < s.head; i += kWave) os[i] = one(xs[i], TWO ? ds[i] : 0.f);
#pragma unroll UNROLL
    for (int q = lane; q < s.nvec; q += kWave) {
        float4 v = *reinterpret_cast<const float4 *>(xs + s.head + 4 * q);
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (TWO) g = *reinterpret_cast<const float4 *>(ds + s.head + 4 * q);
        v.x = one(v.x, g.x);
        v.y = one(v.y, g.y);
        v.z = one(v.z, g.z);
        v.w = one(v.w, g.w);
        *reinterpret_cast<float4 *>(os + s.head + 4 * q) = v;
    }
    if (s.tail0 + lane < n) os[s.tail0 + lane] = one(xs[s.tail0 + lane], TWO ? ds[s.tail0 + lane] : 0.f);
}

// Flat walk.  n floats with no row structure, grid-strided by workgroups of 256: thread i takes the float4 q = i, i + stride, ...
// below n4 = n / 4 (vec == 0, an operand off a 16-byte boundary: none), then the elements e = 4 n4 + i, + stride, ... below n.
// Only the split is shared: a helper that runs the two loops moves the kernel's exit block behind them, and the address
// arithmetic of all four flat kernels comes out differently.
__device__ inline void flat_walk(int64_t n, int vec, int64_t &i, int64_t &stride, int64_t &n4) {
    i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    stride = int64_t(gridDim.x) * 256;
    n4 = vec ? n / 4 : 0;
}

// ------------------------------------------------------------------ host side
inline bool all_aligned16(std::initializer_list<const void *> ps) {
    for (const void *p : ps)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}

// Do the pointers agree mod 16?  Then the rows of a row walk reach their 16-byte boundaries together (its vec).
inline bool same_phase16(std::initializer_list<const void *> ps) {
    for (const void *p : ps)
        if ((reinterpret_cast<uintptr_t>(p) ^ reinterpret_cast<uintptr_t>(*ps.begin())) & 15) return false;
    return true;
}

// Workgroups of a flat walk.
inline unsigned flat_blocks(int64_t n) {
    const int64_t nb = ceil_div64(n, 1024);
    return unsigned(nb < 65536 ? nb : 65536);
}

// Workgroups of a row walk over rows > 0 rows of n floats (four wavefronts each, a wavefront per item), or -1 beyond the grid.
inline int64_t walk_blocks(int64_t rows, int64_t n, int64_t &segs, int64_t &items) {
    segs = ceil_div64(n, kSeg);
    if (segs > kMaxGrid * 4 / rows) return -1;
    items = rows * segs;
    return ceil_div64(items, 4);
}

// Workgroups of a reducing pass = (row, segment) partials of its workspace, or -1 beyond the grid.
inline int64_t reduce_blocks(int64_t rows, int64_t n, int64_t &segs) {
    segs = ceil_div64(n, kRedSeg);
    return segs > kMaxGrid / rows ? -1 : rows * segs;
}

}  // namespace agx
