// Conditioning on a vector (networks/conditioning.py): the FiLM projections, scale-and-shift and their backward, and the sigmoid
// gate of SqueezeExcite with its backward.  All of it is memory-bound fp32 with no atomics; every sum has one fixed order.
#include "rowwise.hpp"

namespace {

using namespace agx;

// One wavefront per output (b, r).
__global__ __launch_bounds__(256) void film_params_kernel(const float *__restrict__ cond, const float *__restrict__ w,
                                                          const float *__restrict__ bias, float *__restrict__ gb,
                                                          int64_t n_out, int D, int R) {
    const int lane = threadIdx.x & 63;
    const int64_t o = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (o >= n_out) return;          // the whole wavefront
    const int64_t b = o / R;
    const int r = int(o - b * R);
    const float *c = cond + b * D, *wr = w + int64_t(r) * D;
    float acc = 0.f;
    for (int d = lane; d < D; d += kWave) acc = fmaf(c[d], wr[d], acc);
    acc = wave_sum(acc);
    if (lane == 0) gb[o] = acc + (bias ? bias[r] : 0.f);
}

template <bool BETA>
__device__ inline float film_one(float x, float g, float b) {
    return BETA ? fmaf(x, g, b) : x * g;
}

// A "slab" is what shares one alignment: the T floats of a (b, c) row (CT) or the T * C floats of a batch row (TC).  One
// wavefront takes kSeg floats of a slab: CT on the row walk (rowwise.hpp), TC on the same split with a channel that moves.
template <int LAYOUT, bool BETA>
__global__ __launch_bounds__(256) void film_apply_kernel(const float *x, const float *__restrict__ gb, float *out, int C,
                                                         int64_t len, int64_t segs, int64_t items, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t item = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (item >= items) return;
    const int64_t slab = item / segs, s0 = (item - slab * segs) * kSeg;
    const int n = int(len - s0 < kSeg ? len - s0 : kSeg);
    const int R = BETA ? 2 * C : C;
    const float *xs = x + slab * len + s0;
    float *os = out + slab * len + s0;
    const RowSplit sp = row_split(xs, n, vec);
    if (LAYOUT == AGX_FILM_CT) {
        const int64_t b = slab / C;
        const int c = int(slab - b * C);
        const float g = gb[b * R + c], be = BETA ? gb[b * R + C + c] : 0.f;
        row_walk<4, false>(sp, xs, nullptr, os, n, lane, [&](float xv, float) { return film_one<BETA>(xv, g, be); });
    } else {
        const int head = sp.head, nvec = sp.nvec, tail0 = sp.tail0;
        const float *gam = gb + slab * R, *bet = gam + C;    // bet is read with BETA only
        for (int i = lane; i < head; i += kWave) {      // all of it where vec == 0
            const int c = int((s0 + i) % C);
            os[i] = film_one<BETA>(xs[i], gam[c], BETA ? bet[c] : 0.f);
        }
        int c0 = int((s0 + head + 4 * lane) % C);
        const int step = (4 * kWave) % C;
#pragma unroll 4
        for (int q = lane; q < nvec; q += kWave) {
            float4 v = *reinterpret_cast<const float4 *>(xs + head + 4 * q);
            float e[4] = {v.x, v.y, v.z, v.w};
            int c = c0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                e[k] = film_one<BETA>(e[k], gam[c], BETA ? bet[c] : 0.f);
                c = c + 1 == C ? 0 : c + 1;
            }
            *reinterpret_cast<float4 *>(os + head + 4 * q) = make_float4(e[0], e[1], e[2], e[3]);
            c0 += step;
            c0 = c0 >= C ? c0 - C : c0;
        }
        if (tail0 + lane < n) {
            const int c = int((s0 + tail0 + lane) % C);
            os[tail0 + lane] = film_one<BETA>(xs[tail0 + lane], gam[c], BETA ? bet[c] : 0.f);
        }
    }
}

// The reduction order of one (b, c), shared by the two backward kernels: walker j of 256 takes t = j, j + 256, ... in
// increasing order; the walkers are added in the workgroup order (rowwise.hpp).

// CT: one workgroup per (b, c) row, thread j is walker j.
template <bool BETA>
__global__ __launch_bounds__(256) void film_bwd_ct_kernel(const float *__restrict__ x, const float *__restrict__ gb,
                                                          const float *__restrict__ dout, float *__restrict__ dx,
                                                          float *__restrict__ dgb, int C, int T) {
    __shared__ float red[2][4];
    const int64_t row = blockIdx.x, b = row / C;
    const int c = int(row - b * C), R = BETA ? 2 * C : C;
    const float g = gb[b * R + c];
    const float *xr = x + row * T, *dr = dout + row * T;
    float *dxr = dx + row * T;
    float a = 0.f, s = 0.f;
#pragma unroll 4
    for (int t = threadIdx.x; t < T; t += 256) {
        const float d = dr[t], xv = xr[t];
        dxr[t] = d * g;
        a = fmaf(d, xv, a);
        if (BETA) s += d;
    }
    a = wave_sum(a);
    if (BETA) s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        dgb[b * R + c] = groups_sum(red[0]);
        if (BETA) dgb[b * R + C + c] = groups_sum(red[1]);
    }
}

// TC: one workgroup per (b, 64 channels).  A lane is a channel, wavefront g holds the 64 walkers 64 g .. 64 g + 63 of its
// channels in registers and walks t = 64 g + m + 256 i: every load is one coalesced channel-fastest row.  The workgroup order
// (rowwise.hpp) is written out here: the 64 walkers of a group are registers of one lane, not lanes.
template <bool BETA>
__global__ __launch_bounds__(256) void film_bwd_tc_kernel(const float *__restrict__ x, const float *__restrict__ gb,
                                                          const float *__restrict__ dout, float *__restrict__ dx,
                                                          float *__restrict__ dgb, int C, int T, int ctiles) {
    __shared__ float red[2][4][kWave];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t b = blockIdx.x / ctiles;
    const int c = int(blockIdx.x - b * ctiles) * kWave + lane, R = BETA ? 2 * C : C;
    const bool on = c < C;
    const float gam = on ? gb[b * R + c] : 0.f;
    const int64_t base = b * T * C + c;
    float a[kWave], s[kWave];
#pragma unroll
    for (int m = 0; m < kWave; ++m) a[m] = s[m] = 0.f;
    for (int t0 = kWave * g; t0 < T; t0 += 256) {
#pragma unroll
        for (int m = 0; m < kWave; ++m) {
            if (on && t0 + m < T) {
                const int64_t i = base + int64_t(t0 + m) * C;
                const float d = dout[i], xv = x[i];
                dx[i] = d * gam;
                a[m] = fmaf(d, xv, a[m]);
                if (BETA) s[m] += d;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int m = 0; m < o; ++m) {
            a[m] += a[m + o];
            if (BETA) s[m] += s[m + o];
        }
    }
    red[0][g][lane] = a[0];
    red[1][g][lane] = s[0];
    __syncthreads();
    if (g == 0 && on) {
        dgb[b * R + c] = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
        if (BETA) dgb[b * R + C + c] = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
    }
}

// One thread per element of dw (R, D), then dbias (R), then dcond (B, D) when asked for.
__global__ __launch_bounds__(256) void film_params_bwd_kernel(const float *__restrict__ cond, const float *__restrict__ w,
                                                              const float *__restrict__ dgb, float *__restrict__ dw,
                                                              float *__restrict__ dbias, float *__restrict__ dcond, int B,
                                                              int D, int R, int64_t total) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x, rd = int64_t(R) * D;
    if (i >= total) return;
    float acc = 0.f;
    if (i < rd) {
        const int64_t r = i / D, d = i - r * D;
#pragma unroll 8
        for (int b = 0; b < B; ++b) acc = fmaf(dgb[int64_t(b) * R + r], cond[int64_t(b) * D + d], acc);
        dw[i] = acc;
    } else if (i < rd + R) {
        const int64_t r = i - rd;
#pragma unroll 8
        for (int b = 0; b < B; ++b) acc += dgb[int64_t(b) * R + r];
        dbias[r] = acc;
    } else {
        const int64_t j = i - rd - R, b = j / D, d = j - b * D;
#pragma unroll 8
        for (int r = 0; r < R; ++r) acc = fmaf(dgb[b * R + r], w[int64_t(r) * D + d], acc);
        dcond[j] = acc;
    }
}

__global__ __launch_bounds__(256) void sigmoid_gate_kernel(const float *x, const float *__restrict__ z, float *out, int64_t n,
                                                           int vec) {
    int64_t i, stride, n4;
    flat_walk(n, vec, i, stride, n4);
    for (int64_t q = i; q < n4; q += stride) {
        float4 v = reinterpret_cast<const float4 *>(x)[q];
        const float4 zz = reinterpret_cast<const float4 *>(z)[q];
        v.x *= sigmoidf(zz.x);
        v.y *= sigmoidf(zz.y);
        v.z *= sigmoidf(zz.z);
        v.w *= sigmoidf(zz.w);
        reinterpret_cast<float4 *>(out)[q] = v;
    }
    for (int64_t e = 4 * n4 + i; e < n; e += stride) out[e] = x[e] * sigmoidf(z[e]);
}

__device__ inline void gate_bwd_one(float x, float z, float d, float &dx, float &dz) {
    const float s = sigmoidf(z);
    dx = d * s;
    dz = (d * x) * (s * (1.f - s));
}

__global__ __launch_bounds__(256) void sigmoid_gate_bwd_kernel(const float *__restrict__ x, const float *__restrict__ z,
                                                               const float *__restrict__ dout, float *__restrict__ dx,
                                                               float *__restrict__ dz, int64_t n, int vec) {
    int64_t i, stride, n4;
    flat_walk(n, vec, i, stride, n4);
    for (int64_t q = i; q < n4; q += stride) {
        const float4 xv = reinterpret_cast<const float4 *>(x)[q], zv = reinterpret_cast<const float4 *>(z)[q];
        const float4 dv = reinterpret_cast<const float4 *>(dout)[q];
        float4 a, b;
        gate_bwd_one(xv.x, zv.x, dv.x, a.x, b.x);
        gate_bwd_one(xv.y, zv.y, dv.y, a.y, b.y);
        gate_bwd_one(xv.z, zv.z, dv.z, a.z, b.z);
        gate_bwd_one(xv.w, zv.w, dv.w, a.w, b.w);
        reinterpret_cast<float4 *>(dx)[q] = a;
        reinterpret_cast<float4 *>(dz)[q] = b;
    }
    for (int64_t e = 4 * n4 + i; e < n; e += stride) gate_bwd_one(x[e], z[e], dout[e], dx[e], dz[e]);
}

inline bool bad_layout(int32_t layout) { return layout != AGX_FILM_CT && layout != AGX_FILM_TC; }

}  // namespace

int agx_film_params(const float *cond, const float *w, const float *bias, float *gb, int32_t B, int32_t D, int32_t R,
                    void *stream) {
    if (B <= 0 || D <= 0 || R <= 0) return AGX_OK;
    if (!cond || !w || !gb) return fail(AGX_ERR_NULL_POINTER, "film_params: NULL pointer");
    const int64_t n_out = int64_t(B) * R, blocks = ceil_div64(n_out, 4);
    if (blocks > kMaxGrid) return fail(AGX_ERR_BAD_SHAPE, "film_params: B * R = %lld outputs exceed the grid", (long long)n_out);
    hipLaunchKernelGGL(film_params_kernel, dim3(unsigned(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), cond, w, bias,
                       gb, n_out, D, R);
    return check_launch("agx_film_params");
}

int agx_film_apply(const float *x, const float *gb, float *out, int32_t B, int32_t C, int32_t T, int32_t has_beta,
                   int32_t layout, void *stream) {
    if (bad_layout(layout)) return fail(AGX_ERR_BAD_SHAPE, "film_apply: layout = %d is neither AGX_FILM_CT nor AGX_FILM_TC", layout);
    if (B <= 0 || C <= 0 || T <= 0) return AGX_OK;
    if (!x || !gb || !out) return fail(AGX_ERR_NULL_POINTER, "film_apply: NULL pointer");
    const bool ct = layout == AGX_FILM_CT;
    const int64_t slabs = ct ? int64_t(B) * C : B, len = ct ? T : int64_t(T) * C;
    int64_t segs, items;
    const int64_t blocks = walk_blocks(slabs, len, segs, items);
    if (blocks < 0) return fail(AGX_ERR_BAD_SHAPE, "film_apply: (%d, %d, %d) exceeds the grid", B, C, T);
    const int vec = same_phase16({x, out});
    hipStream_t st = static_cast<hipStream_t>(stream);
#define AGX_FILM_APPLY(L, BETA) \
    hipLaunchKernelGGL((film_apply_kernel<L, BETA>), dim3(unsigned(blocks)), dim3(256), 0, st, x, gb, out, C, len, segs, items, vec)
    if (ct) {
        if (has_beta) AGX_FILM_APPLY(AGX_FILM_CT, true);
        else AGX_FILM_APPLY(AGX_FILM_CT, false);
    } else {
        if (has_beta) AGX_FILM_APPLY(AGX_FILM_TC, true);
        else AGX_FILM_APPLY(AGX_FILM_TC, false);
    }
#undef AGX_FILM_APPLY
    return check_launch("agx_film_apply");
}

int agx_film_backward(const float *x, const float *gb, const float *dout, float *dx, float *dgb, int32_t B, int32_t C,
                      int32_t T, int32_t has_beta, int32_t layout, void *stream) {
    if (bad_layout(layout)) return fail(AGX_ERR_BAD_SHAPE, "film_backward: layout = %d is neither AGX_FILM_CT nor AGX_FILM_TC", layout);
    if (B <= 0 || C <= 0 || T <= 0) return AGX_OK;
    if (!x || !gb || !dout || !dx || !dgb) return fail(AGX_ERR_NULL_POINTER, "film_backward: NULL pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (layout == AGX_FILM_CT) {
        const int64_t rows = int64_t(B) * C;
        if (rows > kMaxGrid) return fail(AGX_ERR_BAD_SHAPE, "film_backward: B * C = %lld rows exceed the grid", (long long)rows);
        if (has_beta) hipLaunchKernelGGL(film_bwd_ct_kernel<true>, dim3(unsigned(rows)), dim3(256), 0, st, x, gb, dout, dx, dgb, C, T);
        else hipLaunchKernelGGL(film_bwd_ct_kernel<false>, dim3(unsigned(rows)), dim3(256), 0, st, x, gb, dout, dx, dgb, C, T);
    } else {
        const int ctiles = agx::ceil_div(C, kWave);
        const int64_t blocks = int64_t(B) * ctiles;
        if (blocks > kMaxGrid) return fail(AGX_ERR_BAD_SHAPE, "film_backward: (%d, %d, %d) exceeds the grid", B, C, T);
        if (has_beta)
            hipLaunchKernelGGL(film_bwd_tc_kernel<true>, dim3(unsigned(blocks)), dim3(256), 0, st, x, gb, dout, dx, dgb, C, T, ctiles);
        else
            hipLaunchKernelGGL(film_bwd_tc_kernel<false>, dim3(unsigned(blocks)), dim3(256), 0, st, x, gb, dout, dx, dgb, C, T, ctiles);
    }
    return check_launch("agx_film_backward");
}

int agx_film_params_backward(const float *cond, const float *w, const float *dgb, float *dw, float *dbias, float *dcond,
                             int32_t B, int32_t D, int32_t R, void *stream) {
    if (B <= 0 || D <= 0 || R <= 0) return AGX_OK;
    if (!cond || !dgb || !dw || !dbias || (dcond && !w)) return fail(AGX_ERR_NULL_POINTER, "film_params_backward: NULL pointer");
    const int64_t total = int64_t(R) * D + R + (dcond ? int64_t(B) * D : 0), blocks = ceil_div64(total, 256);
    if (blocks > kMaxGrid) return fail(AGX_ERR_BAD_SHAPE, "film_params_backward: (%d, %d, %d) exceeds the grid", B, D, R);
    hipLaunchKernelGGL(film_params_bwd_kernel, dim3(unsigned(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), cond, w, dgb,
                       dw, dbias, dcond, B, D, R, total);
    return check_launch("agx_film_params_backward");
}

int agx_sigmoid_gate(const float *x, const float *z, float *out, int64_t n, void *stream) {
    if (n <= 0) return AGX_OK;
    if (!x || !z || !out) return fail(AGX_ERR_NULL_POINTER, "sigmoid_gate: NULL pointer");
    hipLaunchKernelGGL(sigmoid_gate_kernel, dim3(flat_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x, z, out, n,
                       int(all_aligned16({x, z, out})));
    return check_launch("agx_sigmoid_gate");
}

int agx_sigmoid_gate_backward(const float *x, const float *z, const float *dout, float *dx, float *dz, int64_t n,
                              void *stream) {
    if (n <= 0) return AGX_OK;
    if (!x || !z || !dout || !dx || !dz) return fail(AGX_ERR_NULL_POINTER, "sigmoid_gate_backward: NULL pointer");
    hipLaunchKernelGGL(sigmoid_gate_bwd_kernel, dim3(flat_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x, z, dout,
                       dx, dz, n, int(all_aligned16({x, z, dout, dx, dz})));
    return check_launch("agx_sigmoid_gate_backward");
}
