// The per-channel wavelet of WaveletLayer (wavelets.py:221-231) and its phase sums, shared by the plain fold (wavelet.hip) and the
// table of the streaming out-step (wavelet_stream.hip): both form the same numbers by the same operations in the same order.
#pragma once
#include "common.hpp"

namespace agx {

// A workgroup fills kern[P] = cos(t_p) exp(-t_p^2 / sigma), then s_lo[ph] = sum_{p < ph fold} kern[p] and s_hi[ph] = sum_{p >= ph fold}
// kern[p] (ascending p) for ph < scale.  P, scale <= blockDim.x; ends on a barrier, so every thread may read all three.
__device__ __forceinline__ void wavelet_phase_sums(const float *__restrict__ space, float sg, int P, int scale, float *kern,
                                                   float *s_lo, float *s_hi) {
    const int tid = threadIdx.x;
    if (tid < P) {
        const float t = space[tid];
        kern[tid] = cosf(t) * expf(-(t * t) / sg);
    }
    __syncthreads();
    const int fold = P / scale;
    if (tid < scale) {
        float lo = 0.f, hi = 0.f;
        for (int p = 0; p < tid * fold; ++p) lo += kern[p];
        for (int p = tid * fold; p < P; ++p) hi += kern[p];
        s_lo[tid] = lo;
        s_hi[tid] = hi;
    }
    __syncthreads();
}

}  // namespace agx
