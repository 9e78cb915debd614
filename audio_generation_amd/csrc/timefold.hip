// Time folding for long-clip inference (longform.py): cut a (B, C, L) tensor into S overlapping windows per clip laid
// out as a (B*S, C, W) batch, and crop-and-place the valid part of each window's result back into one (B, C, L') tensor.
//
//   agx_time_fold    dst[b*S + s, c, j]                  = src[b, c, src_off + s*hop + j]        j < W
//   agx_time_unfold  dst[b, c, dst_off + s*keep + j]     = src[b*S + s, c, src_off + j]          j < keep, s < n_win
//
// Pure copies, HBM-bound: every element is read once and written once.  Rows are contiguous in time on both sides but
// start at arbitrary multiples of 4 bytes (window starts, crop offsets), so source and destination are in general NOT
// congruent modulo 16 bytes.  One workgroup copies one span of one row: scalar head until the DESTINATION is 16-byte
// aligned, 16-byte stores over the body (the loads are 16-byte when the source happens to be congruent, four dwords
// otherwise -- still fully coalesced across the wave), scalar tail.  The grid is flat over rows x spans; short rows
// (the latent end: C = 512, tens of frames) take one-wave workgroups, long rows (the waveform end: C = 1 or 2,
// hundreds of thousands of samples) 256-thread ones.  No LDS, no synchronisation, stream-ordered like every agx_* launch.
#include "common.hpp"

namespace agx {

struct RowCopy {
    const float *src;
    float *dst;
    int64_t n_rows;        // rows of `len` elements to copy
    int64_t len;           // elements per row
    int64_t spans;         // spans per row
    int32_t C;             // channels
    int32_t win;           // windows per clip that this launch copies (row = (b * win + s) * C + c)
    int64_t src_b, src_s, src_c, src_0;   // element strides of (clip, window, channel) and the constant offset, source
    int64_t dst_b, dst_s, dst_c, dst_0;   // ... destination
};

struct __attribute__((packed, aligned(4))) f4u {   // four floats at 4-byte alignment
    float x, y, z, w;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void row_copy_kernel(RowCopy p) {
    constexpr int64_t SPAN = int64_t(THREADS) * 4 * 2;    // two 16-byte stores per lane
    const int64_t blk = blockIdx.x;
    const int64_t row = blk / p.spans, span = blk - row * p.spans;
    if (row >= p.n_rows) return;
    const int64_t c = row % p.C, bs = row / p.C;
    const int64_t s = bs % p.win, b = bs / p.win;
    const int64_t first = span * SPAN;
    int64_t n = p.len - first;
    if (n <= 0) return;
    if (n > SPAN) n = SPAN;
    const float *src = p.src + p.src_0 + b * p.src_b + s * p.src_s + c * p.src_c + first;
    float *dst = p.dst + p.dst_0 + b * p.dst_b + s * p.dst_s + c * p.dst_c + first;

    const int tid = threadIdx.x;
    int64_t head = (4 - int64_t((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3;   // floats until dst is 16-byte aligned
    if (head > n) head = n;
    if (tid < head) dst[tid] = src[tid];
    const float *sb = src + head;
    float *db = dst + head;
    const int64_t nv = (n - head) >> 2;
    if ((reinterpret_cast<uintptr_t>(sb) & 15) == 0) {
        for (int64_t v = tid; v < nv; v += THREADS)
            reinterpret_cast<float4 *>(db)[v] = reinterpret_cast<const float4 *>(sb)[v];
    } else {
        for (int64_t v = tid; v < nv; v += THREADS) {
            const f4u t = reinterpret_cast<const f4u *>(sb)[v];
            reinterpret_cast<float4 *>(db)[v] = make_float4(t.x, t.y, t.z, t.w);
        }
    }
    const int64_t done = head + (nv << 2);
    if (tid < n - done) dst[done + tid] = src[done + tid];
}

static int launch_row_copy(RowCopy p, hipStream_t stream, const char *what) {
    const bool small = p.len <= 1024;
    const int64_t span = small ? 64 * 8 : 256 * 8;
    p.spans = ceil_div64(p.len, span);
    const int64_t blocks = p.n_rows * p.spans;
    if (blocks <= 0 || blocks > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: %lld workgroups", what, (long long)blocks);
    if (small)
        hipLaunchKernelGGL(row_copy_kernel<64>, dim3((unsigned)blocks), dim3(64), 0, stream, p);
    else
        hipLaunchKernelGGL(row_copy_kernel<256>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    return check_launch(what);
}

}  // namespace agx

extern "C" {

int agx_time_fold(const float *src, float *dst, int32_t batch, int32_t channels, int64_t length, int32_t windows, int64_t hop,
                  int64_t width, int64_t src_off, void *stream) {
    using namespace agx;
    if (batch <= 0 || channels <= 0 || length <= 0 || windows <= 0 || width <= 0 || hop < 0 || src_off < 0)
        return fail(AGX_ERR_BAD_SHAPE, "time_fold: B=%d C=%d L=%lld S=%d hop=%lld W=%lld off=%lld", batch, channels, (long long)length,
                    windows, (long long)hop, (long long)width, (long long)src_off);
    if (src_off + int64_t(windows - 1) * hop + width > length)
        return fail(AGX_ERR_BAD_SHAPE, "time_fold: the last window [%lld, %lld) leaves the source (L=%lld)",
                    (long long)(src_off + int64_t(windows - 1) * hop), (long long)(src_off + int64_t(windows - 1) * hop + width),
                    (long long)length);
    if (!src || !dst) return fail(AGX_ERR_NULL_POINTER, "time_fold: NULL pointer");
    RowCopy p{};
    p.src = src, p.dst = dst;
    p.n_rows = int64_t(batch) * windows * channels, p.len = width, p.C = channels, p.win = windows;
    p.src_b = int64_t(channels) * length, p.src_s = hop, p.src_c = length, p.src_0 = src_off;
    p.dst_b = int64_t(windows) * channels * width, p.dst_s = int64_t(channels) * width, p.dst_c = width, p.dst_0 = 0;
    return launch_row_copy(p, static_cast<hipStream_t>(stream), "time_fold");
}

int agx_time_unfold(const float *src, float *dst, int32_t batch, int32_t channels, int32_t windows, int64_t width, int64_t dst_length,
                    int32_t n_win, int64_t src_off, int64_t dst_off, int64_t keep, void *stream) {
    using namespace agx;
    if (batch <= 0 || channels <= 0 || windows <= 0 || width <= 0 || dst_length <= 0 || n_win <= 0 || n_win > windows || keep <= 0 ||
        src_off < 0 || dst_off < 0)
        return fail(AGX_ERR_BAD_SHAPE, "time_unfold: B=%d C=%d S=%d W=%lld L=%lld n_win=%d src_off=%lld dst_off=%lld keep=%lld", batch,
                    channels, windows, (long long)width, (long long)dst_length, n_win, (long long)src_off, (long long)dst_off,
                    (long long)keep);
    if (src_off + keep > width)
        return fail(AGX_ERR_BAD_SHAPE, "time_unfold: crop [%lld, %lld) leaves the window (W=%lld)", (long long)src_off,
                    (long long)(src_off + keep), (long long)width);
    if (dst_off + int64_t(n_win) * keep > dst_length)
        return fail(AGX_ERR_BAD_SHAPE, "time_unfold: placement [%lld, %lld) leaves the destination (L=%lld)", (long long)dst_off,
                    (long long)(dst_off + int64_t(n_win) * keep), (long long)dst_length);
    if (!src || !dst) return fail(AGX_ERR_NULL_POINTER, "time_unfold: NULL pointer");
    RowCopy p{};
    p.src = src, p.dst = dst;
    p.n_rows = int64_t(batch) * n_win * channels, p.len = keep, p.C = channels, p.win = n_win;
    p.src_b = int64_t(windows) * channels * width, p.src_s = int64_t(channels) * width, p.src_c = width, p.src_0 = src_off;
    p.dst_b = int64_t(channels) * dst_length, p.dst_s = keep, p.dst_c = dst_length, p.dst_0 = dst_off;
    return launch_row_copy(p, static_cast<hipStream_t>(stream), "time_unfold");
}

}  // extern "C"
