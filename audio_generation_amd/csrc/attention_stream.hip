// Sliding-window causal self-attention on a ring key/value cache whose positions live in device memory, one per batch row:
// row b's first query sits at absolute position pos[b] (an int64 the kernels read), query i at p = i + pos[b], and it sees the
// last W keys, j in [max(0, p - W + 1), p], key j in column j mod ring of a kv row.
//
//     out[b,h,:,i] = sum_j softmax_j( q_i . k_j / scale_div - slope_h (p - j) ) v_j,    j in [max(0, p - W + 1), p]
//
// What a host integer could not do: a captured graph replays with the positions the array holds at replay time, and the rows of
// a batch have ages of their own (a row restarts when its entry is zeroed).  Three kernels: the attention, the write of a chunk's
// K / V rows into the ring at each row's position, and the advance pos[b] += n.
//
// Layouts (channel-major fp32), as attention_window.hip:  q (B, H*Dh, Tq), rows of pitch Tq;  kv (B, 2*H*Dh, .), K rows first,
// then V rows, rows of pitch kv_row_stride >= ring;  out (B, H*Dh, Tq).  q and kv have their own base pointers and batch
// strides, so the Q rows of a (B, 3*H*Dh, Tq) qkv tensor are read in place.
//
// attention_stream_kernel<DVT> is the shared forward body of attention_masked.hpp under WindowMask<false>: the window kernel with
// a mandatory ring (ring >= 1).  The ONLY other difference is where q_pos0 comes from -- there an argument the launcher lowered
// into int32, here pos[b] read and lowered by every workgroup (below).
//
// The position.  b = blockIdx.z, so pos[b] is one workgroup-uniform load: pmax, jlo, the block bounds and the V prefetch stay
// workgroup-uniform and every thread meets every __syncthreads.  A negative entry is read as 0.  The kernel indexes in int32, and
// the host cannot lower a 64-bit position it does not know, so the kernel does what agx_attention_alibi_window does on the host:
// a position beyond W - 1 is lowered by a multiple of period = lcm(64, ring) (passed by value),
//     pos -= ((pos - (W - 1)) / period) * period        -- one 64-bit division per workgroup, outside every loop --
// which keeps the 64-key block alignment (block = j / 64), the ring column (j mod ring) and every p - j, and leaves
// W - 1 <= pos < W - 1 + period, so that the floor "no key before position 0" bites nowhere it did not.  The launcher refuses a
// ring for which period + W + Tq + 128 leaves int32.
//
// Memory safety does not depend on what pos holds.  Columns are formed modulo the ring, and the launcher guarantees
// Tq + W - 1 <= ring <= kv_row_stride without reading pos: pmax - jlo <= Tq + W - 2 < ring for every position (jlo > 0:
// pmax - jlo <= (Tq - 1 + pos) - (q0 + pos - W + 1); jlo = 0: pmax <= Tq - 1 + W - 1 - q0), so the single conditional subtract
// of col_of stays valid, every K / V load lands in a column [0, ring) of its own row, and out is indexed by blockIdx and
// threadIdx alone.  This is stricter than the host-position form at the start of a stream (there: Tq + min(W - 1, pos) <= ring).
// A row at position 0 reads no column it has not written in this call.
#include "attention_masked.hpp"

namespace agx {

template <int DVT>
__global__ __launch_bounds__(256) void attention_stream_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                               int64_t sq, int64_t skv, int krs,
                                                               const int64_t *__restrict__ pos, int64_t period,
                                                               const float *__restrict__ slopes, float *__restrict__ out, int H,
                                                               int Dh, int Tq, int W, int ring, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    // ---- the row's position: workgroup-uniform, lowered into int32 (see the header) ----
    int64_t p64 = pos[b];
    p64 = p64 < 0 ? 0 : p64;
    if (p64 > W - 1) p64 -= (p64 - (W - 1)) / period * period;
    auto v = window_view<false>(q, kv, sq, skv, krs, nullptr, h, b, H, Dh, Tq, int(p64), W, ring);
    v.place(blockIdx.x * 128, Tq);   // the keys this workgroup's 128 queries see
    attn_fwd_body<DVT>(v, out + (size_t(b) * (H * Dh) + size_t(h) * Dh) * Tq, slopes, h, Dh, scale_div);
}

// The counted form (include/agx.h "Per-row frame counts"): row b's chunk holds c_b = clamp(counts[b], 0, Tq) frames, and only their
// K / V rows are in the ring (ring_write_pos_kernel<true>).  The one change is the key range: place() is given c_b for Tq, so
// pmax = pos + c_b - 1 and the ring columns behind the count -- stale frames or unwritten memory, which would meet p = 0 as
// 0 * NaN in the V product -- are not live and are staged as zeros.  For a query below the count jlo, pmax, the block bounds and
// every operand are those of the uncounted kernel on a chunk of c_b frames: the same bits.  A query at or behind the count is
// written like any other (ql = Tq) and holds nothing meaningful -- with no live key it is 0 / 0 -- which the caller masks.
// Memory safety: a smaller pmax only shrinks pmax - jlo; k_col clamps into [jlo, max(jlo, pmax)], v_col is used on live keys only.
template <int DVT>
__global__ __launch_bounds__(256) void attention_stream_counted_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                       int64_t sq, int64_t skv, int krs,
                                                                       const int64_t *__restrict__ pos,
                                                                       const int64_t *__restrict__ counts, int64_t period,
                                                                       const float *__restrict__ slopes, float *__restrict__ out,
                                                                       int H, int Dh, int Tq, int W, int ring, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    int64_t p64 = pos[b];
    p64 = p64 < 0 ? 0 : p64;
    if (p64 > W - 1) p64 -= (p64 - (W - 1)) / period * period;
    const int64_t c64 = counts[b];
    const int cb = int(c64 < 0 ? 0 : c64 > Tq ? Tq : c64);   // workgroup-uniform
    auto v = window_view<false>(q, kv, sq, skv, krs, nullptr, h, b, H, Dh, Tq, int(p64), W, ring);
    v.place(blockIdx.x * 128, cb);   // the keys of the row's own frames only
    attn_fwd_body<DVT>(v, out + (size_t(b) * (H * Dh) + size_t(h) * Dh) * Tq, slopes, h, Dh, scale_div);
}

// A chunk's K / V rows into the ring: buf[b, c, (pos[b] + t) mod ring] = src[b, c, t] for c < C, t < n.  src is read in place
// (base pointer, batch stride ssrc, rows of pitch n: the K / V rows of a qkv tensor); buf has batch stride sbuf and rows of pitch
// brs >= ring.  One launch, wrap included: n <= ring (host), so c0 + t < 2 ring and one conditional subtract forms the column,
// every column is written once, and the column lies in [0, ring) whatever pos holds (a negative entry is read as 0).  One thread
// per element, t fastest: the loads are contiguous and the stores of a row are coalesced along t, in two runs where it wraps.
// CNT: only the row's first clamp(counts[b], 0, n) frames; the columns behind them are neither read nor written.
template <bool CNT>
__global__ __launch_bounds__(256) void ring_write_pos_kernel(float *__restrict__ buf, const float *__restrict__ src, int64_t sbuf,
                                                             int brs, int64_t ssrc, const int64_t *__restrict__ pos,
                                                             const int64_t *__restrict__ counts, int C, int n, int ring) {
    const int b = blockIdx.y;
    int64_t p64 = pos[b];          // workgroup-uniform
    p64 = p64 < 0 ? 0 : p64;
    const int c0 = int(p64 % ring);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= C * n) return;
    const int c = e / n, t = e - c * n;
    if (CNT) {
        const int64_t cb = counts[b];
        if (t >= int(cb < 0 ? 0 : cb > n ? n : cb)) return;
    }
    int col = c0 + t;
    col = col >= ring ? col - ring : col;
    buf[size_t(b) * sbuf + size_t(c) * brs + col] = src[size_t(b) * ssrc + e];
}

// pos[b] += n for every row: the positions advance on the device, once per call, after the last layer has read them.
__global__ __launch_bounds__(256) void stream_advance_kernel(int64_t *__restrict__ pos, int B, int64_t n) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) pos[b] += n;
}

// pos[b] += clamp(counts[b], 0, n): every row by the frames it took of a counted call.
__global__ __launch_bounds__(256) void stream_advance_counted_kernel(int64_t *__restrict__ pos, const int64_t *__restrict__ counts, int B,
                                                                     int64_t n) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int64_t c = counts[b];
    pos[b] += c < 0 ? 0 : c > n ? n : c;
}

// ------------------------------------------------------------------ host side
static MaskedRow<decltype(&attention_stream_kernel<1>)> kAttnStreamRows[3] = AGX_MASKED_ROWS(stream);
static MaskedRow<decltype(&attention_stream_counted_kernel<1>)> kAttnStreamCountedRows[3] = AGX_MASKED_ROWS(stream_counted);

}  // namespace agx

extern "C" {

static int attention_stream(const char *op, const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                            int64_t kv_row_stride, const int64_t *pos, const int64_t *counts, const float *slopes, float *out,
                            int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t window, int32_t kv_ring, float scale_div,
                            void *stream) {
    using namespace agx;
    const MaskedPick k = masked_window_pick(op, batch, heads, head_dim, tq, window);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (kv_ring < 1) return fail(AGX_ERR_BAD_SHAPE, "%s: kv_ring=%d < 1 (the ring is mandatory)", op, kv_ring);
    // The worst case over every position, because the positions are not the host's to read: tq queries and the window - 1 keys
    // behind the first of them must not overwrite one another.
    const int64_t span = int64_t(tq) + window - 1;
    if (span > kv_ring) return fail(AGX_ERR_BAD_SHAPE, "%s: kv_ring=%d < tq + window - 1 = %lld", op, kv_ring, (long long)span);
    if (kv_ring > kv_row_stride) return fail(AGX_ERR_BAD_SHAPE, "%s: kv_ring=%d > kv row stride %lld", op, kv_ring, (long long)kv_row_stride);
    if (kv_row_stride > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: kv row stride %lld is beyond int32", op, (long long)kv_row_stride);
    // The kernel lowers a position to below window - 1 + period and indexes in int32.
    const int64_t period = 64 / gcd64(64, kv_ring) * int64_t(kv_ring);
    if (period + window + tq + 128 > 0x7fffffffLL)
        return fail(AGX_ERR_BAD_SHAPE, "%s: lcm(64, kv_ring=%d) + window + tq is beyond int32", op, kv_ring);
    if (!q || !kv || !pos || !slopes || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_strides(op, q_batch_stride, hd * tq, "q")) return rc;
    if (int rc = check_strides(op, kv_batch_stride, 2 * hd * kv_row_stride, "kv")) return rc;
    if (counts)
        return masked_launch(kAttnStreamCountedRows[k.di], k, "attention_stream_counted", static_cast<hipStream_t>(stream), q, kv,
                             q_batch_stride, kv_batch_stride, int(kv_row_stride), pos, counts, period, slopes, out, heads, head_dim, tq,
                             window, kv_ring, scale_div);
    return masked_launch(kAttnStreamRows[k.di], k, "attention_stream", static_cast<hipStream_t>(stream), q, kv, q_batch_stride,
                         kv_batch_stride, int(kv_row_stride), pos, period, slopes, out, heads, head_dim, tq, window, kv_ring, scale_div);
}

int agx_attention_alibi_stream(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride, int64_t kv_row_stride,
                               const int64_t *pos, const float *slopes, float *out, int32_t batch, int32_t heads, int32_t head_dim,
                               int32_t tq, int32_t window, int32_t kv_ring, float scale_div, void *stream) {
    return attention_stream("attention_alibi_stream", q, kv, q_batch_stride, kv_batch_stride, kv_row_stride, pos, nullptr, slopes, out,
                            batch, heads, head_dim, tq, window, kv_ring, scale_div, stream);
}

int agx_attention_alibi_stream_counted(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                       int64_t kv_row_stride, const int64_t *pos, const int64_t *counts, const float *slopes, float *out,
                                       int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t window, int32_t kv_ring,
                                       float scale_div, void *stream) {
    if (!counts && batch > 0 && heads > 0 && tq > 0) return agx::fail(AGX_ERR_NULL_POINTER, "attention_alibi_stream_counted: NULL counts");
    return attention_stream("attention_alibi_stream_counted", q, kv, q_batch_stride, kv_batch_stride, kv_row_stride, pos, counts, slopes,
                            out, batch, heads, head_dim, tq, window, kv_ring, scale_div, stream);
}

static int ring_write_pos(const char *op, float *buf, const float *src, int64_t buf_batch_stride, int64_t buf_row_stride,
                          int64_t src_batch_stride, const int64_t *pos, const int64_t *counts, int32_t batch, int32_t rows, int32_t n,
                          int32_t ring, void *stream) {
    using namespace agx;
    if (batch <= 0 || rows <= 0 || n <= 0) return AGX_OK;
    if (batch > 65535) return fail(AGX_ERR_BAD_SHAPE, "%s: grid too large", op);
    if (ring < 1) return fail(AGX_ERR_BAD_SHAPE, "%s: ring=%d < 1", op, ring);
    if (n > ring) return fail(AGX_ERR_BAD_SHAPE, "%s: n=%d > ring=%d (a column would be written twice)", op, n, ring);
    if (ring > buf_row_stride) return fail(AGX_ERR_BAD_SHAPE, "%s: ring=%d > buf row stride %lld", op, ring, (long long)buf_row_stride);
    if (buf_row_stride > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: buf row stride %lld is beyond int32", op, (long long)buf_row_stride);
    if (int64_t(rows) * n + 256 > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: rows * n = %lld is beyond int32", op, (long long)rows * n);
    if (!buf || !src || !pos) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    if (int rc = check_strides(op, buf_batch_stride, int64_t(rows) * buf_row_stride, "buf")) return rc;
    if (int rc = check_strides(op, src_batch_stride, int64_t(rows) * n, "src")) return rc;
    const dim3 grid(ceil_div(rows * n, 256), batch);
    if (counts)
        hipLaunchKernelGGL(ring_write_pos_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), buf, src, buf_batch_stride,
                           int(buf_row_stride), src_batch_stride, pos, counts, rows, n, ring);
    else
        hipLaunchKernelGGL(ring_write_pos_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), buf, src, buf_batch_stride,
                           int(buf_row_stride), src_batch_stride, pos, counts, rows, n, ring);
    return check_launch(op);
}

int agx_ring_write_pos(float *buf, const float *src, int64_t buf_batch_stride, int64_t buf_row_stride, int64_t src_batch_stride,
                       const int64_t *pos, int32_t batch, int32_t rows, int32_t n, int32_t ring, void *stream) {
    return ring_write_pos("ring_write_pos", buf, src, buf_batch_stride, buf_row_stride, src_batch_stride, pos, nullptr, batch, rows, n, ring,
                          stream);
}

int agx_ring_write_pos_counted(float *buf, const float *src, int64_t buf_batch_stride, int64_t buf_row_stride, int64_t src_batch_stride,
                               const int64_t *pos, const int64_t *counts, int32_t batch, int32_t rows, int32_t n, int32_t ring,
                               void *stream) {
    if (!counts && batch > 0 && rows > 0 && n > 0) return agx::fail(AGX_ERR_NULL_POINTER, "ring_write_pos_counted: NULL counts");
    return ring_write_pos("ring_write_pos_counted", buf, src, buf_batch_stride, buf_row_stride, src_batch_stride, pos, counts, batch, rows,
                          n, ring, stream);
}

int agx_stream_advance(int64_t *pos, int32_t batch, int64_t n, void *stream) {
    using namespace agx;
    if (batch <= 0) return AGX_OK;
    if (n < 0) return fail(AGX_ERR_BAD_SHAPE, "stream_advance: n=%lld < 0", (long long)n);
    if (!pos) return fail(AGX_ERR_NULL_POINTER, "stream_advance: NULL pointer");
    hipLaunchKernelGGL(stream_advance_kernel, dim3(ceil_div(batch, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pos, batch, n);
    return check_launch("stream_advance");
}

int agx_stream_advance_counted(int64_t *pos, const int64_t *counts, int32_t batch, int64_t n, void *stream) {
    using namespace agx;
    if (batch <= 0) return AGX_OK;
    if (n < 0) return fail(AGX_ERR_BAD_SHAPE, "stream_advance_counted: n=%lld < 0", (long long)n);
    if (!pos || !counts) return fail(AGX_ERR_NULL_POINTER, "stream_advance_counted: NULL pointer");
    hipLaunchKernelGGL(stream_advance_counted_kernel, dim3(ceil_div(batch, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pos,
                       counts, batch, n);
    return check_launch("stream_advance_counted");
}

int agx_attention_stream_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t window, char *buf,
                                     size_t buf_len) {
    using namespace agx;
    const MaskedPick k = masked_window_pick("attention_alibi_stream", batch, heads, head_dim, tq, window);
    return masked_name(k, "agx_attention_stream_kernel_name", kAttnStreamRows[k.di].name, buf, buf_len);
}

}  // extern "C"
