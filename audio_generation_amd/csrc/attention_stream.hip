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
// TWIN CODE: attention_stream_kernel<DVT> is a copy of attention_window_kernel<DVT> of attention_window.hip (itself a copy of
// attention_causal_kernel<DVT> of attention_causal.hip): same tiling, same arithmetic, same block bounds, same two hazards and
// cures.  The ONLY difference is where q_pos0 comes from -- there an argument the launcher lowered into int32, here pos[b]
// read and lowered by every workgroup (below) -- and that the ring is mandatory (ring >= 1).  Kept apart so that the window and
// causal kernels stay the code they were.  A fix to one belongs in the others too.
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
//
// Block bounds and the two hazards -- leading all-masked blocks (ms = mn == -inf ? 0 : mn), stale or unwritten ring columns (V
// staged as zeros outside [jlo, pmax], K gathers clamped into [jlo, pmax], the masked score replaced by a select) -- are those of
// attention_window.hip, word for word; see its header.  A row at position 0 reads no column it has not written in this call.
#include "mfma_tile.hpp"

namespace agx {

template <int DVT>
__global__ __launch_bounds__(256) void attention_stream_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                               int64_t sq, int64_t skv, int krs,
                                                               const int64_t *__restrict__ pos, int64_t period,
                                                               const float *__restrict__ slopes, float *__restrict__ out, int H,
                                                               int Dh, int Tq, int W, int ring, float scale_div) {
    constexpr int KB = 64;         // keys per block (two 32-key accumulator tiles)
    constexpr int DH = 32 * DVT;   // head_dim rounded up to the tile
    constexpr int VP = KB + 1;     // LDS pitch of the V block
    extern __shared__ __attribute__((aligned(16))) float vs[];   // [2][DH][VP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int HD = H * Dh;
    // ---- the row's position: workgroup-uniform, lowered into int32 (see the header) ----
    int64_t p64 = pos[b];
    p64 = p64 < 0 ? 0 : p64;
    if (p64 > W - 1) p64 -= (p64 - (W - 1)) / period * period;
    const int q_pos0 = int(p64);
    const float *qb = q + size_t(b) * sq + size_t(h) * Dh * Tq;
    const float *kb = kv + size_t(b) * skv + size_t(h) * Dh * krs;
    const float *vb = kb + size_t(HD) * krs;
    const int q0 = blockIdx.x * 128;
    const int i = q0 + wave * 32 + li;   // this lane's query
    const int ic = min(i, Tq - 1);
    const int ip = ic + q_pos0;          // its absolute position: the last key it sees
    const float slope = slopes[h], inv_scale = 1.f / scale_div;
    // workgroup-uniform: the positions of the 128 queries, the keys any of them sees, the blocks that hold those keys
    const int pmax = min(q0 + 127, Tq - 1) + q_pos0;
    const int jlo = max(0, q0 + q_pos0 - W + 1);
    const int blk_lo = jlo / KB, blk_hi = pmax / KB;
    const int c0 = jlo % ring;                    // the column of key jlo; pmax - jlo < ring (host check), so one wrap at most
    auto col_of = [&](int j) {                    // the column of key j in [jlo, pmax]
        const int c = c0 + (j - jlo);
        return c >= ring ? c - ring : c;
    };

    // ---- the query fragment stays in registers for the whole key loop ----
    float qf[DH / 2];
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) {
        const int d = 2 * s + lh;
        qf[s] = d < Dh ? qb[size_t(d) * Tq + ic] : 0.f;
    }

    f32x16 o[DVT];
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m = -INFINITY, l = 0.f;

    auto stage_v = [&](int blk, float *dst) {   // V[dv < Dh][64 keys of block blk] -> LDS, zeros outside [jlo, pmax] (stale columns are never read)
        for (int e = tid; e < DH * KB; e += 256) {
            const int dv = e / KB, jj = e - dv * KB, j = blk * KB + jj;
            dst[dv * VP + jj] = (dv < Dh && j >= jlo && j <= pmax) ? vb[size_t(dv) * krs + col_of(j)] : 0.f;
        }
    };
    stage_v(blk_lo, vs + (blk_lo & 1) * DH * VP);
    __syncthreads();

    for (int blk = blk_lo; blk <= blk_hi; ++blk) {
        const int j0 = blk * KB;
        float *vcur = vs + (blk & 1) * DH * VP;
        if (blk + 1 <= blk_hi) stage_v(blk + 1, vs + ((blk + 1) & 1) * DH * VP);   // next block streams in meanwhile

        // ---- S^T = K^T Q for this block: rows = keys, columns = queries ----
        f32x16 acc[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t2][r] = 0.f;
        int kcol[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) kcol[t2] = col_of(max(jlo, min(j0 + t2 * 32 + li, pmax)));
#pragma unroll 4
        for (int s = 0; s < DH / 2; ++s) {
            const int d = min(2 * s + lh, Dh - 1);
            float kf[2];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) kf[t2] = kb[size_t(d) * krs + kcol[t2]];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) acc[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[t2], qf[s], acc[t2], 0, 0, 0);
        }

        // ---- scale, one-sided ALiBi, window mask, online softmax (in-lane over the 32 registers + one shuffle) ----
        float bm = -INFINITY;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + t2 * 32 + acc_row(r, lh);
                float s = acc[t2][r] * inv_scale - float(ip - j) * slope;
                s = (j <= ip && j > ip - W) ? s : -INFINITY;   // a select: whatever the masked score was, it is gone
                acc[t2][r] = s;
                bm = fmaxf(bm, s);
            }
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        const float mn = fmaxf(m, bm);                    // -inf until the row has seen its first key
        const float ms = mn == -INFINITY ? 0.f : mn;      // never (-inf) - (-inf): a leading all-masked block is the identity
        const float alpha = expf(m - ms);                 // m = -inf: exp(-inf) = 0 (l = 0, o = 0 stay); a later all-masked block: exp(0) = 1
        float bl = 0.f;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pe = expf(acc[t2][r] - ms);   // masked: exp(-inf) = 0 exactly
                acc[t2][r] = pe;
                bl += pe;
            }
        bl += __shfl_xor(bl, 32);
        l = l * alpha + bl;
        m = mn;
#pragma unroll
        for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;

        // ---- O^T += V P^T : B operand = the probability registers ----
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int jj = t2 * 32 + acc_row(s, lh);
#pragma unroll
                for (int dt = 0; dt < DVT; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vcur[(dt * 32 + li) * VP + jj], acc[t2][s], o[dt], 0, 0, 0);
            }
        __syncthreads();   // the next block's V has been written by everyone; this block's is free
    }

    const float inv = 1.f / l;
    float *ob = out + (size_t(b) * HD + size_t(h) * Dh) * Tq;
    if (i < Tq) {
#pragma unroll
        for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dv = dt * 32 + acc_row(r, lh);
                if (dv < Dh) ob[size_t(dv) * Tq + i] = o[dt][r] * inv;
            }
    }
}

// A chunk's K / V rows into the ring: buf[b, c, (pos[b] + t) mod ring] = src[b, c, t] for c < C, t < n.  src is read in place
// (base pointer, batch stride ssrc, rows of pitch n: the K / V rows of a qkv tensor); buf has batch stride sbuf and rows of pitch
// brs >= ring.  One launch, wrap included: n <= ring (host), so c0 + t < 2 ring and one conditional subtract forms the column,
// every column is written once, and the column lies in [0, ring) whatever pos holds (a negative entry is read as 0).  One thread
// per element, t fastest: the loads are contiguous and the stores of a row are coalesced along t, in two runs where it wraps.
__global__ __launch_bounds__(256) void ring_write_pos_kernel(float *__restrict__ buf, const float *__restrict__ src, int64_t sbuf,
                                                             int brs, int64_t ssrc, const int64_t *__restrict__ pos, int C, int n,
                                                             int ring) {
    const int b = blockIdx.y;
    int64_t p64 = pos[b];          // workgroup-uniform
    p64 = p64 < 0 ? 0 : p64;
    const int c0 = int(p64 % ring);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= C * n) return;
    const int c = e / n, t = e - c * n;
    int col = c0 + t;
    col = col >= ring ? col - ring : col;
    buf[size_t(b) * sbuf + size_t(c) * brs + col] = src[size_t(b) * ssrc + e];
}

// pos[b] += n for every row: the positions advance on the device, once per call, after the last layer has read them.
__global__ __launch_bounds__(256) void stream_advance_kernel(int64_t *__restrict__ pos, int B, int64_t n) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) pos[b] += n;
}

// ------------------------------------------------------------------ host side: one pick feeds launch and name query
struct AttnStreamPick;
#define AGX_ATTN_STREAM_ARGS                                                                                                        \
    const AttnStreamPick &k, const float *q, const float *kv, int64_t sq, int64_t skv, int krs, const int64_t *pos, int64_t period, \
        const float *slopes, float *out, int H, int Dh, int Tq, int W, int ring, float scale_div, hipStream_t st
struct AttnStreamRow { const char *name; int (*launch)(AGX_ATTN_STREAM_ARGS); };
// empty: batch, heads or tq <= 0 -- the entry points return AGX_OK and launch nothing; code: a refusal (fail() was called)
struct AttnStreamPick { const AttnStreamRow *row; dim3 grid; size_t lds; int lds_limit, code; bool empty; };

template <int DVT>
static int run_attention_stream(AGX_ATTN_STREAM_ARGS) {
    auto kern = attention_stream_kernel<DVT>;
    static DeviceOnce once;
    if (int rc = prepare_kernel(reinterpret_cast<const void *>(kern), once, k.lds_limit, nullptr, "attention_stream")) return rc;
    hipLaunchKernelGGL(kern, k.grid, dim3(256), k.lds, st, q, kv, sq, skv, krs, pos, period, slopes, out, H, Dh, Tq, W, ring, scale_div);
    return check_launch("attention_stream");
}

#define AGX_ATTN_ROW(DVT) {"attention_stream<" #DVT ">", run_attention_stream<DVT>}
static const AttnStreamRow kAttnStreamRows[3] = {AGX_ATTN_ROW(1), AGX_ATTN_ROW(2), AGX_ATTN_ROW(4)};   // [log2(DVT)]
#undef AGX_ATTN_ROW

// the pick of attn_window_pick (attention_window.hip): same tiles, same LDS, same grid
static AttnStreamPick attn_stream_pick(const char *op, int B, int H, int Dh, int Tq, int W) {
    AttnStreamPick k{};
    k.empty = B <= 0 || H <= 0 || Tq <= 0;
    if (Dh <= 0) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: bad shape head_dim=%d", op, Dh);
    else if (Dh > 128) k.code = fail(AGX_ERR_UNSUPPORTED, "%s: head_dim=%d > 128", op, Dh);
    else if (H > 65535 || B > 65535) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: grid too large", op);
    else if (W < 1) k.code = fail(AGX_ERR_BAD_SHAPE, "%s: window=%d < 1", op, W);
    if (k.code || k.empty) return k;
    const int dvt = Dh <= 32 ? 1 : (Dh <= 64 ? 2 : 4), di = dvt / 2;   // 32-row tiles of the head dim; di = log2(dvt)
    k.row = &kAttnStreamRows[di];
    k.lds = size_t(2) * 32 * dvt * 65 * sizeof(float);                 // the double-buffered V block
    k.lds_limit = k.lds > 48 * 1024 ? 96 * 1024 : 0;
    k.grid = dim3(ceil_div(Tq, 128), H, B);
    return k;
}

// a batch stride must hold one item: the kernels index [b * stride + row * pitch + t]
static int check_stream_strides(const char *op, int64_t have, int64_t need, const char *what) {
    return have >= need ? AGX_OK : fail(AGX_ERR_BAD_SHAPE, "%s: %s batch stride %lld < %lld", op, what, (long long)have, (long long)need);
}

static int64_t stream_gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t r = a % b;
        a = b;
        b = r;
    }
    return a;
}

}  // namespace agx

extern "C" {

int agx_attention_alibi_stream(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride, int64_t kv_row_stride,
                               const int64_t *pos, const float *slopes, float *out, int32_t batch, int32_t heads, int32_t head_dim,
                               int32_t tq, int32_t window, int32_t kv_ring, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_stream";
    const AttnStreamPick k = attn_stream_pick(op, batch, heads, head_dim, tq, window);
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
    const int64_t period = 64 / stream_gcd64(64, kv_ring) * int64_t(kv_ring);
    if (period + window + tq + 128 > 0x7fffffffLL)
        return fail(AGX_ERR_BAD_SHAPE, "%s: lcm(64, kv_ring=%d) + window + tq is beyond int32", op, kv_ring);
    if (!q || !kv || !pos || !slopes || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_stream_strides(op, q_batch_stride, hd * tq, "q")) return rc;
    if (int rc = check_stream_strides(op, kv_batch_stride, 2 * hd * kv_row_stride, "kv")) return rc;
    return k.row->launch(k, q, kv, q_batch_stride, kv_batch_stride, int(kv_row_stride), pos, period, slopes, out, heads, head_dim, tq,
                         window, kv_ring, scale_div, static_cast<hipStream_t>(stream));
}

int agx_ring_write_pos(float *buf, const float *src, int64_t buf_batch_stride, int64_t buf_row_stride, int64_t src_batch_stride,
                       const int64_t *pos, int32_t batch, int32_t rows, int32_t n, int32_t ring, void *stream) {
    using namespace agx;
    const char *op = "ring_write_pos";
    if (batch <= 0 || rows <= 0 || n <= 0) return AGX_OK;
    if (batch > 65535) return fail(AGX_ERR_BAD_SHAPE, "%s: grid too large", op);
    if (ring < 1) return fail(AGX_ERR_BAD_SHAPE, "%s: ring=%d < 1", op, ring);
    if (n > ring) return fail(AGX_ERR_BAD_SHAPE, "%s: n=%d > ring=%d (a column would be written twice)", op, n, ring);
    if (ring > buf_row_stride) return fail(AGX_ERR_BAD_SHAPE, "%s: ring=%d > buf row stride %lld", op, ring, (long long)buf_row_stride);
    if (buf_row_stride > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: buf row stride %lld is beyond int32", op, (long long)buf_row_stride);
    if (int64_t(rows) * n + 256 > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: rows * n = %lld is beyond int32", op, (long long)rows * n);
    if (!buf || !src || !pos) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    if (int rc = check_stream_strides(op, buf_batch_stride, int64_t(rows) * buf_row_stride, "buf")) return rc;
    if (int rc = check_stream_strides(op, src_batch_stride, int64_t(rows) * n, "src")) return rc;
    hipLaunchKernelGGL(ring_write_pos_kernel, dim3(ceil_div(rows * n, 256), batch), dim3(256), 0, static_cast<hipStream_t>(stream), buf,
                       src, buf_batch_stride, int(buf_row_stride), src_batch_stride, pos, rows, n, ring);
    return check_launch("ring_write_pos");
}

int agx_stream_advance(int64_t *pos, int32_t batch, int64_t n, void *stream) {
    using namespace agx;
    if (batch <= 0) return AGX_OK;
    if (n < 0) return fail(AGX_ERR_BAD_SHAPE, "stream_advance: n=%lld < 0", (long long)n);
    if (!pos) return fail(AGX_ERR_NULL_POINTER, "stream_advance: NULL pointer");
    hipLaunchKernelGGL(stream_advance_kernel, dim3(ceil_div(batch, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pos, batch, n);
    return check_launch("stream_advance");
}

int agx_attention_stream_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t window, char *buf,
                                     size_t buf_len) {
    using namespace agx;
    const AttnStreamPick k = attn_stream_pick("attention_alibi_stream", batch, heads, head_dim, tq, window);
    if (k.code) return k.code;
    if (!buf || buf_len == 0) return fail(AGX_ERR_NULL_POINTER, "agx_attention_stream_kernel_name: NULL buffer");
    snprintf(buf, buf_len, "%s", k.empty ? "none" : k.row->name);
    return AGX_OK;
}

}  // extern "C"
