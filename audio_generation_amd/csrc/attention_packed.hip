// Packed variable-length batches: symmetric ALiBi attention (self and cross) over sequences concatenated along the time
// axis, and the two layout kernels that move a right-padded (B, C, T) batch into the packed (C, N) form and back.
//
//     q0 = clamp(cu_q[s], 0, nq),  q1 = clamp(cu_q[s + 1], q0, nq),  ql = min(q1 - q0, max_q)      (cu_k / nk / max_k likewise)
//     out[h,:,q0 + i] = sum_{j < kl} softmax_{j < kl}( q_{q0+i} . k_{k0+j} / scale_div - slope_h |i - j| ) v_{k0+j}    for i < ql
//     out[h,:,q0 + i] = 0                                                 for i < ql when kl == 0
//     out[h,:,n]      = 0                                                 for n < clamp(cu_q[0]) and n >= clamp(cu_q[n_seq])
// Positions are relative to the sequence's own start.  Sequence s is blockIdx.z = s; blockIdx.z = n_seq is the slack: the
// columns no sequence owns.  The cu arrays are read from device memory by every workgroup, so a captured graph replays with
// the partition of the replay.  Memory safety does not depend on what they hold: every start and end is clamped into the
// tensor, an end to at least its start, a length to the host-known bound that sized the grid.  For arrays that break the
// contract (decreasing, a first entry that is not 0 -- the columns before it count as slack --, or a sequence longer than
// the bound) the values are unspecified and some columns may stay unwritten, but no access leaves the tensors.
//
// q has H*Dh rows of pitch sq >= nq; kv has K rows then V rows, 2*H*Dh of them, of pitch skv >= nk; out is contiguous
// (H*Dh, nq); dq / dkv have pitches of their own.
//
// The kernels are the shared bodies of attention_masked.hpp under the symmetric mask with the sequence's lengths, the base
// pointers advanced by the sequence's start and the row pitch decoupled from the length; the slack workgroups are handled
// here, before a view exists.  Key and query blocks are aligned to the sequence's start, not to the absolute column, and the
// arithmetic of every element is the ragged kernels', so sequence s computes bit for bit what agx_attention_alibi_ragged
// computes for that sequence cropped and run alone with NULL lengths.  A workgroup beyond its sequence's length owns no column
// (q_end = ql), returns before its first barrier and writes nothing: those columns belong to a neighbour.
#include "attention_masked.hpp"

namespace agx {

struct PackedSpan { int start, len; };

// sequence s of a cu array over n columns: start and end clamped into [0, n], the end to at least the start, the length to cap
static __device__ __forceinline__ PackedSpan packed_span(const int32_t *cu, int s, int n, int cap) {
    const int a = min(max(int(cu[s]), 0), n);
    const int b = min(max(int(cu[s + 1]), a), n);
    return {a, min(b - a, cap)};
}

// the slack of a cu array over n columns: [0, lo) and [hi, n)
static __device__ __forceinline__ void packed_slack(const int32_t *cu, int n_seq, int n, int &lo, int &hi) {
    lo = min(max(int(cu[0]), 0), n);
    hi = min(max(int(cu[n_seq]), 0), n);
}

// rows [0, rows) of pitch `pitch`, slack columns := 0; the workgroups (blockIdx.x of gridDim.x) share the columns
static __device__ __forceinline__ void packed_zero_slack(float *base, int64_t pitch, int rows, int lo, int hi, int n) {
    const int cols = lo + (n - hi);                     // slack columns: c < lo -> c, else hi + (c - lo)
    const int64_t total = int64_t(rows) * cols;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
        const int r = int(e / cols), c = int(e - int64_t(r) * cols);
        base[int64_t(r) * pitch + (c < lo ? c : hi + (c - lo))] = 0.f;
    }
}

using PackedView = AttnView<SymMask<true>, int64_t, int64_t, int>;

// the view of sequence sidx < n_seq (the slack workgroups, sidx == n_seq, must not come here: cu[n_seq + 1] does not exist)
static __device__ __forceinline__ PackedView packed_view(const float *q, const float *kv, int64_t sq, int64_t skv, const int32_t *cu_q,
                                                         const int32_t *cu_k, const float *dout, int h, int sidx, int H, int Dh, int nq,
                                                         int nk, int max_q, int max_k, PackedSpan &qs, PackedSpan &ks) {
    qs = packed_span(cu_q, sidx, nq, max_q);
    ks = packed_span(cu_k, sidx, nk, max_k);
    PackedView v{};
    v.ql = v.q_end = qs.len;
    v.kl = v.k_end = ks.len;
    v.qg = q + size_t(h) * Dh * sq + qs.start;
    v.kg = kv + size_t(h) * Dh * skv + ks.start;
    v.vg = v.kg + size_t(H * Dh) * skv;
    if (dout) v.dg = dout + size_t(h) * Dh * nq + qs.start;   // the backward's dO rows; a forward view has none
    v.pq = sq;
    v.pk = skv;
    v.pd = nq;
    v.so = size_t(h) * nq + qs.start;
    return v;
}

template <int DVT>
__global__ __launch_bounds__(256) void attention_packed_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                               int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                               const int32_t *__restrict__ cu_q, const int32_t *__restrict__ cu_k,
                                                               float *__restrict__ out, int n_seq, int H, int Dh, int nq, int nk,
                                                               int max_q, int max_k, float scale_div) {
    const int h = blockIdx.y, sidx = blockIdx.z;
    if (sidx == n_seq) {                               // the slack workgroups of this head: zeros, no barrier
        int lo, hi;
        packed_slack(cu_q, n_seq, nq, lo, hi);
        packed_zero_slack(out + size_t(h) * Dh * nq, nq, Dh, lo, hi, nq);
        return;
    }
    PackedSpan qs, ks;
    const PackedView v = packed_view(q, kv, sq, skv, cu_q, cu_k, nullptr, h, sidx, H, Dh, nq, nk, max_q, max_k, qs, ks);
    attn_fwd_body<DVT>(v, out + size_t(h) * Dh * nq + qs.start, slopes, h, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_packed_bwd_stats_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                    int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                    const int32_t *__restrict__ cu_q, const int32_t *__restrict__ cu_k,
                                                                    const float *__restrict__ dout, float *__restrict__ lse,
                                                                    float *__restrict__ delta, int n_seq, int H, int Dh, int nq, int nk,
                                                                    int max_q, int max_k, float scale_div) {
    const int h = blockIdx.y, sidx = blockIdx.z;
    if (sidx == n_seq) {            // the slack of lse / delta: every float of the workspace is written
        int lo, hi;
        packed_slack(cu_q, n_seq, nq, lo, hi);
        packed_zero_slack(lse + size_t(h) * nq, nq, 1, lo, hi, nq);
        packed_zero_slack(delta + size_t(h) * nq, nq, 1, lo, hi, nq);
        return;
    }
    PackedSpan qs, ks;
    attn_bwd_stats_body(packed_view(q, kv, sq, skv, cu_q, cu_k, dout, h, sidx, H, Dh, nq, nk, max_q, max_k, qs, ks), slopes, h, lse, delta,
                        Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_packed_bwd_dq_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                 int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                 const int32_t *__restrict__ cu_q, const int32_t *__restrict__ cu_k,
                                                                 const float *__restrict__ dout, const float *__restrict__ lse,
                                                                 const float *__restrict__ delta, float *__restrict__ dq_out, int64_t sdq,
                                                                 int n_seq, int H, int Dh, int nq, int nk, int max_q, int max_k,
                                                                 float scale_div) {
    const int h = blockIdx.y, sidx = blockIdx.z;
    if (sidx == n_seq) {             // the slack columns of dQ: exactly 0
        int lo, hi;
        packed_slack(cu_q, n_seq, nq, lo, hi);
        packed_zero_slack(dq_out + size_t(h) * Dh * sdq, sdq, Dh, lo, hi, nq);
        return;
    }
    PackedSpan qs, ks;
    const PackedView v = packed_view(q, kv, sq, skv, cu_q, cu_k, dout, h, sidx, H, Dh, nq, nk, max_q, max_k, qs, ks);
    attn_bwd_dq_body(v, slopes, h, lse, delta, dq_out + size_t(h) * Dh * sdq + qs.start, sdq, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_packed_bwd_dkv_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                  int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                  const int32_t *__restrict__ cu_q, const int32_t *__restrict__ cu_k,
                                                                  const float *__restrict__ dout, const float *__restrict__ lse,
                                                                  const float *__restrict__ delta, float *__restrict__ dkv, int64_t sdkv,
                                                                  int n_seq, int H, int Dh, int nq, int nk, int max_q, int max_k,
                                                                  float scale_div) {
    const int h = blockIdx.y, sidx = blockIdx.z;
    const int HD = H * Dh;
    if (sidx == n_seq) {             // the slack columns of dK and dV: exactly 0
        int lo, hi;
        packed_slack(cu_k, n_seq, nk, lo, hi);
        packed_zero_slack(dkv + size_t(h) * Dh * sdkv, sdkv, Dh, lo, hi, nk);
        packed_zero_slack(dkv + (size_t(HD) + size_t(h) * Dh) * sdkv, sdkv, Dh, lo, hi, nk);
        return;
    }
    PackedSpan qs, ks;
    const PackedView v = packed_view(q, kv, sq, skv, cu_q, cu_k, dout, h, sidx, H, Dh, nq, nk, max_q, max_k, qs, ks);
    float *dkg = dkv + size_t(h) * Dh * sdkv + ks.start;
    attn_bwd_dkv_body(v, slopes, h, lse, delta, dkg, dkg + size_t(HD) * sdkv, sdkv, Dh, scale_div);
}

// ------------------------------------------------------------------ layout kernels
constexpr int PR_CH = 8;     // channels per thread

// out[c, n] = x[b, c, n - start_b] where sequence b owns column n and n - start_b < t; 0 where no sequence does.  One thread
// per packed column and PR_CH channels: it finds its sequence by bisection over cu (the index stays in [0, n_seq] whatever
// the array holds), checks the ownership it found, then walks its channels.
__global__ __launch_bounds__(256) void pack_rows_kernel(const float *__restrict__ x, const int32_t *__restrict__ cu,
                                                        float *__restrict__ out, int B, int C, int T, int N) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    int lo = 0, hi = B;              // the last b in [0, B) with clamp(cu[b]) <= n, if any
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (min(max(int(cu[mid]), 0), N) <= n) lo = mid; else hi = mid;
    }
    const PackedSpan sp = packed_span(cu, lo, N, T);
    const int i = n - sp.start;
    const bool own = i >= 0 && i < sp.len;
    const int c0 = blockIdx.y * PR_CH;
    const float *xb = x + (size_t(lo) * C + c0) * T + (own ? i : 0);
#pragma unroll
    for (int u = 0; u < PR_CH; ++u)
        if (c0 + u < C) out[size_t(c0 + u) * N + n] = own ? xb[size_t(u) * T] : 0.f;
}

// out[b, c, i] = i < len_b ? xp[c, start_b + i] : 0: a select on the index, the padded positions read nothing
__global__ __launch_bounds__(256) void unpack_rows_kernel(const float *__restrict__ xp, const int32_t *__restrict__ cu,
                                                          float *__restrict__ out, int B, int C, int T, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
    if (i >= T) return;
    const PackedSpan sp = packed_span(cu, b, N, T);
    const bool own = i < sp.len;
    const int c0 = blockIdx.y * PR_CH;
    const float *src = xp + size_t(c0) * N + sp.start + (own ? i : 0);
    float *dst = out + (size_t(b) * C + c0) * T + i;
#pragma unroll
    for (int u = 0; u < PR_CH; ++u)
        if (c0 + u < C) dst[size_t(u) * T] = own ? src[size_t(u) * N] : 0.f;
}

// ------------------------------------------------------------------ host side
static MaskedRow<decltype(&attention_packed_kernel<1>)> kAttnPackedRows[3] = AGX_MASKED_ROWS(packed);
static const char *const kAttnPackedBwdName = "attn_packed_bwd_stats+attn_packed_bwd_dq+attn_packed_bwd_dkv";

// the grid's x extent for sequences of up to `bound` positions in blocks of `block`: at least one, for the slack workgroups
static int packed_blocks(int bound, int block) { return bound > 0 ? ceil_div(bound, block) : 1; }

static MaskedPick attn_packed_pick(const char *op, int n_seq, int H, int Dh, int nq, int nk, int max_q, int max_k) {
    int code = masked_head_dim(op, Dh);
    if (!code && (max_q < 0 || max_k < 0)) code = fail(AGX_ERR_BAD_SHAPE, "%s: max_q=%d, max_k=%d: a bound is >= 0", op, max_q, max_k);
    // the grid's z extent is n_seq + 1 (z = n_seq: the slack workgroups); from n_seq = 65535 on it is beyond the grid and
    // masked_pick refuses it -- 65536 stands in for every such n_seq + 1, which would overflow at INT_MAX
    const int gz = n_seq >= 65535 ? 65536 : n_seq + 1;
    return masked_pick(op, n_seq <= 0 || H <= 0 || nq <= 0 || nk <= 0, code, Dh, packed_blocks(std::min(max_q, nq), 128), H, gz);
}

// the shapes both layout kernels accept; *empty: no output element exists, nothing to launch (out_n: the output is the packed
// tensor; the padded one exists with n == 0 too and is then all padding)
static int pack_rows_check(const char *op, int B, int C, int T, int N, bool out_n, bool *empty) {
    *empty = B <= 0 || C <= 0 || T <= 0 || (out_n ? N <= 0 : N < 0);
    if (*empty) return AGX_OK;
    if (B >= 65535 || ceil_div(C, PR_CH) > 65535) return fail(AGX_ERR_BAD_SHAPE, "%s: (%d, %d, %d) is beyond the grid", op, B, C, T);
    return AGX_OK;
}

}  // namespace agx

extern "C" {

int agx_attention_alibi_packed(const float *q, const float *kv, int64_t q_row_stride, int64_t kv_row_stride, const float *slopes,
                               const int32_t *cu_q, const int32_t *cu_k, float *out, int32_t n_seq, int32_t heads, int32_t head_dim,
                               int32_t nq, int32_t nk, int32_t max_q, int32_t max_k, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_packed";
    const MaskedPick k = attn_packed_pick(op, n_seq, heads, head_dim, nq, nk, max_q, max_k);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (int rc = check_strides(op, q_row_stride, nq, "q", "row")) return rc;
    if (int rc = check_strides(op, kv_row_stride, nk, "kv", "row")) return rc;
    if (!q || !kv || !slopes || !cu_q || !cu_k || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    return masked_launch(kAttnPackedRows[k.di], k, "attention_packed", static_cast<hipStream_t>(stream), q, kv, q_row_stride, kv_row_stride,
                         slopes, cu_q, cu_k, out, n_seq, heads, head_dim, nq, nk, max_q, max_k, scale_div);
}

size_t agx_attention_packed_backward_workspace_bytes(int32_t heads, int32_t nq) {
    if (heads <= 0 || nq <= 0) return 0;
    return size_t(2) * heads * nq * sizeof(float);
}

int agx_attention_alibi_packed_backward(const float *q, const float *kv, int64_t q_row_stride, int64_t kv_row_stride,
                                        const float *slopes, const int32_t *cu_q, const int32_t *cu_k, const float *out,
                                        const float *dout, float *dq, float *dkv, int64_t dq_row_stride, int64_t dkv_row_stride,
                                        float *workspace, size_t workspace_bytes, int32_t n_seq, int32_t heads, int32_t head_dim,
                                        int32_t nq, int32_t nk, int32_t max_q, int32_t max_k, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_packed_backward";
    const MaskedPick k = attn_packed_pick(op, n_seq, heads, head_dim, nq, nk, max_q, max_k);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (int rc = check_strides(op, q_row_stride, nq, "q", "row")) return rc;
    if (int rc = check_strides(op, kv_row_stride, nk, "kv", "row")) return rc;
    if (int rc = check_strides(op, dq_row_stride, nq, "dq", "row")) return rc;
    if (int rc = check_strides(op, dkv_row_stride, nk, "dkv", "row")) return rc;
    if (workspace_bytes < agx_attention_packed_backward_workspace_bytes(heads, nq))
        return fail(AGX_ERR_WORKSPACE, "%s: workspace too small", op);
    (void)out;   // not read: P is recomputed from the row statistics
    if (!q || !kv || !slopes || !cu_q || !cu_k || !dout || !dq || !dkv || !workspace) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    float *lse = workspace, *delta = workspace + size_t(heads) * nq;
    const auto head = std::make_tuple(q, kv, q_row_stride, kv_row_stride, slopes, cu_q, cu_k, dout, lse, delta);
    const auto dims = std::make_tuple(n_seq, heads, head_dim, nq, nk, max_q, max_k, scale_div);
    static DeviceOnce once[3];
    return masked_launch_backward("attention_packed_backward", once, attn_packed_bwd_stats_kernel, attn_packed_bwd_dq_kernel,
                                  attn_packed_bwd_dkv_kernel, dim3(packed_blocks(std::min(max_q, nq), kAttnQB), heads, n_seq + 1),
                                  dim3(packed_blocks(std::min(max_k, nk), kAttnKB), heads, n_seq + 1), head_dim,
                                  static_cast<hipStream_t>(stream), std::tuple_cat(head, dims),
                                  std::tuple_cat(head, std::make_tuple(dq, dq_row_stride), dims),
                                  std::tuple_cat(head, std::make_tuple(dkv, dkv_row_stride), dims));
}

int agx_attention_packed_kernel_name(int32_t n_seq, int32_t heads, int32_t head_dim, int32_t nq, int32_t nk, int32_t max_q,
                                     int32_t max_k, int32_t backward, char *buf, size_t buf_len) {
    using namespace agx;
    const MaskedPick k = attn_packed_pick(backward ? "attention_alibi_packed_backward" : "attention_alibi_packed", n_seq, heads,
                                              head_dim, nq, nk, max_q, max_k);
    return masked_name(k, "agx_attention_packed_kernel_name", backward ? kAttnPackedBwdName : kAttnPackedRows[k.di].name, buf, buf_len);
}

int agx_pack_rows(const float *x, const int32_t *cu, float *out, int32_t batch, int32_t channels, int32_t t, int32_t n, void *stream) {
    using namespace agx;
    bool empty;
    if (int rc = pack_rows_check("pack_rows", batch, channels, t, n, true, &empty)) return rc;
    if (empty) return AGX_OK;
    if (!x || !cu || !out) return fail(AGX_ERR_NULL_POINTER, "pack_rows: NULL pointer");
    hipLaunchKernelGGL(pack_rows_kernel, dim3(ceil_div(n, 256), ceil_div(channels, PR_CH)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       cu, out, batch, channels, t, n);
    return check_launch("pack_rows");
}

int agx_unpack_rows(const float *xp, const int32_t *cu, float *out, int32_t batch, int32_t channels, int32_t t, int32_t n, void *stream) {
    using namespace agx;
    bool empty;
    if (int rc = pack_rows_check("unpack_rows", batch, channels, t, n, false, &empty)) return rc;
    if (empty) return AGX_OK;
    if ((!xp && n > 0) || !cu || !out) return fail(AGX_ERR_NULL_POINTER, "unpack_rows: NULL pointer");   // n == 0: xp is never read
    hipLaunchKernelGGL(unpack_rows_kernel, dim3(ceil_div(t, 256), ceil_div(channels, PR_CH), batch), dim3(256), 0,
                       static_cast<hipStream_t>(stream), xp, cu, out, batch, channels, t, n);
    return check_launch("unpack_rows");
}

}  // extern "C"
