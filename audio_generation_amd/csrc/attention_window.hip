// Sliding-window causal self-attention with the one-sided ALiBi bias: a query at absolute position p = i + q_pos0 sees the
// last W keys, j in [max(0, p - W + 1), p], and nothing else.
//
//     out[b,h,:,i] = sum_j softmax_j( q_i . k_j / scale_div - slope_h (p - j) ) v_j,    j in [max(0, p - W + 1), p]
//
// Build-defined, like the causal form it narrows (attention_causal.hip): W >= p + 1 for every query IS causal attention, W = 1
// returns v_p.  ALiBi needs p - j only, never an absolute position, so the keys may live in a ring: key j sits in column
// j mod ring of a kv row (ring = 0: the linear form, column j), and a stream has no end.
//
// Layouts (channel-major fp32):  q (B, H*Dh, Tq), rows of pitch Tq;  kv (B, 2*H*Dh, .), K rows first, then V rows, rows of
// pitch kv_row_stride;  out (B, H*Dh, Tq).  q and kv have their own base pointers and batch strides, so a (B, 3*H*Dh, T) qkv
// tensor is read in place (linear, q_pos0 = 0).  The keys are the positions 0 .. q_pos0 + Tq - 1: linear needs
// kv_row_stride >= q_pos0 + Tq, a ring needs Tq + min(W - 1, q_pos0) <= ring <= kv_row_stride -- the oldest key the first query
// sees, max(0, q_pos0 - W + 1), must not have been overwritten by the newest, q_pos0 + Tq - 1 (at the start of a stream there is
// nothing older than key 0 to keep).
//
// The kernels are the shared bodies of attention_masked.hpp under WindowMask<true>: block bounds aligned to absolute positions,
// the ring column, and the two hazards the causal kernels did not have (leading all-masked blocks, stale ring columns) are
// written there.  The backward is that of the full windowed self-attention (q_pos0 = 0, Tq = Tk = T, linear kv): stats and dq
// walk the key blocks from the one that holds key max(0, i0 - W + 1) to the last one their 16 queries see; dkv walks the query
// blocks from j0 to min(T, j0 + 63 + W): the queries that see any of its 64 keys.
#include "attention_masked.hpp"

namespace agx {

template <int DVT>
__global__ __launch_bounds__(256) void attention_window_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                               int64_t sq, int64_t skv, int krs,
                                                               const float *__restrict__ slopes, float *__restrict__ out, int H,
                                                               int Dh, int Tq, int q_pos0, int W, int ring, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    auto v = window_view<true>(q, kv, sq, skv, krs, nullptr, h, b, H, Dh, Tq, q_pos0, W, ring);
    v.place(blockIdx.x * 128, Tq);   // the keys this workgroup's 128 queries see
    attn_fwd_body<DVT>(v, out + (size_t(b) * (H * Dh) + size_t(h) * Dh) * Tq, slopes, h, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_window_bwd_stats_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                    int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                    const float *__restrict__ dout, float *__restrict__ lse,
                                                                    float *__restrict__ delta, int H, int Dh, int T, int W,
                                                                    float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    attn_bwd_stats_body(window_view<true>(q, kv, sq, skv, T, dout, h, b, H, Dh, T, 0, W, 0), slopes, h, lse, delta, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_window_bwd_dq_kernel(const float *__restrict__ q, const float *__restrict__ kv, int64_t sq,
                                                                 int64_t skv, const float *__restrict__ slopes,
                                                                 const float *__restrict__ dout, const float *__restrict__ lse,
                                                                 const float *__restrict__ delta, float *__restrict__ dq_out,
                                                                 int64_t sdq, int H, int Dh, int T, int W, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    attn_bwd_dq_body(window_view<true>(q, kv, sq, skv, T, dout, h, b, H, Dh, T, 0, W, 0), slopes, h, lse, delta,
                     dq_out + size_t(b) * sdq + size_t(h) * Dh * T, T, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_window_bwd_dkv_kernel(const float *__restrict__ q, const float *__restrict__ kv, int64_t sq,
                                                                  int64_t skv, const float *__restrict__ slopes,
                                                                  const float *__restrict__ dout, const float *__restrict__ lse,
                                                                  const float *__restrict__ delta, float *__restrict__ dkv,
                                                                  int64_t sdkv, int H, int Dh, int T, int W, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    float *dkg = dkv + size_t(b) * sdkv + size_t(h) * Dh * T;
    attn_bwd_dkv_body(window_view<true>(q, kv, sq, skv, T, dout, h, b, H, Dh, T, 0, W, 0), slopes, h, lse, delta, dkg,
                      dkg + size_t(H * Dh) * T, T, Dh, scale_div);
}

// ------------------------------------------------------------------ host side
static MaskedRow<decltype(&attention_window_kernel<1>)> kAttnWindowRows[3] = AGX_MASKED_ROWS(window);
static const char *const kAttnWindowBwdName = "attn_window_bwd_stats+attn_window_bwd_dq+attn_window_bwd_dkv";

}  // namespace agx

extern "C" {

int agx_attention_alibi_window(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride, int64_t kv_row_stride,
                               const float *slopes, float *out, int32_t batch, int32_t heads, int32_t head_dim, int32_t tq,
                               int64_t q_pos0, int32_t window, int32_t kv_ring, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_window";
    const MaskedPick k = masked_window_pick(op, batch, heads, head_dim, tq, window);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (q_pos0 < 0) return fail(AGX_ERR_BAD_SHAPE, "%s: q_pos0=%lld < 0", op, (long long)q_pos0);
    if (q_pos0 > (int64_t(1) << 62)) return fail(AGX_ERR_BAD_SHAPE, "%s: q_pos0=%lld is beyond 2^62", op, (long long)q_pos0);
    if (kv_ring < 0) return fail(AGX_ERR_BAD_SHAPE, "%s: kv_ring=%d < 0", op, kv_ring);
    if (kv_ring == 0 && kv_row_stride < q_pos0 + tq)
        return fail(AGX_ERR_BAD_SHAPE, "%s: kv row stride %lld < q_pos0 + tq = %lld (linear kv)", op, (long long)kv_row_stride,
                    (long long)(q_pos0 + tq));
    const int64_t span = tq + std::min<int64_t>(window - 1, q_pos0);   // the keys the call reads: max(0, q_pos0 - window + 1) .. q_pos0 + tq - 1
    if (kv_ring > 0 && span > kv_ring)
        return fail(AGX_ERR_BAD_SHAPE, "%s: kv_ring=%d < tq + min(window - 1, q_pos0) = %lld", op, kv_ring, (long long)span);
    if (kv_ring > kv_row_stride) return fail(AGX_ERR_BAD_SHAPE, "%s: kv_ring=%d > kv row stride %lld", op, kv_ring, (long long)kv_row_stride);
    if (kv_row_stride > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: kv row stride %lld is beyond int32", op, (long long)kv_row_stride);
    if (!q || !kv || !slopes || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_strides(op, q_batch_stride, hd * tq, "q")) return rc;
    if (int rc = check_strides(op, kv_batch_stride, 2 * hd * kv_row_stride, "kv")) return rc;
    // No query sees further back than position 0: a window beyond the last position is that position + 1 (and fits int32 below).
    const int64_t w = std::min<int64_t>(window, q_pos0 + tq);
    // The kernel indexes in int32.  On a ring every position may be lowered by a multiple of lcm(64, ring): the 64-key block
    // alignment, the ring column and every p - j stay what they were.  The lowered q_pos0 stays >= w - 1, so that the floor
    // "no key before position 0" still bites nowhere it did not.
    int64_t pos = q_pos0;
    if (kv_ring > 0 && pos > w - 1) {
        const int64_t period = 64 / gcd64(64, kv_ring) * int64_t(kv_ring);
        pos -= (pos - (w - 1)) / period * period;
    }
    if (pos + tq + 128 > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: q_pos0 + tq is beyond int32", op);
    return masked_launch(kAttnWindowRows[k.di], k, "attention_window", static_cast<hipStream_t>(stream), q, kv, q_batch_stride,
                         kv_batch_stride, int(kv_row_stride), slopes, out, heads, head_dim, tq, int(pos), int(w), kv_ring, scale_div);
}

size_t agx_attention_window_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t t) {
    if (batch <= 0 || heads <= 0 || t <= 0) return 0;
    return size_t(2) * batch * heads * t * sizeof(float);
}

int agx_attention_alibi_window_backward(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                        const float *slopes, const float *out, const float *dout, float *dq, float *dkv,
                                        int64_t dq_batch_stride, int64_t dkv_batch_stride, float *workspace, size_t workspace_bytes,
                                        int32_t batch, int32_t heads, int32_t head_dim, int32_t t, int32_t window, float scale_div,
                                        void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_window_backward";
    const MaskedPick k = masked_window_pick(op, batch, heads, head_dim, t, window);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (!q || !kv || !slopes || !out || !dout || !dq || !dkv || !workspace) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    if (workspace_bytes < agx_attention_window_backward_workspace_bytes(batch, heads, t))
        return fail(AGX_ERR_WORKSPACE, "%s: workspace too small", op);
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_strides(op, q_batch_stride, hd * t, "q")) return rc;
    if (int rc = check_strides(op, kv_batch_stride, 2 * hd * t, "kv")) return rc;
    if (int rc = check_strides(op, dq_batch_stride, hd * t, "dq")) return rc;
    if (int rc = check_strides(op, dkv_batch_stride, 2 * hd * t, "dkv")) return rc;
    float *lse = workspace, *delta = workspace + size_t(batch) * heads * t;
    const auto head = std::make_tuple(q, kv, q_batch_stride, kv_batch_stride, slopes, dout, lse, delta);
    const auto dims = std::make_tuple(heads, head_dim, t, std::min(window, t), scale_div);
    static DeviceOnce once[3];
    return masked_launch_backward("attention_window_backward", once, attn_window_bwd_stats_kernel, attn_window_bwd_dq_kernel,
                                  attn_window_bwd_dkv_kernel, dim3(ceil_div(t, kAttnQB), heads, batch),
                                  dim3(ceil_div(t, kAttnKB), heads, batch), head_dim, static_cast<hipStream_t>(stream),
                                  std::tuple_cat(head, dims), std::tuple_cat(head, std::make_tuple(dq, dq_batch_stride), dims),
                                  std::tuple_cat(head, std::make_tuple(dkv, dkv_batch_stride), dims));
}

int agx_attention_window_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t window, int32_t backward,
                                     char *buf, size_t buf_len) {
    using namespace agx;
    const MaskedPick k = masked_window_pick(backward ? "attention_alibi_window_backward" : "attention_alibi_window", batch, heads,
                                          head_dim, tq, window);
    return masked_name(k, "agx_attention_window_kernel_name", backward ? kAttnWindowBwdName : kAttnWindowRows[k.di].name, buf, buf_len);
}

}  // extern "C"
