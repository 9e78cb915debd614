// Causal self-attention with the one-sided ALiBi bias: a query at absolute position p sees the keys j <= p only.
//
//     out[b,h,:,i] = sum_j softmax_j( q_i . k_j / scale_div - slope_h (i + q_pos0 - j) ) v_j,    j in [0, min(i + q_pos0, Tk - 1)]
//
// Build-defined: the reference's Alibi (networks/transformers.py:7-93) is symmetric, -slope_h |i - j| over every key, and has
// no causal branch.  Full causal self-attention is q_pos0 = 0, Tq = Tk = T; a step on a key/value cache that already holds
// Tk - Tq frames is q_pos0 = Tk - Tq.
//
// Layouts (channel-major fp32):  q (B, H*Dh, Tq), rows of pitch Tq;  kv (B, 2*H*Dh, .), K rows first, then V rows, rows of
// pitch kv_row_stride >= Tk (a preallocated cache whose valid length is Tk);  out (B, H*Dh, Tq).  q and kv have their own base
// pointers and batch strides, so a (B, 3*H*Dh, T) qkv tensor is read in place.
//
// The kernels are the shared bodies of attention_masked.hpp under CausalMask (block skipping and the all-masked-block argument
// are written there).  Nothing at or beyond column Tk of a kv row is read.  The backward is that of the full causal
// self-attention (q_pos0 = 0, Tq = Tk = T): q / kv and dq / dkv are reached through base pointers and batch strides (rows of
// pitch T), so qkv is read and dqkv written in place.
#include "attention_masked.hpp"

namespace agx {

template <bool CACHE>
static __device__ __forceinline__ AttnView<CausalMask<CACHE>> causal_view(const float *q, const float *kv, int64_t sq, int64_t skv, int krs,
                                                         const float *dout, int h, int b, int H, int Dh, int Tq, int Tk, int q_pos0) {
    const int HD = H * Dh;
    AttnView<CausalMask<CACHE>> v{};
    v.ql = v.q_end = Tq;
    v.kl = v.k_end = Tk;
    v.q_pos0 = q_pos0;
    v.qg = q + size_t(b) * sq + size_t(h) * Dh * Tq;
    v.kg = kv + size_t(b) * skv + size_t(h) * Dh * krs;
    v.vg = v.kg + size_t(HD) * krs;
    if (dout) v.dg = dout + (size_t(b) * HD + h * Dh) * Tq;   // the backward's dO rows; a forward view has none
    v.pq = v.pd = Tq;
    v.pk = krs;
    v.so = (size_t(b) * H + h) * Tq;
    return v;
}

template <int DVT>
__global__ __launch_bounds__(256) void attention_causal_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                               int64_t sq, int64_t skv, int krs,
                                                               const float *__restrict__ slopes, float *__restrict__ out, int H,
                                                               int Dh, int Tq, int Tk, int q_pos0, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    const auto v = causal_view<true>(q, kv, sq, skv, krs, nullptr, h, b, H, Dh, Tq, Tk, q_pos0);
    attn_fwd_body<DVT>(v, out + (size_t(b) * (H * Dh) + size_t(h) * Dh) * Tq, slopes, h, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_causal_bwd_stats_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                    int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                    const float *__restrict__ dout, float *__restrict__ lse,
                                                                    float *__restrict__ delta, int H, int Dh, int T, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    attn_bwd_stats_body(causal_view<false>(q, kv, sq, skv, T, dout, h, b, H, Dh, T, T, 0), slopes, h, lse, delta, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_causal_bwd_dq_kernel(const float *__restrict__ q, const float *__restrict__ kv, int64_t sq,
                                                                 int64_t skv, const float *__restrict__ slopes,
                                                                 const float *__restrict__ dout, const float *__restrict__ lse,
                                                                 const float *__restrict__ delta, float *__restrict__ dq_out,
                                                                 int64_t sdq, int H, int Dh, int T, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    attn_bwd_dq_body(causal_view<false>(q, kv, sq, skv, T, dout, h, b, H, Dh, T, T, 0), slopes, h, lse, delta,
                     dq_out + size_t(b) * sdq + size_t(h) * Dh * T, T, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_causal_bwd_dkv_kernel(const float *__restrict__ q, const float *__restrict__ kv, int64_t sq,
                                                                  int64_t skv, const float *__restrict__ slopes,
                                                                  const float *__restrict__ dout, const float *__restrict__ lse,
                                                                  const float *__restrict__ delta, float *__restrict__ dkv,
                                                                  int64_t sdkv, int H, int Dh, int T, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    float *dkg = dkv + size_t(b) * sdkv + size_t(h) * Dh * T;
    attn_bwd_dkv_body(causal_view<false>(q, kv, sq, skv, T, dout, h, b, H, Dh, T, T, 0), slopes, h, lse, delta, dkg, dkg + size_t(H * Dh) * T, T,
                      Dh, scale_div);
}

// ------------------------------------------------------------------ host side
static MaskedRow<decltype(&attention_causal_kernel<1>)> kAttnCausalRows[3] = AGX_MASKED_ROWS(causal);
static const char *const kAttnCausalBwdName = "attn_causal_bwd_stats+attn_causal_bwd_dq+attn_causal_bwd_dkv";

static MaskedPick attn_causal_pick(const char *op, int B, int H, int Dh, int Tq, int Tk) {
    return masked_pick(op, B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0, masked_head_dim(op, Dh), Dh, ceil_div(Tq, 128), H, B);
}

}  // namespace agx

extern "C" {

int agx_attention_alibi_causal(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride, int64_t kv_row_stride,
                               const float *slopes, float *out, int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk,
                               int32_t q_pos0, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_causal";
    const MaskedPick k = attn_causal_pick(op, batch, heads, head_dim, tq, tk);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (q_pos0 < 0) return fail(AGX_ERR_BAD_SHAPE, "%s: q_pos0=%d < 0", op, q_pos0);
    if (int64_t(q_pos0) + tq + 128 > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: q_pos0 + tq is beyond int32", op);
    if (kv_row_stride < tk) return fail(AGX_ERR_BAD_SHAPE, "%s: kv row stride %lld < tk=%d", op, (long long)kv_row_stride, tk);
    if (kv_row_stride > 0x7fffffffLL) return fail(AGX_ERR_BAD_SHAPE, "%s: kv row stride %lld is beyond int32", op, (long long)kv_row_stride);
    if (!q || !kv || !slopes || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_strides(op, q_batch_stride, hd * tq, "q")) return rc;
    if (int rc = check_strides(op, kv_batch_stride, 2 * hd * kv_row_stride, "kv")) return rc;
    return masked_launch(kAttnCausalRows[k.di], k, "attention_causal", static_cast<hipStream_t>(stream), q, kv, q_batch_stride,
                         kv_batch_stride, int(kv_row_stride), slopes, out, heads, head_dim, tq, tk, q_pos0, scale_div);
}

size_t agx_attention_causal_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t t) {
    if (batch <= 0 || heads <= 0 || t <= 0) return 0;
    return size_t(2) * batch * heads * t * sizeof(float);
}

int agx_attention_alibi_causal_backward(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                        const float *slopes, const float *out, const float *dout, float *dq, float *dkv,
                                        int64_t dq_batch_stride, int64_t dkv_batch_stride, float *workspace, size_t workspace_bytes,
                                        int32_t batch, int32_t heads, int32_t head_dim, int32_t t, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_causal_backward";
    const MaskedPick k = attn_causal_pick(op, batch, heads, head_dim, t, t);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (!q || !kv || !slopes || !out || !dout || !dq || !dkv || !workspace) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    if (workspace_bytes < agx_attention_causal_backward_workspace_bytes(batch, heads, t))
        return fail(AGX_ERR_WORKSPACE, "%s: workspace too small", op);
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_strides(op, q_batch_stride, hd * t, "q")) return rc;
    if (int rc = check_strides(op, kv_batch_stride, 2 * hd * t, "kv")) return rc;
    if (int rc = check_strides(op, dq_batch_stride, hd * t, "dq")) return rc;
    if (int rc = check_strides(op, dkv_batch_stride, 2 * hd * t, "dkv")) return rc;
    float *lse = workspace, *delta = workspace + size_t(batch) * heads * t;
    const auto head = std::make_tuple(q, kv, q_batch_stride, kv_batch_stride, slopes, dout, lse, delta);
    const auto dims = std::make_tuple(heads, head_dim, t, scale_div);
    static DeviceOnce once[3];
    return masked_launch_backward("attention_causal_backward", once, attn_causal_bwd_stats_kernel, attn_causal_bwd_dq_kernel,
                                  attn_causal_bwd_dkv_kernel, dim3(ceil_div(t, kAttnQB), heads, batch),
                                  dim3(ceil_div(t, kAttnKB), heads, batch), head_dim, static_cast<hipStream_t>(stream),
                                  std::tuple_cat(head, dims), std::tuple_cat(head, std::make_tuple(dq, dq_batch_stride), dims),
                                  std::tuple_cat(head, std::make_tuple(dkv, dkv_batch_stride), dims));
}

int agx_attention_causal_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, int32_t backward,
                                     char *buf, size_t buf_len) {
    using namespace agx;
    const MaskedPick k = attn_causal_pick(backward ? "attention_alibi_causal_backward" : "attention_alibi_causal", batch, heads,
                                          head_dim, tq, tk);
    return masked_name(k, "agx_attention_causal_kernel_name", backward ? kAttnCausalBwdName : kAttnCausalRows[k.di].name, buf, buf_len);
}

}  // extern "C"
