// Cross-attention with the ALiBi bias: queries of one sequence (length Tq), keys and values of another (length Tk).
//
// networks/transformers.py:165-188 with `cross_attention`:  q = W_q LN(x), k = W_k y, v = W_v y,
//     out[b,h,:,i] = sum_j softmax_j( q_i . k_j / scale_div - slope_h |i - j| ) v_j,    j in [0, Tk)
// with i and j the absolute positions in their own sequences (Alibi._create_M :45-77 builds -slope_h |row - col| for both
// orders of the two context lengths; the formula is symmetric, so the reference's transposed (H, context_y, context_x) shape
// does not change a value).
//
// Layouts (channel-major fp32, as the self-attention block):  q (B, H*Dh, Tq);  kv (B, 2*H*Dh, Tk), K rows first, then V
// rows;  out (B, H*Dh, Tq).  q and kv have their own base pointers and their own batch strides.
//
// The kernels are the shared bodies of attention_masked.hpp under the symmetric mask with ql = Tq, kl = Tk: keys >= Tk are
// masked, queries >= Tq are not stored, every global index is clamped into its own sequence.  (`out` stays in the stats
// kernel's signature for the callers; it is not read.)
#include "attention_masked.hpp"

namespace agx {

using CrossView = AttnView<SymMask<false>>;

static __device__ __forceinline__ CrossView cross_view(const float *q, const float *kv, const float *dout, int h, int b, int H, int Dh,
                                                       int Tq, int Tk) {
    const int HD = H * Dh;
    CrossView v{};
    v.ql = v.q_end = Tq;
    v.kl = v.k_end = Tk;
    v.qg = q + (size_t(b) * HD + h * Dh) * Tq;
    v.kg = kv + (size_t(b) * 2 * HD + h * Dh) * Tk;
    v.vg = v.kg + size_t(HD) * Tk;
    if (dout) v.dg = dout + (size_t(b) * HD + h * Dh) * Tq;   // the backward's dO rows; a forward view has none
    v.pq = v.pd = Tq;
    v.pk = Tk;
    v.so = (size_t(b) * H + h) * Tq;
    return v;
}

template <int DVT>
__global__ __launch_bounds__(256) void attention_cross_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                              const float *__restrict__ slopes, float *__restrict__ out,
                                                              int H, int Dh, int Tq, int Tk, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    const CrossView v = cross_view(q, kv, nullptr, h, b, H, Dh, Tq, Tk);
    attn_fwd_body<DVT>(v, out + (size_t(b) * (H * Dh) + size_t(h) * Dh) * Tq, slopes, h, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_cross_bwd_stats_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                   const float *__restrict__ slopes, const float *__restrict__ out,
                                                                   const float *__restrict__ dout, float *__restrict__ lse,
                                                                   float *__restrict__ delta, int H, int Dh, int Tq, int Tk,
                                                                   float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    attn_bwd_stats_body(cross_view(q, kv, dout, h, b, H, Dh, Tq, Tk), slopes, h, lse, delta, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_cross_bwd_dq_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                const float *__restrict__ slopes, const float *__restrict__ dout,
                                                                const float *__restrict__ lse, const float *__restrict__ delta,
                                                                float *__restrict__ dq_out, int H, int Dh, int Tq, int Tk,
                                                                float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    attn_bwd_dq_body(cross_view(q, kv, dout, h, b, H, Dh, Tq, Tk), slopes, h, lse, delta,
                     dq_out + (size_t(b) * (H * Dh) + h * Dh) * Tq, Tq, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_cross_bwd_dkv_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                 const float *__restrict__ slopes, const float *__restrict__ dout,
                                                                 const float *__restrict__ lse, const float *__restrict__ delta,
                                                                 float *__restrict__ dkv, int H, int Dh, int Tq, int Tk,
                                                                 float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    float *dkg = dkv + (size_t(b) * 2 * (H * Dh) + h * Dh) * Tk;
    attn_bwd_dkv_body(cross_view(q, kv, dout, h, b, H, Dh, Tq, Tk), slopes, h, lse, delta, dkg, dkg + size_t(H * Dh) * Tk, Tk, Dh,
                      scale_div);
}

// ------------------------------------------------------------------ host side
static MaskedRow<decltype(&attention_cross_kernel<1>)> kAttnCrossRows[3] = AGX_MASKED_ROWS(cross);
static const char *const kAttnCrossBwdName = "attn_cross_bwd_stats+attn_cross_bwd_dq+attn_cross_bwd_dkv";

static MaskedPick attn_cross_pick(const char *op, int B, int H, int Dh, int Tq, int Tk) {
    return masked_pick(op, B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0, masked_head_dim(op, Dh), Dh, ceil_div(Tq, 128), H, B);
}

}  // namespace agx

extern "C" {

int agx_attention_alibi_cross(const float *q, const float *kv, const float *slopes, float *out, int32_t batch, int32_t heads,
                              int32_t head_dim, int32_t tq, int32_t tk, float scale_div, void *stream) {
    using namespace agx;
    const MaskedPick k = attn_cross_pick("attention_alibi_cross", batch, heads, head_dim, tq, tk);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (!q || !kv || !slopes || !out) return fail(AGX_ERR_NULL_POINTER, "attention_alibi_cross: NULL pointer");
    return masked_launch(kAttnCrossRows[k.di], k, "attention_cross", static_cast<hipStream_t>(stream), q, kv, slopes, out, heads,
                         head_dim, tq, tk, scale_div);
}

size_t agx_attention_cross_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t tq) {
    if (batch <= 0 || heads <= 0 || tq <= 0) return 0;
    return size_t(2) * batch * heads * tq * sizeof(float);
}

int agx_attention_alibi_cross_backward(const float *q, const float *kv, const float *slopes, const float *out, const float *dout,
                                       float *dq, float *dkv, float *workspace, size_t workspace_bytes, int32_t batch,
                                       int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, float scale_div, void *stream) {
    using namespace agx;
    const MaskedPick k = attn_cross_pick("attention_alibi_cross_backward", batch, heads, head_dim, tq, tk);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    if (!q || !kv || !slopes || !out || !dout || !dq || !dkv || !workspace)
        return fail(AGX_ERR_NULL_POINTER, "attention_alibi_cross_backward: NULL pointer");
    if (workspace_bytes < agx_attention_cross_backward_workspace_bytes(batch, heads, tq))
        return fail(AGX_ERR_WORKSPACE, "attention_alibi_cross_backward: workspace too small");
    float *lse = workspace, *delta = workspace + size_t(batch) * heads * tq;
    const auto dims = std::make_tuple(heads, head_dim, tq, tk, scale_div);
    static DeviceOnce once[3];
    return masked_launch_backward("attention_cross_backward", once, attn_cross_bwd_stats_kernel, attn_cross_bwd_dq_kernel,
                                  attn_cross_bwd_dkv_kernel, dim3(ceil_div(tq, kAttnQB), heads, batch),
                                  dim3(ceil_div(tk, kAttnKB), heads, batch), head_dim, static_cast<hipStream_t>(stream),
                                  std::tuple_cat(std::make_tuple(q, kv, slopes, out, dout, lse, delta), dims),
                                  std::tuple_cat(std::make_tuple(q, kv, slopes, dout, lse, delta, dq), dims),
                                  std::tuple_cat(std::make_tuple(q, kv, slopes, dout, lse, delta, dkv), dims));
}

int agx_attention_cross_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, int32_t backward,
                                    char *buf, size_t buf_len) {
    using namespace agx;
    const MaskedPick k = attn_cross_pick(backward ? "attention_alibi_cross_backward" : "attention_alibi_cross", batch, heads,
                                         head_dim, tq, tk);
    return masked_name(k, "agx_attention_cross_kernel_name", backward ? kAttnCrossBwdName : kAttnCrossRows[k.di].name, buf, buf_len);
}

}  // extern "C"
