// Ragged batches: ALiBi attention (self and cross) with a valid length per batch row for the queries and for the keys, and
// the elementwise tail mask of the transformer block.
//
//     ql = clamp(q_len[b], 0, Tq),  kl = clamp(k_len[b], 0, Tk)        (a NULL array: every row is full)
//     out[b,h,:,i] = sum_{j < kl} softmax_{j < kl}( q_i . k_j / scale_div - slope_h |i - j| ) v_j     for i < ql
//     out[b,h,:,i] = 0                                                   for ql <= i < Tq, and for every i when kl == 0
// Positions are absolute and the padding is on the right.  Nothing at or beyond a row's length reaches a result: q at
// i >= ql, K / V at j >= kl and dout at i >= ql may hold anything, NaN included (the contract of the key/value cache's tail).
// The lengths are read from device memory by every workgroup, so a captured graph replays with the lengths of the replay.
//
// Layouts are those of attention_dropout.hip: q and kv (K rows, then V rows) have their own base pointers and batch strides,
// so a (B, 3*H*Dh, T) qkv tensor is q = qkv, kv = qkv + H*Dh*T with both strides 3*H*Dh*T; dq and dkv likewise.
//
// The backward kernels are the shared bodies of attention_masked.hpp under the symmetric mask with the row's lengths; the
// forward is separate code with the same arithmetic (see at the kernel).  In both, Tq and Tk stay
// the row pitches and the columns the row owns: the cross kernels' arithmetic, so a row of length (ql, kl) computes bit for
// bit what the same kernel computes for that row cropped and run alone with NULL lengths.  Every element of out, dq, dkv and
// the workspace is written.
#include "attention_masked.hpp"

namespace agx {

// the valid length of batch row b: clamp(len[b], 0, t); NULL: the full row
static __device__ __forceinline__ int ragged_len(const int32_t *len, int b, int t) { return len ? min(max(int(len[b]), 0), t) : t; }
// the int64 frame counts of a counted streaming step, clamped the same way
static __device__ __forceinline__ int ragged_len(const int64_t *len, int b, int t) {
    const int64_t v = len[b];
    return int(v < 0 ? 0 : v > t ? t : v);
}

using RaggedView = AttnView<SymMask<true>>;

static __device__ __forceinline__ RaggedView ragged_view(const float *q, const float *kv, int64_t sq, int64_t skv, const int32_t *q_len,
                                                         const int32_t *k_len, const float *dout, int h, int b, int H, int Dh, int Tq,
                                                         int Tk) {
    const int HD = H * Dh;
    RaggedView v{};
    v.ql = ragged_len(q_len, b, Tq);
    v.kl = ragged_len(k_len, b, Tk);
    v.q_end = Tq;
    v.k_end = Tk;
    v.qg = q + size_t(b) * sq + size_t(h) * Dh * Tq;
    v.kg = kv + size_t(b) * skv + size_t(h) * Dh * Tk;
    v.vg = v.kg + size_t(HD) * Tk;
    if (dout) v.dg = dout + (size_t(b) * HD + h * Dh) * Tq;   // the backward's dO rows; a forward view has none
    v.pq = v.pd = Tq;
    v.pk = Tk;
    v.so = (size_t(b) * H + h) * Tq;
    return v;
}

// attention_ragged_kernel<DVT> is NOT an instance of attn_fwd_body: the instance measured about 1 % slower than this hand-written
// kernel on rows with lengths in [T/4, T] (75.0-75.4 -> 75.8-76.3 us), so the forward stays the separate code
// it was: the cross instance's arithmetic with ql / kl wherever a position is compared or clamped.  A fix to attn_fwd_body
// belongs here too.
template <int DVT>
__global__ __launch_bounds__(256) void attention_ragged_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                               int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                               const int32_t *__restrict__ q_len, const int32_t *__restrict__ k_len,
                                                               float *__restrict__ out, int H, int Dh, int Tq, int Tk,
                                                               float scale_div) {
    constexpr int KB = 64;         // keys per block (two 32-key accumulator tiles)
    constexpr int DH = 32 * DVT;   // head_dim rounded up to the tile
    constexpr int VP = KB + 1;     // LDS pitch of the V block
    extern __shared__ __attribute__((aligned(16))) float vs[];   // [2][DH][VP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int HD = H * Dh;
    const int ql = ragged_len(q_len, b, Tq), kl = ragged_len(k_len, b, Tk);
    float *ob = out + (size_t(b) * HD + size_t(h) * Dh) * Tq;
    const int wg0 = blockIdx.x * 128;                  // this workgroup's first query
    if (wg0 >= ql || kl == 0) {                        // workgroup-uniform, before the first barrier: nothing valid to compute
        for (int e = tid; e < Dh * 128; e += 256) {
            const int d = e >> 7, ii = wg0 + (e & 127);
            if (ii < Tq) ob[size_t(d) * Tq + ii] = 0.f;
        }
        return;
    }
    const float *qb = q + size_t(b) * sq + size_t(h) * Dh * Tq;
    const float *kb = kv + size_t(b) * skv + size_t(h) * Dh * Tk;
    const float *vb = kb + size_t(HD) * Tk;
    const int i = wg0 + wave * 32 + li;   // this lane's query
    const int ic = min(i, ql - 1);        // ql >= 1 here
    const float slope = slopes[h], inv_scale = 1.f / scale_div;
    const int nblk = (kl + KB - 1) / KB;

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

    auto stage_v = [&](int blk, float *dst) {   // V[dv < Dh][64 keys of block blk] -> LDS, zeros (never the stored value) outside
        for (int e = tid; e < DH * KB; e += 256) {
            const int dv = e / KB, jj = e - dv * KB, j = blk * KB + jj;
            dst[dv * VP + jj] = (dv < Dh && j < kl) ? vb[size_t(dv) * Tk + j] : 0.f;
        }
    };
    stage_v(0, vs);
    __syncthreads();

    for (int blk = 0; blk < nblk; ++blk) {
        const int j0 = blk * KB;
        float *vcur = vs + (blk & 1) * DH * VP;
        if (blk + 1 < nblk) stage_v(blk + 1, vs + ((blk + 1) & 1) * DH * VP);   // next block streams in meanwhile

        // ---- S^T = K^T Q for this block: rows = keys, columns = queries ----
        f32x16 acc[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t2][r] = 0.f;
        int kcol[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) kcol[t2] = min(j0 + t2 * 32 + li, kl - 1);
#pragma unroll 4
        for (int s = 0; s < DH / 2; ++s) {
            const int d = min(2 * s + lh, Dh - 1);
            float kf[2];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) kf[t2] = kb[size_t(d) * Tk + kcol[t2]];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) acc[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[t2], qf[s], acc[t2], 0, 0, 0);
        }

        // ---- scale, ALiBi, online softmax (in-lane over the 32 registers + one shuffle) ----
        float bm = -INFINITY;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + t2 * 32 + acc_row(r, lh);
                float s = acc[t2][r] * inv_scale - fabsf(float(ic - j)) * slope;
                s = j < kl ? s : -INFINITY;
                acc[t2][r] = s;
                bm = fmaxf(bm, s);
            }
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        const float mn = fmaxf(m, bm);            // finite: every block holds at least one key < kl
        const float alpha = expf(m - mn);         // first block: exp(-inf) = 0
        float bl = 0.f;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pe = expf(acc[t2][r] - mn);
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

    const float inv = 1.f / l;    // kl >= 1 here: l >= 1
    if (i < Tq) {
        const bool valid = i < ql;
#pragma unroll
        for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dv = dt * 32 + acc_row(r, lh);
                if (dv < Dh) ob[size_t(dv) * Tq + i] = valid ? o[dt][r] * inv : 0.f;
            }
    }
}

__global__ __launch_bounds__(256) void attn_ragged_bwd_stats_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                    int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                    const int32_t *__restrict__ q_len, const int32_t *__restrict__ k_len,
                                                                    const float *__restrict__ dout, float *__restrict__ lse,
                                                                    float *__restrict__ delta, int H, int Dh, int Tq, int Tk,
                                                                    float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    attn_bwd_stats_body(ragged_view(q, kv, sq, skv, q_len, k_len, dout, h, b, H, Dh, Tq, Tk), slopes, h, lse, delta, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_ragged_bwd_dq_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                 int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                 const int32_t *__restrict__ q_len, const int32_t *__restrict__ k_len,
                                                                 const float *__restrict__ dout, const float *__restrict__ lse,
                                                                 const float *__restrict__ delta, float *__restrict__ dq_out, int64_t sdq,
                                                                 int H, int Dh, int Tq, int Tk, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    attn_bwd_dq_body(ragged_view(q, kv, sq, skv, q_len, k_len, dout, h, b, H, Dh, Tq, Tk), slopes, h, lse, delta,
                     dq_out + size_t(b) * sdq + size_t(h) * Dh * Tq, Tq, Dh, scale_div);
}

__global__ __launch_bounds__(256) void attn_ragged_bwd_dkv_kernel(const float *__restrict__ q, const float *__restrict__ kv,
                                                                  int64_t sq, int64_t skv, const float *__restrict__ slopes,
                                                                  const int32_t *__restrict__ q_len, const int32_t *__restrict__ k_len,
                                                                  const float *__restrict__ dout, const float *__restrict__ lse,
                                                                  const float *__restrict__ delta, float *__restrict__ dkv, int64_t sdkv,
                                                                  int H, int Dh, int Tq, int Tk, float scale_div) {
    const int h = blockIdx.y, b = blockIdx.z;
    float *dkg = dkv + size_t(b) * sdkv + size_t(h) * Dh * Tk;
    attn_bwd_dkv_body(ragged_view(q, kv, sq, skv, q_len, k_len, dout, h, b, H, Dh, Tq, Tk), slopes, h, lse, delta, dkg,
                      dkg + size_t(H * Dh) * Tk, Tk, Dh, scale_div);
}

// out[b,c,i] = i < clamp(len[b], 0, T) ? x[b,c,i] : 0 over a contiguous (B, C, T) tensor: a select, so a NaN tail gives 0.
// A thread owns four consecutive elements of the flat tensor (one 16-byte access when both pointers allow it), reads all of
// them before it writes any: out may alias x.  x and out are deliberately not __restrict__.
template <typename L>   // int32_t: the lengths of a ragged batch; int64_t: the counts of a counted streaming step
__global__ __launch_bounds__(256) void mask_tail_kernel(const float *x, const L *__restrict__ len, float *out, int64_t n, int C, int T,
                                                        int vec) {
    const int64_t e0 = (int64_t(blockIdx.x) * 256 + threadIdx.x) * 4;
    if (e0 >= n) return;
    int64_t row = e0 / T;            // b * C + c
    int i = int(e0 - row * T);
    int lim = ragged_len(len, int(row / C), T);
    const int cnt = int(min(int64_t(4), n - e0));
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec && cnt == 4) {
        const float4 w = *reinterpret_cast<const float4 *>(x + e0);
        v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
    } else {
        for (int u = 0; u < cnt; ++u) v[u] = x[e0 + u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u >= cnt) break;         // the tensor's last quartet: no row, and no length, beyond the end
        while (i >= T) {             // the quartet runs into the next row (T < 4: more than once)
            i -= T;
            ++row;
            lim = ragged_len(len, int(row / C), T);
        }
        v[u] = i < lim ? v[u] : 0.f;
        ++i;
    }
    if (vec && cnt == 4) {
        *reinterpret_cast<float4 *>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int u = 0; u < cnt; ++u) out[e0 + u] = v[u];
    }
}

// ------------------------------------------------------------------ host side
static MaskedRow<decltype(&attention_ragged_kernel<1>)> kAttnRaggedRows[3] = AGX_MASKED_ROWS(ragged);
static const char *const kAttnRaggedBwdName = "attn_ragged_bwd_stats+attn_ragged_bwd_dq+attn_ragged_bwd_dkv";

static MaskedPick attn_ragged_pick(const char *op, int B, int H, int Dh, int Tq, int Tk) {
    return masked_pick(op, B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0, masked_head_dim(op, Dh), Dh, ceil_div(Tq, 128), H, B);
}

template <typename L>
static int mask_tail(const char *op, const float *x, const L *len, float *out, int32_t batch, int32_t channels, int32_t t, void *stream) {
    if (batch <= 0 || channels <= 0 || t <= 0) return AGX_OK;
    const int64_t n = int64_t(batch) * channels * t;
    const int64_t blocks = ceil_div64(ceil_div64(n, 4), 256);
    if (blocks > 0x7fffffff || int64_t(batch) * channels > 0x7fffffff)
        return fail(AGX_ERR_BAD_SHAPE, "%s: (%d, %d, %d) is beyond the grid", op, batch, channels, t);
    if (!x || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);   // len: NULL = every row is full
    const int vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    hipLaunchKernelGGL(mask_tail_kernel<L>, dim3(unsigned(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), x, len, out, n, channels,
                       t, vec);
    return check_launch(op);
}

}  // namespace agx

extern "C" {

int agx_attention_alibi_ragged(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride, const float *slopes,
                               const int32_t *q_len, const int32_t *k_len, float *out, int32_t batch, int32_t heads, int32_t head_dim,
                               int32_t tq, int32_t tk, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_ragged";
    const MaskedPick k = attn_ragged_pick(op, batch, heads, head_dim, tq, tk);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_strides(op, q_batch_stride, hd * tq, "q")) return rc;
    if (int rc = check_strides(op, kv_batch_stride, 2 * hd * tk, "kv")) return rc;
    if (!q || !kv || !slopes || !out) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);   // q_len / k_len: NULL = full
    return masked_launch(kAttnRaggedRows[k.di], k, "attention_ragged", static_cast<hipStream_t>(stream), q, kv, q_batch_stride,
                         kv_batch_stride, slopes, q_len, k_len, out, heads, head_dim, tq, tk, scale_div);
}

size_t agx_attention_ragged_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t tq) {
    if (batch <= 0 || heads <= 0 || tq <= 0) return 0;
    return size_t(2) * batch * heads * tq * sizeof(float);
}

int agx_attention_alibi_ragged_backward(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                        const float *slopes, const int32_t *q_len, const int32_t *k_len, const float *out,
                                        const float *dout, float *dq, float *dkv, int64_t dq_batch_stride, int64_t dkv_batch_stride,
                                        float *workspace, size_t workspace_bytes, int32_t batch, int32_t heads, int32_t head_dim,
                                        int32_t tq, int32_t tk, float scale_div, void *stream) {
    using namespace agx;
    const char *op = "attention_alibi_ragged_backward";
    const MaskedPick k = attn_ragged_pick(op, batch, heads, head_dim, tq, tk);
    if (k.code) return k.code;
    if (k.empty) return AGX_OK;
    const int64_t hd = int64_t(heads) * head_dim;
    if (int rc = check_strides(op, q_batch_stride, hd * tq, "q")) return rc;
    if (int rc = check_strides(op, kv_batch_stride, 2 * hd * tk, "kv")) return rc;
    if (int rc = check_strides(op, dq_batch_stride, hd * tq, "dq")) return rc;
    if (int rc = check_strides(op, dkv_batch_stride, 2 * hd * tk, "dkv")) return rc;
    if (workspace_bytes < agx_attention_ragged_backward_workspace_bytes(batch, heads, tq))
        return fail(AGX_ERR_WORKSPACE, "%s: workspace too small", op);
    if (!q || !kv || !slopes || !out || !dout || !dq || !dkv || !workspace) return fail(AGX_ERR_NULL_POINTER, "%s: NULL pointer", op);
    float *lse = workspace, *delta = workspace + size_t(batch) * heads * tq;
    const auto head = std::make_tuple(q, kv, q_batch_stride, kv_batch_stride, slopes, q_len, k_len, dout, lse, delta);
    const auto dims = std::make_tuple(heads, head_dim, tq, tk, scale_div);
    static DeviceOnce once[3];
    return masked_launch_backward("attention_ragged_backward", once, attn_ragged_bwd_stats_kernel, attn_ragged_bwd_dq_kernel,
                                  attn_ragged_bwd_dkv_kernel, dim3(ceil_div(tq, kAttnQB), heads, batch),
                                  dim3(ceil_div(tk, kAttnKB), heads, batch), head_dim, static_cast<hipStream_t>(stream),
                                  std::tuple_cat(head, dims), std::tuple_cat(head, std::make_tuple(dq, dq_batch_stride), dims),
                                  std::tuple_cat(head, std::make_tuple(dkv, dkv_batch_stride), dims));
}

int agx_attention_ragged_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, int32_t backward,
                                     char *buf, size_t buf_len) {
    using namespace agx;
    const MaskedPick k = attn_ragged_pick(backward ? "attention_alibi_ragged_backward" : "attention_alibi_ragged", batch, heads,
                                          head_dim, tq, tk);
    return masked_name(k, "agx_attention_ragged_kernel_name", backward ? kAttnRaggedBwdName : kAttnRaggedRows[k.di].name, buf, buf_len);
}

int agx_mask_tail(const float *x, const int32_t *len, float *out, int32_t batch, int32_t channels, int32_t t, void *stream) {
    return agx::mask_tail("mask_tail", x, len, out, batch, channels, t, stream);
}

int agx_mask_tail_counted(const float *x, const int64_t *counts, float *out, int32_t batch, int32_t channels, int32_t t, void *stream) {
    if (!counts && batch > 0 && channels > 0 && t > 0) return agx::fail(AGX_ERR_NULL_POINTER, "mask_tail_counted: NULL counts");
    return agx::mask_tail("mask_tail_counted", x, counts, out, batch, channels, t, stream);
}

}  // extern "C"
