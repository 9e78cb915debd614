/* agx.h -- flat C ABI of the MI355X-native neural-audio-codec forward path.
 *
 * This is the drop-in boundary.  The reference has no FFI of its own: its hot
 * path is a chain of ATen calls made from torch.nn.Modules.  Each entry point
 * below replaces the ATen call sequence of one reference function (cited per
 * declaration, paths relative to the reference tree); INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory the caller owns; the library
 *     never allocates, frees or retains a pointer past the call;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *     launches are asynchronous on it and the library never synchronises;
 *   - return value 0 = success, negative = error (AGX_ERR_*); the message of the
 *     last error of the calling thread is returned by agx_last_error();
 *   - tensors are contiguous fp32, "NCL" (batch, channel, time) unless said
 *     otherwise; indices are int64 to match torch.argmin.
 *
 * Pointer alignment, family by family (tests/test_gpu_memory_contract.py::test_operand_placement runs each
 * with its operands 4, 8 and 12 bytes past a 16-byte boundary and requires the bits of the aligned run):
 *   - convolutions, forward (agx_conv_forward, agx_conv_forward_planes, agx_conv_pack*, agx_planes_split): operands
 *     need 4-byte alignment only (bf16 planes: 4-byte as well); the result does not depend on it;
 *   - fused residual block (agx_resblock_forward, agx_resblock_forward_q4): operands need 4-byte alignment only; the
 *     result does not depend on it;
 *   - convolutions, backward (agx_conv_bwd_data*, agx_conv_bwd_weight, agx_conv_grouped_bwd_*): operands need 4-byte
 *     alignment only; the result does not depend on it;
 *   - Conv2d (agx_conv2d_*): operands need 4-byte alignment only; the result does not depend on it;
 *   - RVQ (agx_rvq_forward*, agx_rvq_ema_stats, agx_rvq_dequantize): fp32 operands need 4-byte alignment only, int64
 *     indices and the float64 workspace 8-byte; the result does not depend on it;
 *   - LayerNorm and ALiBi attention (agx_layernorm_ct*, agx_attention_alibi*): operands need 4-byte alignment only;
 *     the result does not depend on it;
 *   - wavelet fold, multires and group sum (agx_wavelet_fold*, agx_multires_*, agx_group_sum): operands need 4-byte
 *     alignment only; the result does not depend on it;
 *   - discriminator ops (agx_spectral_*, agx_reduce_mean*, agx_feature_means*, agx_avgpool1d*, agx_sigmoid*):
 *     operands need 4-byte alignment only; the result does not depend on it (the loss reductions use 16-byte loads
 *     when every pointer allows and 4-byte loads of the same elements in the same order otherwise);
 *   - spectral and signal ops (agx_stft*, agx_fdft_*, agx_preemphasis, agx_lowpass_biquad, agx_resample): operands need 4-byte
 *     alignment only; the result does not depend on it;
 *   - bitstream and time folding (agx_codes_*, agx_time_fold, agx_time_unfold): int64 codes need 8-byte alignment,
 *     fp32 tensors 4-byte, the packed stream none; the result does not depend on it.
 * This is about operands (inputs, parameters, outputs, in/out buffers).  A workspace is 16-byte aligned, as every
 * device allocation is (8-byte where a declaration says so).  No entry point refuses a pointer for its alignment.
 */
#ifndef AGX_H
#define AGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_VERSION 122 /* still 122 with the RVQ streaming step (agx_rvq_step_packet_bytes, agx_rvq_step_workspace_bytes, agx_rvq_step_encode, agx_rvq_step_decode), with the dropout entry points (agx_attention_alibi_dropout, agx_attention_alibi_dropout_backward, agx_attention_dropout_backward_workspace_bytes, agx_attention_dropout_kernel_name, agx_dropout_add) and with the cross-attention entry points (agx_attention_alibi_cross, agx_attention_alibi_cross_backward, agx_attention_cross_backward_workspace_bytes, agx_attention_cross_kernel_name): the ABI only grew -- no existing symbol, struct or meaning changed, so a binding made for 122 keeps working and the number stays; 122: agx_attention_kernel_name, agx_attention_backward_kernel_name (which attention kernel the forward / backward entry points run); 121: agx_conv_bwd_weight_kernel_name, agx_conv2d_bwd_weight_kernel_name, agx_conv_grouped_bwd_weight_kernel_name (kernel, operand copy, contraction slices and items of the weight-gradient ops); 120: activation planes (agx_planes_bytes / agx_planes_split / agx_conv_forward_planes / agx_conv_planes_supported): pre-split bf16x3 input of the decoder's resampling convs; conv_p one-phase geometries (k = 1, "same" k = 11 / 3) with GELU / residual epilogues; 119: agx_rvq_verify_counts + knob rvq_verify (debug: the full defining search beside the fast path); agx_rvq_debug_stamps and the b3_dbg 7/8/9 bound knobs exist in the probe build only; 118: agx_feature_means(_backward) (the feature-matching pair in one pass); 117: agx_rvq_debug_stamps (diagnostic); 116: agx_multires_backward, agx_layernorm_ct one-pass kernel (same signature); agx_rvq_forward (legacy form) needs the workspace of agx_rvq_workspace_bytes since 114; 115: agx_rvq_ema_stats, agx_conv2d_bwd_data_kernel_name; 114: agx_attention_alibi_backward_ex (any T), agx_rvq_forward_ex; 113: tile images (resblock_p / conv_p), agx_attention_alibi_ex, agx_sizeof_*; 0.1.1: agx_conv_desc gained groups / padding (zero = old behaviour); 111: resample, conv2d column split */

#define AGX_OK 0
#define AGX_ERR_BAD_SHAPE (-1)
#define AGX_ERR_NULL_POINTER (-2)
#define AGX_ERR_WORKSPACE (-3)
#define AGX_ERR_LAUNCH (-4)
#define AGX_ERR_UNSUPPORTED (-5)

int agx_version(void);
const char *agx_last_error(void);

/* sizeof() of the two descriptor structs as THIS library was compiled: a binding (ctypes / cgo / JNI stub) asserts
 * its own struct size against these once at load time, so that a descriptor that gained a field cannot be read
 * past the end of a caller's shorter struct. */
int32_t agx_sizeof_conv_desc(void);
int32_t agx_sizeof_conv2d_desc(void);

/* Diagnostic tuning knobs (A/B experiments from one process; defaults are the
 * shipped configuration).  Unknown names return AGX_ERR_BAD_SHAPE.  Process-wide relaxed atomics read at launch
 * time: changing one while another thread launches is defined but pointless -- set them before the first launch.
 *   "rb_cc"  16 | 32   channels per LDS chunk of the fused residual block
 *   "rb_wgs" 0 | 1..3  cap on resident workgroups per CU of the fused residual block (0 = natural)
 *   "rb_sched" 0|1|2   phase scheduling of the fused residual block (csrc/mfma_tile.hpp)
 *   "rb_occ" 2|3       3: fused residual block built under a 168-VGPR cap (3 waves/SIMD); no gain measured
 *   "conv_short" 0|1   128x64 MFMA conv tiles when the 128x128 grid is under two workgroups per CU (default 1)
 *   "conv_cc" 0|8|16|32  force the LDS channel chunk of the MFMA conv (0 = table)
 *   "patch_tie" 0|1      2-D patch tiles: tie between equally padded R x WF splits goes to the fewest staged elements (1) or the widest (0)
 *   "bf_sched" -1|0|1|2  schedule of the bf16x3 main loop of the fused residual block (-1 = per-shape table)
 *   "dw_direct" 0..3   1-D weight gradient on the barrier-free LDS-DMA kernel: 3 every dense layer (default; strided / transposed
 *                      ones through a phase-split copy of x / dy), 2 the stride-1 layers, 1 the k = 1 layers, 0 none
 *   "dw2_direct" 0|1|2 conv2d weight gradient on the barrier-free LDS-DMA kernel: 1 stride-1 "same" layers, 2 (default) also the
 *                      column-strided layers (x through its column-phase planes), 0 the staged kernel everywhere
 *   "dw1_wgs" N        workgroups the 1-D barrier-free weight-gradient kernel aims for (default 768)
 *   "dw_wgs" n         workgroups the conv2d weight-gradient kernel aims for (default 1536)
 *   "dw2_prepad" 0|1   conv2d weight gradient of feature maps narrower than 32 columns: 1 (default) the shared kernel on zero-padded,
 *                      phase-split, flattened copies of x and dy; 0 the staged kernel
 *   "c2b3_sl" -1|0|3..7  bf16x3 Conv2d ring kernel, split of a tile into R rows of 2^SL columns: 0 (default) the split with the least
 *                      padded area x (matrix time + input staging rounds), -1 the least padded area alone, 3..7 forced
 *   "dw2_bf" 0|1       conv2d weight gradient of AGX_IMPL_MFMA_BF16X3 descriptors on the shared kernel: 1 (default) bf16x3
 *                      contraction (both operands split in registers), 0 the fp32 contraction
 *   "dw_xcd" 0|1       conv2d weight gradient: 0 (default); 1 = XCD-aware block order -- the tiles of one contraction slice share
 *                      an L2 (measured SLOWER: 106.6 -> 95.1 TFLOP/s on the 128 -> 128 3 x 3 layer)
 *   "rvq_verify" 0|1   DEBUG: 1 = every agx_rvq_forward(_ex) launch is followed by a checker kernel that runs the full DEFINING
 *                      search (binary64, oracle/rvq_exact.c) of every (frame, stage) on the residual the fast path searched and
 *                      counts the indices that differ (agx_rvq_verify_counts); tens of milliseconds per call at config S
 *   "conv_shape" 0|1   1: 128x128 conv tiles as four row-waves of 1x4 fragments
 *   "rb_q4" 0|1        fused residual block on the fp32 ring kernel: 1 (default) agx_resblock_q4_supported answers 1 where the
 *                      channel count has channel-quad variants, 0 nowhere (the in-process A/B switch of the quad layout)
 *   "rb_impl" 0|1      fused residual block: 1 (default) the persistent ring kernel (csrc/resblock_p.hip) where it applies,
 *                      0 the first kernel (csrc/resblock_mfma.hip) everywhere
 *   "conv_impl" 0|1    resampling / stride-1 1-D layers and the Conv2d layers the ring kernel has a geometry for (forward and
 *                      backward-data): 1 (default) the persistent ring kernel (csrc/conv_p.hip), 0 conv_mfma.hip
 *   "dw2_shared" 0|1|2 conv2d weight gradient: the tiles fetch their operands once per workgroup (two LDS slots, one barrier per
 *                      item): 1 the 128 x 128 tiles, 2 (default) also the 64- and 32-row tiles, 0 wave-private buffers
 *   (the diagnostics of the experiments DESIGN 4.11 lists as dropped -- a DMA-only wave, start staggers, deferred stores --
 *    were removed together with their code)                                                                */
int agx_set_tuning(const char *name, int32_t value);
int agx_get_tuning(const char *name);

/* ------------------------------------------------------------------------- *
 * Convolutions                                                               *
 * ------------------------------------------------------------------------- */

/* Which reference layer a convolution descriptor stands for. */
#define AGX_CONV_CAUSAL 0   /* CausalConv1d,          networks/vae.py:14-43  */
#define AGX_CONV_TRANSPOSED 1 /* CausalConvT1d,       networks/vae.py:45-64  */
#define AGX_CONV_UPSAMPLE 2 /* CausalUpsampleConv1d,  networks/vae.py:66-89  */
#define AGX_CONV_SAME 3     /* Conv1d(padding="same"), networks/wavelets.py:193-201 */
#define AGX_CONV_PADDED 4 /* torch.nn.Conv1d(padding=p, stride, dilation, groups): discriminator.py:33-41 */

/* Which kernel family executes it (AGX_IMPL_AUTO picks by shape). */
#define AGX_IMPL_AUTO 0
#define AGX_IMPL_DIRECT 1 /* fp32 VALU, any shape                            */
#define AGX_IMPL_MFMA 2   /* fp32-input MFMA implicit GEMM (exact fp32 FMA chain) */
#define AGX_IMPL_MFMA_BF16X3 3 /* operands split into 3 bf16 pieces, 6 bf16 MFMAs per product block: fp32-class
                               * accuracy (~1e-7 rel.), not the bitwise fp32 chain; dense 1-D layers with
                               * Cin % 16 == 0 and q*Cout >= 32; its own packed image (agx_conv_pack with this impl) */

/* Epilogue flags (fused into the conv kernel; all optional). */
#define AGX_EPI_LEAKY_PRE 1  /* LeakyReLU(slope) on (acc + bias)   vae.py:99,125,156 */
#define AGX_EPI_RESIDUAL 2   /* += res[b,co,t]                     vae.py:117        */
#define AGX_EPI_LEAKY_POST 4 /* LeakyReLU(slope) after the add     vae.py:131-134    */
#define AGX_EPI_GELU_PRE 8   /* exact (erf) GELU on (acc + bias)   transformers.py:216, wavelets.py:96 */
#define AGX_EPI_MASK 16      /* backward only: v *= (mask[o] > 0 ? 1 : slope), the LeakyReLU gradient     */

typedef struct agx_conv_desc {
    int32_t kind;      /* AGX_CONV_*                                              */
    int32_t batch;     /* B                                                       */
    int32_t c_in;      /* input channels                                          */
    int32_t c_out;     /* output channels                                         */
    int32_t l_in;      /* input length                                            */
    int32_t kernel;    /* K (reference kernel_size)                               */
    int32_t stride;    /* conv stride (CAUSAL) or up-factor (TRANSPOSED/UPSAMPLE) */
    int32_t dilation;  /* CAUSAL only, else 1                                     */
    int32_t epilogue;  /* OR of AGX_EPI_*                                         */
    float slope;       /* LeakyReLU negative slope (reference: 0.1)               */
    int32_t impl;      /* AGX_IMPL_*                                              */
    int32_t groups;    /* PADDED only: conv groups (0 or 1 = dense); grouped layers run on the direct kernel */
    int32_t padding;   /* PADDED only: zeros on both sides (torch Conv1d padding=)  */
} agx_conv_desc;

/* Output length of the layer exactly as the reference computes it
 * (vae.py:32-43 incl. _calc_extra_pad; vae.py:58-64; vae.py:86-89).  <0 on error. */
int64_t agx_conv_out_len(const agx_conv_desc *d);

/* Number of floats of the packed weight image of this layer. */
int64_t agx_conv_packed_floats(const agx_conv_desc *d);

/* Fold weight-norm and repack one conv layer's weight for the kernels.
 *   v : the reference parameter `weight_v` (or the plain `weight` when g == NULL),
 *       torch layout: (c_out, c_in, K) for CAUSAL/UPSAMPLE/SAME, (c_in, c_out, K)
 *       for TRANSPOSED;
 *   g : `weight_g` (dim0,1,1) or NULL.  w = g * v / ||v||, norm over all dims but
 *       0 -- utils.py:34-42 (torch.nn.utils.weight_norm, dim=0);
 *   packed : agx_conv_packed_floats(d) floats.  UPSAMPLE layers are stored as the
 *       `stride` polyphase 3-tap filters of the nearest-upsample + conv pair. */
int agx_conv_pack(const agx_conv_desc *d, const float *v, const float *g, float *packed,
                  void *stream);

/* y = epilogue(conv(x) + bias).  x (B,c_in,l_in); y,res (B,c_out,l_out);
 * bias (c_out) or NULL; res only read when AGX_EPI_RESIDUAL is set.
 * Replaces F.pad + conv1d (vae.py:34-37), conv_transpose1d + crop (vae.py:61-64),
 * interpolate + conv1d (vae.py:86-89). */
int agx_conv_forward(const agx_conv_desc *d, const float *x, const float *packed,
                     const float *bias, const float *res, float *y, void *stream);

/* ---- backward of a conv layer (training.py:380 loss.backward()) ------------
 * The gradient w.r.t. the layer INPUT is the same polyphase convolution with the channel roles
 * swapped and the taps re-indexed (stride-1 convs: flipped kernel; strided convs: transposed-conv
 * phase form; polyphase up-convs: a strided conv), so it runs on the forward kernels with its own
 * packed image:
 *   dx = [mask-gradient]( [add] + conv_bwd(dy) )
 * d is the FORWARD descriptor of the layer (its epilogue field is ignored).
 *   dy   (B, c_out, l_out)  gradient w.r.t. the layer's linear output (pre-activation)
 *   add  (B, c_in, l_in) or NULL: accumulated first (residual branch of vae.py:117)
 *   mask (B, c_in, l_in) or NULL: the layer input as saved by the forward (= the previous layer's
 *        post-LeakyReLU output); the result is multiplied by its activation gradient (1 or slope)
 *   dx   (B, c_in, l_in) */
int64_t agx_conv_bwd_packed_floats(const agx_conv_desc *d);
int agx_conv_pack_bwd(const agx_conv_desc *d, const float *v, const float *g, float *packed, void *stream);
int agx_conv_bwd_data(const agx_conv_desc *d, const float *dy, const float *packed_bwd, const float *add,
                      const float *mask, float slope, float *dx, void *stream);

/* Gradients w.r.t. the layer's parameters.  x (B,c_in,l_in) is the saved layer input, dy the gradient
 * w.r.t. the linear output; v/g are the weight-norm parameters as in agx_conv_pack (g NULL = plain weight).
 * Writes dv (shape of v), dg (dim0) when g != NULL, dbias (c_out) when dbias != NULL.  The time x batch
 * contraction runs on the fp32 MFMA in slices reduced in a fixed order (deterministic). */
size_t agx_conv_bwd_weight_workspace_bytes(const agx_conv_desc *d);
int agx_conv_bwd_weight(const agx_conv_desc *d, const float *x, const float *dy, const float *v, const float *g,
                        float *dv, float *dg, float *dbias, void *workspace, size_t workspace_bytes,
                        void *stream);
/* What agx_conv_bwd_weight runs for `d` (host only):
 * "<kernel instantiation> cfg=<geometry> op=<none|phase_x|phase_dy> slices=<contraction slices> items=<work items>".
 * op names the operand copy made first (phase-split x of a strided layer, phase-split dy of an upsampling /
 * transposed one); items are 32-position chunks (direct kernels, cfg 10..14: slice k takes the contiguous range
 * [k per, (k + 1) per), per = ceil(items / slices)) or 64-position tiles (staged kernel, cfg 0..2). */
int agx_conv_bwd_weight_kernel_name(const agx_conv_desc *d, char *buf, size_t buf_len);

/* Name of the kernel family/tile variant agx_conv_forward would launch for this
 * descriptor (e.g. "conv_mfma<2,2,2,2,16>"), for profilers and bench.py; matches
 * the template arguments in the rocprofv3 kernel names.  Launcher and name query read one selection, so a
 * descriptor the launcher refuses (an impl value that does not exist) gets the launcher's error code and message
 * here too -- as from the three name queries below. */
int agx_conv_kernel_name(const agx_conv_desc *d, char *buf, size_t buf_len);

/* Fused CausalResidualBlock1d + trailing activation (vae.py:113-117 wrapped by
 * the Sequential(..., activation) of vae.py:130-135 / 193-198):
 *   y = leaky( x + conv_k1( leaky( conv_kK,dil(x) + b1 ) ) + b2 )
 * d describes conv1 (kind CAUSAL, stride 1, c_in == c_out; its epilogue field is
 * ignored); packed1/packed2 are the packed images of conv1 and of the k=1 conv2.
 * post_act = 0 skips the trailing activation.  Shapes without a single-kernel
 * implementation run as two fused-epilogue conv launches through `workspace`
 * (agx_resblock_workspace_bytes(d) bytes; the hidden activation). */
size_t agx_resblock_workspace_bytes(const agx_conv_desc *d);
/* Kernel name agx_resblock_forward would launch ("resblock_mfma<..>" when fused,
 * "2x:<conv kernel>" for the two-launch form). */
int agx_resblock_kernel_name(const agx_conv_desc *d, char *buf, size_t buf_len);
int agx_resblock_forward(const agx_conv_desc *d, const float *x, const float *packed1,
                         const float *bias1, const float *packed2, const float *bias2,
                         float *y, int32_t post_act, void *workspace, size_t workspace_bytes,
                         void *stream);

/* Channel quads: a second fp32 activation format carried BETWEEN consecutive residual blocks at inference,
 *   q4[b][C/4][L][4]        element (b, c, t) at ((b * C/4 + c/4) * L + t) * 4 + c % 4
 * -- the four consecutive channels an MFMA accumulator register quad holds at one time step are 16 consecutive bytes, so the
 * fp32 ring kernel (csrc/resblock_p.hip) loads the residual and stores its tile without the LDS transposition of its tile
 * tail, and reads its B operand as 16-byte LDS words.  Same arithmetic in the same order: bit-identical to agx_resblock_forward.
 * agx_resblock_q4_supported: 1 when the block runs on the fp32 ring kernel and its channel count has the quad variants
 * (knob "rb_q4" = 0: 0 everywhere).  agx_resblock_forward_q4: x / y are in quads where x_is_q4 / y_is_q4 != 0 and [B][C][L]
 * otherwise; error conventions of agx_resblock_forward, AGX_ERR_UNSUPPORTED (nothing launched) where the query answers 0.
 * The workspace arguments are accepted for symmetry and unused. */
int agx_resblock_q4_supported(const agx_conv_desc *d);
int agx_resblock_forward_q4(const agx_conv_desc *d, const float *x, const float *packed1,
                            const float *bias1, const float *packed2, const float *bias2,
                            float *y, int32_t post_act, int32_t x_is_q4, int32_t y_is_q4,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- *
 * Residual vector quantiser (external `som_quantizer.ResidualQuantizer`;      *
 * call sites vae.py:245-251, 315-318, 333)                                   *
 * ------------------------------------------------------------------------- */

/* Packed codebook image: per stage the transposed codebook (D,K), the squared
 * norms (K) and max norm; floats needed for Q stages. */
int64_t agx_rvq_packed_floats(int32_t n_q, int32_t k, int32_t dim);
int agx_rvq_pack(const float *codebooks /* (Q,K,D) */, int32_t n_q, int32_t k, int32_t dim,
                 float *packed, void *stream);
/* The same for stages with different codebook sizes (the reference takes one size per quantizer, vae.py:233):
 * codebooks is (Q, K, D) with K = the largest stage, sizes[q] <= K (HOST array, NULL = all K) the number of real
 * codewords of stage q; rows beyond it are padding that agx_rvq_forward can never select.  Q <= 64. */
int agx_rvq_pack_sized(const float *codebooks, const int32_t *sizes, int32_t n_q, int32_t k, int32_t dim, float *packed,
                       void *stream);

/* Nearest-codeword search over q_used residual stages.
 *   x, xq   : frames, element (b,t,d) at  b*stride_b + t*stride_t + d*stride_d
 *             (so both "b l c" and "b c l" tensors are accepted without a copy);
 *   index   : (B,T,q_used) int64, contiguous (utils.py:249);
 *   sq_err  : q_used doubles, = sum over all elements of the squared residual
 *             left after each stage (written, not accumulated; commit loss =
 *             sum(sq_err)/(B*T*D)), reduced over the workgroups in a fixed order
 *             by a second tiny kernel -- deterministic, no float atomics;
 *   workspace: agx_rvq_workspace_bytes() bytes (the per-workgroup partial sums).
 * The arg-min is exact: scores on the bf16 matrix pipe (two pieces per operand) only select candidates under an
 * error bound (fp32 terms: rigorous; the bf16 MFMA's accumulation term: 35 x 2^-24 per instruction, what the aligned-truncation model of the
 * instruction proves -- the model is an empirical characterisation, see the knob "rvq_verify"); ties and near ties are decided by the defining
 * binary64 arithmetic (oracle/rvq_exact.c).
 * One workgroup keeps the fp32 residuals and the bf16 pieces of 32 frames in LDS: D <= 560 (AGX_ERR_UNSUPPORTED beyond). */
size_t agx_rvq_workspace_bytes(int32_t batch, int32_t t, int32_t dim, int32_t k, int32_t q_used);
int agx_rvq_forward(const float *x, int64_t x_sb, int64_t x_st, int64_t x_sd,
                    const float *codebooks /* (Q,K,D) */, const float *packed,
                    int32_t batch, int32_t t, int32_t dim, int32_t k, int32_t q_used,
                    float *xq, int64_t q_sb, int64_t q_st, int64_t q_sd,
                    int64_t *index, double *sq_err, void *workspace, size_t workspace_bytes,
                    void *stream);
/* The same; additionally writes the commit loss sum(sq_err) / (B*T*D) as one float to `commit_loss` (may be NULL). */
int agx_rvq_forward_ex(const float *x, int64_t x_sb, int64_t x_st, int64_t x_sd,
                    const float *codebooks /* (Q,K,D) */, const float *packed,
                    int32_t batch, int32_t t, int32_t dim, int32_t k, int32_t q_used,
                    float *xq, int64_t q_sb, int64_t q_st, int64_t q_sd,
                    int64_t *index, double *sq_err, float *commit_loss, void *workspace, size_t workspace_bytes,
                    void *stream);

/* Assignment statistics of the EMA codebook update (`update_codebook=True`, vae.py:315-318; the update rule itself is
 * build-defined): stats (q_used, K, D+1): [q][k][0] = number of frames whose stage-q index is k, [q][k][1+d] = the
 * sum of their stage-q residuals, added in a fixed order (deterministic; no atomics).  frames (N, D) contiguous, index
 * (N, q_used) int64, codebooks (Q >= q_used, K, D) BEFORE the update.  D <= 1024.  workspace: the per-stage residuals,
 * agx_rvq_ema_workspace_bytes() bytes. */
size_t agx_rvq_ema_workspace_bytes(int64_t n_frames, int32_t dim, int32_t q_used);
int agx_rvq_ema_stats(const float *frames, const float *codebooks, const int64_t *index, float *stats, int64_t n_frames,
                      int32_t dim, int32_t k, int32_t q_used, void *workspace, size_t workspace_bytes, void *stream);

/* Backward of the quantiser's training call (build-defined like the rest of its training semantics).  With
 * N = B*T frames, idx = the indices agx_rvq_forward returned, r_0 = x, r_{q+1} = fl32(r_q - c_q[idx[.][q]]) (the search's
 * residual chain), L = sum_{q < q_used} mean(r_{q+1}^2) (the commit loss of agx_rvq_forward_ex), the suffix sums
 * S_{Q-1} = r_Q, S_q = fl32(S_{q+1} + r_{q+1}) and a = 2 * g_commit / (N * D):
 *   dx[n]          = g_xq[n] + a * S_0[n]                            (straight-through term + commitment term)
 *   dcodebooks[q][k] = -a * sum over {n : idx[n][q] == k} of S_q[n]  (rows in frame order, fixed tree: deterministic, no
 *                    atomics); exactly 0 for codes no frame chose and for stages >= q_used.
 *   x, g_xq, dx : element (b,t,d) at b*stride_b + t*stride_t + d*stride_d, each with its own strides; g_xq NULL = zero;
 *   g_commit    : ONE float on the device (no host read: the call can be captured), NULL = zero;
 *   index       : (N, q_used) int64 contiguous; an index outside [0, K) contributes nothing;
 *   codebooks, dcodebooks : (n_q, K, D) contiguous, q_used <= n_q <= 64; dcodebooks NULL = not wanted (an EMA codebook);
 *   workspace   : the S_q, [q][n][D] floats -- exactly 4 * q_used * N * D bytes, no rounding (agx_rvq_backward_workspace_bytes;
 *                 0 for a non-positive argument).  Read and written only when dcodebooks is given; may be NULL otherwise.
 * q_used == 0: dx = g_xq (or zero), dcodebooks = 0.  D <= 1024 (AGX_ERR_UNSUPPORTED beyond).  Everything is validated
 * before the device is touched. */
size_t agx_rvq_backward_workspace_bytes(int64_t n_frames, int32_t dim, int32_t q_used);
int agx_rvq_backward(const float *x, int64_t x_sb, int64_t x_st, int64_t x_sd, const float *codebooks, const int64_t *index,
                     const float *g_xq, int64_t g_sb, int64_t g_st, int64_t g_sd, const float *g_commit,
                     int32_t batch, int32_t t, int32_t dim, int32_t k, int32_t n_q, int32_t q_used,
                     float *dx, int64_t d_sb, int64_t d_st, int64_t d_sd, float *dcodebooks,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---- Per-row stage counts through the training call: quantiser dropout -----------------------------------------
 * stages is a contiguous int64 (B,) device tensor read by the kernels, never by the host, as in the 4.25 block:
 * q_b = clamp(stages[b], 0, q_used), stage q of frame (b, t) is live when q < q_b, and NULL means q_b = q_used for every row --
 * then the two calls ARE agx_rvq_forward_ex and agx_rvq_backward, the same kernels and the same bits.  The search is greedy, so
 * row b of a staged call is exactly row b quantised alone with q_used = q_b.
 *
 * agx_rvq_forward_staged: agx_rvq_forward_ex with stages after index.
 *   index   : (B, T, q_used); the code where live, -1 where not.
 *   xq      : ((0 + c_0) + c_1) + .. + c_{q_b - 1} in binary32, stage order; exact 0 for q_b == 0.
 *   sq_err  : sq_err[q] = sum over the frames live at stage q of the squared residual left after that stage; exact 0.0 when no
 *             frame is live.  commit_loss = sum_q sq_err[q] / (B T D): the mean over rows of what each row's own q_used = q_b
 *             call returns.
 *   The search still runs all q_used stages for every frame (one workgroup's 32 frames may belong to different rows, and
 *   skipping would save nothing that matters): launches, refusals, LDS and workspace are those of agx_rvq_forward_ex.
 * agx_rvq_backward_staged: agx_rvq_backward with stages after index; index as agx_rvq_forward_staged wrote it.  The residual
 *   chain and the suffix sums S_q of frame (b, t) run over its live stages only:
 *   dx[b, t]         = g_xq[b, t] + a S_0[b, t]  (g_xq alone when q_b == 0), a = 2 g_commit / (B T D) unchanged;
 *   dcodebooks[q][k] = -a * sum of S_q over the frames live at q that chose k (the order and tree of agx_rvq_backward); exact 0
 *                      for rows nobody chose and stages no row runs.
 *   This is not agx_rvq_backward on the masked index: there an index of -1 subtracts nothing but the stage's residual still
 *   enters the loss.  Workspace rows S_q of dead stages are not written (and never read).
 * Both validate everything before the first launch. */
int agx_rvq_forward_staged(const float *x, int64_t x_sb, int64_t x_st, int64_t x_sd,
                           const float *codebooks /* (Q,K,D) */, const float *packed,
                           int32_t batch, int32_t t, int32_t dim, int32_t k, int32_t q_used,
                           float *xq, int64_t q_sb, int64_t q_st, int64_t q_sd,
                           int64_t *index, const int64_t *stages /* may be NULL */, double *sq_err, float *commit_loss,
                           void *workspace, size_t workspace_bytes, void *stream);
int agx_rvq_backward_staged(const float *x, int64_t x_sb, int64_t x_st, int64_t x_sd, const float *codebooks,
                            const int64_t *index, const int64_t *stages /* may be NULL */, const float *g_xq, int64_t g_sb,
                            int64_t g_st, int64_t g_sd, const float *g_commit, int32_t batch, int32_t t, int32_t dim, int32_t k,
                            int32_t n_q, int32_t q_used, float *dx, int64_t d_sb, int64_t d_st, int64_t d_sd, float *dcodebooks,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- *
 * Activation planes (bf16x3 arithmetic, round 4)                              *
 * ------------------------------------------------------------------------- *
 * A bf16x3 layer multiplies three bf16 pieces x = h + m + l of every fp32 operand.  Splitting the INPUT is per-element
 * vector work that every consumer tile repeats (a polyphase up-conv with M = q Cout rows re-splits the same input tile
 * M / 128 times).  "Activation planes" are that split done ONCE, by the producer: for an activation (B, C, L), C % 8 == 0,
 *     planes[b][C / 8][piece 3][L][8]   bf16   (piece 0 = h, 1 = m, 2 = l;  h + m + l == x exactly)
 * -- 6 bytes per element (1.5 x fp32), a cell of 8 channels x 1 time step = 16 bytes, so a consumer stages a 16-channel
 * chunk of its input tile as six contiguous row pieces by LDS-DMA: no register staging, no vector work.
 *   agx_planes_bytes           size of the planes of a (batch, channels, length) activation (0: bad shape)
 *   agx_planes_split           fp32 (B, C, L) contiguous -> planes (a bandwidth-bound pass; producers with a planes
 *                              output write them from their epilogue instead)
 *   agx_conv_planes_supported  0: this descriptor cannot take planes; 1: it can READ planes (AGX_IMPL_MFMA_BF16X3 layers
 *                              with the ring form: CausalUpsampleConv1d x2 / x4 / x5 / x8, CausalConvT1d k7 s1,
 *                              vae.py:45-89); 2: it can also WRITE its output as planes (one output phase)
 *   agx_conv_forward_planes    agx_conv_forward with x given as planes; y_planes != NULL (code 2 layers): the output is
 *                              written as planes [B][Cout / 8][3][Lout][8] INSTEAD of fp32 (y may then be NULL).
 *                              Results are bit-identical to agx_conv_forward on the fp32 input (same pieces, same order). */
size_t agx_planes_bytes(int32_t batch, int32_t channels, int32_t length);
int agx_planes_split(const float *x, void *planes, int32_t batch, int32_t channels, int32_t length, void *stream);
int agx_conv_planes_supported(const agx_conv_desc *d);
int agx_conv_forward_planes(const agx_conv_desc *d, const void *x_planes, const float *packed, const float *bias, float *y,
                            void *y_planes, void *stream);

/* Diagnostic (not part of the reference surface), PROBE BUILD ONLY (-DAGX_RVQ_PROBE: `python tools/rvq_stamps.py build` writes
 * lib/libagx_rvq_probe.so; the product library returns AGX_ERR_UNSUPPORTED and keeps no pointer between calls): the next
 * agx_rvq_forward launches write s_memtime stamps of workgroup w into
 * device_buffer[w * 16 + slot] (64-bit each; slots 0 / 1 / 15 = kernel start / end of the stage loop / kernel end, 2..13 = the
 * phase boundaries of residual stage `stage`, 14 = the (frame, candidate) pairs that went to the binary64 distance).  NULL = off. */
int agx_rvq_debug_stamps(void *device_buffer, int32_t stage);

/* Verify mode (knob "rvq_verify" = 1; debug).  out3[0] = codes where the fast path's index differs from the full defining search
 * run on the same residual, out3[1] = frames with at least one such code, out3[2] = codes checked -- accumulated over every
 * agx_rvq_forward(_ex) launch since the last reset.  Synchronises the device (a blocking copy).  out3 may be NULL (reset only). */
int agx_rvq_verify_counts(int64_t *out3, int32_t reset);

/* quantizers[i].dequantize(idx) (vae.py:333): out[n,:] (+)= codebook[idx[n],:].
 * out element (n,d) at n*stride_n + d*stride_d. */
int agx_rvq_dequantize(const float *codebook /* (K,D) */, const int64_t *idx, int64_t n,
                       int32_t k, int32_t dim, float *out, int64_t o_sn, int64_t o_sd,
                       int32_t accumulate, void *stream);

/* ------------------------------------------------------------------------- *
 * Attention bottleneck (networks/transformers.py:7-279), channel-major layout *
 * ------------------------------------------------------------------------- *
 * The block runs on (B, C, T) tensors -- the layout the encoder produces -- so
 * every Linear is an agx_conv_forward with kernel 1 (AGX_EPI_GELU_PRE /
 * AGX_EPI_RESIDUAL fuse the FFN activation and both residual adds). */

/* torch.nn.LayerNorm over the channel dim of a (B, C, T) tensor
 * (transformers.py:159 and :214): y = (x - mean) / sqrt(var + eps) * w + b. */
int agx_layernorm_ct(const float *x, const float *weight, const float *bias, float *y,
                     int32_t batch, int32_t channels, int32_t t, float eps, void *stream);

/* softmax(Q K^T / scale_div + M) V per (batch, head) with the ALiBi bias
 * M[h,i,j] = -slopes[h] * |i - j| computed in the kernel (transformers.py:175-188;
 * Alibi :38-39, 62-75).  qkv is (B, 3*H*Dh, T): q rows [0,H*Dh), k rows
 * [H*Dh, 2*H*Dh), v rows [2*H*Dh, 3*H*Dh), head-major inside each.  out is
 * (B, H*Dh, T).  fp32-input MFMA for both contractions (exact fp32), any T: a single-pass kernel for T <= 256, the
 * online-softmax (flash) form over key blocks beyond.  Dh <= 128. */
int agx_attention_alibi(const float *qkv, const float *slopes, float *out, int32_t batch,
                        int32_t heads, int32_t head_dim, int32_t t, float scale_div, void *stream);
/* The same with a choice of arithmetic: AGX_ATTN_FP32 (as above) or AGX_ATTN_BF16 -- operands rounded to bf16, both
 * contractions on the bf16 MFMA with fp32 accumulation, fp32 softmax (BASELINE config 3; flash form at every T).
 * `flash` != 0 forces the flash form for fp32 at T <= 256 too (tests). */
#define AGX_ATTN_FP32 0
#define AGX_ATTN_BF16 1
int agx_attention_alibi_ex(const float *qkv, const float *slopes, float *out, int32_t batch, int32_t heads,
                           int32_t head_dim, int32_t t, float scale_div, int32_t precision, int32_t flash, void *stream);
/* Host-only: the kernel instantiation agx_attention_alibi_ex runs for these arguments, from the selection the launcher uses --
 * "attention_alibi<NJ,DVT>" (single pass: fp32, not flash, t <= 256), "attention_bf16_lds<DVT>" (bf16 with K and V of a
 * (head, item) staged in LDS) or "attention_flash<DVT,PREC>" -- or the launcher's refusal (code and message) for a shape it
 * refuses.  The name is truncated to buf_len - 1 characters. */
int agx_attention_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t t, int32_t precision, int32_t flash,
                              char *buf, size_t buf_len);

/* Cross-attention (transformers.py:165-188 with `cross_attention`): queries of one sequence, keys and values of another,
 *     out[b,h,:,i] = sum_j softmax_j( q_i . k_j / scale_div - slopes[h] * |i - j| ) v_j,   j in [0, tk)
 * with i and j the absolute positions in their own sequences (Alibi._create_M :45-77; the reference stores the bias
 * transposed, (H, context_y, context_x), which changes no value: the formula is symmetric).  q is (B, H*Dh, tq); kv is
 * (B, 2*H*Dh, tk), k rows [0, H*Dh), v rows [H*Dh, 2*H*Dh), head-major inside each; out is (B, H*Dh, tq).  fp32-input
 * MFMA for both contractions, online softmax over 64-key blocks (csrc/attention_cross.hip), any tq >= 1 and tk >= 1,
 * Dh <= 128 (AGX_ERR_UNSUPPORTED beyond).  batch, heads, tq or tk <= 0: returns AGX_OK and launches nothing. */
int agx_attention_alibi_cross(const float *q, const float *kv, const float *slopes, float *out, int32_t batch, int32_t heads,
                              int32_t head_dim, int32_t tq, int32_t tk, float scale_div, void *stream);
/* Backward of agx_attention_alibi_cross: dq (B, H*Dh, tq) and dkv (B, 2*H*Dh, tk) from q, kv, the forward's `out` and dout
 * (B, H*Dh, tq).  Three deterministic kernels (row statistics over tq, dQ per 16-query block, dK / dV per 64-key block; P is
 * recomputed from the row statistics, no atomics): two calls on the same inputs agree bit for bit.  workspace: lse + delta
 * = 2 * batch * heads * tq floats = agx_attention_cross_backward_workspace_bytes() bytes (AGX_ERR_WORKSPACE when shorter);
 * every float of it is written.  Empty shapes as above. */
size_t agx_attention_cross_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t tq);
int agx_attention_alibi_cross_backward(const float *q, const float *kv, const float *slopes, const float *out, const float *dout,
                                       float *dq, float *dkv, float *workspace, size_t workspace_bytes, int32_t batch,
                                       int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, float scale_div, void *stream);
/* Host-only: the kernel agx_attention_alibi_cross runs for this shape, "attention_cross<DVT>" (DVT = 1 / 2 / 4 32-row tiles of
 * the head dim), with backward != 0 the three kernels of agx_attention_alibi_cross_backward, "none" for an empty shape, or
 * the launcher's refusal (code and message).  The name is truncated to buf_len - 1 characters. */
int agx_attention_cross_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, int32_t backward,
                                    char *buf, size_t buf_len);

/* Dropout masks (transformers.py:185, :191, :217, :219 in training mode).  No mask tensor is ever stored: a mask is a pure
 * function of its arguments, regenerated by every kernel that needs it (the backward kernels regenerate the forward's).
 *   Generator.  Philox4x32-10, standard constants: multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments 0x9E3779B9 /
 *     0xBB67AE85; one round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
 *     (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then both key words take their increment; ten rounds;
 *     the output is the four 32-bit words of the final counter.
 *   Key.  k0 = the low, k1 = the high 32 bits of `seed`.
 *   Keep rule.  An element is kept iff its word >= thresh, thresh = min(2^32 - 1, floor(p * 2^32 + 1/2)); kept values are
 *     multiplied by scale = (float)(1 / (1 - p)), both computed on the host in double.  0 <= p < 1 (AGX_ERR_BAD_SHAPE
 *     otherwise); p = 0 keeps every element at scale 1.
 *   Attention element (b, h, i, j), i the query and j the key position (absolute, in their own sequences): counter
 *     (j >> 2, i, b * heads + h, stream_id), word j & 3 -- the same for all four attention kernels, whatever their tiling.
 *   Elementwise element e (the linear index in the contiguous tensor): counter (low32(e >> 2), high32(e >> 2), 0,
 *     stream_id), word e & 3.
 * `stream_id` names the call site, so that sites sharing a seed draw independent masks.  There is no parity with any other
 * library's random stream: the guarantee is exact results given the mask, and a mask that is what this paragraph says.
 *
 * Attention with dropout on the probabilities (csrc/attention_dropout.hip):
 *     out[b,h,:,i] = sum_j keep(b,h,i,j) * scale * P_ij * v_j,   P = softmax_j( q_i . k_j / scale_div - slopes[h] * |i - j| )
 * (the softmax is that of the unmasked logits).  Layouts as agx_attention_alibi_cross, with explicit batch strides in floats
 * for q and kv: item b of q starts at q + b * q_batch_stride (>= H*Dh*tq), of kv at kv + b * kv_batch_stride (>= 2*H*Dh*tk;
 * AGX_ERR_BAD_SHAPE when shorter).  Self-attention on a (B, 3*H*Dh, T) qkv tensor is q = qkv, kv = qkv + H*Dh*T, both strides
 * 3*H*Dh*T, tq = tk = T.  out is contiguous (B, H*Dh, tq).  fp32, any tq, tk >= 1, Dh <= 128 (AGX_ERR_UNSUPPORTED beyond);
 * batch, heads, tq or tk <= 0: returns AGX_OK and launches nothing. */
int agx_attention_alibi_dropout(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride, const float *slopes,
                                float *out, int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, float scale_div,
                                double p, uint64_t seed, uint32_t stream_id, void *stream);
/* Its backward, with the forward's p, seed and stream_id: dq and dkv from q, kv and dout (contiguous (B, H*Dh, tq); `out` is
 * not read).  dq and dkv take their own batch strides, so self-attention writes dq = dqkv, dkv = dqkv + H*Dh*T with both
 * strides 3*H*Dh*T.  Three deterministic kernels as agx_attention_alibi_cross_backward (no atomics: two calls agree bit for
 * bit); workspace = 2 * batch * heads * tq floats = agx_attention_dropout_backward_workspace_bytes() bytes, every float of
 * it written (AGX_ERR_WORKSPACE when shorter).  Empty shapes as above. */
size_t agx_attention_dropout_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t tq);
int agx_attention_alibi_dropout_backward(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                         const float *slopes, const float *out, const float *dout, float *dq, float *dkv,
                                         int64_t dq_batch_stride, int64_t dkv_batch_stride, float *workspace, size_t workspace_bytes,
                                         int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, float scale_div,
                                         double p, uint64_t seed, uint32_t stream_id, void *stream);
/* Host-only: "attention_drop<DVT>" (DVT = 1 / 2 / 4 32-row tiles of the head dim), with backward != 0 the three backward
 * kernels, "none" for an empty shape, or the launcher's refusal (code and message; p outside [0, 1) included). */
int agx_attention_dropout_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, double p,
                                      int32_t backward, char *buf, size_t buf_len);
/* Elementwise dropout with an optional residual over n contiguous floats:
 *     out[e] = (res ? res[e] : 0) + (keep(e) ? x[e] * scale : 0)
 * with the product rounded to fp32 before the add.  out may alias x; res may be NULL.  With res = NULL and the forward's
 * (p, seed, stream_id) the call is its own backward.  n <= 0: returns AGX_OK and launches nothing. */
int agx_dropout_add(const float *x, const float *res, float *out, int64_t n, double p, uint64_t seed, uint32_t stream_id,
                    void *stream);

/* Causal self-attention with the one-sided ALiBi bias (csrc/attention_causal.hip; build-defined, the reference has no causal
 * branch): the query at absolute position i + q_pos0 sees the keys j <= i + q_pos0 only,
 *     out[b,h,:,i] = sum_j softmax_j( q_i . k_j / scale_div - slopes[h] * (i + q_pos0 - j) ) v_j,   j in [0, min(i + q_pos0, tk - 1)]
 * q (B, H*Dh, tq) and kv (B, 2*H*Dh, .: K rows, then V rows) with batch strides in floats as agx_attention_alibi_dropout, and
 * kv rows of pitch kv_row_stride >= tk floats: the pitch of a preallocated key/value cache whose valid length is tk.  Nothing
 * at or beyond column tk of a kv row is read, so the tail of a cache may hold anything (NaN included).  Full causal
 * self-attention on a (B, 3*H*Dh, T) qkv tensor is q = qkv, kv = qkv + H*Dh*T, batch strides 3*H*Dh*T, kv_row_stride = T,
 * tq = tk = T, q_pos0 = 0; a step of tq new frames on a cache is q_pos0 = tk - tq.  out is contiguous (B, H*Dh, tq).  Key
 * blocks no query of a workgroup can see are skipped.  fp32, Dh <= 128 (AGX_ERR_UNSUPPORTED beyond); q_pos0 < 0,
 * kv_row_stride < tk or a batch stride too small for the shape: AGX_ERR_BAD_SHAPE; batch, heads, tq or tk <= 0: returns
 * AGX_OK and launches nothing.  Every refusal happens before anything is launched. */
int agx_attention_alibi_causal(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                               int64_t kv_row_stride, const float *slopes, float *out, int32_t batch, int32_t heads,
                               int32_t head_dim, int32_t tq, int32_t tk, int32_t q_pos0, float scale_div, void *stream);
/* Backward of the full causal self-attention (q_pos0 = 0, tq = tk = t, rows of pitch t): dq and dkv from q, kv and dout
 * (contiguous (B, H*Dh, t); `out` is not read), each through its own pointer and batch stride, so dqkv is written in place.
 * Three deterministic kernels as agx_attention_alibi_cross_backward (no atomics: two calls agree bit for bit), skipping the
 * key / query blocks the mask empties; a masked (i, j) pair contributes exactly 0.  workspace = 2 * batch * heads * t floats =
 * agx_attention_causal_backward_workspace_bytes() bytes, every float of it written (AGX_ERR_WORKSPACE when shorter). */
size_t agx_attention_causal_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t t);
int agx_attention_alibi_causal_backward(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                        const float *slopes, const float *out, const float *dout, float *dq, float *dkv,
                                        int64_t dq_batch_stride, int64_t dkv_batch_stride, float *workspace,
                                        size_t workspace_bytes, int32_t batch, int32_t heads, int32_t head_dim, int32_t t,
                                        float scale_div, void *stream);
/* Host-only: "attention_causal<DVT>" (DVT = 1 / 2 / 4 32-row tiles of the head dim), with backward != 0 the three backward
 * kernels, "none" for an empty shape, or the launcher's refusal (code and message). */
int agx_attention_causal_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, int32_t backward,
                                     char *buf, size_t buf_len);

/* Sliding-window causal self-attention (csrc/attention_window.hip; build-defined, the causal form above narrowed to the last
 * `window` keys): the query at absolute position p = i + q_pos0 sees the keys j in [max(0, p - window + 1), p] only,
 *     out[b,h,:,i] = sum_j softmax_j( q_i . k_j / scale_div - slopes[h] * (p - j) ) v_j
 * window >= p + 1 for every query is agx_attention_alibi_causal; window = 1 returns v_p.  q, kv, the strides and out as there.
 * The keys are the positions 0 .. q_pos0 + tq - 1 and key j sits in column j of a kv row (kv_ring = 0, the linear form:
 * kv_row_stride >= q_pos0 + tq) or in column j mod kv_ring (kv_ring > 0, a ring cache: tq + min(window - 1, q_pos0) <= kv_ring <=
 * kv_row_stride, so that the oldest key the first query sees, max(0, q_pos0 - window + 1), has not been overwritten by the
 * newest; from q_pos0 >= window - 1 on that is tq + window - 1 <= kv_ring).  q_pos0 is 64-bit and
 * a stream has no end: on a ring the launcher lowers every position by a multiple of lcm(64, kv_ring), which keeps the
 * 64-key block alignment, the ring column and every p - j, and the kernel indexes in int32 (a lowered q_pos0 + tq beyond
 * int32 -- only a ring of ~2^25 columns and more can get there -- is AGX_ERR_BAD_SHAPE).  Key blocks are aligned to absolute
 * positions (block = j / 64), so a query's result does not depend on the chunk that delivered it, bit for bit.  Only the key
 * blocks some query of a workgroup sees are walked.  A ring column outside a workgroup's window is never read as V and never
 * reaches a score: it may hold anything (an older frame, NaN, unwritten memory).  fp32, Dh <= 128 (AGX_ERR_UNSUPPORTED
 * beyond); window < 1, q_pos0 < 0, kv_ring < 0, kv_ring too small for tq + min(window - 1, q_pos0) or larger than kv_row_stride, a linear
 * kv_row_stride < q_pos0 + tq, or a batch stride too small for the shape: AGX_ERR_BAD_SHAPE; batch, heads or tq <= 0: returns
 * AGX_OK and launches nothing.  Every refusal happens before anything is launched and before any pointer is used. */
int agx_attention_alibi_window(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                               int64_t kv_row_stride, const float *slopes, float *out, int32_t batch, int32_t heads,
                               int32_t head_dim, int32_t tq, int64_t q_pos0, int32_t window, int32_t kv_ring, float scale_div,
                               void *stream);
/* Backward of the full windowed self-attention (q_pos0 = 0, tq = t keys, linear kv, rows of pitch t), as
 * agx_attention_alibi_causal_backward: three deterministic kernels, no atomics, dqkv written in place, `out` not read; the
 * key / query blocks outside the band i - window < j <= i are skipped and a masked (i, j) pair contributes exactly 0.
 * workspace = 2 * batch * heads * t floats, every float of it written (AGX_ERR_WORKSPACE when shorter). */
size_t agx_attention_window_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t t);
int agx_attention_alibi_window_backward(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                        const float *slopes, const float *out, const float *dout, float *dq, float *dkv,
                                        int64_t dq_batch_stride, int64_t dkv_batch_stride, float *workspace,
                                        size_t workspace_bytes, int32_t batch, int32_t heads, int32_t head_dim, int32_t t,
                                        int32_t window, float scale_div, void *stream);
/* Host-only: "attention_window<DVT>" (DVT = 1 / 2 / 4 32-row tiles of the head dim), with backward != 0 the three backward
 * kernels, "none" for an empty shape, or the launcher's refusal (code and message; window < 1 included). */
int agx_attention_window_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t window,
                                     int32_t backward, char *buf, size_t buf_len);

/* Device-held stream positions (csrc/attention_stream.hip; build-defined): agx_attention_alibi_window on a ring cache with the
 * position of every batch row in device memory.  pos is a device array of `batch` int64 entries read by the kernels (no host
 * copy, no sync; a captured graph replays with the positions the array holds at replay time, and rows have ages of their
 * own): row b's query i sits at p = i + max(pos[b], 0) and sees the keys j in [max(0, p - window + 1), p], key j in column
 * j mod kv_ring of a kv row.  q, kv, the strides, slopes and out as agx_attention_alibi_window; the ring is mandatory
 * (kv_ring >= 1).  The host does not know the positions, so the bound is the worst case over all of them,
 * tq + window - 1 <= kv_ring <= kv_row_stride (stricter than the host-position form while pos < window - 1), and the lowering
 * by a multiple of lcm(64, kv_ring) is done by every workgroup; lcm(64, kv_ring) + window + tq + 128 beyond int32 is
 * AGX_ERR_BAD_SHAPE.  Memory safety does not depend on what pos holds: columns are formed modulo the ring and the bound above
 * holds for every position.  Row b computes bit for bit what agx_attention_alibi_window computes for it with q_pos0 = pos[b]
 * on the same ring.  A ring column outside a workgroup's window may hold anything.  pos is never written.  fp32, Dh <= 128
 * (AGX_ERR_UNSUPPORTED beyond); window < 1, kv_ring < tq + window - 1 or > kv_row_stride, a batch stride too small:
 * AGX_ERR_BAD_SHAPE; batch, heads or tq <= 0: returns AGX_OK and launches nothing.  Every refusal happens before anything is
 * launched and before any pointer is used. */
int agx_attention_alibi_stream(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                               int64_t kv_row_stride, const int64_t *pos, const float *slopes, float *out, int32_t batch,
                               int32_t heads, int32_t head_dim, int32_t tq, int32_t window, int32_t kv_ring, float scale_div,
                               void *stream);
/* buf[b, c, (max(pos[b], 0) + t) mod ring] = src[b, c, t] for c < rows, t < n: a chunk's K / V rows into a ring cache at every
 * row's own position, in one launch, wrap included.  src is read in place: rows of pitch n from src + b * src_batch_stride (the
 * K / V rows of a qkv tensor); buf has rows of pitch buf_row_stride >= ring.  Exactly n columns of every row are written and
 * nothing else; pos is not written.  1 <= n <= ring (no column is written twice), else AGX_ERR_BAD_SHAPE; batch, rows or
 * n <= 0: AGX_OK, nothing launched.  Refusals precede every use of a pointer. */
int agx_ring_write_pos(float *buf, const float *src, int64_t buf_batch_stride, int64_t buf_row_stride, int64_t src_batch_stride,
                       const int64_t *pos, int32_t batch, int32_t rows, int32_t n, int32_t ring, void *stream);
/* pos[b] += n for b < batch (exact int64 arithmetic, n >= 0): the advance of a stream, on the device.  Writes pos only. */
int agx_stream_advance(int64_t *pos, int32_t batch, int64_t n, void *stream);
/* Host-only: "attention_stream<DVT>" (DVT = 1 / 2 / 4 32-row tiles of the head dim), "none" for an empty shape, or the
 * launcher's refusal (code and message; window < 1 included). */
int agx_attention_stream_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t window, char *buf,
                                     size_t buf_len);

/* Ragged batches (csrc/attention_ragged.hip; build-defined): symmetric ALiBi attention, self or cross, with a valid length
 * per batch row for the queries and for the keys.  q_len and k_len are device arrays of `batch` int32 entries, read by the
 * kernels (no host copy, no sync; a captured graph replays with the lengths the arrays hold at replay time); either may be
 * NULL, which means every row is full.  With ql = clamp(q_len[b], 0, tq) and kl = clamp(k_len[b], 0, tk), positions absolute
 * and padding on the right:
 *     out[b,h,:,i] = sum_{j < kl} softmax_{j < kl}( q_i . k_j / scale_div - slopes[h] * |i - j| ) v_j     for i < ql
 *     out[b,h,:,i] = 0                                               for ql <= i < tq, and for every i when kl == 0
 * q (rows of pitch tq) and kv (K rows, then V rows, of pitch tk) have their own base pointers and batch strides as in
 * agx_attention_alibi_dropout: self-attention on a (B, 3*H*Dh, T) qkv tensor is q = qkv, kv = qkv + H*Dh*T, both strides
 * 3*H*Dh*T.  out is contiguous (B, H*Dh, tq) and every element of it is written.  Nothing at or beyond a row's length
 * reaches a result: q at i >= ql and K / V at j >= kl are never multiplied (loads are clamped below the length, V is staged
 * as 0) and may hold anything, NaN included -- the contract of the key/value cache's tail.  Only ceil(kl / 64) key blocks
 * are walked, and a workgroup without a valid query stores its zeros and returns.  A row computes bit for bit what the same
 * call computes for that row cropped to (ql, kl) and run alone.  fp32, Dh <= 128 (AGX_ERR_UNSUPPORTED beyond); a batch
 * stride too small for the shape: AGX_ERR_BAD_SHAPE; batch, heads, tq or tk <= 0: returns AGX_OK and launches nothing.
 * Every refusal happens before anything is launched and before any pointer is used. */
int agx_attention_alibi_ragged(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                               const float *slopes, const int32_t *q_len, const int32_t *k_len, float *out, int32_t batch,
                               int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, float scale_div, void *stream);
/* Backward: dq and dkv from q, kv and dout (contiguous (B, H*Dh, tq); `out` is not read), each through its own pointer and
 * batch stride, so a dqkv tensor is written in place.  Three deterministic kernels as agx_attention_alibi_cross_backward
 * (attn_ragged_bwd_stats / _dq / _dkv; P recomputed from the row statistics, no atomics: two calls agree bit for bit).  A
 * masked (i, j) pair contributes exactly 0; dq is exactly 0 at i >= ql, dkv exactly 0 at j >= kl, both 0 for a row with
 * ql == 0 or kl == 0; every element of dq and dkv is written.  Query blocks beyond ql and key blocks beyond kl are not
 * walked.  dout at i >= ql is never read into a result and may hold anything.  workspace = 2 * batch * heads * tq floats
 * (lse, delta) = agx_attention_ragged_backward_workspace_bytes() bytes, every float of it written, masked rows and queries
 * included (AGX_ERR_WORKSPACE when shorter). */
size_t agx_attention_ragged_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t tq);
int agx_attention_alibi_ragged_backward(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                        const float *slopes, const int32_t *q_len, const int32_t *k_len, const float *out,
                                        const float *dout, float *dq, float *dkv, int64_t dq_batch_stride,
                                        int64_t dkv_batch_stride, float *workspace, size_t workspace_bytes, int32_t batch,
                                        int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, float scale_div, void *stream);
/* Host-only: "attention_ragged<DVT>" (DVT = 1 / 2 / 4 32-row tiles of the head dim), with backward != 0 the three backward
 * kernels joined with '+', "none" for an empty shape, or the launcher's refusal (code and message). */
int agx_attention_ragged_kernel_name(int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t tk, int32_t backward,
                                     char *buf, size_t buf_len);
/* out[b,c,i] = i < clamp(len[b], 0, t) ? x[b,c,i] : 0 over contiguous fp32 (batch, channels, t) tensors: a select, not a
 * multiply, so a NaN tail becomes 0.  out may alias x.  It is its own backward.  len: `batch` int32 entries on the device
 * (NULL: a copy).  batch, channels or t <= 0: returns AGX_OK and launches nothing. */
int agx_mask_tail(const float *x, const int32_t *len, float *out, int32_t batch, int32_t channels, int32_t t, void *stream);

/* Packed variable-length batches (csrc/attention_packed.hip; build-defined): symmetric ALiBi attention, self or cross, over
 * n_seq sequences concatenated along the time axis.  cu_q and cu_k are device arrays of n_seq + 1 int32 entries, read by the
 * kernels (no host copy, no sync; a captured graph replays with whatever the arrays hold at replay time).  Sequence s owns the
 * query columns [cu_q[s], cu_q[s+1]) and the key columns [cu_k[s], cu_k[s+1]); positions are relative to the sequence's own
 * start, and with ql / kl the two lengths
 *     out[h,:,cu_q[s] + i] = sum_{j < kl} softmax_{j < kl}( q_i . k_j / scale_div - slopes[h] * |i - j| ) v_j     for i < ql
 * which is agx_attention_alibi_cross applied to that sequence alone; a sequence with kl == 0 gets 0, a sequence with ql == 0
 * gets nothing.  q has heads * head_dim rows of pitch q_row_stride >= nq; kv has the K rows, then the V rows,
 * 2 * heads * head_dim of them, of pitch kv_row_stride >= nk: self-attention on one (1, 3*H*Dh, N) qkv tensor is q = qkv,
 * kv = qkv + H*Dh*N, both strides N, cu_k = cu_q, nq = nk = N.  out is contiguous (H*Dh, nq).  The query columns that no
 * sequence owns -- before cu_q[0], which is 0 in a valid array, and from cu_q[n_seq] on, the slack when nq is a capacity --
 * are written exactly 0, so every element of out is written.  max_q / max_k are host-known upper bounds of the sequence
 * lengths; they size the grid, (ceil(max_q / 128), heads, n_seq + 1), and a workgroup beyond its sequence's length returns
 * at once.  Memory safety does not depend on what the device arrays hold: every start and end is clamped into [0, nq] /
 * [0, nk], an end to at least its start, a length to at most max_q / max_k.  For arrays that violate the contract
 * (decreasing, or a sequence longer than its bound) the values are unspecified and columns may stay unwritten, but no
 * access leaves the tensors.  Nothing outside a sequence reaches its result: loads are clamped below the sequence's end and
 * V is staged as 0 beyond it, so the neighbours and the slack of q and kv may hold anything, NaN included.  Key and query
 * blocks are aligned to the sequence's start: sequence s computes bit for bit what agx_attention_alibi_ragged computes for
 * that sequence cropped and run alone with NULL lengths.  fp32, Dh <= 128 (AGX_ERR_UNSUPPORTED beyond); a row stride too
 * small, max_q < 0 or max_k < 0: AGX_ERR_BAD_SHAPE; n_seq, heads, nq or nk <= 0: returns AGX_OK and launches nothing.
 * Every refusal happens before anything is launched and before any pointer is used. */
int agx_attention_alibi_packed(const float *q, const float *kv, int64_t q_row_stride, int64_t kv_row_stride, const float *slopes,
                               const int32_t *cu_q, const int32_t *cu_k, float *out, int32_t n_seq, int32_t heads,
                               int32_t head_dim, int32_t nq, int32_t nk, int32_t max_q, int32_t max_k, float scale_div,
                               void *stream);
/* Backward: dq and dkv from q, kv and dout (contiguous (H*Dh, nq); `out` is not read), each through its own pointer and row
 * stride (>= nq / >= nk), so a dqkv tensor is written in place.  Three deterministic kernels as
 * agx_attention_alibi_ragged_backward (attn_packed_bwd_stats / _dq / _dkv; no atomics: two calls agree bit for bit), sequence
 * s bit for bit that backward on its crop.  dq / dkv are exactly 0 for a sequence without keys / without queries and in the
 * columns no sequence owns; every element of both is written.  dout outside a sequence never reaches that sequence's
 * gradients and may hold anything.  workspace = 2 * heads * nq floats (lse, delta) =
 * agx_attention_packed_backward_workspace_bytes() bytes, every float of it written (AGX_ERR_WORKSPACE when shorter).  The
 * clamps, the unspecified cases and the refusals are those of the forward. */
size_t agx_attention_packed_backward_workspace_bytes(int32_t heads, int32_t nq);
int agx_attention_alibi_packed_backward(const float *q, const float *kv, int64_t q_row_stride, int64_t kv_row_stride,
                                        const float *slopes, const int32_t *cu_q, const int32_t *cu_k, const float *out,
                                        const float *dout, float *dq, float *dkv, int64_t dq_row_stride, int64_t dkv_row_stride,
                                        float *workspace, size_t workspace_bytes, int32_t n_seq, int32_t heads,
                                        int32_t head_dim, int32_t nq, int32_t nk, int32_t max_q, int32_t max_k, float scale_div,
                                        void *stream);
/* Host-only: "attention_packed<DVT>" (DVT = 1 / 2 / 4 32-row tiles of the head dim), with backward != 0 the three backward
 * kernels joined with '+', "none" for an empty shape, or the launcher's refusal (code and message). */
int agx_attention_packed_kernel_name(int32_t n_seq, int32_t heads, int32_t head_dim, int32_t nq, int32_t nk, int32_t max_q,
                                     int32_t max_k, int32_t backward, char *buf, size_t buf_len);
/* The two layouts of a ragged batch, each kernel the other's adjoint; cu: batch + 1 int32 entries on the device, read by the
 * kernel and clamped as above (start and end into [0, n], the end to at least the start, the length to at most t).
 * agx_pack_rows: x contiguous (batch, channels, t) -> out contiguous (channels, n) with out[c, cu[b] + i] = x[b, c, i] for
 * i < cu[b+1] - cu[b], and exactly 0 in the columns no row owns; the padding of x is never read.  agx_unpack_rows: xp
 * contiguous (channels, n) -> out contiguous (batch, channels, t) with out[b, c, i] = xp[c, cu[b] + i] for i < cu[b+1] - cu[b]
 * and exactly 0 at the padded positions; the slack of xp is never read.  Both are selects on the index: a NaN never becomes
 * anything else and never moves.  Every output element is written.  An empty output (batch, channels or t <= 0; pack: n <= 0;
 * unpack: n < 0): AGX_OK, nothing launched -- agx_unpack_rows with n == 0 writes its zeros and does not read xp. */
int agx_pack_rows(const float *x, const int32_t *cu, float *out, int32_t batch, int32_t channels, int32_t t, int32_t n,
                  void *stream);
int agx_unpack_rows(const float *xp, const int32_t *cu, float *out, int32_t batch, int32_t channels, int32_t t, int32_t n,
                    void *stream);

/* ------------------------------------------------------------------------- *
 * Wavelet / multiresolution layers (networks/wavelets.py)                     *
 * ------------------------------------------------------------------------- */

/* CausalMultiresConv1d.forward (wavelets.py:79-96): depth-level cascade of two
 * depthwise causal filters h0/h1 (C,1,K) with dilation 1,2,4,..., per-channel
 * mixing w (C, depth+2), exact GELU.  x, y (B, C, L).  One launch.
 * Limits: depth 0 .. 20 (AGX_ERR_BAD_SHAPE beyond), and LDS -- two rows of 1024 + (K - 1)(2^depth - 1) floats plus the 2 K
 * taps within 150 KiB, AGX_ERR_UNSUPPORTED beyond.  K itself has no other limit: the taps are staged by a loop strided over
 * the workgroup, so K > 256 runs.  A refusal launches nothing. */
int agx_multires_forward(const float *x, const float *h0, const float *h1, const float *w, float *y,
                         int32_t batch, int32_t channels, int32_t length, int32_t kernel,
                         int32_t depth, void *stream);

/* Backward of agx_multires_forward: dx (B, C, L), dh0 / dh1 (C, 1, K), dw (C, depth + 2) from dout (B, C, L); the
 * cascade is re-formed per tile in LDS (nothing is kept from the forward).  Parameter sums are per-tile partials in
 * `workspace` reduced in a fixed order (deterministic).  Needs 2 K + depth + 2 <= 64. */
size_t agx_multires_backward_workspace_bytes(int32_t batch, int32_t channels, int32_t length, int32_t kernel,
                                             int32_t depth);
int agx_multires_backward(const float *x, const float *dout, const float *h0, const float *h1, const float *w,
                          float *dx, float *dh0, float *dh1, float *dw, void *workspace, size_t workspace_bytes,
                          int32_t batch, int32_t channels, int32_t length, int32_t kernel, int32_t depth,
                          void *stream);

/* Adjoint of a nearest-neighbour upsample by `group` (MultiresScaleBlock, wavelets.py:112-119): out[i] = sum of
 * g[i * group .. i * group + group), i < n_out; with `gelu_pre` != NULL multiplied by the exact-GELU derivative at
 * gelu_pre[i] (the activation of the k = 1 conv that precedes the upsample). */
int agx_group_sum(const float *g, const float *gelu_pre, float *out, int64_t n_out, int32_t group, void *stream);

/* The fold in the middle of WaveletLayer.forward (wavelets.py:221-231):
 * every input step emits an n_points-long wavelet cos(t)exp(-t^2/sigma_c) * h laid
 * end to end, the output is the sliding-window sum (window n_points, hop
 * n_points/scale) plus the reference's raw-sample tail.  h (B, C, L) ->
 * y (B, C, L*scale).  sigma has `sigma_len` entries (C, or 1 when shared). */
int agx_wavelet_fold(const float *h, const float *space, const float *sigma, int32_t sigma_len,
                     float *y, int32_t batch, int32_t channels, int32_t length, int32_t n_points,
                     int32_t scale, void *stream);

/* Backward of agx_wavelet_fold: dh (B,C,L) and dsigma (sigma_len) from dout (B,C,L*scale).
 * workspace: B*C floats (per-row partials of dsigma, reduced in a fixed order). */
int agx_wavelet_fold_backward(const float *h, const float *dout, const float *space, const float *sigma,
                              int32_t sigma_len, float *dh, float *dsigma, float *workspace, int32_t batch,
                              int32_t channels, int32_t length, int32_t n_points, int32_t scale, void *stream);

/* Backward of agx_layernorm_ct: dx = LN'(x)^T (dy * weight) [+ add], dweight[c] = sum dy * xhat, dbias[c] = sum dy.
 * workspace: 2 * batch * ceil(t / 64) * channels floats. */
int agx_layernorm_ct_backward(const float *x, const float *weight, const float *dy, const float *add, float *dx,
                              float *dweight, float *dbias, float *workspace, int32_t batch, int32_t channels,
                              int32_t t, float eps, void *stream);
/* Backward of agx_attention_alibi: dqkv (B, 3*H*Dh, T) from qkv and dout (B, H*Dh, T).  head_dim <= 64, T <= 256. */
int agx_attention_alibi_backward(const float *qkv, const float *slopes, const float *dout, float *dqkv, int32_t batch,
                                 int32_t heads, int32_t head_dim, int32_t t, float scale_div, void *stream);
/* The same for ANY t and head_dim <= 128 (flash-style split into three deterministic kernels: row statistics, dQ per query block,
 * dK / dV per key block; csrc/attention_flash.hip).  `out` = the forward's output (B, H*Dh, T); workspace:
 * agx_attention_backward_workspace_bytes() bytes. */
size_t agx_attention_backward_workspace_bytes(int32_t batch, int32_t heads, int32_t t);
int agx_attention_alibi_backward_ex(const float *qkv, const float *slopes, const float *out, const float *dout, float *dqkv,
                                    float *workspace, size_t workspace_bytes, int32_t batch, int32_t heads, int32_t head_dim,
                                    int32_t t, float scale_div, void *stream);
/* Host-only: split = 0: the kernel agx_attention_alibi_backward runs, "attention_alibi_bwd<16>" or "<8>" (queries per LDS block),
 * or its refusal of the shape (t > 256, head_dim > 64); split != 0: the three kernels of agx_attention_alibi_backward_ex, or its
 * refusal (head_dim > 128).  A caller that has the forward output takes the single launch iff split = 0 answers AGX_OK. */
int agx_attention_backward_kernel_name(int32_t heads, int32_t head_dim, int32_t t, int32_t split, char *buf, size_t buf_len);
/* agx_conv_bwd_data followed by the exact-GELU gradient: dx = (W^T dy [+ add]) * gelu'(pre)  (two launches). */
int agx_conv_bwd_data_gelu(const agx_conv_desc *d, const float *dy, const float *packed_bwd, const float *add,
                           const float *pre, float *dx, void *stream);

/* ------------------------------------------------------------------------- *
 * Discriminators: networks/discriminator.py
 * ------------------------------------------------------------------------- */

/* Spectral norm (torch.nn.utils.spectral_norm, utils.py:34-42 with norm="spectral"): W is the weight
 * viewed as (rows = dim 0, cols = the rest).  power_iterations > 0 (training mode) first updates the
 * buffers in place, v = normalize(W^T u), u = normalize(W v) (eps as F.normalize); then
 * sigma[0] = u . (W v).  sigma stays on the device (consumed by agx_conv_pack_sigma / agx_conv2d_pack).
 * workspace: rows + cols floats. */
int agx_spectral_sigma(const float *w, int32_t rows, int32_t cols, float *u, float *v,
                       int32_t power_iterations, float eps, float *sigma, float *workspace, void *stream);

/* agx_conv_pack for a spectrally normalised layer: every row scaled by 1 / sigma[0] (device scalar). */
int agx_conv_pack_sigma(const agx_conv_desc *d, const float *w, const float *sigma, float *packed,
                        void *stream);

/* Backward of grouped AGX_CONV_PADDED layers (dilation 1), VALU kernels on the torch weight layout
 * w (c_out, c_in / groups, K); sigma (device scalar, may be NULL) divides w.  add / mask / slope as in
 * agx_conv_bwd_data.  bwd_weight returns the PLAIN weight gradient (apply agx_spectral_grad afterwards). */
int agx_conv_grouped_bwd_data(const agx_conv_desc *d, const float *dz, const float *w, const float *sigma,
                              const float *add, const float *mask, float slope, float *dx, void *stream);
size_t agx_conv_grouped_bwd_weight_workspace_bytes(const agx_conv_desc *d);
int agx_conv_grouped_bwd_weight(const agx_conv_desc *d, const float *x, const float *dz, float *dw, float *dbias,
                                void *workspace, size_t workspace_bytes, void *stream);
/* As agx_conv_bwd_weight_kernel_name for agx_conv_grouped_bwd_weight: items are 256-position tiles (tiled kernel) or
 * single output positions (simple kernel). */
int agx_conv_grouped_bwd_weight_kernel_name(const agx_conv_desc *d, char *buf, size_t buf_len);
/* agx_conv_pack_bwd for a spectrally normalised dense layer (rows scaled by 1 / sigma[0]). */
int agx_conv_pack_bwd_sigma(const agx_conv_desc *d, const float *w, const float *sigma, float *packed, void *stream);

/* torch.nn.AvgPool1d(kernel, stride, padding) with count_include_pad=True (discriminator.py:32) over
 * `rows` independent rows of length l_in; returns the output length via agx_avgpool1d_out_len. */
int64_t agx_avgpool1d_out_len(int32_t l_in, int32_t kernel, int32_t stride, int32_t padding);
int agx_avgpool1d(const float *x, float *y, int64_t rows, int32_t l_in, int32_t kernel, int32_t stride,
                  int32_t padding, void *stream);

/* torch.nn.Conv2d(c_in, c_out, (kh, kw), stride, padding) + optional fused LeakyReLU, NCHW fp32
 * (discriminator.py:101-114, 150-167).  Runs on the 1-D MFMA / direct conv kernels with the kernel rows
 * folded into virtual input channels. */
typedef struct agx_conv2d_desc {
    int32_t batch, c_in, c_out, h_in, w_in;
    int32_t kh, kw, stride_h, stride_w, pad_h, pad_w;
    int32_t epilogue; /* AGX_EPI_LEAKY_PRE or 0 */
    float slope;
    int32_t impl;     /* AGX_IMPL_* */
} agx_conv2d_desc;
int agx_conv2d_out_shape(const agx_conv2d_desc *d, int32_t *h_out, int32_t *w_out);
int64_t agx_conv2d_packed_floats(const agx_conv2d_desc *d);
/* w (c_out, c_in, kh, kw); sigma: device scalar of agx_spectral_sigma or NULL (no normalisation). */
int agx_conv2d_pack(const agx_conv2d_desc *d, const float *w, const float *sigma, float *packed, void *stream);
int agx_conv2d_forward(const agx_conv2d_desc *d, const float *x, const float *packed, const float *bias,
                       float *y, void *stream);
int agx_conv2d_kernel_name(const agx_conv2d_desc *d, char *buf, size_t buf_len);
int agx_conv2d_bwd_data_kernel_name(const agx_conv2d_desc *d, char *buf, size_t buf_len);   /* kernel agx_conv2d_bwd_data runs */
/* Backward of the Conv2d layer `d` describes (forward descriptor): gradient w.r.t. its input from the
 * gradient w.r.t. its output, on the same kernels (strided layers as a 2-D polyphase conv over dy);
 * add: optional tensor added to dx (a gradient arriving from another consumer of the input, e.g. the
 * feature-matching loss); mask/slope: optional fused LeakyReLU gradient of the layer that produced the
 * input (mask = its output), applied after the add as in agx_conv_bwd_data. */
int64_t agx_conv2d_bwd_packed_floats(const agx_conv2d_desc *d);
int agx_conv2d_pack_bwd(const agx_conv2d_desc *d, const float *w, const float *sigma, float *packed, void *stream);
int agx_conv2d_bwd_data(const agx_conv2d_desc *d, const float *dy, const float *packed_bwd, const float *add,
                        const float *mask, float slope, float *dx, void *stream);
/* Backward-data of a stride-1 layer with very few input channels (the 2-channel first conv), in two steps:
 * agx_conv2d_colsplit_weights writes the weights of the auxiliary (kh x 1) layer with c_in*kw output rows
 * (wp: c_in*kw x c_out x kh floats; run it with agx_conv2d_forward on dy, padding (kh-1-pad_h, 0)); its output
 * P (B, c_in*kw, h_in, w_out) is folded by agx_conv2d_colsum: dx[c][i][j] = sum_dw P[c*kw+dw][i][j-dw+pad_w] (+ add). */
int agx_conv2d_colsplit_weights(const agx_conv2d_desc *d, const float *w, const float *sigma, float *wp, void *stream);
int agx_conv2d_colsum(const agx_conv2d_desc *d, const float *pbuf, const float *add, float *dx, void *stream);
/* dW (c_out, c_in, kh, kw) and dbias (c_out, may be NULL) of the layer.  With sigma != NULL the layer is
 * spectrally normalised: w is weight_orig, u / v the vectors sigma was computed with, and dw is the
 * gradient w.r.t. weight_orig:  G / sigma - (<G, W> / sigma^2) u v^T  (G = gradient w.r.t. W / sigma). */
size_t agx_conv2d_bwd_weight_workspace_bytes(const agx_conv2d_desc *d);
int agx_conv2d_bwd_weight(const agx_conv2d_desc *d, const float *x, const float *dy, const float *w,
                          const float *sigma, const float *u, const float *v, float *dw, float *dbias,
                          void *workspace, size_t workspace_bytes, void *stream);
/* As agx_conv_bwd_weight_kernel_name for agx_conv2d_bwd_weight: op is none, deinterleave (column-phase planes of x)
 * or prepad (zero-padded, flattened copies of x and dy); items are 32-column chunks of an output row (direct /
 * shared kernels, cfg 10..17; prepad: 32-position chunks of a flattened image) or staged tiles (cfg 0..2). */
int agx_conv2d_bwd_weight_kernel_name(const agx_conv2d_desc *d, char *buf, size_t buf_len);

/* The torch.stft call of STFTDiscriminator.forward (discriminator.py:181-187): rectangular window,
 * center=True (reflect padding), two-sided, optionally normalised by n_fft^-1/2, hop = n_fft / 4.
 * x (B, L) -> y (B, 2, T, n_fft) with T = 1 + L / hop, channel 0 real / 1 imaginary (the layout after the
 * reference's rearrange "b f t c -> b c t f").  The DFT runs as a conv on the MFMA kernels:
 * agx_stft_pack builds its weight image once per n_fft. */
int64_t agx_stft_frames(int32_t length, int32_t n_fft);
int64_t agx_stft_packed_floats(int32_t n_fft);
int agx_stft_pack(int32_t n_fft, int32_t normalized, float *packed, void *stream);
int64_t agx_stft_workspace_bytes(int32_t batch, int32_t length, int32_t n_fft);
int agx_stft_forward(const float *x, const float *packed, float *y, void *workspace, int32_t batch,
                     int32_t length, int32_t n_fft, void *stream);

/* Adjoint of agx_stft_forward: dx (B, L) from dy (B, 2, T, n_fft).  workspace as agx_stft_workspace_bytes;
 * packed_bwd from agx_stft_pack_bwd (agx_stft_packed_floats floats as well). */
int agx_stft_pack_bwd(int32_t n_fft, int32_t normalized, float *packed_bwd, void *stream);
int agx_stft_backward(const float *dy, const float *packed_bwd, float *dx, void *workspace, int32_t batch,
                      int32_t length, int32_t n_fft, void *stream);
/* AvgPool1d backward (count_include_pad): dx (rows, l_in) from dy (rows, l_out); add may be NULL. */
int agx_avgpool1d_backward(const float *dy, const float *add, float *dx, int64_t rows, int32_t l_in, int32_t kernel,
                           int32_t stride, int32_t padding, void *stream);
/* dz = dy * s * (1 - s) with s = the sigmoid OUTPUT. */
int agx_sigmoid_backward(const float *dy, const float *s, float *dz, int64_t n, void *stream);
/* Spectral-norm chain rule in place on a plain weight gradient G (rows x cols, torch layout):
 * G <- G / sigma - (<G, W> / sigma^2) u v^T.  workspace: rows floats. */
int agx_spectral_grad(float *g, const float *w, const float *sigma, const float *u, const float *v, int32_t rows,
                      int32_t cols, float *workspace, void *stream);

/* Reductions of discriminator_generator_loss (discriminator.py:204-246), one launch each, result in
 * out[0] (device):  mode 0 mean(x) | 1 mean(min(x - 1, 0)) | 2 mean(min(-x - 1, 0)) |
 * 3 mean|x - y| | 4 mean|x + 1e-3| | 5 mean (log(x + 1e-8) - log(y + 1e-8))^2 (training.py:74).
 * y only for modes 3 and 5.  workspace: 1024 floats. */
int agx_reduce_mean(const float *x, const float *y, int64_t n, int32_t mode, float *out, float *workspace,
                    void *stream);
/* Gradient of the above: dx = grad[0] * d mean(term) / dx (and dy = -dx for the L1 term; dy may be NULL). */
int agx_reduce_mean_backward(const float *x, const float *y, int64_t n, int32_t mode, const float *grad, float *dx,
                             float *dy, void *stream);
/* The two means of one feature-matching term (discriminator.py:236-243: mean|x - y| and the scale mean|x + 1e-3| of the
 * real feature map) in ONE pass over the pair: out[0] = mean|x - y|, out[1] = mean|x + 1e-3| -- the same values as modes 3
 * and 4 above give.  workspace: 2048 floats.  backward: dx = grad[0] d out[0] / dx + grad[1] d out[1] / dx,
 * dy = grad[0] d out[0] / dy (either may be NULL) -- bit for bit the sum of the two separate gradients. */
int agx_feature_means(const float *x, const float *y, int64_t n, float *out, float *workspace, void *stream);
int agx_feature_means_backward(const float *x, const float *y, int64_t n, const float *grad, float *dx, float *dy,
                               void *stream);
/* final_activation of the discriminators (torch.nn.Sigmoid, discriminator.py:46, 173). */
int agx_sigmoid(const float *x, float *y, int64_t n, void *stream);

/* ------------------------------------------------------------------------- *
 * Training-loop signal ops: torchaudio in the reference -- parity unpinned (torchaudio is not
 * installed in the build container; restated from its documented behaviour, oracle/signal.py)
 * ------------------------------------------------------------------------- */

/* Framed DFT: windowed STFT with hop | n_fft as a polyphase conv on the MFMA conv kernel.
 *   window_kind 0 rectangular | 1 periodic Hann (win_length <= n_fft, centred as torch.stft does)
 *   norm_kind   0 none | 1 n_fft^-1/2 | 2 (sum window^2)^-1/2  (torchaudio Spectrogram(normalized=True))
 * x (B, L) -> y (B, 2 R, T): R = agx_fdft_rows() real rows then R imaginary rows (bins >= F are zero padding),
 * T = 1 + L / hop, reflect-centred.  backward: the adjoint.  workspace: agx_fdft_workspace_bytes. */
int64_t agx_fdft_frames(int32_t length, int32_t n_fft, int32_t hop);
int64_t agx_fdft_rows(int32_t n_fft, int32_t onesided);
int64_t agx_fdft_packed_floats(int32_t n_fft, int32_t win_length, int32_t hop, int32_t onesided, int32_t backward);
int agx_fdft_pack(int32_t n_fft, int32_t win_length, int32_t hop, int32_t onesided, int32_t window_kind,
                  int32_t norm_kind, int32_t backward, float *packed, void *stream);
int64_t agx_fdft_workspace_bytes(int32_t batch, int32_t length, int32_t n_fft, int32_t hop);
int agx_fdft_forward(const float *x, const float *packed, float *y, void *workspace, int32_t batch, int32_t length,
                     int32_t n_fft, int32_t win_length, int32_t hop, int32_t onesided, void *stream);
int agx_fdft_backward(const float *dy, const float *packed_bwd, float *dx, void *workspace, int32_t batch,
                      int32_t length, int32_t n_fft, int32_t win_length, int32_t hop, int32_t onesided, void *stream);
/* mel[b, m, t] = sum_{f < bins} fb[f, m] (re^2 + im^2) on the fdft layout; fb (bins, n_mels) row-major. */
int agx_melpower(const float *cv, const float *fb, float *mel, int32_t batch, int32_t bins, int32_t frames,
                 int32_t n_mels, void *stream);
int agx_melpower_backward(const float *cv, const float *fb, const float *dmel, float *dcv, int32_t batch, int32_t bins,
                          int32_t frames, int32_t n_mels, void *stream);
/* torchaudio.functional.preemphasis (training.py:333-334): y[n] = x[n] - coeff x[n-1]; adjoint != 0: its transpose. */
int agx_preemphasis(const float *x, float *y, int64_t rows, int32_t length, float coeff, int32_t adjoint,
                    void *stream);
/* torchaudio.functional.lowpass_biquad (training.py:316-318): RBJ low-pass, direct form I, output clamped to [-1, 1]. */
int agx_lowpass_biquad(const float *x, float *y, int64_t rows, int32_t length, float sample_rate, float cutoff_freq,
                       float q, void *stream);
/* torchaudio.transforms.Resample (training.py:554, applied per clip by utils.collator utils.py:157-158): y (rows,
 * agx_resample_out_len(length)) = polyphase sinc interpolation of x (rows, length) with the caller's table
 * (new_freq, 2 width + orig_freq) -- orig_freq / new_freq already divided by their gcd. */
int64_t agx_resample_out_len(int64_t length, int32_t orig_freq, int32_t new_freq);
int agx_resample(const float *x, const float *table, float *y, int64_t rows, int32_t length, int32_t orig_freq,
                 int32_t new_freq, int32_t width, void *stream);

/* ------------------------------------------------------------------------- *
 * Codec bitstream (wire size per utils.py:137-147)               *
 * ------------------------------------------------------------------------- */

/* Dense little-endian packing of n_codes indices at `bits` (1..16) bits each: code e occupies
 * bits [e*bits, (e+1)*bits) of the stream.  packed bytes = ceil(n_codes*bits/8). */
int64_t agx_codes_packed_bytes(int64_t n_codes, int32_t bits);
int agx_codes_pack(const int64_t *codes, int64_t n_codes, int32_t bits, uint8_t *out, void *stream);
int agx_codes_unpack(const uint8_t *in, int64_t n_codes, int32_t bits, int64_t *codes, void *stream);

/* Time folding for long-clip inference (fp32, contiguous tensors; pure copies, stream-ordered, no synchronisation).
 * fold:   (B, C, L) -> (B*S, C, W) overlapping windows,  dst[b*S + s, c, j] = src[b, c, src_off + s*hop + j],  j < W;
 *         refused unless src_off + (S-1)*hop + W <= L.
 * unfold: crop-and-place,  dst[b, c, dst_off + s*keep + j] = src[b*S + s, c, src_off + j],  j < keep, s < n_win <= S,
 *         src (B*S, C, W), dst (B, C, dst_length); refused unless src_off + keep <= W and dst_off + n_win*keep <= dst_length.
 *         n_win = 1 places window 0 alone (its longer contribution at the start of a clip), S = 1 a separately run tail. */
int agx_time_fold(const float *src, float *dst, int32_t batch, int32_t channels, int64_t length, int32_t windows, int64_t hop,
                  int64_t width, int64_t src_off, void *stream);
int agx_time_unfold(const float *src, float *dst, int32_t batch, int32_t channels, int32_t windows, int64_t width, int64_t dst_length,
                    int32_t n_win, int64_t src_off, int64_t dst_off, int64_t keep, void *stream);

/* ------------------------------------------------------------------------- *
 * Conditioning on a vector (networks/conditioning.py): FiLM and the gate of SqueezeExcite.  fp32, contiguous tensors,
 * stream-ordered, no synchronisation, no atomics: every result is bitwise reproducible.  Every entry point validates
 * on the host before it touches the device: a non-positive extent returns AGX_OK and launches nothing, a NULL required
 * pointer is AGX_ERR_NULL_POINTER, a layout other than the two below AGX_ERR_BAD_SHAPE.  Every grid is one-dimensional
 * (x only); a shape that needs more than 2^31 - 1 workgroups is AGX_ERR_BAD_SHAPE.
 * ------------------------------------------------------------------------- */
#define AGX_FILM_CT 0 /* x is (B, C, T): channel-major, what the conv stacks and Transformer.run_bct work in */
#define AGX_FILM_TC 1 /* x is (B, T, C): the reference layout, conditioning.py:50 */

/* The two projections of FiLM (conditioning.py:44-46) as one launch:  gb[b, r] = bias[r] + sum_d cond[b, d] w[r, d].
 * cond (B, D), w (R, D) -- gamma.weight stacked over beta.weight, R = C or 2 C --, bias (R) or NULL (zeros), gb (B, R).
 * One wavefront per (b, r): lane l sums d = l, l + 64, ... in increasing order, the 64 partial sums are added in a
 * fixed tree and the bias last.  Any D >= 1. */
int agx_film_params(const float *cond, const float *w, const float *bias, float *gb, int32_t B, int32_t D, int32_t R,
                    void *stream);
/* out = x * gamma + beta (one fma; without beta one multiply) with gamma = gb[b, c] and beta = gb[b, C + c]: gb is
 * (B, 2 C) with has_beta != 0 and (B, C) without.  out may be x.  Loads and stores are 16 bytes wide from the first
 * 16-byte boundary of a row (CT: the T floats of one (b, c); TC: the T * C floats of one b) to its last whole
 * quadruple and scalar at the ragged ends; all scalar where x and out are not equally aligned.  The arithmetic of an
 * element is the same in both layouts. */
int agx_film_apply(const float *x, const float *gb, float *out, int32_t B, int32_t C, int32_t T, int32_t has_beta,
                   int32_t layout, void *stream);
/* Backward of agx_film_apply in one pass that reads x and dout once:
 *   dx = dout * gamma,   dgb[b, c] = sum_t dout * x,   with has_beta: dgb[b, C + c] = sum_t dout.
 * dgb has the shape of gb and every element of it is written.  The sum over t of one (b, c) has one order in both
 * layouts: walker j of 256 takes t = j, j + 256, ... in increasing order (fma for dout * x), the walkers of each group
 * of 64 are added in a halving tree and the four groups as (g0 + g1) + (g2 + g3).  CT: one workgroup per (b, c) row,
 * a thread per walker.  TC: one workgroup per (b, 64 channels), a lane per channel and 64 walkers per thread, every
 * load a coalesced channel-fastest row.  A launch with few rows (CT) or few channel tiles (TC) under-fills the chip. */
int agx_film_backward(const float *x, const float *gb, const float *dout, float *dx, float *dgb, int32_t B, int32_t C,
                      int32_t T, int32_t has_beta, int32_t layout, void *stream);
/* Backward of agx_film_params, one launch, every sum serial in increasing index:
 *   dw[r, d] = sum_b dgb[b, r] cond[b, d],   dbias[r] = sum_b dgb[b, r],   dcond[b, d] = sum_r dgb[b, r] w[r, d].
 * dcond may be NULL (w is then not read and may be NULL too). */
int agx_film_params_backward(const float *cond, const float *w, const float *dgb, float *dw, float *dbias, float *dcond,
                             int32_t B, int32_t D, int32_t R, void *stream);
/* The gate of SqueezeExcite (conditioning.py:23-24): out = x * s with s = 1 / (1 + expf(-z)), elementwise over n
 * floats; out may be x.  z <= -89 gives exactly 0, z >= 17 exactly x; no NaN for finite operands. */
int agx_sigmoid_gate(const float *x, const float *z, float *out, int64_t n, void *stream);
/* Its backward, one launch that writes both:  dx = dout * s,  dz = (dout * x) * (s * (1 - s)). */
int agx_sigmoid_gate_backward(const float *x, const float *z, const float *dout, float *dx, float *dz, int64_t n,
                              void *stream);

/* ------------------------------------------------------------------------- *
 * Snake activations (networks/utils.py:44-105): Snek and SnekReLU.  fp32, contiguous tensors, stream-ordered, no
 * synchronisation, no atomics: every result is bitwise reproducible.  x is rows = B * C contiguous rows of n floats
 * (n = T for (B, C, T), n = H * W for (B, C, H, W)); the channel of a row is row % channels, alpha holds `channels`
 * floats, and channels == 1 is one alpha for every row.  With a = alpha[c], inv = 1 / (a + eps) (fp32, once per row),
 * theta = a * x and (s, c) = sincosf(theta), one range reduction per element:
 *   out       = (variant ? max(x, 0) : x) + inv * s^2
 *   dx        = dout * ((variant ? (x >= 0) : 1) + a * inv * 2 s c)
 *   dalpha[c] = sum over the rows of channel c and their n positions of  dout * inv * (x * 2 s c - inv * s^2)
 * SnekReLU's gradient at x == 0 (either sign of zero) is 1, the convention of torch.clamp.  A channel with a == 0 gives
 * out == x (Snek), dx == dout * (the mask) and dalpha == 0 exactly.
 * rows <= 0 or n <= 0 returns AGX_OK and launches nothing; channels <= 0, rows % channels != 0, a variant other than
 * the two below or a shape beyond the one-dimensional grid (2^31 - 1 workgroups) is AGX_ERR_BAD_SHAPE before anything
 * is launched; a NULL required pointer is AGX_ERR_NULL_POINTER.
 * A non-finite x makes that element of out / dx non-finite and the dalpha of its channel NaN; it reaches no other
 * element and no other channel, and costs no more time than a large finite x.
 * ------------------------------------------------------------------------- */
#define AGX_SNAKE_PLAIN 0 /* Snek:     x + sin^2(alpha x) / (alpha + eps) */
#define AGX_SNAKE_RELU 1  /* SnekReLU: max(x, 0) + sin^2(alpha x) / (alpha + eps) */

/* One launch.  out may be x.  Loads and stores are 16 bytes wide from the first 16-byte boundary of a row to its last
 * whole quadruple and scalar at the ragged ends; all scalar where x and out are not equally aligned. */
int agx_snake_forward(const float *x, const float *alpha, float *out, int64_t rows, int32_t channels, int64_t n,
                      int32_t variant, float eps, void *stream);
/* Bytes of the workspace agx_snake_backward needs when it is asked for dalpha: one float per (row, segment of 2048
 * floats of the row).  0 for an empty or invalid shape. */
size_t agx_snake_backward_workspace_bytes(int64_t rows, int32_t channels, int64_t n);
/* dx and dalpha in one pass over x and dout; either may be NULL (both: nothing is launched).  dx may be dout.
 * dalpha == NULL (frozen alphas) is one launch of the element-wise walk of the forward: no workspace, no reduction;
 * its dx is bitwise the dx of the full call.
 * dalpha != NULL is two launches.  Stage 1: one workgroup per (row, segment of 2048 floats) writes dx and one partial
 * sum into the workspace, every float of which is written (AGX_ERR_WORKSPACE when it is NULL or shorter than the
 * query's answer): walker j of 256 takes the segment's elements j, j + 256, ... in increasing order (one fma per
 * element), the walkers of each group of 64 are added in a halving tree and the four groups as (g0 + g1) + (g2 + g3).
 * Stage 2: one wavefront per channel numbers the channel's partials p = b * segments + segment over its rows
 * b * channels + c; lane l adds p = l, l + 64, ... in increasing order, then the halving tree.  The segment length is
 * a constant and the walk goes by index, never by address: the order of the sum is a function of (rows, channels, n)
 * alone -- not of the device, the launch or the alignment of an operand. */
int agx_snake_backward(const float *x, const float *alpha, const float *dout, float *dx, float *dalpha, void *workspace,
                       size_t workspace_bytes, int64_t rows, int32_t channels, int64_t n, int32_t variant, float eps,
                       void *stream);

/* ------------------------------------------------------------------------- *
 * The convolution module of a Conformer block (networks/transformers.py:281-335) and the SiLU of its feed-forward
 * halves.  fp32, channel-major contiguous (B, C, T), stream-ordered, no synchronisation, no atomics: every result is
 * bitwise reproducible, and every sum has one order that is a function of (B, C, T, K) alone -- elements are walked by
 * index, never by address, so the alignment of an operand changes no bit.  With left = (K - 1) / 2 (torch's "same":
 * K - 1 - left zeros on the right) and sigmoid(v) = 1 / (1 + expf(-v)) as agx_sigmoid_gate has it (v <= -89: exactly
 * 0, v >= 17: exactly 1):
 *   g[b, c, t] = u[b, c, t] * sigmoid(u[b, C + c, t])                   u is (B, 2 C, T); g is never written
 *   z[b, c, t] = bias[c] + sum_k w[c, k] g[b, c, t + k - left]          zeros outside [0, T); one fma per tap, k rising
 *   rstd = 1 / sqrtf(var[c] + eps)    scale = gamma[c] rstd    shift = beta[c] - mean[c] scale    zhat = (z - mean[c]) rstd
 *   a = training ? zhat * gamma[c] + beta[c] : z * scale + shift        y = a * sigmoid(a)
 * A channel whose taps are all zero gives z == bias[c] exactly for finite u.
 * B, C, T <= 0, K outside [1, AGX_CONFORMER_MAX_K] or a shape beyond the one-dimensional grid (2^31 - 1 workgroups) is
 * AGX_ERR_BAD_SHAPE before anything is launched; a NULL required pointer is AGX_ERR_NULL_POINTER; a workspace that is
 * NULL or shorter than its query's answer is AGX_ERR_WORKSPACE.  Every float of a workspace that is read has been written
 * by the same call.  A non-finite value of u, z or dy in channel c stays in channel c -- its outputs, its statistics
 * and its parameter gradients -- and where no statistic is taken (the forward with gamma) within the K positions around
 * it.
 * ------------------------------------------------------------------------- */
#define AGX_CONFORMER_MAX_K 64
/* One launch, one workgroup per (b, c, tile of 1024 positions).  gamma == beta == mean == var == NULL: out = z.  All
 * four given (eval mode, the running statistics): out = y with training = 0 above, and z is not written. */
int agx_glu_dwconv_forward(const float *u, const float *w, const float *bias, const float *gamma, const float *beta,
                           const float *mean, const float *var, float eps, float *out, int32_t B, int32_t C, int32_t T,
                           int32_t K, void *stream);
/* Bytes of the workspace of agx_bn_stats: two floats per (b, c, segment of 2048 positions).  0 for an invalid shape. */
size_t agx_bn_stats_workspace_bytes(int32_t B, int32_t C, int32_t T);
/* mean[c] and the biased variance var[c] of z over (B, T), two launches.  Stage 1: one workgroup per (b, c, segment)
 * writes the segment's mean and M2 = sum (z - mean)^2 about it (two passes over registers, one read).  Stage 2: one
 * wavefront per channel merges the (n, mean, M2) of the segments p = b * segments + segment by Chan's rule -- lane l
 * takes p = l, l + 64, ... in increasing order, then a halving tree with the lower lane on the left -- so no variance is
 * ever formed as E[z^2] - E[z]^2.  The same stage updates, where the pointers are not NULL,
 *   running_mean += momentum (mean - running_mean),  running_var += momentum (M2 / (B T - 1) - running_var)
 * and adds 1 to *num_batches_tracked.  B * T < 2 is AGX_ERR_BAD_SHAPE. */
int agx_bn_stats(const float *z, float *mean, float *var, float *running_mean, float *running_var,
                 int64_t *num_batches_tracked, float momentum, void *workspace, size_t workspace_bytes, int32_t B, int32_t C,
                 int32_t T, void *stream);
/* y from z, one launch on the row walk of agx_snake_forward (16-byte accesses between the row's 16-byte boundaries,
 * scalar at its ragged ends and everywhere when z and y are not equally aligned).  y may be z.  With training == 0 the
 * result is bitwise what agx_glu_dwconv_forward writes for the same z. */
int agx_bn_silu_forward(const float *z, const float *gamma, const float *beta, const float *mean, const float *var,
                        float eps, int32_t training, float *y, int32_t B, int32_t C, int32_t T, void *stream);
/* Bytes of the workspace of agx_bn_silu_backward: two floats per (b, c, segment of 2048 positions) and 2 C. */
size_t agx_bn_silu_backward_workspace_bytes(int32_t B, int32_t C, int32_t T);
/* With da = dy * s (1 + a (1 - s)), s = sigmoid(a):
 *   dbeta[c] = sum da,   dgamma[c] = sum da zhat                                    (over b and t)
 *   training == 0:  dz = da scale                       (frozen statistics; two launches)
 *   training != 0:  dz = scale (da - dbeta[c] / (B T) - zhat dgamma[c] / (B T))      (three launches)
 * Stage 1: one workgroup per (b, c, segment of 2048) sums da and da zhat -- walker j of 256 takes the elements j,
 * j + 256, ... in increasing order, the walkers of a group of 64 are added in a halving tree, the groups as
 * (g0 + g1) + (g2 + g3) -- and writes dz where the statistics are frozen.  Stage 2: one wavefront per channel, lane l
 * adds the partials p = l, l + 64, ... (p = b * segments + segment), then the halving tree.  Stage 3 (training): dz on the
 * row walk of agx_bn_silu_forward.  dz, or dgamma and dbeta, may be NULL (all three: nothing is launched); dz may be dy. */
int agx_bn_silu_backward(const float *dy, const float *z, const float *gamma, const float *beta, const float *mean,
                         const float *var, float eps, int32_t training, float *dz, float *dgamma, float *dbeta,
                         void *workspace, size_t workspace_bytes, int32_t B, int32_t C, int32_t T, void *stream);
/* Bytes of the workspace of agx_glu_dwconv_backward when it is asked for dw and dbias: K + 1 floats per (b, c, tile of
 * 1024 positions). */
size_t agx_glu_dwconv_backward_workspace_bytes(int32_t B, int32_t C, int32_t T, int32_t K);
/* Backward of z(u, w, bias); g and the sigmoid are recomputed from u.
 *   dg[b, c, t] = sum_k w[c, k] dz[b, c, t + left - k]       (one fma per tap, k rising, from 0)
 *   du[b, c, t] = dg s,   du[b, C + c, t] = (dg u[b, c, t]) (s (1 - s)),   s = sigmoid(u[b, C + c, t])
 *   dw[c, k] = sum_{b, t} dz[b, c, t] g[b, c, t + k - left],   dbias[c] = sum_{b, t} dz[b, c, t]
 * du (B, 2 C, T): both halves are written.  du may be NULL; dw and dbias come together or not at all (all NULL: nothing
 * is launched).  Without dw one launch and no workspace; with it two: the tile's share of every sum (walkers, halving
 * tree and groups as above), then one wavefront per channel over the shares p = b * tiles + tile. */
int agx_glu_dwconv_backward(const float *dz, const float *u, const float *w, float *du, float *dw, float *dbias,
                            void *workspace, size_t workspace_bytes, int32_t B, int32_t C, int32_t T, int32_t K, void *stream);
/* ------------------------------------------------------------------------- *
 * The causal form of the module above and its streaming cache.  Everything stated there holds -- formats, determinism,
 * error codes before any launch -- with left = K - 1: an output sees its own frame and the K - 1 before it, nothing
 * later.
 *   z[b, c, t]  = bias[c] + sum_k w[c, k] G[b, c, t + k - (K - 1)]      one fma per tap, k rising, from bias (as above)
 *   G[t] = g[t] for 0 <= t < T;   G[t] = hist[b, c, (K - 1) + t] for -(K - 1) <= t < 0   (0.f where hist == NULL)
 *   dg[b, c, t] = sum_k w[c, k] dz[b, c, t + (K - 1) - k]               zeros at and beyond T
 *   dw[c, k]    = sum_{b, t} dz[b, c, t] g[b, c, t + k - (K - 1)],   dbias[c] = sum_{b, t} dz[b, c, t]
 * hist is (B, C, K - 1) fp32, oldest frame first: the post-GLU values g of the K - 1 frames before the call (half the
 * size of their u, and no sigmoid is taken twice); all zeros is the start of a stream.  A history is an exact operand.
 * A non-finite value stays in its channel, and leaves the stream K - 1 frames after it entered.  Chunked calls are bit
 * for bit the single call: feeding T frames through hist in chunks of any lengths -- agx_glu_dwconv_step, or
 * agx_glu_dwconv_causal_forward(hist) followed by agx_glu_hist_update -- writes the y that one
 * agx_glu_dwconv_causal_forward over the T frames writes, and leaves in hist the last K - 1 values of g.
 * ------------------------------------------------------------------------- */
#define AGX_CONFORMER_MAX_STEP 64
/* agx_glu_dwconv_forward with left = K - 1: the same tile kernel, the same gamma .. var convention (all NULL: out = z,
 * all given: out = y on the running statistics).  hist may be NULL; it is read, never written. */
int agx_glu_dwconv_causal_forward(const float *u, const float *w, const float *bias, const float *gamma, const float *beta,
                                  const float *mean, const float *var, float eps, const float *hist, float *out, int32_t B,
                                  int32_t C, int32_t T, int32_t K, void *stream);
/* The workspace of agx_glu_dwconv_causal_backward: that of agx_glu_dwconv_backward. */
size_t agx_glu_dwconv_causal_backward_workspace_bytes(int32_t B, int32_t C, int32_t T, int32_t K);
/* agx_glu_dwconv_backward with left = K - 1: its stages, reduction orders and NULL conventions.  No history: there is
 * no backward through a cached call. */
int agx_glu_dwconv_causal_backward(const float *dz, const float *u, const float *w, float *du, float *dw, float *dbias,
                                   void *workspace, size_t workspace_bytes, int32_t B, int32_t C, int32_t T, int32_t K,
                                   void *stream);
/* The streaming step, one launch: y (B, C, n) of the n new frames u (B, 2 C, n) from hist and u -- the eval form, every
 * one of gamma .. var required -- and hist rewritten in place with the last K - 1 values of [hist | g(u)]; with
 * n < K - 1 the newest K - 1 - n old values move to the front.  1 <= n <= AGX_CONFORMER_MAX_STEP, else
 * AGX_ERR_BAD_SHAPE; hist may be NULL only for K == 1.  Work is packed by output: a workgroup owns R whole (b, c) rows,
 * R = min(256 / n, what 48 KiB of LDS hold, ceil(B C / 1024)) -- its 256 threads filled with outputs once the batch
 * is large enough to leave 1024 workgroups --, stages their histories, their g and their taps in LDS, and reads every
 * history value before the barrier that precedes its writes; no other workgroup touches those rows.  The fma chain of
 * an output is that of agx_glu_dwconv_causal_forward; R changes no bit. */
int agx_glu_dwconv_step(const float *u, const float *w, const float *bias, const float *gamma, const float *beta,
                        const float *mean, const float *var, float eps, float *hist, float *out, int32_t B, int32_t C,
                        int32_t n, int32_t K, void *stream);
/* hist <- the last K - 1 values of [hist | g(u)] for a chunk u (B, 2 C, T) of any T, one launch: what the step does to
 * hist, for cached calls longer than AGX_CONFORMER_MAX_STEP (agx_glu_dwconv_causal_forward(hist), then this).  A
 * workgroup owns whole rows: it reads, then a barrier, then it writes.  K == 1: nothing is launched. */
int agx_glu_hist_update(const float *u, float *hist, int32_t B, int32_t C, int32_t T, int32_t K, void *stream);

/* out = x * sigmoid(x) over n floats, one launch; out may be x. */
int agx_silu(const float *x, float *out, int64_t n, void *stream);
/* dx = dout * s (1 + x (1 - s)), s = sigmoid(x), one launch; dx may be dout or x. */
int agx_silu_backward(const float *x, const float *dout, float *dx, int64_t n, void *stream);

/* ---- Streaming conv stacks (csrc/conv_stream.hip) -----------------------------------------------------------
 * A stream advances in whole latent frames; pos[b] (int64, device) counts the frames row b has received.  A layer has a rate
 * (columns per frame) and a delay (how many columns its output lags the stream) on either side:
 *     AGX_CONV_CAUSAL (k, s, d):        rate_out = rate_in / s, delay_out = delay_in / s (s must divide both);
 *     AGX_CONV_TRANSPOSED (k, s = 1):   rate_out = rate_in,     delay_out = delay_in;
 *     AGX_CONV_UPSAMPLE (k = 2 s + 1):  rate_out = rate_in s,   delay_out = delay_in s + s.
 * A step of n frames reads the input columns [pos rate_in - delay_in - reach, (pos + n) rate_in - delay_in) -- reach =
 * d (k - 1) - s + 1, k - 1 and 2 -- and produces exactly the n rate_out output columns [pos rate_out - delay_out,
 * (pos + n) rate_out - delay_out), each the polyphase sum of agx_conv_forward on the standard image of agx_conv_pack
 * (impl AGX_IMPL_AUTO) with epilogue = bias, AGX_EPI_LEAKY_PRE, AGX_EPI_RESIDUAL, AGX_EPI_LEAKY_POST in that order.
 *   src   ring (B, c_in, src_cap): column i of the stream sits at (i mod src_cap), floor mod -- indices are negative at the start
 *         of a delayed layer; src_cap >= reach + n rate_in.  src_cap == 0: a plain (B, c_in, n rate_in) tensor holding the
 *         step's own columns (kernel 1, stride 1 only: the hidden activation of a residual unit).
 *   res   AGX_EPI_RESIDUAL: ring (B, c_out, res_cap >= n rate_out) indexed by the OUTPUT column (stride-1 layers).
 *   dst   ring (B, c_out, dst_cap >= n rate_out) written at (index mod dst_cap), or dst_cap == 0: plain (B, c_out, n rate_out).
 *   end   NULL: no mask.  Else int64 (B,): output column j is stored as exact 0 unless 0 <= j < end[b] rate_out;
 *         AGX_STREAM_LIVE = no end yet.  This is the layer's own zero padding in the plain call, on both sides.
 * pos and end are read, never written; only the n rate_out destination columns of every row are written.  fp32; every
 * output is one fixed fmaf chain whatever n, batch or the ring phase (the split of the reduction over the waves of a workgroup is
 * a function of (c_in, taps) alone).  batch or n <= 0: AGX_OK, nothing launched.  Refusals precede every use of a pointer. */
#define AGX_STREAM_LIVE INT64_MAX
int agx_conv_stream_step(int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation, int32_t epilogue,
                         float slope, const float *packed, const float *bias, const float *src, int32_t src_cap, const float *res,
                         int32_t res_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end, int32_t batch, int32_t n,
                         int32_t rate_in, int64_t delay_in, void *stream);
/* Host-only: "conv_stream<KS,NT>" (KS waves split the reduction, a lane carries NT base positions), "none" for an empty step,
 * or the launcher's refusal of the layer. */
int agx_conv_stream_kernel_name(int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation, int32_t n,
                                int32_t rate_in, char *buf, size_t buf_len);
/* buf[b, c, (pos[b] rate + t) mod cap] = src[b, c, t] for src (B, rows, n_cols) contiguous, buf (B, rows, cap), n_cols <= cap:
 * a stack's input chunk (n frames of `rate` columns) into its first ring.  Writes those columns only; pos is not written. */
int agx_ring_write_rate(float *buf, const float *src, const int64_t *pos, int32_t batch, int32_t rows, int32_t n_cols, int32_t cap,
                        int32_t rate, void *stream);
/* end[r] = pos[r] for the n_rows row numbers in `rows` (int64, device; entries outside [0, batch) are skipped), or for every
 * row when rows is NULL: the stream of those rows ends at the frames they have received.  Writes end only. */
int agx_stream_mark_end(const int64_t *pos, int64_t *end, const int64_t *rows, int32_t n_rows, int32_t batch, void *stream);

/* ---- Per-row frame counts -------------------------------------------------------------------------------------
 * The counted form of every streaming step.  counts is int64 (B,) in device memory, read by the kernels and never by the host:
 * row b takes the first c_b = clamp(counts[b], 0, n) frames of the chunk, n still the chunk's width.  A captured step replays
 * with whatever counts holds at the replay.  Memory safety does not depend on the values: every workgroup clamps them (the
 * stance of "a negative position is read as 0").
 *   - the valid part of row b's result -- its first c_b rate_out columns -- is bit for bit what the uncounted entry point
 *     computes for those frames: the count decides which outputs are stored, never how one is computed;
 *   - a plain (non-ring) fp32 output is exact 0 past the count (a select: NaN in the chunk past the count reaches nothing);
 *   - a ring column, a history value and a position past the count are not written: with c_b == 0 nothing of row b changes.
 * Arguments, refusals and kernel choice are those of the uncounted entry point, plus AGX_ERR_NULL_POINTER for counts == NULL.
 * The uncounted entry points run instances with the count compiled out. */
/* agx_conv_stream_step on the first c_b rt base positions of row b (KS, NT and the grid as for n). */
int agx_conv_stream_step_counted(int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation,
                                 int32_t epilogue, float slope, const float *packed, const float *bias, const float *src, int32_t src_cap,
                                 const float *res, int32_t res_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end,
                                 const int64_t *counts, int32_t batch, int32_t n, int32_t rate_in, int64_t delay_in, void *stream);
/* agx_ring_write_rate of the first c_b rate columns of row b, c_b = clamp(counts[b], 0, n_cols / rate). */
int agx_ring_write_rate_counted(float *buf, const float *src, const int64_t *pos, const int64_t *counts, int32_t batch, int32_t rows,
                                int32_t n_cols, int32_t cap, int32_t rate, void *stream);
/* agx_ring_write_pos of the first c_b columns of row b. */
int agx_ring_write_pos_counted(float *buf, const float *src, int64_t buf_batch_stride, int64_t buf_row_stride, int64_t src_batch_stride,
                               const int64_t *pos, const int64_t *counts, int32_t batch, int32_t rows, int32_t n, int32_t ring,
                               void *stream);
/* agx_attention_alibi_stream with the keys of row b ending at its count: the ring columns of the chunk's frames behind c_b --
 * which agx_ring_write_pos_counted left unwritten -- are not live (staged as zeros, never multiplied as stored).  The
 * queries below the count are bit for bit those of the uncounted call on a chunk of c_b frames; every query is written, and
 * what the ones at and behind the count hold means nothing (NaN where a row has no live key): the caller masks them. */
int agx_attention_alibi_stream_counted(const float *q, const float *kv, int64_t q_batch_stride, int64_t kv_batch_stride,
                                       int64_t kv_row_stride, const int64_t *pos, const int64_t *counts, const float *slopes, float *out,
                                       int32_t batch, int32_t heads, int32_t head_dim, int32_t tq, int32_t window, int32_t kv_ring,
                                       float scale_div, void *stream);
/* pos[b] += clamp(counts[b], 0, n). */
int agx_stream_advance_counted(int64_t *pos, const int64_t *counts, int32_t batch, int64_t n, void *stream);
/* agx_glu_dwconv_step on the first c_b frames of batch entry b: out is exact 0 at t >= c_b, and hist becomes the last K - 1
 * values of [hist | g of the first c_b frames] (c_b == 0: not written). */
int agx_glu_dwconv_step_counted(const float *u, const float *w, const float *bias, const float *gamma, const float *beta,
                                const float *mean, const float *var, float eps, float *hist, float *out, const int64_t *counts, int32_t B,
                                int32_t C, int32_t n, int32_t K, void *stream);
/* agx_mask_tail with int64 counts for lengths: out[b, c, i] = i < clamp(counts[b], 0, t) ? x[b, c, i] : 0; out may be x. */
int agx_mask_tail_counted(const float *x, const int64_t *counts, float *out, int32_t batch, int32_t channels, int32_t t, void *stream);

/* ---- RVQ streaming step and its packets -----------------------------------------------------------------------
 * The quantiser of a streaming chunk: batch rows of n <= AGX_RVQ_STEP_MAX_N frames, counts as above (NULL: every row takes n).
 * Frame (b, t) is live when t < c_b.  Every live frame gets the full DEFINING search of oracle/rvq_exact.c over every codeword
 * of every stage (binary64, d ascending, subtract / multiply / add never fused, the smallest k on equal distance,
 * r <- fl32(r - c) between stages): no score pass, no candidates, no error bound, and no input it is slow on.
 *   codebooks : (q_total, K, D) fp32; sizes: host int32[q_total] or NULL, the real codewords of each stage (agx_rvq_pack_sized).
 *   zq        : (B, D, n) by strides, fp32, may be NULL; live: ((0 + c_0) + c_1) + .. in binary32, stage order; dead: exact 0.
 *   index     : (B, n, q_used) int64, contiguous; live: the codes; dead: -1.
 *   packets   : (B, P) uint8, contiguous, P = agx_rvq_step_packet_bytes(n, q_used, bits), may be NULL.  Row b's first
 *               ceil(c_b q_used bits / 8) bytes are the dense little-endian packing of its c_b q_used codes, frame-major and
 *               stage-minor -- what agx_codes_pack gives for index[b, :c_b]; the unused high bits of the last byte and every
 *               byte behind it are 0.  Rows never share a byte, and P does not depend on counts.
 *   workspace : agx_rvq_step_workspace_bytes() bytes, 8-byte aligned; written before it is read.
 * NaN or anything else in a dead frame's latent reaches no output; a NaN in a live frame gives unspecified codes, in bounds.
 * q_used == 0: zq = 0 and P = 0.  One launch per stage and one for the outputs; no workgroup waits for another.
 * Refused before the first launch: n > AGX_RVQ_STEP_MAX_N, q_total > 64, bits outside 1 .. 16, D > 8192, K > 65536, a stage
 * wider than 2^bits when packets are asked for, NULL pointers, a small workspace. */
#define AGX_RVQ_STEP_MAX_N 32
/* ceil(n q_used bits / 8); host only; AGX_ERR_BAD_SHAPE (negative) on n outside 1 .. AGX_RVQ_STEP_MAX_N, q_used outside 0 .. 64
 * or bits outside 1 .. 16. */
int64_t agx_rvq_step_packet_bytes(int32_t n, int32_t q_used, int32_t bits);
size_t agx_rvq_step_workspace_bytes(int32_t batch, int32_t n, int32_t dim, int32_t k, int32_t q_used);
int agx_rvq_step_encode(const float *z, int64_t z_sb, int64_t z_st, int64_t z_sd, const float *codebooks, const int32_t *sizes,
                        const int64_t *counts, int32_t batch, int32_t n, int32_t dim, int32_t k, int32_t q_total, int32_t q_used,
                        int32_t bits, float *zq, int64_t q_sb, int64_t q_st, int64_t q_sd, int64_t *index, uint8_t *packets,
                        void *workspace, size_t workspace_bytes, void *stream);
/* Packets -> zq (and index, may be NULL), one launch.  A code >= sizes[q] (a corrupt packet, or bits wider than the stage)
 * selects no codeword: it adds nothing and reads nothing; index holds it as it was read.  Packet bytes behind a row's first
 * ceil(c_b q_used bits / 8) are not read.  Dead frames: zq exact 0, index -1. */
int agx_rvq_step_decode(const uint8_t *packets, int32_t bits, const float *codebooks, const int32_t *sizes, const int64_t *counts,
                        int32_t batch, int32_t n, int32_t dim, int32_t k, int32_t q_total, int32_t q_used, float *zq, int64_t q_sb,
                        int64_t q_st, int64_t q_sd, int64_t *index, void *stream);

/* ---- Per-row stage counts -------------------------------------------------------------------------------------
 * The first q stages of a frame's codes are a complete, coarser description of it, so a row's bitrate is the number of stages it
 * sends.  stages is a contiguous int64 (B,) device tensor read by the kernels as counts is: q_b = clamp(stages[b], 0, q_used),
 * the host never reads it, and NULL means q_b = q_used for every row.  Stage q of frame (b, t) is live when t < c_b and q < q_b.
 * P = agx_rvq_step_packet_bytes(n, q_used, bits) depends on neither tensor: buffers and captured graphs keep their shapes.
 *
 * agx_rvq_step_encode_staged: agx_rvq_step_encode with stages after counts.
 *   index   : (B, n, q_used); a live entry holds the code, every other entry -1.
 *   zq      : a live frame: ((0 + c_0) + c_1) + .. + c_{q_b - 1} in binary32, stage order; behind the count, or q_b == 0: exact 0.
 *   packets : row b's first ceil(c_b q_b bits / 8) bytes are the dense little-endian packing of index[b, :c_b, :q_b], frame-major
 *             and stage-minor over the row's OWN q_b; the unused high bits of the last byte and every byte behind it are 0.
 *   Row b's zq, index[b, :, :q_b] and live packet bytes are bit for bit what agx_rvq_step_encode gives for that row with
 *   q_used = q_b: the stage count decides what is searched and stored, never how a distance or a sum is computed.  The search
 *   launch of stage q leaves row b's workgroups right after reading counts and stages when q >= q_b: nothing of the frame, the
 *   codebook or the workspace is loaded and no partial is written.  Launches, refusals and the workspace are those of
 *   agx_rvq_step_encode for q_used.
 * agx_rvq_step_decode_staged: agx_rvq_step_decode with stages after counts.  Frame t of row b reads its q_b codes from bit
 *   (t q_b + q) bits on; bytes behind the row's first ceil(c_b q_b bits / 8) are not read; index is -1 where a stage is not
 *   live; a code >= sizes[q] adds and reads nothing, as before.
 * agx_rvq_packets_restage: packets of q_in = clamp(stages_in[b], 0, q_used) stages per row (stages_in NULL: q_used) ->
 *   packets of q_out = min(q_in, clamp(stages_to[b], 0, q_used)) stages, in one launch, without codebooks or workspace: a bit
 *   gather, output byte i collecting the codes whose bits it holds from their input bit positions.  out[b] is byte for byte the
 *   packet agx_rvq_step_encode_staged writes with q_out, zero tail included; stages_out[b] = q_out (may be NULL) is written by
 *   the kernel, so the receiver's stages never pass through the host.  in and out are (B, P) uint8, contiguous; input bytes
 *   behind ceil(c_b q_in bits / 8) are not read.  Refused: in and out sharing a byte (AGX_ERR_BAD_SHAPE), stages_to == NULL
 *   (AGX_ERR_NULL_POINTER), n, q_used or bits outside what agx_rvq_step_packet_bytes takes. */
int agx_rvq_step_encode_staged(const float *z, int64_t z_sb, int64_t z_st, int64_t z_sd, const float *codebooks, const int32_t *sizes,
                               const int64_t *counts, const int64_t *stages, int32_t batch, int32_t n, int32_t dim, int32_t k,
                               int32_t q_total, int32_t q_used, int32_t bits, float *zq, int64_t q_sb, int64_t q_st, int64_t q_sd,
                               int64_t *index, uint8_t *packets, void *workspace, size_t workspace_bytes, void *stream);
int agx_rvq_step_decode_staged(const uint8_t *packets, int32_t bits, const float *codebooks, const int32_t *sizes, const int64_t *counts,
                               const int64_t *stages, int32_t batch, int32_t n, int32_t dim, int32_t k, int32_t q_total, int32_t q_used,
                               float *zq, int64_t q_sb, int64_t q_st, int64_t q_sd, int64_t *index, void *stream);
int agx_rvq_packets_restage(const uint8_t *in, const int64_t *stages_in /* may be NULL */, const int64_t *stages_to,
                            const int64_t *counts /* may be NULL */, int32_t batch, int32_t n, int32_t q_used, int32_t bits, uint8_t *out,
                            int64_t *stages_out /* may be NULL */, void *stream);

/* ---- Streaming wavelet blocks (csrc/wavelet_stream.hip) --------------------------------------------------------
 * A wavelet decoder block (conv_in "same", k_in odd, p_in = (k_in - 1) / 2; fold by scale s >= 2 over n_points P, s | P;
 * conv_out "same", k_out odd, p_out = (k_out - 1) / 2) as two steps of a stream, in the terms of "Streaming conv stacks".  The
 * block sits at rate_in = r columns per frame with delay D; L_b = end[b] r is the length of row b's signal at the block's input,
 * infinite while end[b] == AGX_STREAM_LIVE.
 *   in-step   produces the n r columns [pos r - D_h, (pos + n) r - D_h) of h, D_h = D + p_in, into the ring of h:
 *             h[l] = bias + sum_j W[j] x[l + j - p_in], x from the block's input ring (exact 0 outside [0, L_b) already);
 *             stored as exact 0 unless 0 <= l < L_b.  Reach k_in - 1: src_cap >= k_in - 1 + n r.  rate_h = r, delay_h = D_h.
 *   out-step  produces the n r s columns [pos r s - D_out, (pos + n) r s - D_out), D_out = D_h s + s + p_out:
 *             out[u] = bias + sum_{c, j} Wo[o, c, j] y[c, u + j - p_out], then AGX_EPI_LEAKY_PRE; stored as exact 0 unless
 *             0 <= u < L_b s.  y is never stored; with l0 = floor(v / s), ph = v - l0 s:
 *                 y[c, v] = 0                                                          v < 0 or v >= L_b s
 *                 y[c, v] = ph == 0 ? h[c, l0] S_hi[c, 0]
 *                                   : fmaf(h[c, l0 + 1], S_lo[c, ph], h[c, l0] * S_hi[c, ph])    v < (L_b - 1) s + 1
 *                 y[c, v] = tail[c, v - ((L_b - 1) s + 1)] * h[c, L_b - 1]              the last s - 1 live columns
 *             -- agx_wavelet_fold's two taps and raw tail, the tail decided by the device-held end.  Every case is a select
 *             on the index, never a product with a 0 of the table or of a mask: the column l0 + 1 behind ph == 0 may be one the
 *             ring has not received, and it is not read.  Reach in h: 1 + ceil(2 p_out / s); h_cap >= that + n r.
 *   table     (hidden, 3 s - 1) fp32 per channel: S_hi[0 .. s), S_lo[0 .. s), tail[0 .. s - 1) = kern[P - (s - 1) .. P), with
 *             kern, S_hi and S_lo formed by the code of agx_wavelet_fold.  agx_wavelet_fold_table writes it in one launch.
 * With these delays a step reads no column of h that has not been produced, and every tail column is computed in a step after
 * end was set (D_out > s - 1).  Both steps are the kernel of agx_conv_stream_step -- the same fixed fmaf chain per output, KS a
 * function of the layer alone -- on the standard image of agx_conv_pack for AGX_CONV_SAME; the out-step forms its operands on
 * the fly.  dst of the out-step: a ring (dst_cap >= n r s) or, dst_cap == 0, a plain (B, c_out, n r s) tensor.  The _counted
 * forms follow "Per-row frame counts".  batch or n <= 0: AGX_OK, nothing launched.  Refused before any launch or use of a
 * pointer: s < 2, s not dividing P, an even kernel, a capacity too small, NULL pointers (end included), dst aliasing a source. */
int agx_wavelet_fold_table(const float *space, const float *sigma, int32_t sigma_len, float *table, int32_t channels, int32_t n_points,
                           int32_t scale, void *stream);
int agx_wavelet_stream_in_step(int32_t c_in, int32_t hidden, int32_t kernel, const float *packed, const float *bias, const float *src,
                               int32_t src_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end, int32_t batch, int32_t n,
                               int32_t rate_in, int64_t delay_in, void *stream);
int agx_wavelet_stream_in_step_counted(int32_t c_in, int32_t hidden, int32_t kernel, const float *packed, const float *bias, const float *src,
                                       int32_t src_cap, float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end,
                                       const int64_t *counts, int32_t batch, int32_t n, int32_t rate_in, int64_t delay_in, void *stream);
int agx_wavelet_stream_out_step(int32_t hidden, int32_t c_out, int32_t kernel, int32_t scale, int32_t epilogue, float slope,
                                const float *packed, const float *bias, const float *table, const float *h, int32_t h_cap, float *dst,
                                int32_t dst_cap, const int64_t *pos, const int64_t *end, int32_t batch, int32_t n, int32_t rate_h,
                                int64_t delay_h, void *stream);
int agx_wavelet_stream_out_step_counted(int32_t hidden, int32_t c_out, int32_t kernel, int32_t scale, int32_t epilogue, float slope,
                                        const float *packed, const float *bias, const float *table, const float *h, int32_t h_cap,
                                        float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end, const int64_t *counts,
                                        int32_t batch, int32_t n, int32_t rate_h, int64_t delay_h, void *stream);
/* Host-only, in the style of agx_conv_stream_kernel_name: "conv_stream<KS,NT>" / "wavelet_stream_out<KS,NT>", "none" for an empty
 * step, or the launcher's refusal.  KS does not move with n. */
int agx_wavelet_stream_in_kernel_name(int32_t c_in, int32_t hidden, int32_t kernel, int32_t n, int32_t rate_in, char *buf, size_t buf_len);
int agx_wavelet_stream_out_kernel_name(int32_t hidden, int32_t c_out, int32_t kernel, int32_t scale, int32_t n, int32_t rate_h, char *buf,
                                       size_t buf_len);

/* ---- Streaming multires layers and depthwise residual blocks (csrc/multires_stream.hip, csrc/conv_stream.hip) -----
 * Both keep state only in the ring of their own input, in the terms of "Streaming conv stacks"; rate_out = rate_in and
 * delay_out = delay_in for both.
 *
 * agx_multires_stream_step: one chunk of n frames of a (B, C, src_cap) ring through the whole cascade of agx_multires_forward,
 * one launch.  With j = pos[b] rate - delay + t the stream index of output column t < n rate:
 *     lo_0 = x;  level lvl = depth .. 1 has dilation dil = 2^(depth - lvl):
 *         hi_lvl[j] = sum_k h1[c, k] lo[j - (K - 1 - k) dil],  lo'[j] = sum_k h0[c, k] lo[j - (K - 1 - k) dil]
 *     (each an fmaf chain from 0 over the taps in ascending k), and
 *     y[c, j] = gelu(fmaf(x[c, j], w[c, depth + 1], fmaf(w[c, 0], lo_depth[c, j], acc))),
 *     acc = fmaf(w[c, 1], hi_1, .. fmaf(w[c, depth], hi_depth, 0)) -- the order of agx_multires_forward, the same erf GELU.
 * reach = (K - 1)(2^depth - 1); src_cap >= reach + n rate.  Input columns of stream index < 0 are 0 in the ring (it starts
 * zero-filled and every producer stores exact 0 there), so the cascade needs no select on the index.  An output with j < 0 or
 * j >= end[b] rate is stored as exact 0 (end == NULL: no mask).  dst: the consumer's ring (dst_cap >= n rate, written at
 * j mod dst_cap) or, dst_cap == 0, a plain (B, C, n rate) tensor.  Work is packed by outputs: a workgroup of 256 threads owns
 * R = max(1, 256 / tile) channel rows of one batch entry and one tile of min(n rate, AGX_MULTIRES_STREAM_TILE) columns, with
 * the reach as left halo, two LDS rows per channel row; the chain of an output does not depend on R, the tile, n or the ring
 * phase.  The counted form follows "Per-row frame counts": no source column behind a row's count is read.
 * Refused before any launch or use of a pointer: K < 1, depth outside 0 .. 20, a reach + tile whose two LDS rows and taps
 * exceed AGX_MULTIRES_STREAM_LDS_BYTES (AGX_ERR_UNSUPPORTED), src_cap < reach + n rate, 0 < dst_cap < n rate, dst == src,
 * NULL pointers, sizes beyond the grid.  batch or n <= 0: AGX_OK, nothing launched. */
#define AGX_MULTIRES_STREAM_TILE 1024
#define AGX_MULTIRES_STREAM_LDS_BYTES 65536
int agx_multires_stream_step(const float *h0, const float *h1, const float *w, const float *src, int32_t src_cap, float *dst,
                             int32_t dst_cap, const int64_t *pos, const int64_t *end, int32_t batch, int32_t channels, int32_t n,
                             int32_t kernel, int32_t depth, int32_t rate, int64_t delay, void *stream);
int agx_multires_stream_step_counted(const float *h0, const float *h1, const float *w, const float *src, int32_t src_cap, float *dst,
                                     int32_t dst_cap, const int64_t *pos, const int64_t *end, const int64_t *counts, int32_t batch,
                                     int32_t channels, int32_t n, int32_t kernel, int32_t depth, int32_t rate, int64_t delay,
                                     void *stream);
/* agx_conv_stream_step with a per-channel affine in the operand fetch -- the dilated conv of a depthwise residual block, whose
 * grouped k = 1 conv (folded weight scale[c], bias shift[c]) is never stored.  The operand of channel c at stream column i is
 *     i >= 0 && c < c_in ? fmaf(scale[c], x[c, i], shift[c]) : 0
 * a select on the index, never a product with 0: before the start of the stream the conv sees its own zero padding, not the
 * affine's bias, and the channels that pad the last group of 16 give 0.  Everything else -- the image, the chain of an output,
 * the epilogue, the mask, the kernel choice -- is agx_conv_stream_step's.  AGX_CONV_CAUSAL with stride 1 from a ring only
 * (src_cap > 0): everything else is AGX_ERR_UNSUPPORTED; scale or shift NULL: AGX_ERR_NULL_POINTER. */
int agx_conv_stream_step_affine(int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation,
                                int32_t epilogue, float slope, const float *packed, const float *bias, const float *scale,
                                const float *shift, const float *src, int32_t src_cap, const float *res, int32_t res_cap, float *dst,
                                int32_t dst_cap, const int64_t *pos, const int64_t *end, int32_t batch, int32_t n, int32_t rate_in,
                                int64_t delay_in, void *stream);
int agx_conv_stream_step_affine_counted(int32_t kind, int32_t c_in, int32_t c_out, int32_t kernel, int32_t stride, int32_t dilation,
                                        int32_t epilogue, float slope, const float *packed, const float *bias, const float *scale,
                                        const float *shift, const float *src, int32_t src_cap, const float *res, int32_t res_cap,
                                        float *dst, int32_t dst_cap, const int64_t *pos, const int64_t *end, const int64_t *counts,
                                        int32_t batch, int32_t n, int32_t rate_in, int64_t delay_in, void *stream);

/* ---- Code prior (csrc/prior.hip) --------------------------------------------------------------------------------
 * The operations between a Transformer and the quantiser's codes.  Operands are fp32 or int64, contiguous; every argument is
 * validated before the first launch; no call allocates or reads device data on the host, so every call can be captured.
 * n_q <= 64 (AGX_ERR_UNSUPPORTED beyond).  `sizes` (HOST, n_q int32, 1 <= sizes[q] <= k; NULL: k everywhere) travels by value.
 * `counts` / `stages` (int64 (B,), device, may be NULL) follow "Per-row frame counts" / "Per-row stage counts": c_b =
 * clamp(counts[b], 0, n), q_b = clamp(stages[b], 0, n_q), NULL = n / n_q.
 *
 * agx_codes_embed: tables (n_q, rows, dim), index (B, n, n_q) -> out (B, dim, n), channel-major:
 *     out[b, :, i] = ((0 + tables[0][index[b,i,0]]) + tables[1][index[b,i,1]]) + ...      in binary32, in stage order;
 * an index outside [0, rows) contributes nothing (this covers -1); the columns i >= c_b are exact 0 and their indices are not
 * read.  One launch for all stages. */
int agx_codes_embed(const float *tables, const int64_t *index, const int64_t *counts /* may be NULL */, float *out, int32_t batch,
                    int32_t n, int32_t n_q, int32_t rows, int32_t dim, void *stream);
/* Its backward: dout (B, dim, n) -> dtables (n_q, rows, dim), every element written:
 *     dtables[q][r] = the sum of dout[b, :, i] over the frames (b, i), i < c_b, with index[b,i,q] == r,
 * ONE binary32 chain per element that starts at 0 and takes the frames in ascending (b, i) order -- no float atomics, two calls
 * agree bit for bit (the convention of agx_rvq_backward's dcodebooks); exact 0 for a row nobody chose.  Three launches (dout as
 * rows, the index as int32 per stage, the sums).  The workspace (8-byte aligned, AGX_ERR_WORKSPACE when short) is
 * agx_codes_embed_backward_workspace_bytes(batch, n, n_q, dim) = B n (4 dim + 4 n_q) bytes rounded up to 8 twice. */
size_t agx_codes_embed_backward_workspace_bytes(int32_t batch, int32_t n, int32_t n_q, int32_t dim);
int agx_codes_embed_backward(const float *dout, const int64_t *index, const int64_t *counts /* may be NULL */, float *dtables,
                             int32_t batch, int32_t n, int32_t n_q, int32_t rows, int32_t dim, void *workspace, size_t workspace_bytes,
                             void *stream);
/* agx_codes_cross_entropy: logits (B, n_q * k, t) -- the head conv's output as it stands, channel q * k + c --, target (B, t, n_q).
 * Entry (b, t, q) is live when 0 <= target < sizes[q].  lse[b,t,q] = log sum_{c < sizes[q]} exp(logit_c) (online maximum and sum,
 * binary32); nll[b,t,q] = lse - logit[target]; both exact 0 where dead.  *n_live (int64) = the live entries, counted on the device;
 * *loss = sum(nll) / n_live, 0 when n_live == 0.  The sum runs in a fixed order in two stages -- the 64 entries of a workgroup on a
 * tree, then the workgroups' partials (binary64) in ascending order on a tree of 256: two launches, no atomics.  The maximum and
 * the sum of an entry are formed over four quarters of k and merged in ascending order.  Workspace:
 * agx_codes_cross_entropy_workspace_bytes(batch, t, n_q) = 16 ceil(B t n_q / 64) bytes, 8-byte aligned.  B t n_q <= 2^36. */
size_t agx_codes_cross_entropy_workspace_bytes(int32_t batch, int32_t t, int32_t n_q);
int agx_codes_cross_entropy(const float *logits, const int64_t *target, const int32_t *sizes /* host, may be NULL */, int32_t batch,
                            int32_t t, int32_t n_q, int32_t k, float *nll, float *lse, float *loss, int64_t *n_live, void *workspace,
                            size_t workspace_bytes, void *stream);
/* Its backward, from the forward's lse and n_live and one device float g (the gradient of loss): every element of dlogits
 * (B, n_q * k, t) is written,
 *     dlogits[b, q k + c, t] = g * (exp(logit_c - lse) - [c == target]) / n_live      at live entries, c < sizes[q],
 * and exact 0 at dead entries, at c >= sizes[q] and everywhere when n_live == 0.  One launch. */
int agx_codes_cross_entropy_backward(const float *logits, const int64_t *target, const int32_t *sizes /* host, may be NULL */,
                                     const float *lse, const int64_t *n_live, const float *g, int32_t batch, int32_t t, int32_t n_q,
                                     int32_t k, float *dlogits, void *stream);
/* agx_codes_sample: logits (B, n_q * k, n) -> codes (B, n, n_q) int64.  seeds, frame0, top_k: int64 (B,); temperature, top_p:
 * fp32 (B,) -- per row, so one captured step serves rows with different settings.  k <= AGX_CODES_SAMPLE_MAX_K
 * (AGX_ERR_UNSUPPORTED beyond: the order and the prefix sums of one stage live in LDS).
 * Row (b, i, q), i < c_b, q < q_b, over l_c, c < sizes[q]; every decision is made in binary64:
 *   1. tau = temperature[b] <= 0: the code is the argmax, the lowest c on ties.  Otherwise:
 *   2. the codes are ordered by (l_c descending, c ascending); the comparisons are exact (-0 == +0).
 *   3. top_k[b] > 0 keeps the first min(top_k, size) of that order.
 *   4. z = (double)l / (double)tau; e = exp(z - z_max) (1 where z == z_max); C_j = the prefix sums of e in that order.
 *   5. top_p[b] < 1 keeps the shortest prefix with C_j / C_all >= top_p, and at least one code.
 *   6. u = (w + 0.5) / 2^32, w = word 0 of Philox4x32-10 ("Dropout masks": the generator) at the counter
 *      (lo32(f), hi32(f), q, AGX_CODES_SAMPLE_STREAM), f = frame0[b] + i, under the key (lo32(seeds[b]), hi32(seeds[b])).
 *   7. the code is the first j of the kept prefix with C_j >= u * C_kept.
 * The prefix sums may be formed in any order of additions (a workgroup scan): a result is pinned where the decisions of 5 and 7
 * hold with a margin of 2^-36 of the kept mass (tests/prior_ref.py "decided").  codes is -1 at i >= c_b and at q >= q_b.
 * `carry` (B, n_q) int64, may be NULL: carry[b] becomes the codes of frame c_b - 1 when c_b >= 1 and is untouched otherwise -- a
 * paused row changes nothing.  A draw is a pure function of (seed, f, q, logits, settings): not of the chunking, the batch slot
 * or a replay count.  NaN logits or settings give an unspecified code in [-1, size); no write goes out of bounds. */
#define AGX_CODES_SAMPLE_MAX_K 2048
#define AGX_CODES_SAMPLE_STREAM 0x53414D50u /* "SAMP": apart from every dropout site's stream id (4 l + 0 .. 3) */
int agx_codes_sample(const float *logits, const int32_t *sizes /* host, may be NULL */, const int64_t *seeds, const int64_t *frame0,
                     const float *temperature, const int64_t *top_k, const float *top_p, const int64_t *counts /* may be NULL */,
                     const int64_t *stages /* may be NULL */, int64_t *carry /* may be NULL, in/out */, int64_t *codes, int32_t batch,
                     int32_t n, int32_t n_q, int32_t k, void *stream);

/* ---- Entropy coding (csrc/entropy.hip) --------------------------------------------------------------------------
 * The code prior's logits as the probability model of a byte-wise rANS coder for the stream packets.  Operands are fp32, int32,
 * int64 or uint8, contiguous; every argument is validated before the first launch; no call allocates or reads device data on the
 * host, so every call can be captured.  `sizes` (HOST, n_q int32, 1 <= sizes[q] <= k; NULL: k everywhere) travels by value.
 * `counts` / `stages` (int64 (B,), device, may be NULL): c_b = clamp(counts[b], 0, n), q_b = clamp(stages[b], 0, n_q), NULL = n /
 * n_q.  n_q <= 64 and k <= AGX_CODES_CUM_MAX_K (the frequencies and the table of one stage live in LDS, as the sampler's order
 * does); n * n_q <= AGX_RANS_MAX_SYMBOLS for the coder (a row's symbols and bytes live in LDS); AGX_ERR_UNSUPPORTED beyond.
 * M = 2^AGX_RANS_SCALE_BITS is the total of a table, L = AGX_RANS_L the coder's lower bound: its state x lies in [L, 2^31).
 *
 * agx_codes_cum: logits (B, n_q * k, n), as the head writes them -> cum, int32 (B, n_cum, n_q, k + 1): frame i of the call lands
 * at frame i_cum + i of the table buffer (0 <= i_cum <= n_cum - n) and no other frame of it is touched.  Entry (b, i, q) is live
 * when i < c_b and q < q_b; size = sizes[q].  A live entry, every decision in binary64:
 *   1. e_c = exp((double)l_c - l_max), c < size; S = sum e_c, in any order (a workgroup reduction).
 *   2. r_c = (M - size) * e_c / S; f_c = 1 + floor(r_c).
 *   3. the lowest argmax a of the binary32 logits (-0 == +0) takes the rest: f_a += M - sum_c f_c.
 *   4. cum[0] = 0, cum[c + 1] = cum[c] + f_c, cum[c] = M for size < c <= k.
 * So f_c >= 1 below size, 0 at or above it, and cum[size] == M exactly, whatever the floating-point sums do.  A frequency is
 * pinned where r_c keeps 2^-24 from the integer it could cross (tests/entropy_ref.py "decided").  A dead entry's table is exact
 * 0 and its logits are not read.  NaN or infinite logits give unspecified frequencies that still obey the line above.  One
 * launch, one workgroup per entry. */
#define AGX_RANS_SCALE_BITS 16
#define AGX_RANS_L (1u << 23)
#define AGX_CODES_CUM_MAX_K 2048
#define AGX_RANS_MAX_SYMBOLS 8192
int agx_codes_cum(const float *logits, const int32_t *sizes /* host, may be NULL */, const int64_t *counts /* may be NULL */,
                  const int64_t *stages /* may be NULL */, int32_t *cum, int32_t batch, int32_t n, int32_t n_q, int32_t k, int32_t n_cum,
                  int32_t i_cum, void *stream);
/* agx_codes_rans_encode: cum (B, n, n_q, k + 1), codes (B, n, n_q) int64 -> packets (B, P) uint8 with P = 2 n n_q + 4, nbytes
 * (B,) int64, status (B,) int64.  A row's symbols are its live entries in (i, q) order, s_1 .. s_N:
 *   1. x = L.
 *   2. for j = N .. 1, with (start, f) = (cum[s_j], cum[s_j + 1] - cum[s_j]):
 *        while x >= ((L >> 16) << 8) * f: push x & 255, x >>= 8;        then x = ((x / f) << 16) + (x % f) + start.
 *   3. push the four bytes of x, least significant first.
 *   4. the packet is the pushed bytes REVERSED: packet[0..3] is x big-endian.
 * nbytes[b] is the packet's length, 0 when N == 0; every byte of the row behind it is 0.  A live code outside [0, size) -- or one
 * whose pair is not that of a table (f < 1, start < 0, start + f > M) -- is skipped and sets bit 0 of status[b]; otherwise
 * status[b] = 0.  x < 2^31 before every symbol and the threshold is >= 2^15, so a symbol pushes two bytes at the most and P always
 * suffices (2 N + 4 is reached when every coded f is 1).  One launch, one wave per row. */
int agx_codes_rans_encode(const int32_t *cum, const int64_t *codes, const int32_t *sizes /* host, may be NULL */,
                          const int64_t *counts /* may be NULL */, const int64_t *stages /* may be NULL */, uint8_t *packets,
                          int64_t *nbytes, int64_t *status, int32_t batch, int32_t n, int32_t n_q, int32_t k, void *stream);
/* agx_codes_rans_decode: the receiver, a call for frames i0 .. i0 + n - 1 of a hop of `hop` frames (0 <= i0 <= hop - n; here c_b =
 * clamp(counts[b], 0, hop)).  cum (B, hop, n_q, k + 1): the tables of the hop, of which the call reads frames i0 .. i0 + n - 1;
 * packets (B, p) uint8 with any p >= 1; nbytes (B,) int64.  state (B, 2) int64, in/out: x and the read cursor; status (B,) int64,
 * in/out: a call with i0 == 0 starts both anew, a later one continues them.  codes (B, n, n_q) int64, out.
 * Row b decodes frames i0 <= i < min(i0 + n, c_b):
 *   1. at i0 == 0: x = packet[0..3] big-endian, cursor = 4.
 *   2. per symbol: slot = x & 0xffff; the code is the c < size with cum[c] <= slot < cum[c + 1]; x = f * (x >> 16) + slot - cum[c].
 *   3. while x < L: x = (x << 8) | next byte -- two bytes at the most, as the coder pushes; bit 2 of status[b] if x < L remains.
 *   4. a read at or past min(nbytes[b], p) is not performed: it yields 0 and sets bit 1 of status[b].
 *   5. when the call decodes the row's last frame c_b - 1, bit 2 is set unless x == L and the cursor equals nbytes[b].
 * codes is -1 at i >= c_b and at q >= q_b.  `carry` (B, n_q) int64, may be NULL, the sampler's semantics per call: carry[b]
 * becomes the codes of the last frame of the row that this call decoded, frame min(i0 + n, c_b) - 1, with -1 at q >= q_b, and is
 * untouched when the call decoded none -- after the hop it holds frame c_b - 1.  A row with c_b == 0 or q_b == 0 writes only its
 * -1s (those of `carry` included where i0 < c_b and q_b == 0, as the sampler does) and status 0 at i0 == 0.  A corrupt packet gives codes in [-1, size) and a nonzero status; with any packet and any table
 * no access leaves the operands.  Decoding a hop in one call is bit for bit decoding it in n calls of one frame.  One launch, one
 * wave per row; the search of a table is shared by the lanes (compare, then ballot). */
int agx_codes_rans_decode(const int32_t *cum, const uint8_t *packets, const int64_t *nbytes, const int32_t *sizes /* host, may be NULL */,
                          const int64_t *counts /* may be NULL */, const int64_t *stages /* may be NULL */, int64_t *state /* in/out */,
                          int64_t *codes, int64_t *carry /* may be NULL, in/out */, int64_t *status /* in/out */, int32_t batch,
                          int32_t hop, int32_t i0, int32_t n, int32_t n_q, int32_t k, int32_t p, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_H */
