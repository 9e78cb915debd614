// Entry points of the convolution kernel families: can THIS plan run on it (`*_supported`), the instantiation it would run on
// (`*_variant`, the template arguments of the rocprofv3 kernel name) and the launch.  Each C-ABI op picks a family in one selection
// function (conv_api.hip: conv_kernel / resblock_kernel, conv2d.hip: conv2d_kernel / conv2d_bwd_kernel) its launcher and name query share.
#pragma once
#include "common.hpp"

namespace agx {
// conv_direct.hip: fp32 VALU, any plan (grouped layers, few rows, narrow maps)
const char *conv_direct_variant(const ConvPlan &p);
int launch_conv_direct(const ConvPlan &p, const float *x, const float *wp, const float *bias, const float *res, float *y, hipStream_t st);
// conv_mfma.hip: MFMA implicit GEMM on staged tiles (fp32 or bf16x3 by p.prec; 1-D, row-folded and patch-mode 2-D plans)
bool conv_mfma_supported(const ConvPlan &p);
const char *conv_mfma_variant(const ConvPlan &p);
int launch_conv_mfma(const ConvPlan &p, const float *x, const float *wp, const float *bias, const float *res, float *y, hipStream_t st);
// conv_p.hip: persistent fp32 ring kernels on the tile image, 1-D and patch-mode Conv2d plans
bool conv_p_supported(const ConvPlan &p);
const char *conv_p_variant(const ConvPlan &p);
int launch_conv_p(const ConvPlan &p, const float *x, const float *wp, const float *bias, const float *res, float *y, hipStream_t st);
bool conv_p2d_supported(const ConvPlan &p);
const char *conv_p2d_variant(const ConvPlan &p);
int launch_conv_p2d(const ConvPlan &p, const float *x, const float *wp, const float *bias, const float *res, float *y, hipStream_t st);
// conv_b3.hip: bf16x3 ring kernels on the B3 tile image (fp32 input, or pre-split activation planes), 1-D and Conv2d
bool conv_b3_supported(const ConvPlan &p);
const char *conv_b3_variant(const ConvPlan &p);
int launch_conv_b3(const ConvPlan &p, const float *x, const float *wp, const float *bias, float *y, hipStream_t st);
int conv_b3_planes(const ConvPlan &p);   // 0: fp32 input only, 1: the kernel can read activation planes, 2: and write them
int launch_conv_b3_planes(const ConvPlan &p, const void *x_planes, const float *wp, const float *bias, float *y, void *y_planes, hipStream_t st);
int launch_planes_split(const float *x, void *planes, int batch, int channels, int length, hipStream_t st);
bool conv2d_b3_supported(const ConvPlan &p);
const char *conv2d_b3_variant(const ConvPlan &p);
int launch_conv2d_b3(const ConvPlan &p, const float *x, const float *wp, const float *bias, const float *res, float *y, hipStream_t st);
// the residual block in one kernel: resblock_p.hip (fp32 ring), resblock_b3.hip (bf16x3 ring), resblock_mfma.hip (staged tiles)
bool resblock_p_supported(const ConvPlan &p);
const char *resblock_p_variant(const ConvPlan &p);
int launch_resblock_p(const ConvPlan &p, const float *x, const float *w1, const float *b1, const float *w2, const float *b2, float *y, int post_act, hipStream_t st);
// ... with x and / or y in channel quads (include/agx.h): knob rb_q4, resblock_p_supported and the row's flag
bool resblock_p_quads(const ConvPlan &p);
int launch_resblock_p_quads(const ConvPlan &p, const float *x, const float *w1, const float *b1, const float *w2, const float *b2, float *y, int post_act,
                            bool x_quads, bool y_quads, hipStream_t st);
bool resblock_b3_supported(const ConvPlan &p);
const char *resblock_b3_variant(const ConvPlan &p);
int launch_resblock_b3(const ConvPlan &p, const float *x, const float *w1, const float *b1, const float *w2, const float *b2, float *y, int post_act, hipStream_t st);
bool resblock_fused_supported(const ConvPlan &p);
const char *resblock_variant(const ConvPlan &p);
int launch_resblock_fused(const ConvPlan &p, const float *x, const float *w1, const float *b1, const float *w2, const float *b2, float *y, int post_act, hipStream_t st);

}  // namespace agx
