// Host functions one convolution / weight-gradient file calls in another.  Each is declared here and nowhere else, and the file that
// defines one includes this header, so a changed signature is a compile error instead of a wrong link.
#pragma once
#include "common.h"

namespace rd {

// conv16.hip: the 16 -> 16 channel 3x3 / stride-1 convolutions on the 16x16x4 fp32 MFMA (dispatched from gconv.hip's plans)
bool conv16_eligible(const RdConvDesc& d);
int conv16_tiles_per_image(const RdConvDesc& d);
int launch_conv16(const RdConvDesc& d, const float* in, const float* w_packed, float* out, const float* addend, int ld_add,
                  float* stat, hipStream_t s);
// wgrad16.hip: the weight gradient of the same layers (slabs in wgrad.hip's layout)
bool wgrad16_eligible(const RdConvDesc& d);
void wgrad16_splits(const RdConvDesc& d, int& total_tiles, int& n_splits);
int launch_wgrad16(const RdConvDesc& d, const float* x, const float* dout, float* slabs, hipStream_t s);
// wgrad1x1.hip: the weight gradient of the 1x1 convolutions (>= 64 channels each side) as a pixel-reduction GEMM
bool wgrad1x1_eligible(const RdConvDesc& d);
void wgrad1x1_splits(const RdConvDesc& d, int& n_splits, long long& pix_per_split);
int launch_wgrad1x1(const RdConvDesc& d, const float* x, const float* dout, float* slabs, hipStream_t s);
// stem16.hip: forward of the 16-channel depth stem on the 16x16x4 MFMA (dispatched from stem.hip's rd_stem_fwd[_t])
bool stem16_eligible(int Cin, int Cout);
int launch_stem16_fwd(int io16, const float* const* planes, const int64_t* strides, int Cin, int N, int H, int W, const float* w_packed, int Cout,
                      void* out, float* stat_partial, hipStream_t s);

// gconv_bf16p.hip: the persistent bf16-storage convolution (dispatched from rd_gconv_bf16_t for the descriptors it serves)
int gconv_bf16p_supported(const RdConvDesc* d);
int gconv_bf16p_plan_all(int on);
int gconv_bf16p_stat_tiles(const RdConvDesc* d);
int gconv_bf16p_plan_info(const RdConvDesc* d, int32_t* out);
int launch_gconv_bf16p(const RdConvDesc* d, const void* in, const void* w_packed_bf16, void* out, const float* bias, int32_t act, int32_t act_cols,
                       const void* addend, int32_t ld_add, float* stat_partial, hipStream_t s);

// gemm1_split.hip: one-tap descriptors of rd_gconv_split
int gemm1_split_supported(const RdConvDesc* d);
int gemm1_split_stat_tiles(const RdConvDesc* d);
int gemm1_split_plan_info(const RdConvDesc* d, int32_t* out);
int launch_gemm1_split(const RdConvDesc* d, const float* in, const void* w_split, int64_t piece_elems, float* out, const float* bias, int32_t act,
                       int32_t act_cols, const float* addend, int32_t ld_add, float* stat_partial, hipStream_t s);

// wgrad.hip: stage 1 (once per slab set, when co_off == 0) + stage 2 of the slab reduction into an OIHW gradient
int launch_slab_reduce(const float* slabs, int n_splits, int64_t E, float* tmp, float* grad_oihw, int S, int Cin, int Cout,
                       int O, int I, int co_off, int accumulate, hipStream_t s);
// wgrad_bf16.hip: shape of a descriptor's slab reduction (rd_wgrad_reduce_job, wgrad.hip)
bool wgrad_bf16_reduce_shape(const RdConvDesc* d, int* slab_splits, int* S);
// norm_act.hip: the BatchNorm-backward coefficient kernel without the apply pass (rd_stem_wgrad_split_bn_t)
int launch_bn_bwd_coeffs(const float* red_partial, int n_tiles, int C, int which, double count, const float* gamma, const float* invstd,
                         float* dgamma, float* dbeta, float* coef_ws, hipStream_t s);

}  // namespace rd
