// group_norm_relu.h -- what the fp32 unit (group_norm_relu.hip) and the bf16 unit (group_norm_relu_bf16.hip) share:
// the channel block of a workgroup, the supported (C, G) set and the dtype-free parameter-gradient reduction.
#pragma once
#include "common.h"

namespace shr {

constexpr int kGnBlockC = 32;    // channels per workgroup: whole groups for C/G in {4, 8, 16, 32}

bool gn_supported(int C, int G);   // group_norm_relu.hip

// dgamma / dbeta / dpre [C] = the per-sample partials [N][C] summed over the samples in a fixed order
// (group_norm_param_grad_kernel, group_norm_relu.hip; fp32 in, fp32 out: the same for either activation type)
void gn_launch_param_grad(const float *dgamma_partial, const float *dbeta_partial, const float *dpre_partial, int N, int C,
                          float *dgamma, float *dbeta, float *dpre, hipStream_t stream);

}  // namespace shr
