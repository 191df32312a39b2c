// Global-norm gradient clipping: what k_grad_clip (optim_clip.hip) and k_cnn_opt_clip (cnn_fused.hip) share, so
// both derive the coefficient with the same operations.
#pragma once
#include "common.cuh"
#include "pde_kernels.h"

namespace pde {
namespace clipdev {

// min(1, max_norm / (total + 1e-6)) as torch.clamp(max=1) takes it: a NaN stays a NaN (error_if_nonfinite=False),
// an infinite total gives 0.
__device__ __forceinline__ float clip_coef(float total, float max_norm) {
  const float c = __fdiv_rn(max_norm, __fadd_rn(total, 1e-6f));
  return c > 1.f ? 1.f : c;
}

// Four waves' partial sums (one per wave, already butterfly-reduced) through LDS, summed in wave order; every thread
// returns the same bits.  One barrier; `part` must not be rewritten before the caller's next barrier.
__device__ __forceinline__ float block_sum4(float wave_total, float* part) {
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = wave_total;
  __syncthreads();
  return __fadd_rn(__fadd_rn(__fadd_rn(part[0], part[1]), part[2]), part[3]);
}

}  // namespace clipdev
}  // namespace pde
