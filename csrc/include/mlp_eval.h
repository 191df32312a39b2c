// One-launch MLP evaluation (csrc/kernels/mlp_eval.hip): argument block and entry points.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mlp_train.h"

namespace pde {

// Forward of a Linear(+ReLU) stack, log-softmax, argmax, hit count and summed NLL in ONE ordinary launch
// (k_mlp_eval): a workgroup carries mlp_eval_rows_per_workgroup() batch rows through every layer with the
// activations in LDS; workgroups meet only at the arrival ticket of the totals.  Layer l: the bf16 weight copy
// w [out][in] (row-major, 16-byte aligned) and the fp32 bias.  2 <= nl <= kMlpMaxLayers; every in and every hidden
// out a multiple of 8 and at most 1024; the last out <= 16; B >= 1.  Every output is optional (nullptr):
//   pred [B] int64 (lowest index on a tie), logits / logp [B][last out] fp32,
//   stats: the four 8-byte words of CnnEvalStats {loss_sum as float64, correct, count, ticket} that the launch ADDS
//   the batch to -- per-workgroup partials in loss_part (ceil(B / rows per workgroup) floats), combined in workgroup
//   order by the last workgroup to arrive; the ticket must be 0 at launch and is left 0.  stats needs tgt and
//   loss_part.  Reads x [B][in_0] fp32 (16-byte aligned), writes nothing but its outputs.
struct MlpEvalLayer {
  const uint16_t* w;
  const float* b;
  int in, out;
};
struct MlpEvalArgs {
  MlpEvalLayer L[kMlpMaxLayers];
  int nl, B;
  const float* x;
  const int64_t* tgt;
  int64_t* pred;
  float *logits, *logp;
  void* stats;
  float* loss_part;
};
int mlp_eval_rows_per_workgroup();
hipError_t mlp_eval(const MlpEvalArgs& a, hipStream_t s);

}  // namespace pde
