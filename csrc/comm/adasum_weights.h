// Adasum as a linear combination (hvd.Adasum; Maleki et al., "Scaling Distributed Training with Adaptive
// Summation").  Two gradients combine as
//     adasum(a, b) = (1 - a.b / (2 |a|^2)) a + (1 - a.b / (2 |b|^2)) b
// and N = 2^k ranks as the tree over contiguous halves, A(lo, hi) = adasum(A(lo, mid), A(mid, hi)) -- Horovod's
// distance-doubling pairs (0,1), (2,3), then (01, 23), ...  Every tree node is a linear combination of the N rank
// vectors, so every dot product and norm of the tree follows from the Gram matrix G[i][j] = x_i . x_j, and the
// whole tree collapses to N weights: adasum(x_0 .. x_{N-1}) = sum_r w_r x_r.  One function for the host (the
// binding the tests compare against hvd/adasum.py) and the device (k_xgmi_adasum_combine).
#pragma once

#include <hip/hip_runtime.h>

namespace pde {

// a coefficient is 1 when its vector's squared norm is below this (a zero gradient passes the other one through)
constexpr double kAdasumEps = 1e-8;

// G: N x N row-major Gram matrix (symmetric); w: N weights out.  N a power of two.
__host__ __device__ inline void adasum_weights(const double* G, int N, double* w) {
  for (int r = 0; r < N; ++r) w[r] = 1.0;
  for (int span = 1; span < N; span *= 2) {
    for (int lo = 0; lo < N; lo += 2 * span) {
      const int mid = lo + span, hi = mid + span;
      double na = 0.0, nb = 0.0, dot = 0.0;
      for (int i = lo; i < mid; ++i)
        for (int j = lo; j < mid; ++j) na += w[i] * w[j] * G[i * N + j];
      for (int i = mid; i < hi; ++i)
        for (int j = mid; j < hi; ++j) nb += w[i] * w[j] * G[i * N + j];
      for (int i = lo; i < mid; ++i)
        for (int j = mid; j < hi; ++j) dot += w[i] * w[j] * G[i * N + j];
      const double ca = na < kAdasumEps ? 1.0 : 1.0 - dot / (2.0 * na);
      const double cb = nb < kAdasumEps ? 1.0 : 1.0 - dot / (2.0 * nb);
      for (int i = lo; i < mid; ++i) w[i] *= ca;
      for (int i = mid; i < hi; ++i) w[i] *= cb;
    }
  }
}

}  // namespace pde
