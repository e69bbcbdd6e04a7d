// lm_solve.h -- the 26 x 26 damped solve of the Levenberg-Marquardt loops (pose_ik.hip: keypoints -> pose; pose_icp.hip:
// the step of the mesh fit), by ONE wave in fp64: the Cholesky factor column by column, lane i owning row i, then the
// forward and backward substitutions, one unknown per step.  Every sum in index order: the same bits wherever it runs.
// S: the wave's LDS, with double A[26 * 26] (lower triangle read), L[26 * 26], x[26] and piv.
#pragma once
#include "common.h"

namespace shr {

constexpr int kLmN = 26;             // pose parameters

// L L^T = A + lam diag(A), column by column, lane i owning row i.  false: a pivot that is not positive and finite.
template <class S>
__device__ __forceinline__ bool lm_cholesky(S &s, double lam, int lane) {
#pragma unroll 1
  for (int k = 0; k < kLmN; k++) {
    double v = 0.0;
    if (lane >= k && lane < kLmN) {
      v = s.A[lane * kLmN + k];
      if (lane == k) v += lam * v;
#pragma unroll 2
      for (int m = 0; m < k; m++) v -= s.L[lane * kLmN + m] * s.L[k * kLmN + m];
      if (lane == k) s.piv = v;
    }
    __syncthreads();
    const double d = s.piv;
    if (!(d > 0.0 && d < __builtin_inf())) return false;
    const double root = sqrt(d);
    if (lane >= k && lane < kLmN) s.L[lane * kLmN + k] = lane == k ? root : v / root;
    __syncthreads();
  }
  return true;
}

// s.x = (L L^T)^-1 rhs (lane i < 26 brings rhs_i): forward then backward substitution, one unknown per step
template <class S>
__device__ __forceinline__ void lm_solve(S &s, double rhs, int lane) {
  double acc = 0.0;
#pragma unroll 1
  for (int k = 0; k < kLmN; k++) {
    if (lane == k) s.x[k] = (rhs - acc) / s.L[k * kLmN + k];
    __syncthreads();
    if (lane > k && lane < kLmN) acc += s.L[lane * kLmN + k] * s.x[k];
  }
  const double z = lane < kLmN ? s.x[lane] : 0.0;
  acc = 0.0;
  __syncthreads();
#pragma unroll 1
  for (int k = kLmN - 1; k >= 0; k--) {
    if (lane == k) s.x[k] = (z - acc) / s.L[k * kLmN + k];
    __syncthreads();
    if (lane < k) acc += s.L[k * kLmN + lane] * s.x[k];
  }
  __syncthreads();
}

}  // namespace shr
