// lm_solve.h -- the 26 x 26 damped solve of the Levenberg-Marquardt loops (pose_ik.hip: keypoints -> pose; pose_icp.hip:
// the step of the mesh fit; lm_band.h and lm_shared.hip: the block steps), by ONE wave in fp64: the Cholesky factor column
// by column, lane i owning row i, then the forward and backward substitutions, one unknown per step.  Every sum in index
// order: the same bits wherever it runs.
// S: the wave's LDS, with double A[26 * 26] (lower triangle read), L[26 * 26], x[26] and piv.
#pragma once
#include "normal_eq.h"

namespace shr {

constexpr int kLmN = kNeqN;          // pose parameters (normal_eq.h)

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

// s.x = L^-1 rhs (lane i < 26 brings rhs_i): forward substitution, one unknown per step
template <class S>
__device__ __forceinline__ void lm_forward(S &s, double rhs, int lane) {
  double acc = 0.0;
#pragma unroll 1
  for (int k = 0; k < kLmN; k++) {
    if (lane == k) s.x[k] = (rhs - acc) / s.L[k * kLmN + k];
    __syncthreads();
    if (lane > k && lane < kLmN) acc += s.L[lane * kLmN + k] * s.x[k];
  }
}

// s.x = L^-T z (lane i < 26 brings z_i, read from s.x BEFORE a barrier where it is lm_forward's): backward substitution
template <class S>
__device__ __forceinline__ void lm_backward(S &s, double z, int lane) {
  double acc = 0.0;
#pragma unroll 1
  for (int k = kLmN - 1; k >= 0; k--) {
    if (lane == k) s.x[k] = (z - acc) / s.L[k * kLmN + k];
    __syncthreads();
    if (lane < k) acc += s.L[k * kLmN + lane] * s.x[k];
  }
}

// s.x = (L L^T)^-1 rhs (lane i < 26 brings rhs_i): the two in a row
template <class S>
__device__ __forceinline__ void lm_solve(S &s, double rhs, int lane) {
  lm_forward(s, rhs, lane);
  const double z = lane < kLmN ? s.x[lane] : 0.0;
  __syncthreads();
  lm_backward(s, z, lane);
  __syncthreads();
}

// Triangular solves side by side: column `lane` of X (X[m * ld + lane], m = 0 ... 25) := the solution z of L z = that
// column, in place, m ascending.  A lane touches its own column only: no barrier between the 26 steps.
template <class S>
__device__ __forceinline__ void lm_columns(const S &s, double *X, int ld, int lane) {
#pragma unroll 1
  for (int m = 0; m < kLmN; m++) {
    double v = X[m * ld + lane];
#pragma unroll 2
    for (int j = 0; j < m; j++) v -= s.L[m * kLmN + j] * X[j * ld + lane];
    X[m * ld + lane] = v / s.L[m * kLmN + m];
  }
}

}  // namespace shr
