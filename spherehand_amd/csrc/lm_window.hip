// lm_window.hip -- the two entries of the sliding-window tracker (include/spherehand_hip.h, the section of
// shr_pose_window_marginalize): the frame that leaves a window is folded into a Gaussian prior on the next two frames
// (shr_pose_window_marginalize), and that prior is a term of the window's normal equations (shr_pose_window_prior_normal).
//
// Inverts (reference file:line): nothing; the reference has no counterpart of the sequence solve or of its marginals.
//
//   marginalize   one workgroup of 256 threads per sequence, as lm_covariance.hip's chain kernel; only frames 0 ... min(T, 3) - 1
//                 of the sequence are read.  M_0 = A_0 + diag(mu) is factorised in place by lm_solve.h's column recurrence taken
//                 RIGHT-LOOKING; the 26 + 1 + 26 right-hand sides [E_0 | b_0 | F_0] stand side by side in ONE [26 x 53] block and
//                 go through lm_covariance.hip's row recurrence together, right-looking likewise; then the 1378 entries of the
//                 lower triangle of Lambda [52 x 52], the 52 of eta and the offset are dealt over the threads, each ONE chain
//                 from 0 over the 26 rows of X, subtracted once.  Every entry's bits are independent of its owner.
//   prior         one workgroup of 256 threads PER FRAME, as sphere_accel_kernel; frames 2 ... T - 1 and the frames of a sequence
//                 that is not active return at once.  d = trial - point of the two frames and Lambda d (one chain per row, the
//                 columns ascending) live in LDS; then one owner per entry of A's lower triangle, of g and of E, one add each.
//   Everything fp64, every sum in index order, nothing contracted, no atomics, no matrix-core instruction.
//   LDS: marginalize L [26 x 26], X [26 x 53] and the 26 stiffness terms of the cost, 16 640 bytes; prior d and Lambda d, 832.
#include "lm_solve.h"

namespace shr {

constexpr int kWmThreads = 256;
constexpr int kWmNN = kLmN * kLmN;                         // 676
constexpr int kWmP = 2 * kLmN;                             // the prior's unknowns: two frames
constexpr int kWmTri = kWmP * (kWmP + 1) / 2;              // 1378
constexpr int kWmColB = kLmN, kWmColF = kLmN + 1, kWmCols = 2 * kLmN + 1;      // X = [X_E | y | X_F]

struct WmLds {
  double L[kWmNN];
  double X[kLmN * kWmCols];
  double sq[kLmN];                                         // mu (p_0 - prior_0)^2 per parameter
};

// sum_k X[k][a] X[k][b], a chain from 0, k ascending, all 26 terms
__device__ __forceinline__ double wm_dot(const double *X, int a, int b) {
  double c = 0.0;
#pragma unroll 2
  for (int k = 0; k < kLmN; k++) c += X[k * kWmCols + a] * X[k * kWmCols + b];
  return c;
}

__global__ void __launch_bounds__(kWmThreads)
pose_window_marginalize_kernel(const double *__restrict__ A, const double *__restrict__ g, const double *__restrict__ E,
                               const double *__restrict__ F, const double *__restrict__ cost_data,
                               const float *__restrict__ trial, const float *__restrict__ prior,
                               const float *__restrict__ stiffness, int T, double *__restrict__ Lambda, double *__restrict__ eta,
                               double *__restrict__ offset, float *__restrict__ point, int32_t *__restrict__ status) {
  __shared__ WmLds s;
  const int q = blockIdx.x, tid = threadIdx.x;
  const size_t first = (size_t)q * T;
  const bool band1 = E != nullptr && T >= 2;               // frame 1 exists and is coupled to frame 0
  const bool two = band1 && T >= 3;                        // frame 2 exists
  const bool band2 = two && F != nullptr;
  const int nc = band2 ? kWmCols : kWmColF;                // the columns of X that are formed
  double *Lq = Lambda + (size_t)q * kWmP * kWmP, *eq = eta + (size_t)q * kWmP;
  // the linearisation point: the trial poses of frames 1 and 2, +0 where the frame does not exist
  for (int e = tid; e < kWmP; e += kWmThreads) {
    const int t = 1 + e / kLmN;
    point[(size_t)q * kWmP + e] = t < T ? trial[(first + t) * kLmN + e % kLmN] : 0.f;
  }
  // M_0's lower triangle, the upper one 0; X := [E_0 | b_0 | F_0]
  for (int e = tid; e < kWmNN; e += kWmThreads) {
    const int i = e / kLmN, k = e % kLmN;
    double v = 0.0;
    if (i >= k) {
      v = A[first * kWmNN + e];
      if (i == k && stiffness) v += (double)stiffness[i];
    }
    s.L[e] = v;
    s.X[i * kWmCols + k] = band1 ? E[first * kWmNN + e] : 0.0;
    if (band2) s.X[i * kWmCols + kWmColF + k] = F[first * kWmNN + e];
  }
  if (tid < kLmN) {
    const double mu = stiffness ? (double)stiffness[tid] : 0.0;
    const double d = prior ? (double)trial[first * kLmN + tid] - (double)prior[first * kLmN + tid] : 0.0;
    s.X[tid * kWmCols + kWmColB] = g[first * kLmN + tid] + mu * d;
    s.sq[tid] = mu * (d * d);
  }
  __syncthreads();
  // L L^T = M_0 in place, right-looking
  bool ok = true;
#pragma unroll 1
  for (int k = 0; k < kLmN; k++) {
    const double d = s.L[k * kLmN + k];
    if (!(d > 0.0 && d < __builtin_inf())) {
      ok = false;
      break;
    }
    const double root = sqrt(d);
    __syncthreads();                                       // every thread has read the pivot
    if (tid >= k && tid < kLmN) s.L[tid * kLmN + k] = tid == k ? root : s.L[tid * kLmN + k] / root;
    __syncthreads();
    for (int e = tid; e < (kLmN - 1 - k) * kLmN; e += kWmThreads) {
      const int i = k + 1 + e / kLmN, j = e % kLmN;
      if (j > k && j <= i) s.L[i * kLmN + j] -= s.L[i * kLmN + k] * s.L[j * kLmN + k];
    }
    __syncthreads();
  }
  if (tid == 0) status[q] = ok ? 0 : 1;
  if (!ok) {                                               // the information is dropped: an exact +0 record
    for (int e = tid; e < kWmP * kWmP; e += kWmThreads) Lq[e] = 0.0;
    if (tid < kWmP) eq[tid] = 0.0;
    if (tid == 0) offset[q] = 0.0;
    return;
  }
  // X := L^-1 X row by row: X[k][:] = (X[k][:] - sum_{m<k} L[k][m] X[m][:]) / L[k][k], m ascending
#pragma unroll 1
  for (int k = 0; k < kLmN; k++) {
    if (tid < nc) s.X[k * kWmCols + tid] = s.X[k * kWmCols + tid] / s.L[k * kLmN + k];
    __syncthreads();
    for (int e = tid; e < (kLmN - 1 - k) * nc; e += kWmThreads) {
      const int i = k + 1 + e / nc, j = e % nc;
      s.X[i * kWmCols + j] -= s.L[i * kLmN + k] * s.X[k * kWmCols + j];
    }
    __syncthreads();
  }
  const double *A1 = A + (first + 1) * kWmNN, *A2 = A + (first + 2) * kWmNN;       // (read only where the frame exists)
  for (int e = tid; e < kWmTri + kWmP + 1; e += kWmThreads) {
    if (e < kWmTri) {                                      // Lambda's lower triangle, mirrored
      int r = 0;
      while ((r + 1) * (r + 2) / 2 <= e) r++;
      const int c = e - r * (r + 1) / 2;                   // r >= c
      double v = 0.0;
      if (r < kLmN) {
        if (band1) v = A1[r * kLmN + c] - wm_dot(s.X, r, c);
      } else if (two && c < kLmN) {                        // Lambda_12[c][r - 26]: frame 1's rows, frame 2's columns
        v = E[(first + 1) * kWmNN + c * kLmN + (r - kLmN)];
        if (band2) v = v - wm_dot(s.X, c, kWmColF + r - kLmN);
      } else if (two) {
        v = A2[(r - kLmN) * kLmN + (c - kLmN)];
        if (band2) v = v - wm_dot(s.X, kWmColF + r - kLmN, kWmColF + c - kLmN);
      }
      Lq[r * kWmP + c] = v;
      Lq[c * kWmP + r] = v;
    } else if (e < kWmTri + kWmP) {
      const int i = e - kWmTri;
      double v = 0.0;
      if (i < kLmN) {
        if (band1) v = g[(first + 1) * kLmN + i] - wm_dot(s.X, i, kWmColB);
      } else if (two) {
        v = g[(first + 2) * kLmN + i - kLmN];
        if (band2) v = v - wm_dot(s.X, kWmColF + i - kLmN, kWmColB);
      }
      eq[i] = v;
    } else {                                               // ((cost_0 + sum mu d^2) + cost_1 + cost_2) - y.y
      double c = cost_data[first];
#pragma unroll 1
      for (int i = 0; i < kLmN; i++) c += s.sq[i];
      if (T >= 2) c = c + cost_data[first + 1];
      if (T >= 3) c = c + cost_data[first + 2];
      offset[q] = c - wm_dot(s.X, kWmColB, kWmColB);
    }
  }
}

struct WpLds {
  double d[kWmP];
  double ld[kWmP];
};

__global__ void __launch_bounds__(kWmThreads)
pose_window_prior_kernel(const float *__restrict__ trial, const double *__restrict__ Lambda, const double *__restrict__ eta,
                         const double *__restrict__ offset, const float *__restrict__ point, const int32_t *__restrict__ active,
                         int T, int add, int add_E, double *__restrict__ A, double *__restrict__ g, double *__restrict__ E,
                         double *__restrict__ cost) {
  __shared__ WpLds s;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int t = b % T, q = b / T;
  if (t >= 2) return;                                      // the prior is on the first two frames
  if (active && active[q] == 0) return;                    // a sequence without a prior: left alone
  const int n = T == 1 ? kLmN : kWmP;
  const size_t first = (size_t)q * T;
  const double *Lq = Lambda + (size_t)q * kWmP * kWmP, *eq = eta + (size_t)q * kWmP;
  if (tid < n) s.d[tid] = (double)trial[first * kLmN + tid] - (double)point[(size_t)q * kWmP + tid];
  __syncthreads();
  if (tid < n) {
    double c = 0.0;
#pragma unroll 2
    for (int j = 0; j < n; j++) c += Lq[tid * kWmP + j] * s.d[j];
    s.ld[tid] = c;
  }
  __syncthreads();
  const int o = t * kLmN;
  constexpr int kTri = kLmN * (kLmN + 1) / 2;              // 351
  for (int idx = tid; idx < kTri + kLmN; idx += kWmThreads) {
    if (idx < kTri) {
      int r = 0;
      while ((r + 1) * (r + 2) / 2 <= idx) r++;
      const int c = idx - r * (r + 1) / 2;                 // r >= c
      const double mine = Lq[(o + r) * kWmP + o + c];
      double *low = A + ((size_t)b * kLmN + r) * kLmN + c;
      const double v = add ? *low + mine : mine;
      *low = v;
      A[((size_t)b * kLmN + c) * kLmN + r] = v;
    } else {
      const int r = idx - kTri;
      const double mine = s.ld[o + r] + eq[o + r];
      double *out = g + (size_t)b * kLmN + r;
      *out = add ? *out + mine : mine;
    }
  }
  if (t == 0 && T >= 2) {                                  // Lambda_01: frame 0's rows, frame 1's columns
    for (int idx = tid; idx < kWmNN; idx += kWmThreads) {
      const int r = idx / kLmN, c = idx - r * kLmN;
      const double mine = Lq[r * kWmP + kLmN + c];
      double *out = E + (size_t)b * kWmNN + idx;
      *out = add_E ? *out + mine : mine;
    }
  }
  if (tid == kWmThreads - 1) {                             // the term's cost belongs to the sequence's first frame
    if (t == 0) {
      double quad = 0.0, lin = 0.0;
#pragma unroll 1
      for (int i = 0; i < n; i++) quad += s.d[i] * s.ld[i];
#pragma unroll 1
      for (int i = 0; i < n; i++) lin += eq[i] * s.d[i];
      const double c = (quad + 2.0 * lin) + offset[q];
      cost[b] = add ? cost[b] + c : c;
    } else if (!add) {
      cost[b] = 0.0;
    }
  }
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_pose_window_marginalize_workspace_bytes(int B, int T) {
  if (B < 0 || T < 0) return -1;
  return 0;
}

extern "C" int shr_pose_window_marginalize(const double *A, const double *g, const double *E, const double *F,
                                           const double *cost_data, const float *trial, const float *prior,
                                           const float *stiffness, int B, int T, double *Lambda, double *eta, double *offset,
                                           float *point, int32_t *status, void *workspace, void *stream) {
  if (B < 0 || T < 1 || B % T != 0) return SHR_EINVAL;
  if (B > 65535) return SHR_ETOOLARGE;
  if (B == 0) return SHR_OK;
  if (!A || !g || !cost_data || !trial || !Lambda || !eta || !offset || !point || !status) return SHR_EINVAL;
  if ((((uintptr_t)A | (uintptr_t)g | (uintptr_t)E | (uintptr_t)F | (uintptr_t)cost_data | (uintptr_t)Lambda | (uintptr_t)eta |
        (uintptr_t)offset) & 7u) != 0)
    return SHR_EINVAL;
  if ((((uintptr_t)trial | (uintptr_t)prior | (uintptr_t)stiffness | (uintptr_t)point | (uintptr_t)status |
        (uintptr_t)workspace) & 3u) != 0)
    return SHR_EINVAL;
  hipLaunchKernelGGL(pose_window_marginalize_kernel, dim3((unsigned)(B / T)), dim3(kWmThreads), 0, (hipStream_t)stream, A, g, E,
                     F, cost_data, trial, prior, stiffness, T, Lambda, eta, offset, point, status);
  return (int)hipGetLastError();
}

extern "C" long long shr_pose_window_prior_normal_workspace_bytes(int B, int T) {
  if (B < 0 || T < 0) return -1;
  return 0;
}

extern "C" int shr_pose_window_prior_normal(const float *trial, const double *Lambda, const double *eta, const double *offset,
                                            const float *point, const int32_t *active, int B, int T, int accumulate,
                                            int accumulate_E, double *A, double *g, double *E, double *cost, void *workspace,
                                            void *stream) {
  if (B < 0 || T < 1 || B % T != 0 || (accumulate != 0 && accumulate != 1)) return SHR_EINVAL;
  if (accumulate_E != 0 && accumulate_E != 1) return SHR_EINVAL;
  if (B > 65535) return SHR_ETOOLARGE;
  if (B == 0) return SHR_OK;
  if (!trial || !Lambda || !eta || !offset || !point || !A || !g || !cost || (!E && T > 1)) return SHR_EINVAL;
  if ((((uintptr_t)Lambda | (uintptr_t)eta | (uintptr_t)offset | (uintptr_t)A | (uintptr_t)g | (uintptr_t)E | (uintptr_t)cost) &
       7u) != 0)
    return SHR_EINVAL;
  if ((((uintptr_t)trial | (uintptr_t)point | (uintptr_t)active | (uintptr_t)workspace) & 3u) != 0) return SHR_EINVAL;
  hipLaunchKernelGGL(pose_window_prior_kernel, dim3((unsigned)B), dim3(kWmThreads), 0, (hipStream_t)stream, trial, Lambda, eta,
                     offset, point, active, T, accumulate, accumulate_E, A, g, E, cost);
  return (int)hipGetLastError();
}
