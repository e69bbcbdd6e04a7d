// lm_covariance.hip -- the marginal covariances of the sequence fit (shr_pose_lm_seq2_covariance): the diagonal blocks
// Z_tt of the inverse of the UNDAMPED block-pentadiagonal matrix that shr_pose_lm_seq2_step factorises (lm_seq2.hip), and
// their projection onto the spheres, C_j(t) = Jc_j(t) Z_tt Jc_j(t)^T.
//
// Inverts (reference file:line): nothing; the reference has no counterpart of the solve or of its covariance.
//
//   chain     one workgroup of 256 threads per sequence; the frames are taken one after the other, forward and then back,
//             so a sequence is a latency chain of 2 T frames.  Every output entry is ONE fixed-order fp64 chain, so its
//             bits do not depend on the thread that owns it: the 676 entries of a block are dealt over the 256 threads.
//   forward   lm_band.h's factorisation at lambda = 0, the same operations per entry in the same order:
//             D_t = M_t - W_{t-1} W_{t-1}^T - V_{t-2} V_{t-2}^T, M_t = A_t + diag(mu), per entry the W product subtracted
//             first, then the V product, each m ascending; L_t L_t^T = D_t by lm_solve.h's column recurrence, taken
//             RIGHT-LOOKING (column m is subtracted from every later column as soon as it is finished: per entry the same
//             subtractions, m ascending); W_t = (E_t^T - V_{t-1} W_{t-1}^T) L_t^-T, V_t = F_t^T L_t^-T and N_t = L_t^-1
//             by the row recurrence of lm_solve.h's lm_columns, the three side by side and right-looking likewise.
//             N_t, W_t and V_t go to the workspace.
//   back      backward over t, with P_t = W_t N_t and Q_t = V_t N_t (chains from 0, k ascending):
//             Z_{t+1,t} = (-(Z_{t+1,t+1} P_t)) - Z_{t+2,t+1}^T Q_t;  Z_{t+2,t} = (-(Z_{t+2,t+1} P_t)) - Z_{t+2,t+2} Q_t;
//             Z_tt = (N_t^T N_t - P_t^T Z_{t+1,t}) - Q_t^T Z_{t+2,t}, the lower triangle computed and mirrored.
//   project   a second launch, one workgroup per frame: per sphere and entry (a, b), a <= b,
//             sum_k (sum_m Jc[a][m] Z[m][k]) Jc[b][k], k and m ascending.
//   Everything fp64, every sum in index order, the W (P) term before the V (Q) term, nothing contracted, no atomics.
//   LDS: nine blocks [26 x 26] -- forward D/L, N, the two W and three V; backward N, P, Q, the three kept Z blocks and the
//   three being formed, W_t and V_t staged where Z_{t+1,t} and Z_{t+2,t} are formed afterwards -- 48 672 bytes.  W and V are
//   held TRANSPOSED (W[k * 26 + i] = W_t[i][k]) as in lm_band.h, so that a wave reads consecutive doubles.
#include "lm_solve.h"

namespace shr {

constexpr int kCvNN = kLmN * kLmN, kCvThreads = 256;
// The workspace: B x kCvWs doubles (N_t [26 x 26], W_t transposed, V_t transposed, each padded to a multiple of 8).
constexpr int kCvWsN = 0, kCvWsW = 680, kCvWsV = 1360, kCvWs = 2040;
static_assert(kCvNN <= kCvWsW && kCvWsW % 8 == 0 && kCvWs == 3 * kCvWsW, "the workspace's fields");

struct CvLds {
  double blk[9][kCvNN];
};

// X (and Y, unless it is null) := the solution of L X = X row by row, in place: lm_columns' recurrence for every column at
// once, right-looking.  X[k][:] = (X[k][:] - sum_{m<k} L[k][m] X[m][:]) / L[k][k], m ascending.  With Z the same for Z.
__device__ __forceinline__ void cv_rows(const double *L, double *X, double *Y, double *Z, int tid) {
  const int which = tid >> 6, col = tid & 63;              // wave 0: X, wave 1: Y, wave 2: Z
  double *mine = which == 0 ? X : which == 1 ? Y : which == 2 ? Z : nullptr;
#pragma unroll 1
  for (int k = 0; k < kLmN; k++) {
    if (mine && col < kLmN) mine[k * kLmN + col] = mine[k * kLmN + col] / L[k * kLmN + k];
    __syncthreads();
    for (int e = tid; e < (kLmN - 1 - k) * kLmN; e += kCvThreads) {
      const int i = k + 1 + e / kLmN, j = e % kLmN;
      const double l = L[i * kLmN + k];
      X[i * kLmN + j] -= l * X[k * kLmN + j];
      if (Y) Y[i * kLmN + j] -= l * Y[k * kLmN + j];
      if (Z) Z[i * kLmN + j] -= l * Z[k * kLmN + j];
    }
    __syncthreads();
  }
}

// out[i][j] = sum_k (ta ? a[k][i] : a[i][k]) b[k][j], a chain from 0, k ascending
__device__ __forceinline__ double cv_dot(const double *a, bool ta, const double *b, int i, int j) {
  double c = 0.0;
  if (ta) {
#pragma unroll 2
    for (int k = 0; k < kLmN; k++) c += a[k * kLmN + i] * b[k * kLmN + j];
  } else {
#pragma unroll 2
    for (int k = 0; k < kLmN; k++) c += a[i * kLmN + k] * b[k * kLmN + j];
  }
  return c;
}

__global__ void __launch_bounds__(kCvThreads)
pose_lm_seq2_covariance_chain_kernel(const double *__restrict__ A, const double *__restrict__ E, const double *__restrict__ F,
                                     const float *__restrict__ stiffness, int T, double *__restrict__ cov,
                                     int32_t *__restrict__ status, double *__restrict__ ws) {
  __shared__ CvLds s;
  const int q = blockIdx.x, tid = threadIdx.x;
  const size_t first = (size_t)q * T;
  const bool band1 = E != nullptr, band2 = band1 && F != nullptr;
  // forward: D (L in place), N, W_{t-1} and the W being formed, V_{t-1}, V_{t-2} and the V being formed
  double *D = s.blk[0], *N = s.blk[1], *Wp = s.blk[2], *Wn = s.blk[3], *V1 = s.blk[4], *V2 = s.blk[5], *Vn = s.blk[6];
  int bad = -1;
#pragma unroll 1
  for (int t = 0; t < T; t++) {
    const size_t f = first + t;
    const bool prev = band1 && t > 0, far = band2 && t > 1;
    const bool hasW = band1 && t < T - 1, hasV = band2 && t < T - 2;
    // D_t's lower triangle, the upper one 0; N := I
    for (int e = tid; e < kCvNN; e += kCvThreads) {
      const int i = e / kLmN, k = e % kLmN;
      double v = 0.0;
      if (i >= k) {
        v = A[f * kCvNN + e];
        if (i == k && stiffness) v += (double)stiffness[i];
        if (prev) {
#pragma unroll 2
          for (int m = 0; m < kLmN; m++) v -= Wp[m * kLmN + i] * Wp[m * kLmN + k];
        }
        if (far) {
#pragma unroll 2
          for (int m = 0; m < kLmN; m++) v -= V2[m * kLmN + i] * V2[m * kLmN + k];
        }
      }
      D[e] = v;
      N[e] = i == k ? 1.0 : 0.0;
    }
    __syncthreads();
    // L_t L_t^T = D_t in place, right-looking
    bool ok = true;
#pragma unroll 1
    for (int k = 0; k < kLmN; k++) {
      const double d = D[k * kLmN + k];
      if (!(d > 0.0 && d < __builtin_inf())) {
        ok = false;
        break;
      }
      const double root = sqrt(d);
      __syncthreads();                                     // every thread has read the pivot
      if (tid >= k && tid < kLmN) D[tid * kLmN + k] = tid == k ? root : D[tid * kLmN + k] / root;
      __syncthreads();
      for (int e = tid; e < (kLmN - 1 - k) * kLmN; e += kCvThreads) {
        const int i = k + 1 + e / kLmN, j = e % kLmN;
        if (j > k && j <= i) D[i * kLmN + j] -= D[i * kLmN + k] * D[j * kLmN + k];
      }
      __syncthreads();
    }
    if (!ok) {
      bad = t;
      break;
    }
    // the right-hand sides of W_t and V_t, transposed: (E_t^T - V_{t-1} W_{t-1}^T)[i][k] at [k][i], and F_t as it is
    if (hasW) {
      for (int e = tid; e < kCvNN; e += kCvThreads) {
        const int k = e / kLmN, i = e % kLmN;
        double v = E[f * kCvNN + e];
        if (band2 && t > 0) {
          double c = 0.0;
#pragma unroll 2
          for (int m = 0; m < kLmN; m++) c += V1[m * kLmN + i] * Wp[m * kLmN + k];
          v = v - c;
        }
        Wn[e] = v;
        if (hasV) Vn[e] = F[f * kCvNN + e];
      }
    }
    __syncthreads();
    cv_rows(D, N, hasW ? Wn : nullptr, hasV ? Vn : nullptr, tid);
    double *wf = ws + f * kCvWs;
    for (int e = tid; e < kCvNN; e += kCvThreads) {
      wf[kCvWsN + e] = N[e];
      if (hasW) wf[kCvWsW + e] = Wn[e];
      if (hasV) wf[kCvWsV + e] = Vn[e];
    }
    double *w = Wp;                                        // W_t becomes the previous W; the oldest V leaves
    Wp = Wn, Wn = w;
    double *v = V2;
    V2 = V1, V1 = Vn, Vn = v;
    __syncthreads();
  }
  if (tid == 0) status[q] = bad < 0 ? 0 : 1 + bad;
  if (bad >= 0) {                                          // a pivot that is not positive and finite: the whole sequence is NaN
    const double nan = __builtin_nan("");
    for (size_t e = tid; e < (size_t)T * kCvNN; e += kCvThreads) cov[first * kCvNN + e] = nan;
    return;
  }
  // back: N, P, Q; Z11 = Z_{t+1,t+1}, Z21 = Z_{t+2,t+1}, Z22 = Z_{t+2,t+2} kept; Z10 = Z_{t+1,t}, Z20 = Z_{t+2,t}, Z00 = Z_tt
  // formed.  (s.blk[1] holds the last frame's N.)
  double *P = s.blk[0], *Q = s.blk[2], *Z11 = s.blk[3], *Z21 = s.blk[4], *Z22 = s.blk[5], *Z10 = s.blk[6], *Z20 = s.blk[7],
         *Z00 = s.blk[8];
#pragma unroll 1
  for (int t = T - 1; t >= 0; t--) {
    const size_t f = first + t;
    const bool hasP = band1 && t < T - 1, hasQ = band2 && t < T - 2;
    if (t < T - 1) {
      const double *wf = ws + f * kCvWs;
      for (int e = tid; e < kCvNN; e += kCvThreads) {      // W_t and V_t where Z10 and Z20 are formed afterwards
        N[e] = wf[kCvWsN + e];
        if (hasP) Z10[e] = wf[kCvWsW + e];
        if (hasQ) Z20[e] = wf[kCvWsV + e];
      }
      __syncthreads();
    }
    if (hasP) {
      for (int e = tid; e < kCvNN; e += kCvThreads) {
        const int i = e / kLmN, j = e % kLmN;
        P[e] = cv_dot(Z10, true, N, i, j);
        if (hasQ) Q[e] = cv_dot(Z20, true, N, i, j);
      }
      __syncthreads();
      for (int e = tid; e < kCvNN; e += kCvThreads) {
        const int i = e / kLmN, j = e % kLmN;
        double z = -cv_dot(Z11, false, P, i, j);
        if (hasQ) {
          z = z - cv_dot(Z21, true, Q, i, j);
          Z20[e] = (-cv_dot(Z21, false, P, i, j)) - cv_dot(Z22, false, Q, i, j);
        }
        Z10[e] = z;
      }
      __syncthreads();
    }
    for (int e = tid; e < kCvNN; e += kCvThreads) {
      const int i = e / kLmN, j = e % kLmN;
      if (i < j) continue;
      double z = cv_dot(N, true, N, i, j);
      if (hasP) z = z - cv_dot(P, true, Z10, i, j);
      if (hasQ) z = z - cv_dot(Q, true, Z20, i, j);
      Z00[i * kLmN + j] = Z00[j * kLmN + i] = z;
      cov[f * kCvNN + i * kLmN + j] = cov[f * kCvNN + j * kLmN + i] = z;
    }
    double *z22 = Z22, *z21 = Z21;                         // frame t + 2 leaves
    Z22 = Z11, Z21 = Z10, Z11 = Z00;
    Z10 = z21, Z00 = z22;
    __syncthreads();
  }
}

struct CvProjectLds {
  double Z[kCvNN];
  float jac[3 * 64 * kLmN];
};

__global__ void __launch_bounds__(kCvThreads)
pose_lm_seq2_covariance_project_kernel(const double *__restrict__ cov, const float *__restrict__ jac,
                                       const int32_t *__restrict__ status, int T, int J, double *__restrict__ sphere_cov) {
  __shared__ CvProjectLds s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const bool failed = status[b / T] != 0;
  for (int e = tid; e < kCvNN; e += kCvThreads) s.Z[e] = cov[(size_t)b * kCvNN + e];
  for (int e = tid; e < 3 * J * kLmN; e += kCvThreads) s.jac[e] = jac[(size_t)b * 3 * J * kLmN + e];
  __syncthreads();
  for (int e = tid; e < 6 * J; e += kCvThreads) {
    const int j = e / 6, ab = e % 6;                       // xx xy xz yy yz zz
    const int a = ab < 3 ? 0 : ab < 5 ? 1 : 2, c = ab < 3 ? ab : ab < 5 ? ab - 2 : 2;
    const float *ra = s.jac + (3 * j + a) * kLmN, *rc = s.jac + (3 * j + c) * kLmN;
    double sum = 0.0;
#pragma unroll 1
    for (int k = 0; k < kLmN; k++) {
      double y = 0.0;
#pragma unroll 2
      for (int m = 0; m < kLmN; m++) y += (double)ra[m] * s.Z[m * kLmN + k];
      sum += y * (double)rc[k];
    }
    sphere_cov[(size_t)b * 6 * J + e] = failed ? __builtin_nan("") : sum;
  }
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_pose_lm_seq2_covariance_workspace_bytes(int B) {
  if (B < 0) return -1;
  return (long long)B * kCvWs * 8;
}

extern "C" int shr_pose_lm_seq2_covariance(const double *A, const double *E, const double *F, const float *stiffness,
                                           const float *jac, int B, int T, int J, double *cov, double *sphere_cov,
                                           int32_t *status, void *workspace, void *stream) {
  if (B < 0 || T < 1 || B % T != 0 || J < 1) return SHR_EINVAL;
  if (B > 65535 || J > 64) return SHR_ETOOLARGE;
  if (B == 0) return SHR_OK;
  if (!A || !cov || !status || !workspace || (jac == nullptr) != (sphere_cov == nullptr)) return SHR_EINVAL;
  if ((((uintptr_t)A | (uintptr_t)E | (uintptr_t)F | (uintptr_t)cov | (uintptr_t)sphere_cov) & 7u) != 0) return SHR_EINVAL;
  if ((((uintptr_t)stiffness | (uintptr_t)jac | (uintptr_t)status) & 3u) != 0 || (((uintptr_t)workspace) & 15u) != 0)
    return SHR_EINVAL;
  hipLaunchKernelGGL(pose_lm_seq2_covariance_chain_kernel, dim3((unsigned)(B / T)), dim3(kCvThreads), 0, (hipStream_t)stream, A,
                     E, F, stiffness, T, cov, status, reinterpret_cast<double *>(workspace));
  if (int rc = (int)hipGetLastError()) return rc;
  if (!jac) return SHR_OK;
  hipLaunchKernelGGL(pose_lm_seq2_covariance_project_kernel, dim3((unsigned)B), dim3(kCvThreads), 0, (hipStream_t)stream, cov,
                     jac, status, T, J, sphere_cov);
  return (int)hipGetLastError();
}
