// lm_seq.hip -- the Levenberg-Marquardt bookkeeping of pose_icp.hip's shr_pose_lm_begin / shr_pose_lm_step with the unit
// of decision raised from the crop to the SEQUENCE (shr_pose_lm_seq_begin / shr_pose_lm_seq_step): B = S T frames, the T
// frames of a sequence adjacent, one lambda, one cost and one accept decision per sequence, and the damped solve of the
// block-tridiagonal normal equations a term that couples consecutive frames leaves (sphere_temporal.hip's E).
//
// Inverts (reference file:line): the energy of TemporalSmoothnessLoss (network/util_modules.py:360-381) beside the
// per-frame terms; the reference has no counterpart of the solve.
//
//   one workgroup of ONE wave per sequence, lane i owning row i of the frame's 26 unknowns, as lm_solve.h's solve does; the
//   frames are taken one after the other, so a sequence is a latency chain of T frames.
//   total     the chain over t ascending of (cost_data_t + the stiffness term of frame t, shr_pose_lm_step's sum); accept,
//             lambda and the counters are shr_pose_lm_step's rules on the sequence's total.
//   keep      on accept every frame's A, E, g and trial go to the state; params is the state's pose.
//   factor    forward over t: D_t = M_t + lambda diag(M_t) - W_{t-1} W_{t-1}^T, M_t = A_t + diag(mu); L_t L_t^T = D_t by
//             lm_solve.h's column-by-column recurrence (the previous factor's outer product subtracted first, then the
//             columns' own); y_t from L_t y_t = r_t - W_{t-1} y_{t-1}; W_t = E_t^T L_t^-T, lane i solving L_t z = E_t[:, i]
//             for row i of W_t (26 triangular solves side by side).  L_t, W_t and y_t go to the workspace.
//   back      backward over t: L_t^T x_t = y_t - W_t^T x_{t+1}; trial_out = (float)(p + x).
//   With T = 1 every operation is shr_pose_lm_step's in its order: the same bits.
//   LDS: A, L, W [26 x 26] and x, y [26] in fp64 and the pivot: 16 648 bytes.  W is held TRANSPOSED (W[k * 26 + i] =
//   W_t[i][k]), so that the lanes of the triangular solves and of the outer product read consecutive doubles.
#include "lm_solve.h"

namespace shr {

// A frame's state, in doubles: the accepted pose's A [26 x 26], E [26 x 26] and g [26], the pose, params0; then, used in the
// FIRST frame of a sequence only, the sequence's total cost, lambda, `fresh`, `moved`, the accept and reject counters.
constexpr int kSqA = 0, kSqE = kLmN * kLmN, kSqG = 2 * kLmN * kLmN, kSqP = kSqG + kLmN, kSqP0 = kSqP + kLmN, kSqCost = kSqP0 + kLmN,
              kSqLambda = kSqCost + 1, kSqFresh = kSqCost + 2, kSqMoved = kSqCost + 3, kSqAccepts = kSqCost + 4,
              kSqRejects = kSqCost + 5, kSqState = 1440;
static_assert(kSqRejects < kSqState, "the state's fields");
// A frame's workspace, in doubles: L_t [26 x 26], W_t transposed [26 x 26], y_t [26], padded to a multiple of 8
constexpr int kSqWsL = 0, kSqWsW = kLmN * kLmN, kSqWsY = 2 * kLmN * kLmN, kSqWs = 1384;
static_assert(kSqWsY + kLmN <= kSqWs, "the workspace's fields");

__global__ void __launch_bounds__(64)
pose_lm_seq_begin_kernel(const float *__restrict__ params0, float lambda0, double *__restrict__ state, float *__restrict__ trial) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double *st = state + (size_t)b * kSqState;
  for (int e = lane; e < kSqP; e += 64) st[e] = 0.0;
  if (lane < kLmN) {
    const float p = params0[(size_t)b * kLmN + lane];
    st[kSqP + lane] = st[kSqP0 + lane] = (double)p;
    trial[(size_t)b * kLmN + lane] = p;
  }
  if (lane == 0) {
    st[kSqCost] = __builtin_inf();
    st[kSqLambda] = (double)lambda0;
    st[kSqFresh] = 1.0;
    st[kSqMoved] = st[kSqAccepts] = st[kSqRejects] = 0.0;
  }
}

struct SqLds {
  double A[kLmN * kLmN], L[kLmN * kLmN], W[kLmN * kLmN], x[kLmN], y[kLmN], piv;
};

// L L^T = A + lam diag(A) - W W^T (the last only with `prev`), lm_cholesky's recurrence.  false: a pivot that is not
// positive and finite.
__device__ __forceinline__ bool sq_cholesky(SqLds &s, double lam, int lane, bool prev) {
#pragma unroll 1
  for (int k = 0; k < kLmN; k++) {
    double v = 0.0;
    if (lane >= k && lane < kLmN) {
      v = s.A[lane * kLmN + k];
      if (lane == k) v += lam * v;
      if (prev) {
#pragma unroll 2
        for (int m = 0; m < kLmN; m++) v -= s.W[m * kLmN + lane] * s.W[m * kLmN + k];
      }
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

__global__ void __launch_bounds__(64)
pose_lm_seq_step_kernel(double *__restrict__ state, const double *__restrict__ A, const double *__restrict__ g,
                        const double *__restrict__ E, const double *__restrict__ cost_data, const float *trial,
                        const float *__restrict__ prior, const float *__restrict__ stiffness, int solve, int T, float *trial_out,
                        float *__restrict__ params, float *__restrict__ cost, float *__restrict__ cost0,
                        double *__restrict__ ws) {
  __shared__ SqLds s;
  const int q = blockIdx.x, lane = threadIdx.x;
  const size_t first = (size_t)q * T;
  double *sq = state + first * kSqState;                   // the sequence's fields live in its first frame
  const bool own = lane < kLmN;
  const double mu = own && stiffness ? (double)stiffness[lane] : 0.0;
  const double cur = sq[kSqCost], lam0 = sq[kSqLambda];
  const bool fresh = sq[kSqFresh] != 0.0, moved = sq[kSqMoved] != 0.0;
  const double accepts = sq[kSqAccepts], rejects = sq[kSqRejects];
  // total: the frames' totals, t ascending; a frame's total is shr_pose_lm_step's chain
  double total = 0.0;
#pragma unroll 1
  for (int t = 0; t < T; t++) {
    const size_t f = first + t;
    if (own) {
      const double pr = prior ? (double)prior[f * kLmN + lane] : state[f * kSqState + kSqP0 + lane];
      const double d = (double)trial[f * kLmN + lane] - pr;
      s.x[lane] = mu * (d * d);
    }
    __syncthreads();
    double mine = cost_data[f];
#pragma unroll 1
    for (int i = 0; i < kLmN; i++) mine += s.x[i];
    total = t == 0 ? mine : total + mine;
    __syncthreads();
  }
  const bool accept = total < cur && total > -__builtin_inf();        // (false for a NaN, and for +inf)
  const double lam = fmin(fmax(lam0 * (accept ? (moved ? 0.3 : 1.0) : 10.0), 1e-9), 1e6);
  // keep: the trial's equations and poses become the state's where the sequence is accepted
#pragma unroll 1
  for (int t = 0; t < T; t++) {
    const size_t f = first + t;
    double *st = state + f * kSqState;
    if (accept) {
      for (int e = lane; e < kLmN * kLmN; e += 64) st[kSqA + e] = A[f * kLmN * kLmN + e];
      if (E)
        for (int e = lane; e < kLmN * kLmN; e += 64) st[kSqE + e] = E[f * kLmN * kLmN + e];
      if (own) {
        st[kSqG + lane] = g[f * kLmN + lane];
        st[kSqP + lane] = (double)trial[f * kLmN + lane];
      }
    }
    if (own) params[f * kLmN + lane] = (float)(accept ? (double)trial[f * kLmN + lane] : st[kSqP + lane]);
  }
  if (lane == 0) {
    sq[kSqCost] = accept ? total : cur;
    sq[kSqLambda] = lam;
    sq[kSqFresh] = 0.0;
    sq[kSqMoved] = (moved || accept) ? 1.0 : 0.0;
    sq[kSqAccepts] = accepts + (accept ? 1.0 : 0.0);
    sq[kSqRejects] = rejects + (accept ? 0.0 : 1.0);
    cost[q] = (float)(accept ? total : cur);
    if (fresh) cost0[q] = (float)total;
  }
  if (!solve) return;
  __syncthreads();                                         // the state written above is read below
  bool ok = true;
  // factor, forward over t
#pragma unroll 1
  for (int t = 0; t < T && ok; t++) {
    const size_t f = first + t;
    const double *st = state + f * kSqState;
    double *wf = ws + f * kSqWs;
    for (int e = lane; e < kLmN * kLmN; e += 64) s.A[e] = st[kSqA + e];
    const double pa = own ? st[kSqP + lane] : 0.0, ga = own ? st[kSqG + lane] : 0.0;
    const double pr = !own ? 0.0 : prior ? (double)prior[f * kLmN + lane] : st[kSqP0 + lane];
    __syncthreads();
    if (own) s.A[lane * kLmN + lane] += mu;                // M = A + diag(mu)
    __syncthreads();
    ok = sq_cholesky(s, lam, lane, t > 0);
    __syncthreads();
    if (!ok) break;
    double rhs = -(ga + mu * (pa - pr));
    if (t > 0 && own) {                                    // r_t - W_{t-1} y_{t-1}
      double c = 0.0;
#pragma unroll 2
      for (int k = 0; k < kLmN; k++) c += s.W[k * kLmN + lane] * s.y[k];
      rhs = rhs - c;
    }
    __syncthreads();
    double acc = 0.0;
#pragma unroll 1
    for (int k = 0; k < kLmN; k++) {                       // lm_solve's forward substitution
      if (lane == k) s.x[k] = (rhs - acc) / s.L[k * kLmN + k];
      __syncthreads();
      if (lane > k && lane < kLmN) acc += s.L[lane * kLmN + k] * s.x[k];
    }
    if (own) s.y[lane] = s.x[lane];
    if (t < T - 1) {
      for (int e = lane; e < kLmN * kLmN; e += 64) {
        wf[kSqWsL + e] = s.L[e];
        s.W[e] = st[kSqE + e];
      }
      if (own) wf[kSqWsY + lane] = s.x[lane];
      __syncthreads();
      if (own) {                                           // row `lane` of W_t: L_t z = E_t[:, lane], in place
#pragma unroll 1
        for (int k = 0; k < kLmN; k++) {
          double v = s.W[k * kLmN + lane];
#pragma unroll 2
          for (int m = 0; m < k; m++) v -= s.L[k * kLmN + m] * s.W[m * kLmN + lane];
          s.W[k * kLmN + lane] = v / s.L[k * kLmN + k];
        }
      }
      __syncthreads();
      for (int e = lane; e < kLmN * kLmN; e += 64) wf[kSqWsW + e] = s.W[e];
    }
    __syncthreads();
  }
  if (!ok) {                                               // a pivot that is not positive and finite: the whole sequence stays
    for (int t = 0; t < T; t++) {
      const size_t f = first + t;
      if (own) trial_out[f * kLmN + lane] = (float)state[f * kSqState + kSqP + lane];
    }
    return;
  }
  // back, backward over t: s.L and s.x hold the last frame's L and y
#pragma unroll 1
  for (int t = T - 1; t >= 0; t--) {
    const size_t f = first + t;
    double z = 0.0;
    if (t < T - 1) {
      const double *wf = ws + f * kSqWs;
      for (int e = lane; e < kLmN * kLmN; e += 64) {
        s.L[e] = wf[kSqWsL + e];
        s.W[e] = wf[kSqWsW + e];
      }
      __syncthreads();
      if (own) {                                           // y_t - W_t^T x_{t+1}
        double c = 0.0;
#pragma unroll 2
        for (int i = 0; i < kLmN; i++) c += s.W[lane * kLmN + i] * s.y[i];
        z = wf[kSqWsY + lane] - c;
      }
    } else {
      z = own ? s.x[lane] : 0.0;
    }
    double acc = 0.0;
    __syncthreads();
#pragma unroll 1
    for (int k = kLmN - 1; k >= 0; k--) {                  // lm_solve's backward substitution
      if (lane == k) s.x[k] = (z - acc) / s.L[k * kLmN + k];
      __syncthreads();
      if (lane < k) acc += s.L[k * kLmN + lane] * s.x[k];
    }
    __syncthreads();
    if (own) {
      trial_out[f * kLmN + lane] = (float)(state[f * kSqState + kSqP + lane] + s.x[lane]);
      s.y[lane] = s.x[lane];
    }
    __syncthreads();
  }
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_pose_lm_seq_state_bytes(int B) {
  if (B < 0) return -1;
  return (long long)B * kSqState * 8;
}

extern "C" long long shr_pose_lm_seq_workspace_bytes(int B) {
  if (B < 0) return -1;
  return (long long)B * kSqWs * 8;
}

static int lm_seq_check(const void *state, int B, int T) {
  if (!state || B < 0 || T < 1 || B % T != 0 || (((uintptr_t)state) & 7u) != 0) return SHR_EINVAL;
  if (B > (1 << 24)) return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" int shr_pose_lm_seq_begin(const float *params0, int B, int T, float lambda0, void *state, float *trial, void *stream) {
  if (int rc = lm_seq_check(state, B, T)) return rc;
  if (B == 0) return SHR_OK;
  if (!params0 || !trial || !(lambda0 > 0.0f) || (((uintptr_t)params0 | (uintptr_t)trial) & 3u) != 0) return SHR_EINVAL;
  hipLaunchKernelGGL(pose_lm_seq_begin_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, params0, lambda0,
                     reinterpret_cast<double *>(state), trial);
  return (int)hipGetLastError();
}

extern "C" int shr_pose_lm_seq_step(void *state, const double *A, const double *g, const double *E, const double *cost_data,
                                    const float *trial, const float *prior, const float *stiffness, int solve, int B, int T,
                                    float *trial_out, float *params, float *cost, float *cost0, void *workspace, void *stream) {
  if (int rc = lm_seq_check(state, B, T)) return rc;
  if (B == 0) return SHR_OK;
  if (!A || !g || (!E && T > 1) || !cost_data || !trial || !params || !cost || !cost0 || (solve && (!trial_out || !workspace)))
    return SHR_EINVAL;
  if ((((uintptr_t)A | (uintptr_t)g | (uintptr_t)E | (uintptr_t)cost_data | (uintptr_t)workspace) & 7u) != 0) return SHR_EINVAL;
  if ((((uintptr_t)trial | (uintptr_t)prior | (uintptr_t)stiffness | (uintptr_t)trial_out | (uintptr_t)params | (uintptr_t)cost |
        (uintptr_t)cost0) & 3u) != 0)
    return SHR_EINVAL;
  hipLaunchKernelGGL(pose_lm_seq_step_kernel, dim3((unsigned)(B / T)), dim3(64), 0, (hipStream_t)stream,
                     reinterpret_cast<double *>(state), A, g, E, cost_data, trial, prior, stiffness, solve ? 1 : 0, T, trial_out,
                     params, cost, cost0, reinterpret_cast<double *>(workspace));
  return (int)hipGetLastError();
}
