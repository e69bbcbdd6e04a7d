// lm_seq2.hip -- lm_seq.hip's sequence step for normal equations with a SECOND off-diagonal block
// (shr_pose_lm_seq2_begin / shr_pose_lm_seq2_step): the bookkeeping per sequence, the cost chain, the accept rule, lambda,
// cost0 and trial_out = p on a bad pivot are shr_pose_lm_seq_step's, and the damped solve is of the block-PENTAdiagonal
// system a term that couples three consecutive frames leaves (sphere_accel.hip's E and F).
//
// Inverts (reference file:line): nothing; the energy's family is network/util_modules.py:349-381.  The reference has no
// counterpart of the solve.
//
//   one workgroup of ONE wave per sequence, lane i owning row i of the frame's 26 unknowns; the frames are taken one after
//   the other, so a sequence is a latency chain of T frames.
//   total, keep   lm_seq.hip's, with F kept beside E on accept.
//   factor    block Cholesky with bandwidth two, forward over t:
//             D_t = (M_t + lambda diag M_t) - W_{t-1} W_{t-1}^T - V_{t-2} V_{t-2}^T, M_t = A_t + diag(mu): per entry the W
//             product is subtracted first, then the V product, each m ascending, then lm_solve.h's column recurrence;
//             L_t L_t^T = D_t;  L_t y_t = r_t - W_{t-1} y_{t-1} - V_{t-2} y_{t-2};
//             W_t = (E_t^T - V_{t-1} W_{t-1}^T) L_t^-T for t <= T - 2;  V_t = F_t^T L_t^-T for t <= T - 3;
//             each of W_t and V_t by 26 triangular solves side by side, lane i owning row i.  L_t, W_t, y_t and, behind
//             them, V_t go to the workspace.
//   back      backward over t: L_t^T x_t = y_t - W_t^T x_{t+1} - V_t^T x_{t+2}; trial_out = (float)(p + x).
//   Everything fp64, every sum in index order, the W term before the V term.  With F == NULL the entry IS
//   shr_pose_lm_seq_step: the state and the workspace begin with that entry's own, so the call is handed on as it is.
//   LDS: A, L, W, the two previous V blocks and the cross product [26 x 26], x, y, the y (or x) before it [26] in fp64 and
//   the pivot: 33 080 bytes.  W and V are held TRANSPOSED (W[k * 26 + i] = W_t[i][k]), so that the lanes of the triangular
//   solves and of the outer products read consecutive doubles.
#include "lm_solve.h"

namespace shr {

// The state is lm_seq.hip's, frame by frame, followed by the accepted F of every frame: B x kS2State doubles (the accepted
// pose's A [26 x 26], E [26 x 26] and g [26], the pose, params0; then, used in the FIRST frame of a sequence only, the
// sequence's total cost, lambda, `fresh`, `moved`, the accept and reject counters), then B x kS2Block doubles (F [26 x 26],
// padded to a multiple of 8).  The offsets below are lm_seq.hip's kSq*: without F the step is handed to shr_pose_lm_seq_step.
constexpr int kS2A = 0, kS2E = kLmN * kLmN, kS2G = 2 * kLmN * kLmN, kS2P = kS2G + kLmN, kS2P0 = kS2P + kLmN, kS2Cost = kS2P0 + kLmN,
              kS2Lambda = kS2Cost + 1, kS2Fresh = kS2Cost + 2, kS2Moved = kS2Cost + 3, kS2Accepts = kS2Cost + 4,
              kS2Rejects = kS2Cost + 5, kS2State = 1440, kS2Block = 680;
static_assert(kS2Rejects < kS2State && kS2State % 8 == 0 && kLmN * kLmN <= kS2Block && kS2Block % 8 == 0, "the state's fields");
// The workspace likewise: B x kS2Ws doubles (L_t [26 x 26], W_t transposed [26 x 26], y_t [26], padded to a multiple of 8),
// then B x kS2Block doubles (V_t transposed).
constexpr int kS2WsL = 0, kS2WsW = kLmN * kLmN, kS2WsY = 2 * kLmN * kLmN, kS2Ws = 1384;
static_assert(kS2WsY + kLmN <= kS2Ws && kS2Ws % 8 == 0, "the workspace's fields");

__global__ void __launch_bounds__(64)
pose_lm_seq2_begin_kernel(const float *__restrict__ params0, float lambda0, double *__restrict__ state, float *__restrict__ trial) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double *st = state + (size_t)b * kS2State;
  double *stF = state + (size_t)gridDim.x * kS2State + (size_t)b * kS2Block;
  for (int e = lane; e < kS2P; e += 64) st[e] = 0.0;
  for (int e = lane; e < kS2Block; e += 64) stF[e] = 0.0;
  if (lane < kLmN) {
    const float p = params0[(size_t)b * kLmN + lane];
    st[kS2P + lane] = st[kS2P0 + lane] = (double)p;
    trial[(size_t)b * kLmN + lane] = p;
  }
  if (lane == 0) {
    st[kS2Cost] = __builtin_inf();
    st[kS2Lambda] = (double)lambda0;
    st[kS2Fresh] = 1.0;
    st[kS2Moved] = st[kS2Accepts] = st[kS2Rejects] = 0.0;
  }
}

struct S2Lds {
  double A[kLmN * kLmN], L[kLmN * kLmN], W[kLmN * kLmN], V[2][kLmN * kLmN], C[kLmN * kLmN], x[kLmN], y[kLmN], y2[kLmN], piv;
};

// L L^T = A + lam diag(A) - W W^T (with `prev`) - V V^T, V = s.V[v2] (with v2 >= 0), lm_cholesky's recurrence.  false: a
// pivot that is not positive and finite.
__device__ __forceinline__ bool s2_cholesky(S2Lds &s, double lam, int lane, bool prev, int v2) {
  const double *V2 = s.V[v2 < 0 ? 0 : v2];
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
      if (v2 >= 0) {
#pragma unroll 2
        for (int m = 0; m < kLmN; m++) v -= V2[m * kLmN + lane] * V2[m * kLmN + k];
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

// column `lane` of X (X[k * 26 + lane], k = 0 ... 25) := the solution z of L z = that column, in place
__device__ __forceinline__ void s2_rows(const S2Lds &s, double *X, int lane) {
#pragma unroll 1
  for (int k = 0; k < kLmN; k++) {
    double v = X[k * kLmN + lane];
#pragma unroll 2
    for (int m = 0; m < k; m++) v -= s.L[k * kLmN + m] * X[m * kLmN + lane];
    X[k * kLmN + lane] = v / s.L[k * kLmN + k];
  }
}

__global__ void __launch_bounds__(64)
pose_lm_seq2_step_kernel(double *__restrict__ state, const double *__restrict__ A, const double *__restrict__ g,
                         const double *__restrict__ E, const double *__restrict__ F, const double *__restrict__ cost_data,
                         const float *trial, const float *__restrict__ prior, const float *__restrict__ stiffness, int solve, int T,
                         float *trial_out, float *__restrict__ params, float *__restrict__ cost, float *__restrict__ cost0,
                         double *__restrict__ ws) {
  __shared__ S2Lds s;
  const int q = blockIdx.x, lane = threadIdx.x;
  const size_t first = (size_t)q * T;
  double *sq = state + first * kS2State;                   // the sequence's fields live in its first frame
  double *stF = state + (size_t)gridDim.x * T * kS2State;  // the accepted F of every frame, after the frames' own fields
  double *wsV = ws + (size_t)gridDim.x * T * kS2Ws;        // V_t of every frame, after the frames' L_t, W_t, y_t
  const bool own = lane < kLmN;
  const double mu = own && stiffness ? (double)stiffness[lane] : 0.0;
  const double cur = sq[kS2Cost], lam0 = sq[kS2Lambda];
  const bool fresh = sq[kS2Fresh] != 0.0, moved = sq[kS2Moved] != 0.0;
  const double accepts = sq[kS2Accepts], rejects = sq[kS2Rejects];
  // total: the frames' totals, t ascending; a frame's total is shr_pose_lm_step's chain
  double total = 0.0;
#pragma unroll 1
  for (int t = 0; t < T; t++) {
    const size_t f = first + t;
    if (own) {
      const double pr = prior ? (double)prior[f * kLmN + lane] : state[f * kS2State + kS2P0 + lane];
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
    double *st = state + f * kS2State;
    if (accept) {
      for (int e = lane; e < kLmN * kLmN; e += 64) st[kS2A + e] = A[f * kLmN * kLmN + e];
      if (E)
        for (int e = lane; e < kLmN * kLmN; e += 64) st[kS2E + e] = E[f * kLmN * kLmN + e];
      for (int e = lane; e < kLmN * kLmN; e += 64) stF[f * kS2Block + e] = F[f * kLmN * kLmN + e];
      if (own) {
        st[kS2G + lane] = g[f * kLmN + lane];
        st[kS2P + lane] = (double)trial[f * kLmN + lane];
      }
    }
    if (own) params[f * kLmN + lane] = (float)(accept ? (double)trial[f * kLmN + lane] : st[kS2P + lane]);
  }
  if (lane == 0) {
    sq[kS2Cost] = accept ? total : cur;
    sq[kS2Lambda] = lam;
    sq[kS2Fresh] = 0.0;
    sq[kS2Moved] = (moved || accept) ? 1.0 : 0.0;
    sq[kS2Accepts] = accepts + (accept ? 1.0 : 0.0);
    sq[kS2Rejects] = rejects + (accept ? 0.0 : 1.0);
    cost[q] = (float)(accept ? total : cur);
    if (fresh) cost0[q] = (float)total;
  }
  if (!solve) return;
  __syncthreads();                                         // the state written above is read below
  bool ok = true;
  int v1 = 0;                                              // s.V[v1] is V_{t-1}, s.V[1 - v1] V_{t-2}, transposed
  // factor, forward over t
#pragma unroll 1
  for (int t = 0; t < T && ok; t++) {
    const size_t f = first + t;
    const double *st = state + f * kS2State;
    double *wf = ws + f * kS2Ws;
    for (int e = lane; e < kLmN * kLmN; e += 64) s.A[e] = st[kS2A + e];
    const double pa = own ? st[kS2P + lane] : 0.0, ga = own ? st[kS2G + lane] : 0.0;
    const double pr = !own ? 0.0 : prior ? (double)prior[f * kLmN + lane] : st[kS2P0 + lane];
    __syncthreads();
    if (own) s.A[lane * kLmN + lane] += mu;                // M = A + diag(mu)
    __syncthreads();
    const bool far = t > 1;                                // V_{t-2} exists
    ok = s2_cholesky(s, lam, lane, t > 0, far ? 1 - v1 : -1);
    __syncthreads();
    if (!ok) break;
    double rhs = -(ga + mu * (pa - pr));
    if (t > 0 && own) {                                    // r_t - W_{t-1} y_{t-1}
      double c = 0.0;
#pragma unroll 2
      for (int k = 0; k < kLmN; k++) c += s.W[k * kLmN + lane] * s.y[k];
      rhs = rhs - c;
    }
    if (far && own) {                                      // ... - V_{t-2} y_{t-2}
      double c = 0.0;
#pragma unroll 2
      for (int k = 0; k < kLmN; k++) c += s.V[1 - v1][k * kLmN + lane] * s.y2[k];
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
    if (own) {
      if (t > 0) s.y2[lane] = s.y[lane];
      s.y[lane] = s.x[lane];
    }
    if (t < T - 1) {
      if (t > 0) {                                         // E_t^T - V_{t-1} W_{t-1}^T, lane i its column i of the transposed block
        if (own) {
#pragma unroll 1
          for (int k = 0; k < kLmN; k++) {
            double c = 0.0;
#pragma unroll 2
            for (int m = 0; m < kLmN; m++) c += s.V[v1][m * kLmN + lane] * s.W[m * kLmN + k];
            s.C[k * kLmN + lane] = st[kS2E + k * kLmN + lane] - c;
          }
        }
        __syncthreads();                                   // every lane has read the previous W
        for (int e = lane; e < kLmN * kLmN; e += 64) {
          wf[kS2WsL + e] = s.L[e];
          s.W[e] = s.C[e];
        }
      } else {
        for (int e = lane; e < kLmN * kLmN; e += 64) {
          wf[kS2WsL + e] = s.L[e];
          s.W[e] = st[kS2E + e];
        }
      }
      if (own) wf[kS2WsY + lane] = s.x[lane];
      __syncthreads();
      if (own) s2_rows(s, s.W, lane);                      // row `lane` of W_t: L_t z = (E_t^T - ...)[lane, :], in place
      __syncthreads();
      for (int e = lane; e < kLmN * kLmN; e += 64) wf[kS2WsW + e] = s.W[e];
    }
    v1 = 1 - v1;                                           // the older V leaves; V_t takes its place
    if (t < T - 2) {
      for (int e = lane; e < kLmN * kLmN; e += 64) s.V[v1][e] = stF[f * kS2Block + e];
      __syncthreads();
      if (own) s2_rows(s, s.V[v1], lane);                  // row `lane` of V_t: L_t z = F_t[:, lane]
      __syncthreads();
      for (int e = lane; e < kLmN * kLmN; e += 64) wsV[f * kS2Block + e] = s.V[v1][e];
    }
    __syncthreads();
  }
  if (!ok) {                                               // a pivot that is not positive and finite: the whole sequence stays
    for (int t = 0; t < T; t++) {
      const size_t f = first + t;
      if (own) trial_out[f * kLmN + lane] = (float)state[f * kS2State + kS2P + lane];
    }
    return;
  }
  // back, backward over t: s.L and s.x hold the last frame's L and y; s.y is x_{t+1}, s.y2 x_{t+2}
#pragma unroll 1
  for (int t = T - 1; t >= 0; t--) {
    const size_t f = first + t;
    const bool far = t < T - 2;                            // V_t exists
    double z = 0.0;
    if (t < T - 1) {
      const double *wf = ws + f * kS2Ws;
      for (int e = lane; e < kLmN * kLmN; e += 64) {
        s.L[e] = wf[kS2WsL + e];
        s.W[e] = wf[kS2WsW + e];
      }
      if (far)
        for (int e = lane; e < kLmN * kLmN; e += 64) s.V[0][e] = wsV[f * kS2Block + e];
      __syncthreads();
      if (own) {                                           // y_t - W_t^T x_{t+1}
        double c = 0.0;
#pragma unroll 2
        for (int i = 0; i < kLmN; i++) c += s.W[lane * kLmN + i] * s.y[i];
        z = wf[kS2WsY + lane] - c;
      }
      if (far && own) {                                    // ... - V_t^T x_{t+2}
        double c = 0.0;
#pragma unroll 2
        for (int i = 0; i < kLmN; i++) c += s.V[0][lane * kLmN + i] * s.y2[i];
        z = z - c;
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
      trial_out[f * kLmN + lane] = (float)(state[f * kS2State + kS2P + lane] + s.x[lane]);
      if (t < T - 1) s.y2[lane] = s.y[lane];
      s.y[lane] = s.x[lane];
    }
    __syncthreads();
  }
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_pose_lm_seq2_state_bytes(int B) {
  if (B < 0) return -1;
  return (long long)B * (kS2State + kS2Block) * 8;
}

extern "C" long long shr_pose_lm_seq2_workspace_bytes(int B) {
  if (B < 0) return -1;
  return (long long)B * (kS2Ws + kS2Block) * 8;
}

static int lm_seq2_check(const void *state, int B, int T) {
  if (!state || B < 0 || T < 1 || B % T != 0 || (((uintptr_t)state) & 7u) != 0) return SHR_EINVAL;
  if (B > (1 << 24)) return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" int shr_pose_lm_seq2_begin(const float *params0, int B, int T, float lambda0, void *state, float *trial, void *stream) {
  if (int rc = lm_seq2_check(state, B, T)) return rc;
  if (B == 0) return SHR_OK;
  if (!params0 || !trial || !(lambda0 > 0.0f) || (((uintptr_t)params0 | (uintptr_t)trial) & 3u) != 0) return SHR_EINVAL;
  hipLaunchKernelGGL(pose_lm_seq2_begin_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, params0, lambda0,
                     reinterpret_cast<double *>(state), trial);
  return (int)hipGetLastError();
}

extern "C" int shr_pose_lm_seq2_step(void *state, const double *A, const double *g, const double *E, const double *F,
                                     const double *cost_data, const float *trial, const float *prior, const float *stiffness,
                                     int solve, int B, int T, float *trial_out, float *params, float *cost, float *cost0,
                                     void *workspace, void *stream) {
  // without F: the tridiagonal step on the state's and the workspace's leading part, which are that entry's own
  if (!F)
    return shr_pose_lm_seq_step(state, A, g, E, cost_data, trial, prior, stiffness, solve, B, T, trial_out, params, cost, cost0,
                                workspace, stream);
  if (int rc = lm_seq2_check(state, B, T)) return rc;
  if (B == 0) return SHR_OK;
  if (!A || !g || (!E && T > 1) || !cost_data || !trial || !params || !cost || !cost0 || (solve && (!trial_out || !workspace)))
    return SHR_EINVAL;
  if ((((uintptr_t)A | (uintptr_t)g | (uintptr_t)E | (uintptr_t)F | (uintptr_t)cost_data | (uintptr_t)workspace) & 7u) != 0)
    return SHR_EINVAL;
  if ((((uintptr_t)trial | (uintptr_t)prior | (uintptr_t)stiffness | (uintptr_t)trial_out | (uintptr_t)params | (uintptr_t)cost |
        (uintptr_t)cost0) & 3u) != 0)
    return SHR_EINVAL;
  hipLaunchKernelGGL(pose_lm_seq2_step_kernel, dim3((unsigned)(B / T)), dim3(64), 0, (hipStream_t)stream,
                     reinterpret_cast<double *>(state), A, g, E, F, cost_data, trial, prior, stiffness, solve ? 1 : 0, T, trial_out,
                     params, cost, cost0, reinterpret_cast<double *>(workspace));
  return (int)hipGetLastError();
}
