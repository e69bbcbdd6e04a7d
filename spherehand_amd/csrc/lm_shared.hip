// lm_shared.hip -- the Levenberg-Marquardt bookkeeping of pose_icp.hip's shr_pose_lm_begin / shr_pose_lm_step with the unit
// of decision raised from the crop to the GROUP (shr_pose_lm_shared_begin / shr_pose_lm_shared_step): B = G N frames, the N
// frames of a group adjacent, one lambda, one cost and one accept decision per group, and a vector sigma [K] of parameters
// the frames of a group SHARE (a person's sphere radii over the frames of that person).  A shared parameter couples every
// frame of its group, so the normal equations are bordered block-diagonal -- an arrowhead: N pose blocks A_b [26 x 26], one
// shared block R [K x K] and a coupling C_b [26 x K] per frame -- and the damped solve is the Schur complement on the shared
// block.
//
// Inverts (reference file:line): the observation of DataToModelLoss (mesh/render.py:93-142) taken with the model's own
// constants as unknowns; the reference has no counterpart of the shared solve.
//
//   decide   one wave per group: total = the chain over the frames, ascending, of shr_pose_lm_step's per-frame total, then
//            + nu_k (sigma_k - prior_k)^2, k ascending; accept, lambda and the counters are shr_pose_lm_step's rules on the
//            group's total and live in the state of the group's FIRST frame.  On accept sigma, R and gs go to the state.
//   frame    one wave per frame: on accept A, g, the pose and C go to the state; params is the state's pose.  Then
//            M = A + diag(mu), L L^T = M + lambda diag(M) (lm_solve.h), z = L^-1 rhs by lm_solve.h's forward substitution
//            and Y = L^-1 C, lane k solving column k: K triangular solves side by side, no barrier between their 26 steps.
//            L, z, Y and the factor's verdict go to the workspace.
//   schur    one workgroup of 256 threads per group: S = T + lambda diag(T) - sum_b Y_b^T Y_b with T = R + diag(nu), one
//            thread per entry of the lower triangle, a frame's Y staged in LDS, frames ascending and m ascending inside; the
//            right-hand side likewise; S = L_s L_s^T IN PLACE by the column recurrence, thread i owning row i; d sigma by the
//            two substitutions.  Rows of S are 65 doubles apart so that the threads of a column step meet distinct banks.
//   back     one wave per frame: L^T delta = z - Y d sigma (k ascending); trial_out = (float)(p + delta).
//   With K = 0 there is no shared block (no schur pass, every frame's step its own); with K = 0 and N = 1 the call is handed
//   to shr_pose_lm_step, whose state is the leading part of this one.
//   LDS: frame 24 344 bytes (A, L [26 x 26], x [26], the pivot, Y [26 x 64]), schur 47 328 bytes (S [64 x 65], Y [26 x 64],
//   z [26], x [64], the pivot and the verdict), back 6 128 bytes.
#include "lm_state.h"

extern "C" int shr_pose_lm_step(void *state, const double *A, const double *g, const double *cost_data, const float *trial,
                                const float *prior, const float *stiffness, int solve, int B, float *trial_out, float *params,
                                float *cost, float *cost0, void *stream);

namespace shr {

constexpr int kShMaxK = 64;          // shared parameters at most: one wave owns the rows of S
constexpr int kShLd = kShMaxK + 1;   // the row stride of S in LDS
constexpr int kShThreads = 256;      // the schur pass
// A frame's state is shr_pose_lm_step's (lm_state.h's frame without E), the group's fields in the group's FIRST frame: with
// K == 0 and N == 1 the step is handed to that entry, which must find every field where this unit's begin put it.
using St = LmCropState;
// BEHIND the B frames: per group sigma [K], shape0 [K], gs [K], R [K x K]; behind the groups, per frame C [26 x K].
__host__ __device__ constexpr size_t sh_group_doubles(int K) { return (size_t)K * (3 + K); }
__host__ __device__ constexpr size_t sh_state_doubles(int B, int G, int K) {
  return (size_t)B * St::kSize + (size_t)G * sh_group_doubles(K) + (size_t)B * kLmN * K;
}
static_assert(sh_state_doubles(5, 5, 0) == 5 * LmCropState::kSize, "without a shared block the state is shr_pose_lm_step's");
// The workspace, in doubles: per frame L [26 x 26], z [26], the factor's verdict (704 with the padding), Y [26 x K]; behind
// the frames, per group: accept, lambda, the group's verdict (8 with the padding), d sigma [K].
constexpr int kShWsZ = kLmN * kLmN, kShWsOk = kShWsZ + kLmN, kShWsY = 704, kShWsGroup = 8;
static_assert(kShWsOk < kShWsY, "the workspace's fields");
__host__ __device__ inline size_t sh_ws_frame(int K) { return (size_t)kShWsY + (size_t)kLmN * K; }
__host__ __device__ inline size_t sh_ws_doubles(int B, int G, int K) {
  return (size_t)B * sh_ws_frame(K) + (size_t)G * (kShWsGroup + K);
}

__global__ void __launch_bounds__(64)
pose_lm_shared_begin_kernel(const float *__restrict__ params0, const float *__restrict__ shape0, float lambda0, int B, int N, int K,
                            double *__restrict__ state, float *__restrict__ trial, float *__restrict__ trial_shape) {
  const int b = blockIdx.x, lane = threadIdx.x;
  lm_begin_frame<St>(params0, lambda0, state + (size_t)b * St::kSize, trial, (size_t)b, lane);
  if (K == 0) return;
  const int G = B / N;
  double *sc = state + (size_t)B * St::kSize + (size_t)G * sh_group_doubles(K) + (size_t)b * kLmN * K;
  for (int e = lane; e < kLmN * K; e += 64) sc[e] = 0.0;
  if (b % N != 0) return;
  const int q = b / N;
  double *sg = state + (size_t)B * St::kSize + (size_t)q * sh_group_doubles(K);
  if (lane < K) {
    const float v = shape0[(size_t)q * K + lane];
    sg[lane] = sg[K + lane] = (double)v;
    sg[2 * K + lane] = 0.0;
    trial_shape[(size_t)q * K + lane] = v;
  }
  for (int e = lane; e < K * K; e += 64) sg[3 * K + e] = 0.0;
}

struct ShDecideLds {
  double x[kShMaxK];
};

__global__ void __launch_bounds__(64)
pose_lm_shared_decide_kernel(double *__restrict__ state, const double *__restrict__ R, const double *__restrict__ gs,
                             const double *__restrict__ cost_data, const float *trial, const float *trial_shape,
                             const float *__restrict__ prior, const float *__restrict__ stiffness,
                             const float *__restrict__ shape_prior, const float *__restrict__ shape_stiffness, int B, int N, int K,
                             float *__restrict__ shape, float *__restrict__ cost, float *__restrict__ cost0,
                             double *__restrict__ ws) {
  __shared__ ShDecideLds s;
  const int q = blockIdx.x, lane = threadIdx.x;
  const size_t first = (size_t)q * N;
  double *sq = state + first * St::kSize;                   // the group's fields live in its first frame
  double *sg = state + (size_t)B * St::kSize + (size_t)q * sh_group_doubles(K);
  double *wg = ws + (size_t)B * sh_ws_frame(K) + (size_t)q * (kShWsGroup + K);
  const double mu = lane < kLmN && stiffness ? (double)stiffness[lane] : 0.0;
  const LmBook bk = lm_book<St>(sq);
  double total = lm_frames_total<St>(s, state, first, N, cost_data, trial, prior, mu, lane);
  const float ts = lane < K ? trial_shape[(size_t)q * K + lane] : 0.f;
  if (K > 0) {                                             // + nu_k (sigma_k - prior_k)^2, k ascending
    if (lane < K) {
      const double nu = shape_stiffness ? (double)shape_stiffness[lane] : 0.0;
      const double d = (double)ts - (shape_prior ? (double)shape_prior[(size_t)q * K + lane] : sg[K + lane]);
      s.x[lane] = nu * (d * d);
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < K; k++) total += s.x[k];
  }
  const LmDecision dec = lm_decide(bk, total);
  const bool accept = dec.accept;
  if (lane < K) {
    const double sa = accept ? (double)ts : sg[lane];
    if (accept) {
      sg[lane] = sa;
      sg[2 * K + lane] = gs[(size_t)q * K + lane];
    }
    shape[(size_t)q * K + lane] = (float)sa;
  }
  if (accept)
    for (int e = lane; e < K * K; e += 64) sg[3 * K + e] = R[(size_t)q * K * K + e];
  if (lane == 0) {
    lm_record<St>(sq, bk, total, dec, cost + q, cost0 + q);
    wg[0] = accept ? 1.0 : 0.0;                            // what the frames' waves need of the decision
    wg[1] = dec.lam;
    wg[2] = 1.0;
  }
}

struct ShFrameLds {
  double A[kLmN * kLmN], L[kLmN * kLmN], x[kLmN], piv, Y[kLmN * kShMaxK];
};

__global__ void __launch_bounds__(64)
pose_lm_shared_frame_kernel(double *__restrict__ state, const double *__restrict__ A, const double *__restrict__ g,
                            const double *__restrict__ C, const float *trial, const float *__restrict__ prior,
                            const float *__restrict__ stiffness, int solve, int B, int N, int K, float *__restrict__ params,
                            double *__restrict__ ws) {
  __shared__ ShFrameLds s;
  const int b = blockIdx.x, lane = threadIdx.x, G = B / N, q = b / N;
  double *st = state + (size_t)b * St::kSize;
  double *sc = state + (size_t)B * St::kSize + (size_t)G * sh_group_doubles(K) + (size_t)b * kLmN * K;
  const double *wg = ws + (size_t)B * sh_ws_frame(K) + (size_t)q * (kShWsGroup + K);
  double *wf = ws + (size_t)b * sh_ws_frame(K);
  const bool accept = wg[0] != 0.0;
  const double lam = wg[1];
  const bool own = lane < kLmN;
  const float tq = own ? trial[(size_t)b * kLmN + lane] : 0.f;
  const double pr = !own ? 0.0 : prior ? (double)prior[(size_t)b * kLmN + lane] : st[St::kP0 + lane];
  const double mu = own && stiffness ? (double)stiffness[lane] : 0.0;
  // the accepted pose and its equations: the trial's where the group is accepted, the state's otherwise
  const double *As = accept ? A + (size_t)b * kLmN * kLmN : st + St::kA;
  for (int e = lane; e < kLmN * kLmN; e += 64) s.A[e] = As[e];
  const double *Cs = accept ? C + (size_t)b * kLmN * K : sc;
  for (int e = lane; e < kLmN * K; e += 64) s.Y[e] = Cs[e];
  const double pa = !own ? 0.0 : accept ? (double)tq : st[St::kP + lane];
  const double ga = !own ? 0.0 : accept ? g[(size_t)b * kLmN + lane] : st[St::kG + lane];
  __syncthreads();
  if (accept) {
    for (int e = lane; e < kLmN * kLmN; e += 64) st[St::kA + e] = s.A[e];
    for (int e = lane; e < kLmN * K; e += 64) sc[e] = s.Y[e];
    if (own) { st[St::kG + lane] = ga; st[St::kP + lane] = pa; }
  }
  if (own) params[(size_t)b * kLmN + lane] = (float)pa;
  if (!solve) return;
  __syncthreads();
  if (own) s.A[lane * kLmN + lane] += mu;                              // M = A + diag(mu)
  __syncthreads();
  const bool ok = lm_cholesky(s, lam, lane);
  __syncthreads();
  if (!ok) {
    if (lane == 0) wf[kShWsOk] = 0.0;
    return;
  }
  lm_forward(s, -(ga + mu * (pa - pr)), lane);
  if (lane < K) lm_columns(s, s.Y, K, lane);                           // column `lane` of Y: L y = C[:, lane], in place
  __syncthreads();
  for (int e = lane; e < kLmN * kLmN; e += 64) wf[e] = s.L[e];
  for (int e = lane; e < kLmN * K; e += 64) wf[kShWsY + e] = s.Y[e];
  if (own) wf[kShWsZ + lane] = s.x[lane];
  if (lane == 0) wf[kShWsOk] = 1.0;
}

struct ShSchurLds {
  double S[kShMaxK * kShLd], Y[kLmN * kShMaxK], z[kLmN], x[kShMaxK], piv;
  int bad;
};

__global__ void __launch_bounds__(kShThreads)
pose_lm_shared_schur_kernel(const double *__restrict__ state, const float *__restrict__ shape_prior,
                            const float *__restrict__ shape_stiffness, int B, int N, int K, float *__restrict__ trial_shape_out,
                            double *__restrict__ ws) {
  __shared__ ShSchurLds s;
  const int q = blockIdx.x, tid = threadIdx.x;
  const size_t first = (size_t)q * N;
  const double *sg = state + (size_t)B * St::kSize + (size_t)q * sh_group_doubles(K);
  double *wg = ws + (size_t)B * sh_ws_frame(K) + (size_t)q * (kShWsGroup + K);
  const double lam = wg[1];
  const bool mine = tid < K;
  const double sigma = mine ? sg[tid] : 0.0;
  if (tid == 0) s.bad = 0;
  __syncthreads();
  for (int t = tid; t < N; t += kShThreads)
    if (ws[(first + t) * sh_ws_frame(K) + kShWsOk] == 0.0) s.bad = 1;
  __syncthreads();
  bool ok = s.bad == 0;
  double rhs = 0.0;
  if (ok) {
    // S = T + lambda diag(T), T = R + diag(nu): the lower triangle
    const double nu = mine && shape_stiffness ? (double)shape_stiffness[tid] : 0.0;
    for (int e = tid; e < K * K; e += kShThreads) {
      const int k = e / K, l = e - k * K;
      if (l > k) continue;
      double v = sg[3 * K + e];
      if (l == k) {
        v += shape_stiffness ? (double)shape_stiffness[k] : 0.0;
        v += lam * v;
      }
      s.S[k * kShLd + l] = v;
    }
    if (mine) rhs = -(sg[2 * K + tid] + nu * (sigma - (shape_prior ? (double)shape_prior[(size_t)q * K + tid] : sg[K + tid])));
#pragma unroll 1
    for (int t = 0; t < N; t++) {                          // - Y_b^T Y_b and - Y_b^T z_b, frames ascending, m ascending
      const double *wf = ws + (first + t) * sh_ws_frame(K);
      __syncthreads();
      for (int e = tid; e < kLmN * K; e += kShThreads) s.Y[e] = wf[kShWsY + e];
      if (tid < kLmN) s.z[tid] = wf[kShWsZ + tid];
      __syncthreads();
      for (int e = tid; e < K * K; e += kShThreads) {
        const int k = e / K, l = e - k * K;
        if (l > k) continue;
        double v = s.S[k * kShLd + l];
#pragma unroll 2
        for (int m = 0; m < kLmN; m++) v -= s.Y[m * K + k] * s.Y[m * K + l];
        s.S[k * kShLd + l] = v;
      }
      if (mine) {
#pragma unroll 2
        for (int m = 0; m < kLmN; m++) rhs -= s.Y[m * K + tid] * s.z[m];
      }
    }
    __syncthreads();
    // S = L_s L_s^T in place, column by column, thread i owning row i
#pragma unroll 1
    for (int k = 0; k < K; k++) {
      double v = 0.0;
      if (tid >= k && mine) {
        v = s.S[tid * kShLd + k];
#pragma unroll 2
        for (int m = 0; m < k; m++) v -= s.S[tid * kShLd + m] * s.S[k * kShLd + m];
        if (tid == k) s.piv = v;
      }
      __syncthreads();
      const double d = s.piv;
      if (!(d > 0.0 && d < __builtin_inf())) { ok = false; break; }
      const double root = sqrt(d);
      if (tid >= k && mine) s.S[tid * kShLd + k] = tid == k ? root : v / root;
      __syncthreads();
    }
  }
  if (!ok) {                                               // a pivot that is not positive and finite: the whole group stays
    if (mine) trial_shape_out[(size_t)q * K + tid] = (float)sigma;
    if (tid == 0) wg[2] = 0.0;
    return;
  }
  double acc = 0.0;
#pragma unroll 1
  for (int k = 0; k < K; k++) {                            // lm_solve's substitutions at size K
    if (tid == k) s.x[k] = (rhs - acc) / s.S[k * kShLd + k];
    __syncthreads();
    if (tid > k && mine) acc += s.S[tid * kShLd + k] * s.x[k];
  }
  const double z = mine ? s.x[tid] : 0.0;
  acc = 0.0;
  __syncthreads();
#pragma unroll 1
  for (int k = K - 1; k >= 0; k--) {
    if (tid == k) s.x[k] = (z - acc) / s.S[k * kShLd + k];
    __syncthreads();
    if (tid < k) acc += s.S[k * kShLd + tid] * s.x[k];
  }
  __syncthreads();
  if (mine) {
    wg[kShWsGroup + tid] = s.x[tid];
    trial_shape_out[(size_t)q * K + tid] = (float)(sigma + s.x[tid]);
  }
}

struct ShBackLds {
  double L[kLmN * kLmN], x[kLmN], v[kShMaxK];
};

__global__ void __launch_bounds__(64)
pose_lm_shared_back_kernel(const double *__restrict__ state, int B, int N, int K, float *__restrict__ trial_out,
                           const double *__restrict__ ws) {
  __shared__ ShBackLds s;
  const int b = blockIdx.x, lane = threadIdx.x, q = b / N;
  const double *st = state + (size_t)b * St::kSize;
  const double *wg = ws + (size_t)B * sh_ws_frame(K) + (size_t)q * (kShWsGroup + K);
  const double *wf = ws + (size_t)b * sh_ws_frame(K);
  const bool own = lane < kLmN;
  const double pa = own ? st[St::kP + lane] : 0.0;
  // with a shared block the verdict is the group's (which holds every frame's); without one the frame's own
  const bool ok = K > 0 ? wg[2] != 0.0 : wf[kShWsOk] != 0.0;
  if (!ok) {
    if (own) trial_out[(size_t)b * kLmN + lane] = (float)pa;
    return;
  }
  for (int e = lane; e < kLmN * kLmN; e += 64) s.L[e] = wf[e];
  if (lane < K) s.v[lane] = wg[kShWsGroup + lane];
  __syncthreads();
  double z = own ? wf[kShWsZ + lane] : 0.0;
  if (K > 0 && own) {                                      // z - Y d sigma, k ascending
    double c = 0.0;
#pragma unroll 2
    for (int k = 0; k < K; k++) c += wf[kShWsY + lane * K + k] * s.v[k];
    z = z - c;
  }
  lm_backward(s, z, lane);
  __syncthreads();
  if (own) trial_out[(size_t)b * kLmN + lane] = (float)(pa + s.x[lane]);
}

}  // namespace shr

using namespace shr;

static bool sh_sizes(int B, int G, int K) { return B >= 0 && G >= 0 && K >= 0; }

extern "C" long long shr_pose_lm_shared_state_bytes(int B, int G, int K) {
  if (!sh_sizes(B, G, K)) return -1;
  return (long long)sh_state_doubles(B, G, K) * 8;
}

extern "C" long long shr_pose_lm_shared_workspace_bytes(int B, int G, int K) {
  if (!sh_sizes(B, G, K)) return -1;
  return (long long)sh_ws_doubles(B, G, K) * 8;
}

static int lm_shared_check(const void *state, int B, int N, int K) {
  if (!state || B < 0 || N < 1 || B % N != 0 || K < 0 || (((uintptr_t)state) & 7u) != 0) return SHR_EINVAL;
  if (B > (1 << 24) || K > kShMaxK) return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" int shr_pose_lm_shared_begin(const float *params0, const float *shape0, int B, int N, int K, float lambda0,
                                        void *state, float *trial, float *trial_shape, void *stream) {
  if (int rc = lm_shared_check(state, B, N, K)) return rc;
  if (B == 0) return SHR_OK;
  if (!params0 || !trial || !(lambda0 > 0.0f) || (K > 0 && (!shape0 || !trial_shape))) return SHR_EINVAL;
  if ((((uintptr_t)params0 | (uintptr_t)trial | (uintptr_t)shape0 | (uintptr_t)trial_shape) & 3u) != 0) return SHR_EINVAL;
  hipLaunchKernelGGL(pose_lm_shared_begin_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, params0, shape0, lambda0, B,
                     N, K, reinterpret_cast<double *>(state), trial, trial_shape);
  return (int)hipGetLastError();
}

extern "C" int shr_pose_lm_shared_step(void *state, const double *A, const double *g, const double *C, const double *R,
                                       const double *gs, const double *cost_data, const float *trial, const float *trial_shape,
                                       const float *prior, const float *stiffness, const float *shape_prior,
                                       const float *shape_stiffness, int solve, int B, int N, int K, float *trial_out,
                                       float *trial_shape_out, float *params, float *shape, float *cost, float *cost0,
                                       void *workspace, void *stream) {
  if (int rc = lm_shared_check(state, B, N, K)) return rc;
  // without a shared block and with groups of one frame: the crop's step on the state's leading part, which is that entry's own
  if (K == 0 && N == 1)
    return shr_pose_lm_step(state, A, g, cost_data, trial, prior, stiffness, solve, B, trial_out, params, cost, cost0, stream);
  if (B == 0) return SHR_OK;
  if (!A || !g || !cost_data || !trial || !params || !cost || !cost0 || !workspace || (solve && !trial_out)) return SHR_EINVAL;
  if (K > 0 && (!C || !R || !gs || !trial_shape || !shape || (solve && !trial_shape_out))) return SHR_EINVAL;
  if ((((uintptr_t)A | (uintptr_t)g | (uintptr_t)C | (uintptr_t)R | (uintptr_t)gs | (uintptr_t)cost_data | (uintptr_t)workspace) &
       7u) != 0)
    return SHR_EINVAL;
  if ((((uintptr_t)trial | (uintptr_t)trial_shape | (uintptr_t)prior | (uintptr_t)stiffness | (uintptr_t)shape_prior |
        (uintptr_t)shape_stiffness | (uintptr_t)trial_out | (uintptr_t)trial_shape_out | (uintptr_t)params | (uintptr_t)shape |
        (uintptr_t)cost | (uintptr_t)cost0) & 3u) != 0)
    return SHR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int G = B / N;
  double *st = reinterpret_cast<double *>(state), *ws = reinterpret_cast<double *>(workspace);
  hipLaunchKernelGGL(pose_lm_shared_decide_kernel, dim3((unsigned)G), dim3(64), 0, s, st, R, gs, cost_data, trial, trial_shape,
                     prior, stiffness, shape_prior, shape_stiffness, B, N, K, shape, cost, cost0, ws);
  hipLaunchKernelGGL(pose_lm_shared_frame_kernel, dim3((unsigned)B), dim3(64), 0, s, st, A, g, C, trial, prior, stiffness,
                     solve ? 1 : 0, B, N, K, params, ws);
  if (solve) {
    if (K > 0)
      hipLaunchKernelGGL(pose_lm_shared_schur_kernel, dim3((unsigned)G), dim3(kShThreads), 0, s, st, shape_prior, shape_stiffness, B,
                         N, K, trial_shape_out, ws);
    hipLaunchKernelGGL(pose_lm_shared_back_kernel, dim3((unsigned)B), dim3(64), 0, s, st, B, N, K, trial_out, ws);
  }
  return (int)hipGetLastError();
}
