// lm_band.h -- the sequence step of the Levenberg-Marquardt loop, stated once for both of its bandwidths: lm_state.h's
// bookkeeping with the unit of decision raised from the crop to the SEQUENCE (B = S T frames, the T frames of a sequence
// adjacent, one lambda, one cost and one accept decision per sequence) and the damped solve of the BANDED normal equations
// that terms coupling consecutive frames leave.  lm_seq.hip wraps the body with kBand2 = false (block-TRIdiagonal:
// sphere_temporal.hip's E), lm_seq2.hip with kBand2 = true (block-PENTAdiagonal: sphere_accel.hip's E and F); everything
// that touches F, V, the cross product C or y2 is under `if constexpr (kBand2)`, so the tridiagonal kernel carries none.
//
//   one workgroup of ONE wave per sequence, lane i owning row i of the frame's 26 unknowns, as lm_solve.h's solve does; the
//   frames are taken one after the other, so a sequence is a latency chain of T frames.
//   total     lm_state.h's chain over t ascending; accept, lambda and the counters are shr_pose_lm_step's rules on the
//             sequence's total.
//   keep      on accept every frame's A, E, (F,) g and trial go to the state; params is the state's pose.
//   factor    block Cholesky, forward over t:
//             D_t = (M_t + lambda diag M_t) - W_{t-1} W_{t-1}^T (- V_{t-2} V_{t-2}^T), M_t = A_t + diag(mu): per entry the W
//             product is subtracted first, then the V product, each m ascending, then lm_solve.h's column recurrence;
//             L_t L_t^T = D_t;  L_t y_t = r_t - W_{t-1} y_{t-1} (- V_{t-2} y_{t-2});
//             W_t = (E_t^T (- V_{t-1} W_{t-1}^T)) L_t^-T for t <= T - 2;  V_t = F_t^T L_t^-T for t <= T - 3;
//             each of W_t and V_t by lm_solve.h's 26 triangular solves side by side, lane i owning row i.  L_t, W_t, y_t
//             and, behind them, V_t go to the workspace.
//   back      backward over t: L_t^T x_t = y_t - W_t^T x_{t+1} (- V_t^T x_{t+2}); trial_out = (float)(p + x).
//   Everything fp64, every sum in index order, the W term before the V term.  With T = 1 every operation is
//   shr_pose_lm_step's in its order: the same bits.  A pivot that is not positive and finite: trial_out = p on the whole
//   sequence.
//   LDS: A, L, W [26 x 26] and x, y [26] in fp64 and the pivot: 16 648 bytes; with the second band also the two previous V
//   blocks, the cross product [26 x 26] and the y (or x) before the last [26]: 33 080 bytes.  W and V are held TRANSPOSED
//   (W[k * 26 + i] = W_t[i][k]), so that the lanes of the triangular solves and of the outer products read consecutive
//   doubles.
#pragma once
#include "lm_state.h"

namespace shr {

template <bool kBand2>
struct LmBandLds;
template <>
struct LmBandLds<false> {
  double A[kLmN * kLmN], L[kLmN * kLmN], W[kLmN * kLmN], x[kLmN], y[kLmN], piv;
};
template <>
struct LmBandLds<true> {
  double A[kLmN * kLmN], L[kLmN * kLmN], W[kLmN * kLmN], V[2][kLmN * kLmN], C[kLmN * kLmN], x[kLmN], y[kLmN], y2[kLmN], piv;
};

// L L^T = A + lam diag(A) - W W^T (with `prev`) - V V^T, V = s.V[v2] (with the second band and v2 >= 0), lm_cholesky's
// recurrence.  false: a pivot that is not positive and finite.
template <bool kBand2>
__device__ __forceinline__ bool lm_band_cholesky(LmBandLds<kBand2> &s, double lam, int lane, bool prev, int v2) {
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
      if constexpr (kBand2) {
        if (v2 >= 0) {
          const double *V2 = s.V[v2];
#pragma unroll 2
          for (int m = 0; m < kLmN; m++) v -= V2[m * kLmN + lane] * V2[m * kLmN + k];
        }
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

// One workgroup per FRAME: lm_state.h's begin; with the second band the frame's F block, behind all the frames, zeroed too
template <bool kBand2>
__device__ __forceinline__ void lm_band_begin_body(const float *__restrict__ params0, float lambda0, double *__restrict__ state,
                                                   float *__restrict__ trial) {
  using St = LmSeqState;
  const int b = blockIdx.x, lane = threadIdx.x;
  lm_begin_frame<St>(params0, lambda0, state + (size_t)b * St::kSize, trial, (size_t)b, lane);
  if constexpr (kBand2) {
    double *stF = state + (size_t)gridDim.x * St::kSize + (size_t)b * kLmBlock;
    for (int e = lane; e < kLmBlock; e += 64) stF[e] = 0.0;
  }
}

// One workgroup per SEQUENCE.  F is read with kBand2 only.
template <bool kBand2>
__device__ __forceinline__ void lm_band_step_body(double *__restrict__ state, const double *__restrict__ A,
                                                  const double *__restrict__ g, const double *__restrict__ E,
                                                  const double *__restrict__ F, const double *__restrict__ cost_data,
                                                  const float *trial, const float *__restrict__ prior,
                                                  const float *__restrict__ stiffness, int solve, int T, float *trial_out,
                                                  float *__restrict__ params, float *__restrict__ cost,
                                                  float *__restrict__ cost0, double *__restrict__ ws) {
  using St = LmSeqState;
  constexpr int kNN = kLmN * kLmN;
  __shared__ LmBandLds<kBand2> s;
  const int q = blockIdx.x, lane = threadIdx.x;
  const size_t first = (size_t)q * T;
  double *sq = state + first * St::kSize;                  // the sequence's fields live in its first frame
  double *stF = state + (size_t)gridDim.x * T * St::kSize; // the accepted F of every frame, after the frames' own fields
  double *wsV = ws + (size_t)gridDim.x * T * kLmWs;        // V_t of every frame, after the frames' L_t, W_t, y_t
  const bool own = lane < kLmN;
  const double mu = own && stiffness ? (double)stiffness[lane] : 0.0;
  const LmBook bk = lm_book<St>(sq);
  const double total = lm_frames_total<St>(s, state, first, T, cost_data, trial, prior, mu, lane);
  const LmDecision dec = lm_decide(bk, total);
  const bool accept = dec.accept;
  const double lam = dec.lam;
  // keep: the trial's equations and poses become the state's where the sequence is accepted
#pragma unroll 1
  for (int t = 0; t < T; t++) {
    const size_t f = first + t;
    double *st = state + f * St::kSize;
    if (accept) {
      for (int e = lane; e < kNN; e += 64) st[St::kA + e] = A[f * kNN + e];
      if (E)
        for (int e = lane; e < kNN; e += 64) st[St::kE + e] = E[f * kNN + e];
      if constexpr (kBand2)
        for (int e = lane; e < kNN; e += 64) stF[f * kLmBlock + e] = F[f * kNN + e];
      if (own) {
        st[St::kG + lane] = g[f * kLmN + lane];
        st[St::kP + lane] = (double)trial[f * kLmN + lane];
      }
    }
    if (own) params[f * kLmN + lane] = (float)(accept ? (double)trial[f * kLmN + lane] : st[St::kP + lane]);
  }
  if (lane == 0) lm_record<St>(sq, bk, total, dec, cost + q, cost0 + q);
  if (!solve) return;
  __syncthreads();                                         // the state written above is read below
  bool ok = true;
  int v1 = 0;                                              // s.V[v1] is V_{t-1}, s.V[1 - v1] V_{t-2}, transposed
  // factor, forward over t
#pragma unroll 1
  for (int t = 0; t < T && ok; t++) {
    const size_t f = first + t;
    const double *st = state + f * St::kSize;
    double *wf = ws + f * kLmWs;
    for (int e = lane; e < kNN; e += 64) s.A[e] = st[St::kA + e];
    const double pa = own ? st[St::kP + lane] : 0.0, ga = own ? st[St::kG + lane] : 0.0;
    const double pr = !own ? 0.0 : prior ? (double)prior[f * kLmN + lane] : st[St::kP0 + lane];
    __syncthreads();
    if (own) s.A[lane * kLmN + lane] += mu;                // M = A + diag(mu)
    __syncthreads();
    const bool far = kBand2 && t > 1;                      // V_{t-2} exists
    ok = lm_band_cholesky(s, lam, lane, t > 0, far ? 1 - v1 : -1);
    __syncthreads();
    if (!ok) break;
    double rhs = -(ga + mu * (pa - pr));
    if (t > 0 && own) {                                    // r_t - W_{t-1} y_{t-1}
      double c = 0.0;
#pragma unroll 2
      for (int k = 0; k < kLmN; k++) c += s.W[k * kLmN + lane] * s.y[k];
      rhs = rhs - c;
    }
    if constexpr (kBand2) {
      if (far && own) {                                    // ... - V_{t-2} y_{t-2}
        double c = 0.0;
#pragma unroll 2
        for (int k = 0; k < kLmN; k++) c += s.V[1 - v1][k * kLmN + lane] * s.y2[k];
        rhs = rhs - c;
      }
    }
    __syncthreads();
    lm_forward(s, rhs, lane);
    if (own) {
      if constexpr (kBand2)
        if (t > 0) s.y2[lane] = s.y[lane];
      s.y[lane] = s.x[lane];
    }
    if (t < T - 1) {
      if (kBand2 && t > 0) {                               // E_t^T - V_{t-1} W_{t-1}^T, lane i its column i of the transposed block
        if constexpr (kBand2) {
          if (own) {
#pragma unroll 1
            for (int k = 0; k < kLmN; k++) {
              double c = 0.0;
#pragma unroll 2
              for (int m = 0; m < kLmN; m++) c += s.V[v1][m * kLmN + lane] * s.W[m * kLmN + k];
              s.C[k * kLmN + lane] = st[St::kE + k * kLmN + lane] - c;
            }
          }
          __syncthreads();                                 // every lane has read the previous W
          for (int e = lane; e < kNN; e += 64) {
            wf[kLmWsL + e] = s.L[e];
            s.W[e] = s.C[e];
          }
        }
      } else {
        for (int e = lane; e < kNN; e += 64) {
          wf[kLmWsL + e] = s.L[e];
          s.W[e] = st[St::kE + e];
        }
      }
      if (own) wf[kLmWsY + lane] = s.x[lane];
      __syncthreads();
      if (own) lm_columns(s, s.W, kLmN, lane);             // row `lane` of W_t: L_t z = (E_t^T - ...)[lane, :], in place
      __syncthreads();
      for (int e = lane; e < kNN; e += 64) wf[kLmWsW + e] = s.W[e];
    }
    if constexpr (kBand2) {
      v1 = 1 - v1;                                         // the older V leaves; V_t takes its place
      if (t < T - 2) {
        for (int e = lane; e < kNN; e += 64) s.V[v1][e] = stF[f * kLmBlock + e];
        __syncthreads();
        if (own) lm_columns(s, s.V[v1], kLmN, lane);       // row `lane` of V_t: L_t z = F_t[:, lane]
        __syncthreads();
        for (int e = lane; e < kNN; e += 64) wsV[f * kLmBlock + e] = s.V[v1][e];
      }
    }
    __syncthreads();
  }
  if (!ok) {                                               // a pivot that is not positive and finite: the whole sequence stays
    for (int t = 0; t < T; t++) {
      const size_t f = first + t;
      if (own) trial_out[f * kLmN + lane] = (float)state[f * St::kSize + St::kP + lane];
    }
    return;
  }
  // back, backward over t: s.L and s.x hold the last frame's L and y; s.y is x_{t+1}, s.y2 x_{t+2}
#pragma unroll 1
  for (int t = T - 1; t >= 0; t--) {
    const size_t f = first + t;
    double z = 0.0;
    if (t < T - 1) {
      const double *wf = ws + f * kLmWs;
      for (int e = lane; e < kNN; e += 64) {
        s.L[e] = wf[kLmWsL + e];
        s.W[e] = wf[kLmWsW + e];
      }
      const bool far = kBand2 && t < T - 2;                // V_t exists
      if constexpr (kBand2)
        if (far)
          for (int e = lane; e < kNN; e += 64) s.V[0][e] = wsV[f * kLmBlock + e];
      __syncthreads();
      if (own) {                                           // y_t - W_t^T x_{t+1}
        double c = 0.0;
#pragma unroll 2
        for (int i = 0; i < kLmN; i++) c += s.W[lane * kLmN + i] * s.y[i];
        z = wf[kLmWsY + lane] - c;
      }
      if constexpr (kBand2) {
        if (far && own) {                                  // ... - V_t^T x_{t+2}
          double c = 0.0;
#pragma unroll 2
          for (int i = 0; i < kLmN; i++) c += s.V[0][lane * kLmN + i] * s.y2[i];
          z = z - c;
        }
      }
    } else {
      z = own ? s.x[lane] : 0.0;
    }
    __syncthreads();
    lm_backward(s, z, lane);
    __syncthreads();
    if (own) {
      trial_out[f * kLmN + lane] = (float)(state[f * St::kSize + St::kP + lane] + s.x[lane]);
      if constexpr (kBand2)
        if (t < T - 1) s.y2[lane] = s.y[lane];
      s.y[lane] = s.x[lane];
    }
    __syncthreads();
  }
}

}  // namespace shr
