// lm_state.h -- what every Levenberg-Marquardt step entry keeps on the device and decides the same way (pose_icp.hip's
// shr_pose_lm_step per crop; lm_band.h's sequence steps per sequence; lm_shared.hip's per group): the layout of a frame's
// state, the begin kernel's writes, the cost chain over a unit's frames, the accept rule with lambda, lane 0's record of the
// decision, and the host's check of the state's arguments.  ONE wave per unit of decision, lane i owning parameter i.
#pragma once
#include "lm_solve.h"

namespace shr {

// A frame's state, in doubles: the accepted pose's A [26 x 26], with kWithE its E [26 x 26] (the block that couples the frame to
// the next one), g [26], the pose itself, params0; then -- used in the FIRST frame of a unit of decision only (the crop, the
// sequence, the group) -- the unit's total cost, lambda, `fresh` (no step since begin), `moved` (a trial has been accepted
// since begin), the accept and reject counters.  760 doubles without E, 1440 with.
template <bool kWithE>
struct LmState {
  static constexpr int kA = 0, kE = kLmN * kLmN, kG = (kWithE ? 2 : 1) * kLmN * kLmN, kP = kG + kLmN, kP0 = kP + kLmN,
                       kCost = kP0 + kLmN, kLambda = kCost + 1, kFresh = kCost + 2, kMoved = kCost + 3, kAccepts = kCost + 4,
                       kRejects = kCost + 5, kSize = kWithE ? 1440 : 760;
  static_assert(kRejects < kSize && kSize % 8 == 0, "the state's fields");
};
using LmCropState = LmState<false>;  // shr_pose_lm_step's, and lm_shared.hip's frames: with K == 0 and N == 1 that entry hands
                                     // its state to shr_pose_lm_step as it is
using LmSeqState = LmState<true>;    // both sequence steps': without F shr_pose_lm_seq2_step hands its state and its workspace
                                     // to shr_pose_lm_seq_step as they are
// A frame's workspace of the sequence steps, in doubles: L_t [26 x 26], W_t transposed [26 x 26], y_t [26], padded to a
// multiple of 8.  Behind ALL the frames' states the pentadiagonal step keeps the accepted F of every frame, and behind all
// their workspaces V_t transposed: kLmBlock doubles each ([26 x 26], padded to a multiple of 8).
constexpr int kLmWsL = 0, kLmWsW = kLmN * kLmN, kLmWsY = 2 * kLmN * kLmN, kLmWs = 1384, kLmBlock = 680;
static_assert(kLmWsY + kLmN <= kLmWs && kLmWs % 8 == 0, "the workspace's fields");
static_assert(kLmN * kLmN <= kLmBlock && kLmBlock % 8 == 0, "the F and V blocks");
// the sizes the header documents and the *_bytes entries return: a field added here must not move them silently
static_assert(LmCropState::kSize == 760 && LmSeqState::kSize == 1440 && LmSeqState::kG - LmCropState::kG == kLmN * kLmN,
              "the two layouts");

// The begin kernels' frame: the equations zeroed, the pose and params0, trial = params0, no cost yet
template <class St>
__device__ __forceinline__ void lm_begin_frame(const float *__restrict__ params0, float lambda0, double *__restrict__ st,
                                               float *__restrict__ trial, size_t b, int lane) {
  for (int e = lane; e < St::kP; e += 64) st[e] = 0.0;
  if (lane < kLmN) {
    const float p = params0[b * kLmN + lane];
    st[St::kP + lane] = st[St::kP0 + lane] = (double)p;
    trial[b * kLmN + lane] = p;
  }
  if (lane == 0) {
    st[St::kCost] = __builtin_inf();
    st[St::kLambda] = (double)lambda0;
    st[St::kFresh] = 1.0;
    st[St::kMoved] = st[St::kAccepts] = st[St::kRejects] = 0.0;
  }
}

// The unit's fields as a step finds them (sq: the unit's first frame), read before anything is written
struct LmBook {
  double cur, lam0;
  bool fresh, moved;
  double accepts, rejects;
};
template <class St>
__device__ __forceinline__ LmBook lm_book(const double *sq) {
  return {sq[St::kCost], sq[St::kLambda], sq[St::kFresh] != 0.0, sq[St::kMoved] != 0.0, sq[St::kAccepts], sq[St::kRejects]};
}

// total: the chain over the unit's n frames from `first`, ascending, of a frame's total: cost_data + mu_i (trial_i -
// prior_i)^2, i ascending (prior NULL: params0).  s.x [>= 26] is the wave's; every lane returns the total.
template <class St, class S>
__device__ __forceinline__ double lm_frames_total(S &s, const double *state, size_t first, int n,
                                                  const double *__restrict__ cost_data, const float *trial,
                                                  const float *__restrict__ prior, double mu, int lane) {
  double total = 0.0;
#pragma unroll 1
  for (int t = 0; t < n; t++) {
    const size_t f = first + t;
    if (lane < kLmN) {
      const double pr = prior ? (double)prior[f * kLmN + lane] : state[f * St::kSize + St::kP0 + lane];
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
  return total;
}

// The accept rule and the next lambda
struct LmDecision {
  bool accept;
  double lam;
};
__device__ __forceinline__ LmDecision lm_decide(const LmBook &bk, double total) {
  const bool accept = total < bk.cur && total > -__builtin_inf();     // (false for a NaN, and for +inf)
  return {accept, fmin(fmax(bk.lam0 * (accept ? (bk.moved ? 0.3 : 1.0) : 10.0), 1e-9), 1e6)};
}

// Lane 0's record of the decision: the unit's fields, cost, and cost0 on the first step after begin
template <class St>
__device__ __forceinline__ void lm_record(double *sq, const LmBook &bk, double total, const LmDecision &d, float *cost,
                                          float *cost0) {
  sq[St::kCost] = d.accept ? total : bk.cur;
  sq[St::kLambda] = d.lam;
  sq[St::kFresh] = 0.0;
  sq[St::kMoved] = (bk.moved || d.accept) ? 1.0 : 0.0;
  sq[St::kAccepts] = bk.accepts + (d.accept ? 1.0 : 0.0);
  sq[St::kRejects] = bk.rejects + (d.accept ? 0.0 : 1.0);
  *cost = (float)(d.accept ? total : bk.cur);
  if (bk.fresh) *cost0 = (float)total;
}

// The host's check of a state for B frames in units of T (the crop step: T = 1)
inline int lm_check(const void *state, int B, int T) {
  if (!state || B < 0 || T < 1 || B % T != 0 || (((uintptr_t)state) & 7u) != 0) return SHR_EINVAL;
  if (B > (1 << 24)) return SHR_ETOOLARGE;
  return SHR_OK;
}

}  // namespace shr
