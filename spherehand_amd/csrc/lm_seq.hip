// lm_seq.hip -- the sequence step of the Levenberg-Marquardt loop for BLOCK-TRIDIAGONAL normal equations
// (shr_pose_lm_seq_begin / shr_pose_lm_seq_step): B = S T frames, one lambda, one cost and one accept decision per sequence,
// and the damped solve of the system a term that couples consecutive frames leaves (sphere_temporal.hip's E).
//
// Inverts (reference file:line): the energy of TemporalSmoothnessLoss (network/util_modules.py:360-381) beside the
// per-frame terms; the reference has no counterpart of the solve.
//
// The kernels are lm_band.h's bodies with kBand2 = false, where the mathematics, the order of every sum and the LDS
// (16 648 bytes) are described; the state and the workspace are lm_state.h's.  This unit holds the kernels' names, the sizes
// and the entries with their argument rules.
#include "lm_band.h"

namespace shr {

__global__ void __launch_bounds__(64)
pose_lm_seq_begin_kernel(const float *__restrict__ params0, float lambda0, double *__restrict__ state, float *__restrict__ trial) {
  lm_band_begin_body<false>(params0, lambda0, state, trial);
}

__global__ void __launch_bounds__(64)
pose_lm_seq_step_kernel(double *__restrict__ state, const double *__restrict__ A, const double *__restrict__ g,
                        const double *__restrict__ E, const double *__restrict__ cost_data, const float *trial,
                        const float *__restrict__ prior, const float *__restrict__ stiffness, int solve, int T, float *trial_out,
                        float *__restrict__ params, float *__restrict__ cost, float *__restrict__ cost0,
                        double *__restrict__ ws) {
  lm_band_step_body<false>(state, A, g, E, nullptr, cost_data, trial, prior, stiffness, solve, T, trial_out, params, cost, cost0, ws);
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_pose_lm_seq_state_bytes(int B) {
  if (B < 0) return -1;
  return (long long)B * LmSeqState::kSize * 8;
}

extern "C" long long shr_pose_lm_seq_workspace_bytes(int B) {
  if (B < 0) return -1;
  return (long long)B * kLmWs * 8;
}

extern "C" int shr_pose_lm_seq_begin(const float *params0, int B, int T, float lambda0, void *state, float *trial, void *stream) {
  if (int rc = lm_check(state, B, T)) return rc;
  if (B == 0) return SHR_OK;
  if (!params0 || !trial || !(lambda0 > 0.0f) || (((uintptr_t)params0 | (uintptr_t)trial) & 3u) != 0) return SHR_EINVAL;
  hipLaunchKernelGGL(pose_lm_seq_begin_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, params0, lambda0,
                     reinterpret_cast<double *>(state), trial);
  return (int)hipGetLastError();
}

extern "C" int shr_pose_lm_seq_step(void *state, const double *A, const double *g, const double *E, const double *cost_data,
                                    const float *trial, const float *prior, const float *stiffness, int solve, int B, int T,
                                    float *trial_out, float *params, float *cost, float *cost0, void *workspace, void *stream) {
  if (int rc = lm_check(state, B, T)) return rc;
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
