// pose_icp.hip -- the pose fitted to observed depth points: the Gauss-Newton normal equations of the mesh data-to-model
// distance with respect to the 26 pose parameters (shr_pose_icp_normal), and the Levenberg-Marquardt bookkeeping around
// them, kept on the device (shr_pose_lm_begin / shr_pose_lm_step).
//
// Inverts (reference file:line): HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by
// LinearBlendSkinning.forward (mesh/pointTransformation.py:39-46), against the observation of DataToModelLoss
// (mesh/render.py:93-142) taken to the triangles (shr_mesh_d2m_fwd).  The reference has no counterpart.
//
//   tiles    a workgroup of 256 threads owns kIcpTilePix consecutive pixels of one crop.  Wave 0 forms the crop's bone
//            transforms and the finger tangents in LDS (fk_rows.h: pose_ik.hip's machinery).  Four rounds of 256 pixels:
//            a thread takes one pixel, recomputes the closest point on its saved face in fp64 (d2m_tap.h: what
//            shr_mesh_d2m_bwd does) and leaves the row J = d dist / d params in LDS, fp32: with cm = -w_k u in the model
//            frame, a skin entry (bone, wv) of corner k at pos = T_bone wv adds cm . (omega x (pos - wv.w t)) to a palm
//            angle (as omega . ((pos - wv.w t) x cm): one cross product per entry), wv.w cm to the translation and
//            cm . (dT wv) to the bone's finger angles.  Nothing is assumed about which fingers a row touches.  Then thread
//            t sums entry t (and t + 256) of [A's lower triangle | g | cost | count] over the round's pixels in pixel order.
//   reduce   one workgroup per crop adds the tiles' sums in tile order and writes A (both triangles), g, cost, count.
//            (Both bodies are icp_tile.h's, which the multi-view entry of pose_icp_views.hip shares.)
//   lm       one wave per crop: the accept test, lambda, and lm_solve.h's damped solve -- pose_ik.hip's iteration, split
//            where the cost evaluation needs other kernels.
#include "icp_tile.h"
#include "lm_state.h"

namespace shr {

__global__ void __launch_bounds__(kIcpThreads)
pose_icp_tiles_kernel(const float *__restrict__ observed, const float4 *__restrict__ vertices, const int *__restrict__ faces,
                      const float *__restrict__ dist, const int *__restrict__ face, const float *__restrict__ params,
                      const float *__restrict__ offset, const float *__restrict__ offset_inv, const int *__restrict__ vstart,
                      const int *__restrict__ sbone, const float4 *__restrict__ swv, float sx, int NV, int F, int W, int H,
                      float ax, float bx, float ay, float by, float fg_max, float max_dist, double *__restrict__ part) {
  const int b = blockIdx.y;
  icp_tile_body<false>(observed, vertices, faces, dist, face, params, offset, offset_inv, vstart, sbone, swv, sx, NV, F, W, H, ax,
                       bx, ay, by, fg_max, max_dist, b, (size_t)b, nullptr, part);
}

__global__ void __launch_bounds__(kIcpSlots)
pose_icp_reduce_kernel(const double *__restrict__ part, int tiles, double *__restrict__ A, double *__restrict__ g,
                       double *__restrict__ cost, int *__restrict__ count) {
  icp_reduce_body(part, tiles, (int)blockIdx.x, (int)threadIdx.x, A, g, cost, count);
}

using St = LmCropState;              // a crop's state: lm_state.h's frame without E, the crop its own unit of decision

__global__ void __launch_bounds__(64)
pose_lm_begin_kernel(const float *__restrict__ params0, float lambda0, double *__restrict__ state, float *__restrict__ trial) {
  const int b = blockIdx.x;
  lm_begin_frame<St>(params0, lambda0, state + (size_t)b * St::kSize, trial, (size_t)b, (int)threadIdx.x);
}

struct LmLds {
  double A[kLmN * kLmN], L[kLmN * kLmN], x[kLmN], piv;
};

__global__ void __launch_bounds__(64)
pose_lm_step_kernel(double *__restrict__ state, const double *__restrict__ A, const double *__restrict__ g,
                    const double *__restrict__ cost_data, const float *trial, const float *__restrict__ prior,
                    const float *__restrict__ stiffness, int solve, float *trial_out, float *__restrict__ params,
                    float *__restrict__ cost, float *__restrict__ cost0) {
  __shared__ LmLds s;
  const int b = blockIdx.x, lane = threadIdx.x;
  double *st = state + (size_t)b * St::kSize;
  const bool own = lane < kLmN;
  const double mu = own && stiffness ? (double)stiffness[lane] : 0.0;
  const LmBook bk = lm_book<St>(st);
  const double total = lm_frames_total<St>(s, state, (size_t)b, 1, cost_data, trial, prior, mu, lane);
  const float tq = own ? trial[(size_t)b * kLmN + lane] : 0.f;
  const double pr = !own ? 0.0 : prior ? (double)prior[(size_t)b * kLmN + lane] : st[St::kP0 + lane];
  const LmDecision dec = lm_decide(bk, total);
  const bool accept = dec.accept;
  const double lam = dec.lam;
  // the accepted pose and its equations: the trial's where it is accepted, the state's otherwise -- all read before the state is written
  const double *As = accept ? A + (size_t)b * kLmN * kLmN : st + St::kA;
  for (int e = lane; e < kLmN * kLmN; e += 64) s.A[e] = As[e];
  const double pa = !own ? 0.0 : accept ? (double)tq : st[St::kP + lane];
  const double ga = !own ? 0.0 : accept ? g[(size_t)b * kLmN + lane] : st[St::kG + lane];
  __syncthreads();
  if (accept) {
    for (int e = lane; e < kLmN * kLmN; e += 64) st[St::kA + e] = s.A[e];
    if (own) { st[St::kG + lane] = ga; st[St::kP + lane] = pa; }
  }
  if (lane == 0) lm_record<St>(st, bk, total, dec, cost + b, cost0 + b);
  if (own) params[(size_t)b * kLmN + lane] = (float)pa;
  if (!solve) return;
  __syncthreads();
  if (own) s.A[lane * kLmN + lane] += mu;                              // M = A + diag(mu)
  __syncthreads();
  const bool ok = lm_cholesky(s, lam, lane);
  __syncthreads();
  if (ok) lm_solve(s, -(ga + mu * (pa - pr)), lane);
  if (own) trial_out[(size_t)b * kLmN + lane] = ok ? (float)(pa + s.x[lane]) : (float)pa;
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_pose_icp_normal_workspace_bytes(int B, int W, int H) {
  if (B < 0 || W < 0 || H < 0) return -1;
  return (long long)B * icp_tiles(W, H) * kIcpSlots * 8;
}

extern "C" int shr_pose_icp_normal(const float *observed, const float *vertices, const int32_t *faces, const float *dist,
                                   const int32_t *face, const float *params, const float *offset, const float *offset_inv,
                                   const int32_t *skin_vertex_start, const int32_t *skin_bone, const float *skin_wv,
                                   int right_hand, int B, int NV, int F, int W, int H, float ax, float bx, float ay, float by,
                                   float fg_max, float max_dist, double *A, double *g, double *cost, int32_t *count,
                                   void *workspace, void *stream) {
  if (int rc = d2m_check(B, NV, F, W, H, max_dist)) return rc;
  if (B == 0) return SHR_OK;
  if (!observed || !vertices || (!faces && F > 0) || !dist || !face || !skin_vertex_start || !skin_bone || !skin_wv || !A || !g ||
      !cost || !count || !workspace)
    return SHR_EINVAL;
  if (int rc = fk_check(params, B, offset, offset_inv)) return rc;
  if ((((uintptr_t)observed | (uintptr_t)faces | (uintptr_t)dist | (uintptr_t)face | (uintptr_t)params |
        (uintptr_t)skin_vertex_start | (uintptr_t)skin_bone | (uintptr_t)count) & 3u) != 0)
    return SHR_EINVAL;
  if ((((uintptr_t)A | (uintptr_t)g | (uintptr_t)cost) & 7u) != 0) return SHR_EINVAL;
  if ((((uintptr_t)vertices | (uintptr_t)skin_wv | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  if ((long long)B * NV > (1LL << 30)) return SHR_ETOOLARGE;
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (int)icp_tiles(W, H);
  double *part = reinterpret_cast<double *>(workspace);
  hipLaunchKernelGGL(pose_icp_tiles_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(kIcpThreads), 0, s, observed,
                     reinterpret_cast<const float4 *>(vertices), faces, dist, face, params, offset, offset_inv,
                     skin_vertex_start, skin_bone, reinterpret_cast<const float4 *>(skin_wv), right_hand ? -1.0f : 1.0f, NV, F,
                     W, H, ax, bx, ay, by, fg_max, max_dist, part);
  hipLaunchKernelGGL(pose_icp_reduce_kernel, dim3((unsigned)B), dim3(kIcpSlots), 0, s, part, tiles, A, g, cost, count);
  return (int)hipGetLastError();
}

extern "C" long long shr_pose_lm_state_bytes(int B) {
  if (B < 0) return -1;
  return (long long)B * St::kSize * 8;
}

extern "C" int shr_pose_lm_begin(const float *params0, int B, float lambda0, void *state, float *trial, void *stream) {
  if (B == 0) return SHR_OK;
  if (int rc = lm_check(state, B, 1)) return rc;
  if (!params0 || !trial || !(lambda0 > 0.0f) || (((uintptr_t)params0 | (uintptr_t)trial) & 3u) != 0) return SHR_EINVAL;
  hipLaunchKernelGGL(pose_lm_begin_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, params0, lambda0,
                     reinterpret_cast<double *>(state), trial);
  return (int)hipGetLastError();
}

extern "C" int shr_pose_lm_step(void *state, const double *A, const double *g, const double *cost_data, const float *trial,
                                const float *prior, const float *stiffness, int solve, int B, float *trial_out, float *params,
                                float *cost, float *cost0, void *stream) {
  if (B == 0) return SHR_OK;
  if (int rc = lm_check(state, B, 1)) return rc;
  if (!A || !g || !cost_data || !trial || !params || !cost || !cost0 || (solve && !trial_out)) return SHR_EINVAL;
  if ((((uintptr_t)A | (uintptr_t)g | (uintptr_t)cost_data) & 7u) != 0) return SHR_EINVAL;
  if ((((uintptr_t)trial | (uintptr_t)prior | (uintptr_t)stiffness | (uintptr_t)trial_out | (uintptr_t)params | (uintptr_t)cost |
        (uintptr_t)cost0) & 3u) != 0)
    return SHR_EINVAL;
  hipLaunchKernelGGL(pose_lm_step_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<double *>(state),
                     A, g, cost_data, trial, prior, stiffness, solve ? 1 : 0, trial_out, params, cost, cost0);
  return (int)hipGetLastError();
}
