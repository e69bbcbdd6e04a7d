// sphere_icp.hip -- the Gauss-Newton normal equations of the sphere model against observed depth points
// (shr_sphere_icp_normal): per data point the owning sphere, min_j | |p - c_j| - r_j |, the signed residual and its unit
// direction, summed per sphere into ten moments; A and g are then formed from the moments and the centres' Jacobian.
//
// Inverts (reference file:line): HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by the
// key-point skinning of HandBallPrimitiveRender (mesh/render.py:65-88), against the observation of DataToModelLoss
// (mesh/render.py:93-142), whose distance this is.  The reference has no counterpart.
//
//   scan, assemble   sphere_icp_scan.h's bodies with twelve moments per sphere -- [uu^T (6) | d u (3) | d^2 | rows | 0] -- which
//             the entry with radius columns (sphere_icp_radii.hip) shares: the launch shapes, the record in LDS, the
//             one-owner-per-entry chains and the (hi, lo) cost are described there, once.
#include "sphere_icp_scan.h"

namespace shr {

constexpr int kSicpMom = 12;                               // doubles per sphere: the layout of `moments`

__global__ void __launch_bounds__(kNeqThreads, 4)
sphere_icp_scan_kernel(const float *__restrict__ observed, const float4 *__restrict__ centres, const float *__restrict__ radii,
                       const float *__restrict__ view, int J, int W, int H, float ax, float bx, float ay, float by, float fg_max,
                       float max_dist, double *__restrict__ part, float *__restrict__ dist, int *__restrict__ owner) {
  __shared__ SicpLds<kSicpMom> s;
  sicp_scan_body<kSicpMom>(s, observed, centres, radii, view, J, W, H, ax, bx, ay, by, fg_max, max_dist, part, dist, owner);
}

__global__ void __launch_bounds__(kNeqThreads)
sphere_icp_assemble_kernel(const double *__restrict__ part, const float *__restrict__ jac, int J, int records,
                           double *__restrict__ A, double *__restrict__ g, double *__restrict__ cost, int *__restrict__ count,
                           double *__restrict__ moments) {
  __shared__ SicpAsmLds<kSicpMom> s;
  sicp_assemble_body<kSicpMom>(s, part, jac, J, records, false, A, g, cost, count, moments);
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_sphere_icp_normal_workspace_bytes(int B, int V, int J, int W, int H) {
  if (B < 0 || V < 0 || J < 0 || W < 0 || H < 0) return -1;
  return (long long)B * V * sicp_tiles(W, H) * sicp_stride<kSicpMom>(J) * 8;
}

extern "C" int shr_sphere_icp_normal(const float *observed, const float *view_centres, const float *radii, const float *view,
                                     const float *jac, int B, int V, int J, int W, int H, float ax, float bx, float ay, float by,
                                     float fg_max, float max_dist, double *A, double *g, double *cost, int32_t *count,
                                     double *moments, float *dist, int32_t *owner, void *workspace, void *stream) {
  if (int rc = sicp_check(B, V, J, W, H, max_dist)) return rc;
  if (B == 0) return SHR_OK;
  if (!observed || !view_centres || !radii || !view || !jac || !A || !g || !cost || !count || !workspace) return SHR_EINVAL;
  if (!neq_aligned(4, observed, radii, view, jac, count, dist, owner) || !neq_aligned(8, A, g, cost, moments) ||
      !neq_aligned(16, view_centres, workspace))
    return SHR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (int)sicp_tiles(W, H);
  double *part = reinterpret_cast<double *>(workspace);
  hipLaunchKernelGGL(sphere_icp_scan_kernel, dim3((unsigned)tiles, (unsigned)V, (unsigned)B), dim3(kNeqThreads), 0, s, observed,
                     reinterpret_cast<const float4 *>(view_centres), radii, view, J, W, H, ax, bx, ay, by, fg_max, max_dist, part,
                     dist, owner);
  hipLaunchKernelGGL(sphere_icp_assemble_kernel, dim3((unsigned)B), dim3(kNeqThreads), 0, s, part, jac, J, V * tiles, A, g, cost,
                     count, moments);
  return (int)hipGetLastError();
}
