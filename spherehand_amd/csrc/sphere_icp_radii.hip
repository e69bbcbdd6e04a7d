// sphere_icp_radii.hip -- the normal equations of the sphere model against observed depth points with the sphere RADII
// among the unknowns (shr_sphere_icp_radii_normal): shr_sphere_icp_normal's rows with one more column per sphere,
// d d / d r_j = -1, the radii one table per GROUP of frames (B = G N, frame b in group b / N).  The pose blocks A, g and the
// cost are that entry's; the coupling C [B,26,J], the shared block R [G,J,J] and its gradient gs [G,J] are what
// shr_pose_lm_shared_step (lm_shared.hip) takes beside them.
//
// Inverts (reference file:line): the key-point skinning of HandBallPrimitiveRender (mesh/render.py:65-88) against the
// observation of DataToModelLoss (mesh/render.py:93-142), with the radii of mesh/render.py:65-88's spheres as unknowns.
// The reference has no counterpart.
//
//   scan      sphere_icp_scan.h's, sixteen moments per sphere: sphere_icp.hip's twelve, then sum u (3, model frame) and sum d,
//             by the same one-owner-per-entry chains in the same order; the crop's radii are its group's.
//   assemble  sphere_icp_scan.h's, one workgroup per frame; then C[b,a,j] = (Jc[0,a] su_0 + Jc[1,a] su_1) + Jc[2,a] su_2 from
//             the moments and the Jacobian in LDS, and the frame's rows and sum d per sphere for the group pass.
//   group     one wave per group: R_jj = the chain over the group's frames, ascending, of the rows of sphere j (integers:
//             exact), every other entry of R an exact +0; gs_j = 0 - the chain of sum d.
//   A group with a radius that is not finite or not > 0 is void: cost = +inf, A = g = C = 0 for its frames, R = gs = 0.
#include "sphere_icp_scan.h"

namespace shr {

constexpr int kSradMom = 16;                               // doubles per sphere: the twelve, sum u (3), sum d

// (uniform over the workgroup) the group's radii hold one that is not finite or not > 0
__device__ __forceinline__ bool srad_void(const float *__restrict__ radii, int J) {
  bool bad = false;
  for (int j = 0; j < J; j++) {
    const float r = radii[j];
    bad = bad || !(r > 0.f && r < __builtin_inff());
  }
  return bad;
}

__global__ void __launch_bounds__(kNeqThreads, 4)
sphere_icp_radii_scan_kernel(const float *__restrict__ observed, const float4 *__restrict__ centres,
                             const float *__restrict__ radii, const float *__restrict__ view, int J, int N, int W, int H, float ax,
                             float bx, float ay, float by, float fg_max, float max_dist, double *__restrict__ part,
                             float *__restrict__ dist, int *__restrict__ owner) {
  __shared__ SicpLds<kSradMom> s;
  sicp_scan_body<kSradMom>(s, observed, centres, radii + (size_t)(blockIdx.z / N) * J, view, J, W, H, ax, bx, ay, by, fg_max,
                           max_dist, part, dist, owner);
}

__global__ void __launch_bounds__(kNeqThreads)
sphere_icp_radii_assemble_kernel(const double *__restrict__ part, const float *__restrict__ jac,
                                 const float *__restrict__ radii, int J, int N, int records, double *__restrict__ A,
                                 double *__restrict__ g, double *__restrict__ cost, int *__restrict__ count,
                                 double *__restrict__ moments, double *__restrict__ C, double *__restrict__ sums) {
  __shared__ SicpAsmLds<kSradMom> s;
  const int tid = threadIdx.x, b = blockIdx.x;
  const bool void_all = srad_void(radii + (size_t)(b / N) * J, J);
  sicp_assemble_body<kSradMom>(s, part, jac, J, records, void_all, A, g, cost, count, moments);
  // (the body's barrier stands between the moments and the Jacobian in LDS and these reads)
  for (int idx = tid; idx < kNeqN * J; idx += kNeqThreads) {
    const int a = idx / J, j = idx - a * J;
    const double *m = s.mom + j * kSradMom;
    const float *q = s.jac + 3 * j * kNeqN;
    double v = 0.0;                                        // a sphere without a row: an exact +0
    if (m[10] != 0.0 && !void_all)
      v = ((double)q[a] * m[12] + (double)q[kNeqN + a] * m[13]) + (double)q[2 * kNeqN + a] * m[14];
    C[(size_t)b * kNeqN * J + idx] = v;
  }
  if (tid < J) {
    sums[((size_t)b * J + tid) * 2] = s.mom[tid * kSradMom + 10];
    sums[((size_t)b * J + tid) * 2 + 1] = s.mom[tid * kSradMom + 15];
  }
}

__global__ void __launch_bounds__(kWave)
sphere_icp_radii_group_kernel(const double *__restrict__ sums, const float *__restrict__ radii, int J, int N,
                              double *__restrict__ R, double *__restrict__ gs) {
  const int q = blockIdx.x, j = threadIdx.x;
  const bool void_all = srad_void(radii + (size_t)q * J, J);
  if (j >= J) return;
  double rows = 0.0, sd = 0.0;
#pragma unroll 1
  for (int t = 0; t < N; t++) {                            // the group's frames, ascending
    const double *f = sums + (((size_t)q * N + t) * J + j) * 2;
    rows += f[0];
    sd += f[1];
  }
  for (int l = 0; l < J; l++) R[((size_t)q * J + j) * J + l] = l == j && !void_all ? rows : 0.0;
  gs[(size_t)q * J + j] = void_all ? 0.0 : 0.0 - sd;
}

static inline long long srad_part_doubles(int B, int V, int J, int W, int H) {
  return (long long)B * V * sicp_tiles(W, H) * sicp_stride<kSradMom>(J);
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_sphere_icp_radii_normal_workspace_bytes(int B, int V, int J, int W, int H) {
  if (B < 0 || V < 0 || J < 0 || W < 0 || H < 0) return -1;
  return (srad_part_doubles(B, V, J, W, H) + (long long)B * J * 2) * 8;
}

extern "C" int shr_sphere_icp_radii_normal(const float *observed, const float *view_centres, const float *radii,
                                           const float *view, const float *jac, int B, int V, int J, int W, int H, int N, float ax,
                                           float bx, float ay, float by, float fg_max, float max_dist, double *A, double *g,
                                           double *cost, int32_t *count, double *C, double *R, double *gs, double *moments,
                                           float *dist, int32_t *owner, void *workspace, void *stream) {
  if (int rc = sicp_check(B, V, J, W, H, max_dist)) return rc;
  if (N < 1 || B % N != 0) return SHR_EINVAL;
  if (B == 0) return SHR_OK;
  if (!observed || !view_centres || !radii || !view || !jac || !A || !g || !cost || !count || !C || !R || !gs || !workspace)
    return SHR_EINVAL;
  if (!neq_aligned(4, observed, radii, view, jac, count, dist, owner) || !neq_aligned(8, A, g, cost, C, R, gs, moments) ||
      !neq_aligned(16, view_centres, workspace))
    return SHR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (int)sicp_tiles(W, H);
  double *part = reinterpret_cast<double *>(workspace);
  double *sums = part + srad_part_doubles(B, V, J, W, H);
  hipLaunchKernelGGL(sphere_icp_radii_scan_kernel, dim3((unsigned)tiles, (unsigned)V, (unsigned)B), dim3(kNeqThreads), 0, s,
                     observed, reinterpret_cast<const float4 *>(view_centres), radii, view, J, N, W, H, ax, bx, ay, by, fg_max,
                     max_dist, part, dist, owner);
  hipLaunchKernelGGL(sphere_icp_radii_assemble_kernel, dim3((unsigned)B), dim3(kNeqThreads), 0, s, part, jac, radii, J, N,
                     V * tiles, A, g, cost, count, moments, C, sums);
  hipLaunchKernelGGL(sphere_icp_radii_group_kernel, dim3((unsigned)(B / N)), dim3(kWave), 0, s, sums, radii, J, N, R, gs);
  return (int)hipGetLastError();
}
