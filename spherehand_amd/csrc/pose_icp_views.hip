// pose_icp_views.hip -- one pose fitted to several depth views: the model-space vertices taken into every view's frame
// (shr_view_vertices_fwd) and the Gauss-Newton normal equations of the sum of all views' point-to-mesh costs with respect
// to the 26 pose parameters (shr_pose_icp_normal_views).  The search between the two is shr_mesh_d2m_fwd over the B V crops,
// the step shr_pose_lm_step: neither knows about views.
//
// Inverts (reference file:line): HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by
// LinearBlendSkinning.forward (mesh/pointTransformation.py:39-46), against the observation of DataToModelLoss
// (mesh/render.py:93-142) in each camera of MutualTransformation (mesh/multiview_utility.py:13-30).  The reference has no counterpart.
//
//   view     one thread per (sample, view, vertex): x_v = R x + t in fp32, the 4th float copied.
//   tiles    icp_tile.h's tile with kViews: one workgroup per (tile, view, sample).  params and the LDS tables are sample
//            b's; observed, dist, face and the vertices crop b V + v's.  A distance does not change under a rigid map, so
//            the row with respect to the pose needs only the closest point's unit direction taken back to the model frame,
//            u = R^T u_v; the nine entries of R are workgroup-uniform and are read from a uniform address (scalar loads).
//            __launch_bounds__(256, 4): four workgroups per CU, pose_icp.hip's residency (128 VGPRs; LDS allows four).
//   reduce   icp_tile.h's reduction over the V tiles records of a sample, laid out [b][v][tile]: tiles ascending inside a
//            view, views ascending -- the contract's order.
#include "icp_tile.h"

namespace shr {

constexpr int kViewThreads = 256;

__global__ void __launch_bounds__(kViewThreads)
view_vertices_kernel(const float4 *__restrict__ vertices, const float4 *__restrict__ view, int NV, int V,
                     float4 *__restrict__ out) {
  const int n = blockIdx.x * kViewThreads + threadIdx.x, v = blockIdx.y, b = blockIdx.z;
  if (n >= NV) return;
  const float4 *m = view + ((size_t)b * V + v) * 4;     // (uniform: scalar loads)
  const float4 m0 = m[0], m1 = m[1], m2 = m[2];
  const float4 p = vertices[(size_t)b * NV + n];
  float4 o;
  o.x = ((m0.x * p.x + m0.y * p.y) + m0.z * p.z) + m0.w;
  o.y = ((m1.x * p.x + m1.y * p.y) + m1.z * p.z) + m1.w;
  o.z = ((m2.x * p.x + m2.y * p.y) + m2.z * p.z) + m2.w;
  o.w = p.w;
  out[((size_t)b * V + v) * NV + n] = o;
}

__global__ void __launch_bounds__(kIcpThreads, 4)
pose_icp_views_tiles_kernel(const float *__restrict__ observed, const float4 *__restrict__ vertices, const int *__restrict__ faces,
                            const float *__restrict__ dist, const int *__restrict__ face, const float *__restrict__ view,
                            const float *__restrict__ params, const float *__restrict__ offset,
                            const float *__restrict__ offset_inv, const int *__restrict__ vstart, const int *__restrict__ sbone,
                            const float4 *__restrict__ swv, float sx, int NV, int F, int W, int H, float ax, float bx, float ay,
                            float by, float fg_max, float max_dist, double *__restrict__ part) {
  const int b = blockIdx.z;
  const size_t crop = (size_t)b * gridDim.y + blockIdx.y;
  icp_tile_body<true>(observed, vertices, faces, dist, face, params, offset, offset_inv, vstart, sbone, swv, sx, NV, F, W, H, ax,
                      bx, ay, by, fg_max, max_dist, b, crop, view + crop * 16, part);
}

__global__ void __launch_bounds__(kIcpSlots)
pose_icp_views_reduce_kernel(const double *__restrict__ part, int tiles, double *__restrict__ A, double *__restrict__ g,
                             double *__restrict__ cost, int *__restrict__ count) {
  icp_reduce_body(part, tiles, (int)blockIdx.x, (int)threadIdx.x, A, g, cost, count);
}

}  // namespace shr

using namespace shr;

// the rules both entries share: shr_pose_icp_normal's on B and the mesh, 1 <= V, B V <= 65535
static int views_check(int B, int V, int NV) {
  if (B < 0 || V < 1 || NV <= 0) return SHR_EINVAL;
  if (B > 65535 || (long long)B * V > 65535) return SHR_ETOOLARGE;
  if ((long long)NV * 3 >= (1LL << 31) || (long long)B * V * NV > (1LL << 30)) return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" int shr_view_vertices_fwd(const float *vertices, const float *view, int B, int V, int NV, float *out, void *stream) {
  if (int rc = views_check(B, V, NV)) return rc;
  if (B == 0) return SHR_OK;
  if (!vertices || !view || !out) return SHR_EINVAL;
  if ((((uintptr_t)vertices | (uintptr_t)view | (uintptr_t)out) & 15u) != 0) return SHR_EINVAL;
  hipLaunchKernelGGL(view_vertices_kernel, dim3((unsigned)((NV + kViewThreads - 1) / kViewThreads), (unsigned)V, (unsigned)B),
                     dim3(kViewThreads), 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(vertices),
                     reinterpret_cast<const float4 *>(view), NV, V, reinterpret_cast<float4 *>(out));
  return (int)hipGetLastError();
}

extern "C" long long shr_pose_icp_normal_views_workspace_bytes(int B, int V, int W, int H) {
  if (B < 0 || V < 0 || W < 0 || H < 0) return -1;
  return (long long)B * V * icp_tiles(W, H) * kIcpSlots * 8;
}

extern "C" int shr_pose_icp_normal_views(const float *observed, const float *view_vertices, const int32_t *faces, const float *dist,
                                         const int32_t *face, const float *view, const float *params, const float *offset,
                                         const float *offset_inv, const int32_t *skin_vertex_start, const int32_t *skin_bone,
                                         const float *skin_wv, int right_hand, int B, int V, int NV, int F, int W, int H, float ax,
                                         float bx, float ay, float by, float fg_max, float max_dist, double *A, double *g,
                                         double *cost, int32_t *count, void *workspace, void *stream) {
  if (int rc = d2m_check(B, NV, F, W, H, max_dist)) return rc;
  if (int rc = views_check(B, V, NV)) return rc;
  if (B == 0) return SHR_OK;
  if (!observed || !view_vertices || (!faces && F > 0) || !dist || !face || !view || !skin_vertex_start || !skin_bone || !skin_wv ||
      !A || !g || !cost || !count || !workspace)
    return SHR_EINVAL;
  if (int rc = fk_check(params, B, offset, offset_inv)) return rc;
  if ((((uintptr_t)observed | (uintptr_t)faces | (uintptr_t)dist | (uintptr_t)face | (uintptr_t)params |
        (uintptr_t)skin_vertex_start | (uintptr_t)skin_bone | (uintptr_t)count) & 3u) != 0)
    return SHR_EINVAL;
  if ((((uintptr_t)A | (uintptr_t)g | (uintptr_t)cost) & 7u) != 0) return SHR_EINVAL;
  if ((((uintptr_t)view_vertices | (uintptr_t)view | (uintptr_t)skin_wv | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (int)icp_tiles(W, H);
  double *part = reinterpret_cast<double *>(workspace);
  hipLaunchKernelGGL(pose_icp_views_tiles_kernel, dim3((unsigned)tiles, (unsigned)V, (unsigned)B), dim3(kIcpThreads), 0, s, observed,
                     reinterpret_cast<const float4 *>(view_vertices), faces, dist, face, view, params, offset, offset_inv,
                     skin_vertex_start, skin_bone, reinterpret_cast<const float4 *>(skin_wv), right_hand ? -1.0f : 1.0f, NV, F,
                     W, H, ax, bx, ay, by, fg_max, max_dist, part);
  hipLaunchKernelGGL(pose_icp_views_reduce_kernel, dim3((unsigned)B), dim3(kIcpSlots), 0, s, part, V * tiles, A, g, cost, count);
  return (int)hipGetLastError();
}
