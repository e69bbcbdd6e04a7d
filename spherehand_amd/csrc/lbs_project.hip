// lbs_project.hip -- linear blend skinning + orthographic camera of the mesh path, forward and backward.
//
// Replaces (reference file:line):
//   mesh/pointTransformation.py:39-46 LinearBlendSkinning.forward and :84-99
//   OthographicalProjection.forward                           -> shr_lbs_project
//   their autograd backward down to the bone transforms       -> shr_lbs_project_bwd (project = 1),
//                                                                shr_lbs_vertices_bwd (either mode)
// The per-entry arithmetic (lbs_add_entry, lbs_finish) is common.h's, shared with the fused mesh_lattice_kernel
// (mesh_depth.hip) and the heat-map renderer (synth_post.hip).
#include "common.h"

namespace shr {

typedef uint32_t v4u_t __attribute__((ext_vector_type(4)));

// Skinning + camera.  One thread per vertex and kLbsCrops samples: the samples' bone matrices are staged in LDS, a
// vertex's skin entries (bone, weight * vertex) are read ONCE for the kLbsCrops samples (one sample per workgroup row
// re-read the shared 0.5-MB table for every sample: 21 -> 1x us for 256 crops, round 3).  Visits only the non-zero
// (bone, vertex) pairs of the reference's dense sum, in ascending bone order (association documented in DESIGN.md);
// per sample the arithmetic is unchanged.
__global__ void __launch_bounds__(256)
lbs_project_kernel(const float *__restrict__ T, int B, int NB, int NV, const int *__restrict__ vstart,
                   const int *__restrict__ sbone, const float4 *__restrict__ swv, int right_hand, int project,
                   float cx, float cy, float fx, float fy, const float *__restrict__ rand_f,
                   float4 *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float s_T[];   // [kLbsCrops][NB][16]
  const int b0 = blockIdx.y * kLbsCrops;
  const int nb = min(kLbsCrops, B - b0);
  for (int i = threadIdx.x; i < nb * NB * 16; i += blockDim.x) s_T[i] = T[(size_t)b0 * NB * 16 + i];
  __syncthreads();
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= NV) return;
  float acc[kLbsCrops][4];
#pragma unroll
  for (int c = 0; c < kLbsCrops; c++)
#pragma unroll
    for (int r = 0; r < 4; r++) acc[c][r] = 0.f;
  for (int e = vstart[v]; e < vstart[v + 1]; e++) {
    const int bone = sbone[e];
    const float4 q = swv[e];
#pragma unroll
    for (int c = 0; c < kLbsCrops; c++) {
      if (c >= nb) continue;
      lbs_add_entry(acc[c], s_T + (c * NB + bone) * 16, q);
    }
  }
#pragma unroll
  for (int c = 0; c < kLbsCrops; c++) {
    if (c >= nb) continue;
    const int b = b0 + c;
    const float4 o = lbs_finish(acc[c], right_hand, project, cx, cy, fx, fy, rand_f != nullptr, rand_f ? rand_f[b] : 0.f);
    // (written through: the vertices are read next by the rasterizer, left dirty they are flushed at the kernel's end)
    const v4u_t t = {__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), __float_as_uint(o.w)};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(out + (size_t)b * NV + v), "v"(t) : "memory");
  }
}

// Skinning + camera backward: grad_T[b][k] = sum over the skin entries e of bone k of dacc_v(e) (x) wv_e.  One workgroup
// per crop, one wave per bone (bones dealt round robin), lanes striding over the vertices in a fixed assignment, fp64
// partial sums and a fixed butterfly (common.h lbs_bone_grad_wave): the same order whatever the batch -- bitwise
// reproducible.  project = 0: the derivative of the skinned points alone (the camera arguments and rand_f unused).
__global__ void __launch_bounds__(1024)
lbs_project_bwd_kernel(const float4 *__restrict__ grad_vertices, int NB, int NV, const int *__restrict__ vstart,
                       const int *__restrict__ sbone, const float4 *__restrict__ swv, int right_hand, int project, float cx,
                       float cy, float fx, float fy, const float *__restrict__ rand_f, float *__restrict__ grad_T) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const float4 *gv = grad_vertices + (size_t)b * NV;
  const bool has_rand = project && rand_f != nullptr;
  const LbsCamera cam = {right_hand, project, cx, cy, fx, fy, has_rand, has_rand ? rand_f[b] : 1.0f};
  for (int k = wave; k < NB; k += waves) {
    double a[16];
    lbs_bone_grad_wave(a, k, lane, gv, NV, vstart, sbone, swv, cam);
    if (lane < 16) grad_T[((size_t)b * NB + k) * 16 + lane] = lbs_bone_grad_entry(a, lane);
  }
}

}  // namespace shr

using namespace shr;

extern "C" int shr_lbs_project(const float *T, int B, int NB, int NV, const int32_t *skin_vertex_start,
                               const int32_t *skin_bone, const float *skin_wv, int right_hand, int project, float cx,
                               float cy, float fx, float fy, const float *rand_f, float *out, void *stream) {
  if (B == 0 || NV == 0) return SHR_OK;
  if (!T || !skin_vertex_start || !skin_bone || !skin_wv || !out || B < 0 || NB <= 0 || NV < 0) return SHR_EINVAL;
  if ((((uintptr_t)skin_wv | (uintptr_t)out) & 15u) != 0) return SHR_EINVAL;
  if (B > 65535 * kLbsCrops || NB > 160) return SHR_ETOOLARGE;   // (kLbsCrops x NB matrices of 64 bytes in LDS)
  dim3 grid((unsigned)((NV + 255) / 256), (unsigned)((B + kLbsCrops - 1) / kLbsCrops));
  hipLaunchKernelGGL(lbs_project_kernel, grid, dim3(256), (size_t)kLbsCrops * NB * 64, (hipStream_t)stream, T, B, NB, NV,
                     skin_vertex_start, skin_bone, reinterpret_cast<const float4 *>(skin_wv), right_hand, project, cx,
                     cy, fx, fy, rand_f, reinterpret_cast<float4 *>(out));
  return (int)hipGetLastError();
}

static int lbs_bwd_launch(const float *grad_vertices, int B, int NB, int NV, const int32_t *skin_vertex_start,
                          const int32_t *skin_bone, const float *skin_wv, int right_hand, int project, float cx, float cy,
                          float fx, float fy, const float *rand_f, float *grad_T, void *stream) {
  if ((((uintptr_t)grad_vertices | (uintptr_t)skin_wv) & 15u) != 0) return SHR_EINVAL;
  if (B > (1 << 30)) return SHR_ETOOLARGE;
  hipLaunchKernelGGL(lbs_project_bwd_kernel, dim3((unsigned)B), dim3(NB >= 16 ? 1024 : 64 * NB), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4 *>(grad_vertices), NB, NV, skin_vertex_start, skin_bone,
                     reinterpret_cast<const float4 *>(skin_wv), right_hand, project, cx, cy, fx, fy, rand_f, grad_T);
  return (int)hipGetLastError();
}

extern "C" int shr_lbs_project_bwd(const float *grad_vertices, int B, int NB, int NV, const int32_t *skin_vertex_start,
                                   const int32_t *skin_bone, const float *skin_wv, int right_hand, float cx, float cy,
                                   float fx, float fy, const float *rand_f, float *grad_T, void *stream) {
  if (B == 0) return SHR_OK;
  if (!grad_vertices || !skin_vertex_start || !skin_bone || !skin_wv || !grad_T || B < 0 || NB <= 0 || NV <= 0)
    return SHR_EINVAL;
  return lbs_bwd_launch(grad_vertices, B, NB, NV, skin_vertex_start, skin_bone, skin_wv, right_hand, 1, cx, cy, fx, fy,
                        rand_f, grad_T, stream);
}

extern "C" int shr_lbs_vertices_bwd(const float *grad_vertices, int B, int NB, int NV, const int32_t *skin_vertex_start,
                                    const int32_t *skin_bone, const float *skin_wv, int right_hand, int project, float cx,
                                    float cy, float fx, float fy, const float *rand_f, float *grad_T, void *stream) {
  if (B == 0 || NV == 0) return SHR_OK;
  if (!grad_vertices || !skin_vertex_start || !skin_bone || !skin_wv || !grad_T || B < 0 || NB <= 0 || NV < 0)
    return SHR_EINVAL;
  return lbs_bwd_launch(grad_vertices, B, NB, NV, skin_vertex_start, skin_bone, skin_wv, right_hand, project ? 1 : 0, cx,
                        cy, fx, fy, rand_f, grad_T, stream);
}
