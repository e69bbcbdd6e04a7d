// pose_vertices.hip -- pose -> mesh vertices and back in one launch per direction: the mesh counterpart of fk.hip's
// pose -> sphere records (shr_pose_spheres_fwd / _bwd).
//
// Replaces (reference file:line): HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by
// LinearBlendSkinning.forward (mesh/pointTransformation.py:39-46) and OthographicalProjection.forward (:84-99), and the
// autograd backward of that chain, without the bone transforms visiting HBM:
//   shr_pose_vertices_fwd = shr_fk_fwd -> shr_lbs_project          (fk_rows.h pose_transforms_wave, common.h lbs_*)
//   shr_pose_vertices_bwd = shr_lbs_vertices_bwd -> shr_fk_bwd     (common.h lbs_bone_grad_wave, fk_rows.h pose_reverse_rows)
// Every device function is the one the two-launch entries call, in the same order: the same bits.
#include "fk_rows.h"

namespace shr {

// lbs_project_kernel's shape -- 256 threads take 256 vertices of kLbsCrops crops -- with the staging of T replaced by
// the forward kinematics: wave c forms crop b0 + c's 17 transforms in LDS.  Every workgroup of a crop group repeats
// that (docs/EXPERIMENTS.md has what amortising it over several vertex blocks measured); the one with blockIdx.x == 0
// also writes T when asked.
__global__ void __launch_bounds__(64 * kLbsCrops)
pose_vertices_fwd_kernel(const float *__restrict__ params, const float *__restrict__ offset,
                         const float *__restrict__ offset_inv, int B, int NV, const int *__restrict__ vstart,
                         const int *__restrict__ sbone, const float4 *__restrict__ swv, int right_hand, int project,
                         float cx, float cy, float fx, float fy, const float *__restrict__ rand_f,
                         float4 *__restrict__ out, float *__restrict__ T) {
  __shared__ __attribute__((aligned(16))) float s_T[kLbsCrops * kBones * 16];
  __shared__ Rot sc[kLbsCrops][kAngles];
  const int b0 = blockIdx.y * kLbsCrops;
  const int nb = min(kLbsCrops, B - b0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave < nb)
    pose_transforms_wave<false>(params, offset, offset_inv, b0 + wave, lane, sc[wave], nullptr,
                                reinterpret_cast<float4 *>(s_T + wave * kBones * 16), SynthDraws{});
  __syncthreads();
  if (T != nullptr && blockIdx.x == 0)
    for (int i = threadIdx.x; i < nb * kBones * 16; i += blockDim.x) T[(size_t)b0 * kBones * 16 + i] = s_T[i];
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= NV) return;
  float acc[kLbsCrops][4];
#pragma unroll
  for (int c = 0; c < kLbsCrops; c++)
#pragma unroll
    for (int r = 0; r < 4; r++) acc[c][r] = 0.f;
  for (int e = vstart[v]; e < vstart[v + 1]; e++) {
    const int bone = min(max(sbone[e], 0), kBones - 1);   // (a bone number outside the hand's 17 reads a matrix of the table)
    const float4 q = swv[e];
#pragma unroll
    for (int c = 0; c < kLbsCrops; c++) {
      if (c >= nb) continue;
      lbs_add_entry(acc[c], s_T + (c * kBones + bone) * 16, q);
    }
  }
#pragma unroll
  for (int c = 0; c < kLbsCrops; c++) {
    if (c >= nb) continue;
    const int b = b0 + c;
    out[(size_t)b * NV + v] = lbs_finish(acc[c], right_hand, project, cx, cy, fx, fy, rand_f != nullptr, rand_f ? rand_f[b] : 0.f);
  }
}

// One workgroup of 16 waves per crop.  The waves form lbs_project_bwd_kernel's sums bone by bone (dealt round robin, the
// same lanes, the same order) and leave rows 0 .. 2 of each, rounded to fp32, in LDS: the homogeneous row takes no part
// in the kinematics.  Wave kChainWave, which has one bone where wave 0 has two, requests the chain's constants and
// fills the sincos table before the barrier and runs pose_bwd_kernel's reverse row chain behind it.
constexpr int kChainWave = 1;
__global__ void __launch_bounds__(1024)
pose_vertices_bwd_kernel(const float *__restrict__ params, const float *__restrict__ offset,
                         const float *__restrict__ offset_inv, int NV, const int *__restrict__ vstart,
                         const int *__restrict__ sbone, const float4 *__restrict__ swv, int right_hand, int project,
                         float cx, float cy, float fx, float fy, const float *__restrict__ rand_f,
                         const float4 *__restrict__ grad_vertices, float *__restrict__ grad_params) {
  __shared__ Rot sc[kAngles];
  __shared__ float4 gT[kBones * 3];    // d loss / d T[b, bone, row < 3, :]
  __shared__ float4 pbar[6 * 3];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const float4 *gv = grad_vertices + (size_t)b * NV;
  const bool has_rand = project && rand_f != nullptr;
  const LbsCamera cam = {right_hand, project, cx, cy, fx, fy, has_rand, has_rand ? rand_f[b] : 1.0f};
  for (int k = wave; k < kBones; k += waves) {
    double a[16];
    lbs_bone_grad_wave(a, k, lane, gv, NV, vstart, sbone, swv, cam);
    if (lane < 12) reinterpret_cast<float *>(gT)[12 * k + lane] = lbs_bone_grad_entry(a, lane);
  }
  const bool chain_wave = wave == kChainWave;
  const float *p = params + (size_t)b * 26;
  BoneConst k1, k2, k3;
  float t = 0.f;
  if (chain_wave) {
    const int g = lane >> 2, i = lane & 3;
    const bool chain = lane < 24 && i < 3, finger = chain && g < 5;
    const int b0 = 2 + 3 * (finger ? g : 0);
    if (finger) {
      k1 = load_bone(offset, offset_inv, b0);
      k2 = load_bone(offset, offset_inv, b0 + 1);
      k3 = load_bone(offset, offset_inv, b0 + 2);
    }
    t = chain ? p[3 + i] : 0.f;
    sincos_phase(p, lane, sc);
  }
  __syncthreads();
  if (chain_wave)
    pose_reverse_rows(lane, k1, k2, k3, t, sc, gT, pbar, grad_params + (size_t)b * 26, [] {
      __builtin_amdgcn_s_waitcnt(0xc07f);        // this wave's LDS writes have landed
      __builtin_amdgcn_wave_barrier();
    });
}

}  // namespace shr

using namespace shr;

static int pose_vertices_check(const void *params, int B, const void *offset, const void *offset_inv, int NV,
                               const void *skin_vertex_start, const void *skin_bone, const void *skin_wv,
                               const void *vertices) {
  if (!skin_vertex_start || !skin_bone || !skin_wv || !vertices || NV < 0) return SHR_EINVAL;
  if ((((uintptr_t)skin_wv | (uintptr_t)vertices) & 15u) != 0) return SHR_EINVAL;
  if (int rc = fk_check(params, B, offset, offset_inv)) return rc;
  if ((long long)B * NV > (1LL << 30)) return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" int shr_pose_vertices_fwd(const float *params, int B, const float *offset, const float *offset_inv, int NV,
                                     const int32_t *skin_vertex_start, const int32_t *skin_bone, const float *skin_wv,
                                     int right_hand, int project, float cx, float cy, float fx, float fy,
                                     const float *rand_f, float *vertices, float *T, void *stream) {
  if (B == 0 || NV == 0) return SHR_OK;
  if (int rc = pose_vertices_check(params, B, offset, offset_inv, NV, skin_vertex_start, skin_bone, skin_wv, vertices))
    return rc;
  if ((((uintptr_t)T) & 15u) != 0) return SHR_EINVAL;
  if (B > 65535 * kLbsCrops) return SHR_ETOOLARGE;
  dim3 grid((unsigned)((NV + 64 * kLbsCrops - 1) / (64 * kLbsCrops)), (unsigned)((B + kLbsCrops - 1) / kLbsCrops));
  hipLaunchKernelGGL(pose_vertices_fwd_kernel, grid, dim3(64 * kLbsCrops), 0, (hipStream_t)stream, params, offset,
                     offset_inv, B, NV, skin_vertex_start, skin_bone, reinterpret_cast<const float4 *>(skin_wv),
                     right_hand, project ? 1 : 0, cx, cy, fx, fy, rand_f, reinterpret_cast<float4 *>(vertices), T);
  return (int)hipGetLastError();
}

extern "C" int shr_pose_vertices_bwd(const float *params, int B, const float *offset, const float *offset_inv, int NV,
                                     const int32_t *skin_vertex_start, const int32_t *skin_bone, const float *skin_wv,
                                     int right_hand, int project, float cx, float cy, float fx, float fy,
                                     const float *rand_f, const float *grad_vertices, float *grad_params, void *stream) {
  if (B == 0 || NV == 0) return SHR_OK;
  if (int rc = pose_vertices_check(params, B, offset, offset_inv, NV, skin_vertex_start, skin_bone, skin_wv,
                                   grad_vertices))
    return rc;
  if (!grad_params || (((uintptr_t)grad_params) & 7u) != 0) return SHR_EINVAL;
  hipLaunchKernelGGL(pose_vertices_bwd_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)stream, params, offset,
                     offset_inv, NV, skin_vertex_start, skin_bone, reinterpret_cast<const float4 *>(skin_wv), right_hand,
                     project ? 1 : 0, cx, cy, fx, fy, rand_f, reinterpret_cast<const float4 *>(grad_vertices), grad_params);
  return (int)hipGetLastError();
}
