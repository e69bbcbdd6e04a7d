// pose_ik.hip -- keypoints -> pose: the inverse of fk.hip's pose -> sphere records (shr_pose_spheres_fwd), as a batched
// Levenberg-Marquardt refinement from a start pose, its Jacobian entry and its implicit-function backward.
//
// Inverts (reference file:line): HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by the
// key-point skinning of HandBallPrimitiveRender (mesh/render.py:65-88).  The reference has no counterpart.
//
// One wave per crop in all three kernels; everything a crop needs lives in LDS and registers (no workspace):
//   * the bone transforms by fk_rows.h's pose_transforms_wave<false> and the keypoints by fk.hip's expression: the bits
//     of shr_pose_spheres_fwd;
//   * the Jacobian, fp32, [3 J][26] in LDS.  Palm angles: w x (k - t) about the palm translation, w = P e_x, Rz e_y, e_z
//     (P = Trans Rz Ry Rx is rigid, so this is the chain's own derivative); translations: the identity; finger angles:
//     fk_rows.h's tangent rows times the rest point (the offset matrices are rigid only to 7e-7, which a geometric form
//     would show as 5e-5 mm/rad); row x of the right hand negated;
//   * the normal equations, the Cholesky factor, both solves and the costs in fp64 (the fp32 Jacobian and residuals are
//     the only fp32 roundings of an iteration), every sum in a fixed order: lane `idx mod 64` sums entry idx over the
//     points in index order, the factor goes column by column, lane i owning row i (lm_solve.h, shared with pose_icp.hip).
// Lane-uniform control: every lane derives lambda, the costs and the accept decision from the same LDS values.
#include "fk_rows.h"
#include "lm_solve.h"

namespace shr {

constexpr int kIkPoints = 64;        // key-points per crop (lane j owns point j)
constexpr int kIkN = kLmN;           // pose parameters

struct IkPoint {                     // lane j's point: bone, rest position, weight and the keypoint at the last evaluation
  int bone;
  float4 v;
  float w;
  float kx, ky, kz;                  // model frame (x not negated)
};

struct IkLds {
  Rot sc[kAngles];
  float4 T[kBones * 4];
  float4 dT[5 * kFingerTangents * 3];
  float jac[3 * kIkPoints * kIkN];
  double A[kIkN * kIkN], L[kIkN * kIkN];
  double g[kIkN], x[kIkN], red[kIkPoints];
  double piv;
  float r[3 * kIkPoints], w[kIkPoints];
  float p[kIkN], q[kIkN], p0[kIkN], mu[kIkN];
};

__device__ __forceinline__ IkPoint ik_load_point(int lane, int J, const int *__restrict__ bone, const float4 *__restrict__ wv) {
  IkPoint pt;
  pt.bone = 0;
  pt.v = make_float4(0.f, 0.f, 0.f, 0.f);
  pt.w = 0.f;
  pt.kx = pt.ky = pt.kz = 0.f;
  if (lane < J) {
    pt.bone = min(max(bone[lane], 0), kBones - 1);   // (as shr_pose_spheres_fwd: a row of the table, not beyond it)
    pt.v = wv[lane];
  }
  return pt;
}

// The transforms of the pose at p[b] into s.T (and its sincos table into s.sc), lane j's keypoint into pt
__device__ __forceinline__ void ik_keypoints(IkLds &s, IkPoint &pt, const float *p, int b, const float *__restrict__ offset,
                                             const float *__restrict__ offset_inv, int lane, int J) {
  pose_transforms_wave<false>(p, offset, offset_inv, b, lane, s.sc, nullptr, s.T, SynthDraws{});
  __syncthreads();
  if (lane < J) {
    const float4 r0 = s.T[4 * pt.bone], r1 = s.T[4 * pt.bone + 1], r2 = s.T[4 * pt.bone + 2], v = pt.v;
    pt.kx = ((r0.x * v.x + r0.y * v.y) + r0.z * v.z) + r0.w * v.w;
    pt.ky = ((r1.x * v.x + r1.y * v.y) + r1.z * v.z) + r1.w * v.w;
    pt.kz = ((r2.x * v.x + r2.y * v.y) + r2.z * v.z) + r2.w * v.w;
  }
}

// The cost of the pose in LDS at p: residuals to s.r, sum_j w_j |k_j - y_j|^2 + sum_i mu_i (p_i - p0_i)^2 in index order
__device__ __forceinline__ double ik_cost(IkLds &s, IkPoint &pt, const float *p, float sx, float yx, float yy, float yz,
                                          const float *__restrict__ offset, const float *__restrict__ offset_inv, int lane,
                                          int J) {
  ik_keypoints(s, pt, p, 0, offset, offset_inv, lane, J);
  if (lane < J) {
    const float rx = sx * pt.kx - yx, ry = pt.ky - yy, rz = pt.kz - yz;
    s.r[3 * lane] = rx; s.r[3 * lane + 1] = ry; s.r[3 * lane + 2] = rz;
    s.red[lane] = (double)pt.w * (((double)rx * rx + (double)ry * ry) + (double)rz * rz);
  }
  __syncthreads();
  double c = 0.0;
#pragma unroll 1
  for (int j = 0; j < J; j++) c += s.red[j];
  for (int i = 0; i < kIkN; i++) {
    const double d = (double)p[i] - (double)s.p0[i];
    c += (double)s.mu[i] * d * d;
  }
  return c;
}

// s.jac at the pose whose transforms, sincos table and keypoints the last ik_keypoints left (p: its parameters)
__device__ __forceinline__ void ik_jacobian(IkLds &s, const IkPoint &pt, const float *p, float sx, const float *__restrict__ offset,
                                            const float *__restrict__ offset_inv, int lane, int J) {
  pose_finger_tangents_wave(p, offset, offset_inv, lane, s.sc, s.dT);
  if (lane < J) {
    float *row = s.jac + 3 * lane * kIkN;
    for (int e = 0; e < 3 * kIkN; e++) row[e] = 0.f;
    const float4 r0 = s.T[0], r1 = s.T[1], r2 = s.T[2];
    const float dx = pt.kx - r0.w, dy = pt.ky - r1.w, dz = pt.kz - r2.w;
    const Rot rz = s.sc[2];
    // w x d for w = P e_x, Rz e_y = (-s, c, 0), e_z
    row[0] = sx * (r1.x * dz - r2.x * dy);
    row[kIkN] = r2.x * dx - r0.x * dz;
    row[2 * kIkN] = r0.x * dy - r1.x * dx;
    row[1] = sx * (rz.c * dz);
    row[kIkN + 1] = rz.s * dz;
    row[2 * kIkN + 1] = -(rz.s * dy) - rz.c * dx;
    row[2] = sx * -dy;
    row[kIkN + 2] = dx;
    row[3] = sx;
    row[kIkN + 4] = 1.f;
    row[2 * kIkN + 5] = 1.f;
  }
  __syncthreads();
  if (lane < J && pt.bone >= 2) {
    const int f = (pt.bone - 2) / 3, level = (pt.bone - 2) - 3 * f;
    const float4 v = pt.v;
    float *row = s.jac + 3 * lane * kIkN + 6 + 4 * f;
    for (int a = 0; a < 4; a++) {
      if (a > level + 1) break;
      const float4 *d = s.dT + (kFingerTangents * f + tangent_slot(a, level)) * 3;
      row[a] = sx * (((d[0].x * v.x + d[0].y * v.y) + d[0].z * v.z) + d[0].w * v.w);
      row[kIkN + a] = ((d[1].x * v.x + d[1].y * v.y) + d[1].z * v.z) + d[1].w * v.w;
      row[2 * kIkN + a] = ((d[2].x * v.x + d[2].y * v.y) + d[2].z * v.z) + d[2].w * v.w;
    }
  }
  __syncthreads();
}

// A = J^T W J + diag(mu) (lower triangle) and, WANT_G, g = J^T W r + mu (p - p0): entry idx by lane idx mod 64, the
// points in index order.  Two finger columns of different fingers share no point: that entry is 0.
template <bool WANT_G>
__device__ __forceinline__ void ik_normal(IkLds &s, const float *p, int lane, int J) {
#pragma unroll 1
  for (int idx = lane; idx < kNeqTri + (WANT_G ? kIkN : 0); idx += 64) {
    if (idx < kNeqTri) {
      const NeqEntry e = neq_entry(idx);
      const int a = e.a, c = e.c;
      double acc = 0.0;
      if (!(c >= 6 && (a - 6) / 4 != (c - 6) / 4)) {
#pragma unroll 2
        for (int j = 0; j < J; j++) {
          const double w = (double)s.w[j];
          const float *row = s.jac + 3 * j * kIkN;
#pragma unroll
          for (int k = 0; k < 3; k++) acc = fma(w * (double)row[k * kIkN + a], (double)row[k * kIkN + c], acc);
        }
      }
      if (a == c) acc += (double)s.mu[a];
      s.A[a * kIkN + c] = acc;
    } else {
      const int a = idx - kNeqTri;
      double acc = 0.0;
#pragma unroll 1
      for (int j = 0; j < J; j++) {
        const double w = (double)s.w[j];
        const float *row = s.jac + 3 * j * kIkN;
#pragma unroll
        for (int k = 0; k < 3; k++) acc = fma(w * (double)row[k * kIkN + a], (double)s.r[3 * j + k], acc);
      }
      s.g[a] = acc + (double)s.mu[a] * ((double)p[a] - (double)s.p0[a]);
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(64)
pose_keypoints_jacobian_kernel(const float *__restrict__ params, const float *__restrict__ offset,
                               const float *__restrict__ offset_inv, int J, const int *__restrict__ bone,
                               const float4 *__restrict__ wv, float sx, float4 *__restrict__ keypoints,
                               float *__restrict__ jac) {
  __shared__ IkLds s;
  const int b = blockIdx.x, lane = threadIdx.x;
  IkPoint pt = ik_load_point(lane, J, bone, wv);
  ik_keypoints(s, pt, params, b, offset, offset_inv, lane, J);
  if (lane < J) keypoints[(size_t)b * J + lane] = make_float4(sx * pt.kx, pt.ky, pt.kz, 1.0f);
  ik_jacobian(s, pt, params + (size_t)b * kIkN, sx, offset, offset_inv, lane, J);
  float *out = jac + (size_t)b * 3 * J * kIkN;
  for (int e = lane; e < 3 * J * kIkN; e += 64) out[e] = s.jac[e];
}

__global__ void __launch_bounds__(64)
pose_ik_fwd_kernel(const float *__restrict__ target, const float *__restrict__ params0, const float *__restrict__ offset,
                   const float *__restrict__ offset_inv, int J, const int *__restrict__ bone, const float4 *__restrict__ wv,
                   float sx, const float *__restrict__ weights, int weight_stride, const float *__restrict__ stiffness,
                   int iters, float lambda0, float *__restrict__ params, float *__restrict__ cost0, float *__restrict__ cost) {
  __shared__ IkLds s;
  const int b = blockIdx.x, lane = threadIdx.x;
  IkPoint pt = ik_load_point(lane, J, bone, wv);
  float yx = 0.f, yy = 0.f, yz = 0.f;
  if (lane < J) {
    const float *y = target + ((size_t)b * J + lane) * 3;
    yx = y[0]; yy = y[1]; yz = y[2];
    pt.w = weights ? weights[(size_t)b * weight_stride + lane] : 1.0f;
    s.w[lane] = pt.w;
  }
  if (lane < kIkN) {
    s.q[lane] = s.p[lane] = s.p0[lane] = params0[(size_t)b * kIkN + lane];
    s.mu[lane] = stiffness ? stiffness[lane] : 0.f;
  }
  __syncthreads();
  // One pass per cost evaluation: pass 0 takes the start pose s.q, pass n > 0 judges iteration n's step p + delta in s.q.
  double c = 0.0, lam = (double)lambda0;
  bool tried = true;                  // s.q holds a step to evaluate (false: the factorisation met a bad pivot)
#pragma unroll 1
  for (int pass = 0;; pass++) {
    bool accept = false;
    if (tried) {
      const double ct = ik_cost(s, pt, s.q, sx, yx, yy, yz, offset, offset_inv, lane, J);
      accept = pass == 0 || (ct < c && ct > -__builtin_inf());     // (false for a NaN)
      if (accept) {
        c = ct;
        if (lane < kIkN) s.p[lane] = s.q[lane];
      }
      __syncthreads();
    }
    if (pass == 0) {
      if (lane == 0) cost0[b] = (float)c;
    } else {
      lam = fmin(fmax(lam * (accept ? 0.3 : 10.0), 1e-9), 1e6);
    }
    if (pass == iters) break;
    if (accept) {                     // the pose moved: the transforms in LDS are its own, the normal equations are rebuilt
      ik_jacobian(s, pt, s.p, sx, offset, offset_inv, lane, J);
      ik_normal<true>(s, s.p, lane, J);
    }
    tried = lm_cholesky(s, lam, lane);
    __syncthreads();
    if (tried) {
      lm_solve(s, lane < kIkN ? -s.g[lane] : 0.0, lane);
      if (lane < kIkN) s.q[lane] = (float)((double)s.p[lane] + s.x[lane]);
      __syncthreads();
    }
  }
  if (lane < kIkN) params[(size_t)b * kIkN + lane] = s.p[lane];
  if (lane == 0) cost[b] = (float)c;
}

__global__ void __launch_bounds__(64)
pose_ik_bwd_kernel(const float *__restrict__ params, const float *__restrict__ grad_params, const float *__restrict__ offset,
                   const float *__restrict__ offset_inv, int J, const int *__restrict__ bone, const float4 *__restrict__ wv,
                   float sx, const float *__restrict__ weights, int weight_stride, const float *__restrict__ stiffness,
                   float *__restrict__ grad_target) {
  __shared__ IkLds s;
  const int b = blockIdx.x, lane = threadIdx.x;
  IkPoint pt = ik_load_point(lane, J, bone, wv);
  if (lane < J) {
    pt.w = weights ? weights[(size_t)b * weight_stride + lane] : 1.0f;
    s.w[lane] = pt.w;
  }
  if (lane < kIkN) s.mu[lane] = stiffness ? stiffness[lane] : 0.f;
  const double gp = lane < kIkN ? (double)grad_params[(size_t)b * kIkN + lane] : 0.0;
  ik_keypoints(s, pt, params, b, offset, offset_inv, lane, J);
  ik_jacobian(s, pt, params + (size_t)b * kIkN, sx, offset, offset_inv, lane, J);
  ik_normal<false>(s, nullptr, lane, J);
  const bool ok = lm_cholesky(s, 0.0, lane);
  __syncthreads();
  if (ok) lm_solve(s, gp, lane);
  if (lane < J) {
    float *o = grad_target + ((size_t)b * J + lane) * 3;
    const float *row = s.jac + 3 * lane * kIkN;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      double acc = 0.0;
      if (ok)
        for (int a = 0; a < kIkN; a++) acc = fma((double)row[k * kIkN + a], s.x[a], acc);
      o[k] = ok ? (float)((double)pt.w * acc) : 0.f;
    }
  }
}

}  // namespace shr

using namespace shr;

static int pose_ik_check(const void *params, int B, const void *offset, const void *offset_inv, int J, const void *bone,
                         const void *wv) {
  if (!bone || !wv || J < 1) return SHR_EINVAL;
  if ((((uintptr_t)wv) & 15u) != 0 || (((uintptr_t)params | (uintptr_t)bone) & 3u) != 0) return SHR_EINVAL;
  if (int rc = fk_check(params, B, offset, offset_inv)) return rc;
  if (J > kIkPoints) return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" int shr_pose_keypoints_jacobian(const float *params, int B, const float *offset, const float *offset_inv, int J,
                                           const int32_t *bone, const float *wv, int right_hand, float *keypoints,
                                           float *jac, void *stream) {
  if (B == 0) return SHR_OK;
  if (int rc = pose_ik_check(params, B, offset, offset_inv, J, bone, wv)) return rc;
  if (!keypoints || !jac || (((uintptr_t)keypoints) & 15u) != 0 || (((uintptr_t)jac) & 3u) != 0) return SHR_EINVAL;
  hipLaunchKernelGGL(pose_keypoints_jacobian_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, params, offset,
                     offset_inv, J, bone, reinterpret_cast<const float4 *>(wv), right_hand ? -1.0f : 1.0f,
                     reinterpret_cast<float4 *>(keypoints), jac);
  return (int)hipGetLastError();
}

extern "C" int shr_pose_ik_fwd(const float *target, const float *params0, int B, const float *offset, const float *offset_inv,
                               int J, const int32_t *bone, const float *wv, int right_hand, const float *weights,
                               int weight_stride, const float *stiffness, int iters, float lambda0, float *params,
                               float *cost0, float *cost, void *stream) {
  if (B == 0) return SHR_OK;
  if (int rc = pose_ik_check(params0, B, offset, offset_inv, J, bone, wv)) return rc;
  if (!target || !params || !cost0 || !cost || iters < 0 || !(lambda0 > 0.0f)) return SHR_EINVAL;
  if (weights && weight_stride != 0 && weight_stride != J) return SHR_EINVAL;
  if ((((uintptr_t)target | (uintptr_t)params | (uintptr_t)cost0 | (uintptr_t)cost | (uintptr_t)weights |
        (uintptr_t)stiffness) & 3u) != 0)
    return SHR_EINVAL;
  hipLaunchKernelGGL(pose_ik_fwd_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, target, params0, offset,
                     offset_inv, J, bone, reinterpret_cast<const float4 *>(wv), right_hand ? -1.0f : 1.0f, weights,
                     weight_stride, stiffness, iters, lambda0, params, cost0, cost);
  return (int)hipGetLastError();
}

extern "C" int shr_pose_ik_bwd(const float *params, const float *grad_params, int B, const float *offset,
                               const float *offset_inv, int J, const int32_t *bone, const float *wv, int right_hand,
                               const float *weights, int weight_stride, const float *stiffness, float *grad_target,
                               void *stream) {
  if (B == 0) return SHR_OK;
  if (int rc = pose_ik_check(params, B, offset, offset_inv, J, bone, wv)) return rc;
  if (!grad_params || !grad_target) return SHR_EINVAL;
  if (weights && weight_stride != 0 && weight_stride != J) return SHR_EINVAL;
  if ((((uintptr_t)grad_params | (uintptr_t)grad_target | (uintptr_t)weights | (uintptr_t)stiffness) & 3u) != 0)
    return SHR_EINVAL;
  hipLaunchKernelGGL(pose_ik_bwd_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, params, grad_params, offset,
                     offset_inv, J, bone, reinterpret_cast<const float4 *>(wv), right_hand ? -1.0f : 1.0f, weights,
                     weight_stride, stiffness, grad_target);
  return (int)hipGetLastError();
}
