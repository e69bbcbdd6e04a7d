// icp_tile.h -- the tile and the reduction of the pose fit's normal equations, stated once for the single-view entry
// (pose_icp.hip: shr_pose_icp_normal) and the multi-view one (pose_icp_views.hip: shr_pose_icp_normal_views).
//   icp_tile_body<kViews>   a workgroup of 256 threads owns kIcpTilePix consecutive pixels of one crop and leaves the tile's
//                           record [A's lower triangle | g | cost | count] in the workspace (pose_icp.hip has the description).
//                           kViews: the crop is view v of sample b -- the maps and the vertices are the crop's, in the view's
//                           frame, params and the LDS tables sample b's, and the row's unit direction is taken back to the
//                           model frame, u = R^T u_v in fp64, before the row is formed.  !kViews: u = u_v, the same code.
//   icp_reduce_body         one workgroup per sample adds `tiles` consecutive records in order and writes A, g, cost, count.
#pragma once
#include "d2m_tap.h"
#include "fk_rows.h"
#include "lm_solve.h"

namespace shr {

constexpr int kIcpThreads = 256;
constexpr int kIcpRounds = 4;
constexpr int kIcpTilePix = kIcpThreads * kIcpRounds;   // the unit of the summation order: part of the contract
constexpr int kIcpSlots = 384;                          // doubles of a tile's record in the workspace: A's lower triangle, g,
static_assert(kNeqTri + kLmN + 2 <= kIcpSlots, "");     // cost, count (379), one thread of the reduction each
constexpr int kIcpRow = kLmN + 1;                       // a row's stride in LDS (27: the threads' rows start in different banks)

struct IcpLds {
  Rot sc[kAngles];
  float4 T[kBones * 4];
  float4 dT[5 * kFingerTangents * 3];
  float jac[kIcpThreads * kIcpRow];
  double d[kIcpThreads];                                // the row's distance, 0: the pixel has no row
  double c2[kIcpThreads];                               // the pixel's dist^2 of the forward's map
};

enum { kIcpA = 0, kIcpG = 1, kIcpCost = 2, kIcpCount = 3, kIcpNone = 4 };

// entry idx of a tile's record: (kind, a, c)
__device__ __forceinline__ int icp_entry(int idx, int &a, int &c) {
  a = c = 0;
  if (idx < kNeqTri) {
    const NeqEntry e = neq_entry(idx);
    a = e.a;
    c = e.c;
    return kIcpA;
  }
  if (idx < kNeqTri + kLmN) { a = idx - kNeqTri; return kIcpG; }
  return idx == kNeqTri + kLmN ? kIcpCost : idx == kNeqTri + kLmN + 1 ? kIcpCount : kIcpNone;
}

// A workgroup-uniform float re-read from its scalar register where it is used.  The nine entries of a view's rotation are
// converted to fp64 inside the branch that forms a row: hoisted out of the rounds, the nine fp64 values would occupy
// eighteen vector registers for the whole kernel, which has none to spare at four workgroups per CU.
__device__ __forceinline__ float uniform_f32(float x) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

// Tile blockIdx.x of crop `crop` (observed, dist, face: the crop's maps; vertices: the crop's NV), the pose and tables of
// sample b; rot (kViews): the crop's view [4,4] row-major, a workgroup-uniform address; the tile's record is number
// crop * gridDim.x + blockIdx.x of `part`.
template <bool kViews>
__device__ __forceinline__ void icp_tile_body(const float *__restrict__ observed, const float4 *__restrict__ vertices,
                                              const int *__restrict__ faces, const float *__restrict__ dist,
                                              const int *__restrict__ face, const float *__restrict__ params,
                                              const float *__restrict__ offset, const float *__restrict__ offset_inv,
                                              const int *__restrict__ vstart, const int *__restrict__ sbone,
                                              const float4 *__restrict__ swv, float sx, int NV, int F, int W, int H, float ax,
                                              float bx, float ay, float by, float fg_max, float max_dist, int b, size_t crop,
                                              const float *__restrict__ rot, double *__restrict__ part) {
  __shared__ IcpLds s;
  const int tid = threadIdx.x;
  const size_t npix = (size_t)H * W, base = (size_t)blockIdx.x * kIcpTilePix;
  if (tid < 64) pose_transforms_wave<false>(params, offset, offset_inv, b, tid, s.sc, nullptr, s.T, SynthDraws{});
  __syncthreads();
  if (tid < 64) pose_finger_tangents_wave(params + (size_t)b * kLmN, offset, offset_inv, tid, s.sc, s.dT);
  int a0, c0, a1, c1;
  icp_entry(tid, a0, c0);                               // (tid < 256 < 351: an entry of A)
  const int kind1 = icp_entry(tid + kIcpThreads, a1, c1);
  double acc0 = 0.0, acc1 = 0.0;
  float *row = s.jac + tid * kIcpRow;
  float R[9] = {};                                      // (kViews: workgroup-uniform)
  if constexpr (kViews) {
#pragma unroll
    for (int q = 0; q < 9; q++) R[q] = rot[4 * (q / 3) + q % 3];
  }
#pragma unroll 1
  for (int r = 0; r < kIcpRounds; r++) {
    const size_t i = base + (size_t)(r * kIcpThreads + tid);
    double dn = 0.0, c2 = 0.0;
    bool live = false;
    D2mClosest t;
    if (i < npix) {
      const float z = observed[crop * npix + i], d = dist[crop * npix + i];
      c2 = (double)d * (double)d;
      if (d2m_measured(z, d, fg_max, max_dist))
        live = d2m_closest(vertices + crop * NV, faces, NV, F, face[crop * npix + i], i, W, ax, bx, ay, by, z, t);
    }
    // (a barrier: the last round's sums have read the rows, and the first round's tangents are in LDS)
    if (__syncthreads_or(live || c2 != 0.0) == 0) continue;
    for (int q = 0; q < kLmN; q++) row[q] = 0.f;
    if (live) {
      dn = t.n;
      double u[3] = {t.e[0] / t.n, t.e[1] / t.n, t.e[2] / t.n};
      if constexpr (kViews) {                           // u = R^T u_v: column j of R against u_v, summed in index order
        const double u0 = u[0], u1 = u[1], u2 = u[2];
#pragma unroll
        for (int j = 0; j < 3; j++)
          u[j] = ((double)uniform_f32(R[j]) * u0 + (double)uniform_f32(R[3 + j]) * u1) + (double)uniform_f32(R[6 + j]) * u2;
      }
      const float4 r0 = s.T[0], r1 = s.T[1], r2 = s.T[2];
      double mx = 0.0, my = 0.0, mz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double cx = (double)sx * -(t.wk[k] * u[0]), cy = -(t.wk[k] * u[1]), cz = -(t.wk[k] * u[2]);
        const int v = t.pid[k];                         // in [0, NV): d2m_closest checked it
#pragma unroll 1
        for (int e = vstart[v]; e < vstart[v + 1]; e++) {
          const int bone = min(max(sbone[e], 0), kBones - 1);   // (as shr_pose_vertices_fwd: a matrix of the table)
          const float4 q = swv[e];
          const float4 m0 = s.T[4 * bone], m1 = s.T[4 * bone + 1], m2 = s.T[4 * bone + 2];
          const float px = ((m0.x * q.x + m0.y * q.y) + m0.z * q.z) + m0.w * q.w;
          const float py = ((m1.x * q.x + m1.y * q.y) + m1.z * q.z) + m1.w * q.w;
          const float pz = ((m2.x * q.x + m2.y * q.y) + m2.z * q.z) + m2.w * q.w;
          const double rx = (double)(px - q.w * r0.w), ry = (double)(py - q.w * r1.w), rz = (double)(pz - q.w * r2.w);
          mx += ry * cz - rz * cy; my += rz * cx - rx * cz; mz += rx * cy - ry * cx;
          tx += (double)q.w * cx; ty += (double)q.w * cy; tz += (double)q.w * cz;
          if (bone >= 2) {
            const int f = (bone - 2) / 3, level = (bone - 2) - 3 * f;
            float *fr = row + 6 + 4 * f;
            for (int a = 0; a < 4; a++) {
              if (a > level + 1) break;
              const float4 *d = s.dT + (kFingerTangents * f + tangent_slot(a, level)) * 3;
              const float dx = ((d[0].x * q.x + d[0].y * q.y) + d[0].z * q.z) + d[0].w * q.w;
              const float dy = ((d[1].x * q.x + d[1].y * q.y) + d[1].z * q.z) + d[1].w * q.w;
              const float dz = ((d[2].x * q.x + d[2].y * q.y) + d[2].z * q.z) + d[2].w * q.w;
              fr[a] += (float)((cx * (double)dx + cy * (double)dy) + cz * (double)dz);
            }
          }
        }
      }
      // omega . m for omega = P e_x, Rz e_y = (-s, c, 0), e_z (pose_ik.hip's palm columns)
      const Rot az = s.sc[2];
      row[0] = (float)(((double)r0.x * mx + (double)r1.x * my) + (double)r2.x * mz);
      row[1] = (float)((double)az.c * my - (double)az.s * mx);
      row[2] = (float)mz;
      row[3] = (float)tx; row[4] = (float)ty; row[5] = (float)tz;
    }
    s.d[tid] = dn;
    s.c2[tid] = c2;
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < kIcpThreads; j++) {
      const double dj = s.d[j], cj = s.c2[j];
      if (dj == 0.0 && cj == 0.0) continue;             // (uniform; a NaN c2 is carried into the cost)
      const float *rj = s.jac + j * kIcpRow;
      acc0 = fma((double)rj[a0], (double)rj[c0], acc0);
      if (kind1 == kIcpA) acc1 = fma((double)rj[a1], (double)rj[c1], acc1);
      else if (kind1 == kIcpG) acc1 = fma(dj, (double)rj[a1], acc1);
      else if (kind1 == kIcpCost) acc1 += cj;
      else if (kind1 == kIcpCount) acc1 += dj != 0.0 ? 1.0 : 0.0;
    }
  }
  double *out = part + (crop * gridDim.x + blockIdx.x) * kIcpSlots;
  out[tid] = acc0;
  if (kind1 != kIcpNone) out[tid + kIcpThreads] = acc1;
}

// Sample b's `tiles` records, consecutive in `part`, added from 0 in ascending order by thread idx of kIcpSlots.
__device__ __forceinline__ void icp_reduce_body(const double *__restrict__ part, int tiles, int b, int idx, double *__restrict__ A,
                                                double *__restrict__ g, double *__restrict__ cost, int *__restrict__ count) {
  int a, c;
  const int kind = icp_entry(idx, a, c);
  if (kind == kIcpNone) return;
  const double *in = part + (size_t)b * tiles * kIcpSlots + idx;
  double acc = 0.0;
#pragma unroll 4
  for (int t = 0; t < tiles; t++) acc += in[(size_t)t * kIcpSlots];
  if (kind == kIcpA) {
    A[((size_t)b * kLmN + a) * kLmN + c] = acc;
    A[((size_t)b * kLmN + c) * kLmN + a] = acc;
  } else if (kind == kIcpG) {
    g[(size_t)b * kLmN + a] = acc;
  } else if (kind == kIcpCost) {
    cost[b] = acc;
  } else {
    count[b] = (int)acc;
  }
}

static inline long long icp_tiles(int W, int H) { return ((long long)W * H + kIcpTilePix - 1) / kIcpTilePix; }

}  // namespace shr
