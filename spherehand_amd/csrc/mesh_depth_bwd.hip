// mesh_depth_bwd.hip -- the backward of the differentiable DepthRender / DepthRasterization: owner taps -> vertex
// gradient (on to the bone transforms: lbs_project.hip); and of the owner raster at its own resolution (shr_tri_raster_owner_fwd): one
// tap of weight 1 per owned pixel -> face-corner or vertex gradient (PixelTaps below).  The reference defines no backward for the mesh path (mesh/render.py:282-287);
// the contract is the sphere backward's (ops.SphereDepthRaster): the gradient routes to the owner and holds coverage
// fixed -- no edge, silhouette or visibility terms.
//
// An output pixel of the fused forward (mesh_depth.hip) is clamp(raw, max) -> ATen bilinear over up to four taps of the
// 640 x 640 raster; a tap's raw depth is, for its owner face (shr_mesh_depth_owner_fwd),
//     zp = 1 / sum_k (c_k / s) / z_k,   c_k = clamp(w_k, 0, 1),  s = sum_k c_k,  w_k = fi_k . (x, y, 1)
// over the face's x-sorted corners (depth_rasterization_cuda_kernel.cu:57-110).  With n_k = cross(P_{k+1} - P, P_{k+2} - P)
// and den = sum_k n_k, w_k = n_k / den, so
//     d zp / d z_k = zp^2 (c_k / s) / z_k^2,   d zp / d c_k = -zp^2 (1 / z_k - 1 / zp) / s,
//     d w_k = (d n_k - w_k d den) / den,
// a weight clamped strictly outside [0, 1] contributing nothing (torch's clamp passes at 0 and 1).  The clamp decisions
// are the forward's fp32 arithmetic, the derivatives are evaluated in fp64.  tri_tap.h states the part every backward of
// the triangle family shares (owned_tap: decisions and weights; weight_chain: d w_k -> the corners' x, y; tri_corners: the
// checked gather of PixelTaps); tap_terms below adds the depth's q, zp and z terms.
//
// Sums: fixed_point.h -- 64-bit fixed point in a per-crop unit computed on the device, bitwise reproducible and
// independent of the batch and of the launch shape.
#include "fixed_point.h"
#include "tri_tap.h"

namespace shr {

// One tap's nine partial derivatives, times its upstream gradient: corner k of the face fv (x, y, z of its corners in
// their ORIGINAL order) gets (d/du, d/dv, d/dz) in g[k][0..2].  (A degenerate face's NaN terms are dropped by the sums.)
// tri_tap.h's owned_tap gives the weights; the depth's own part is q = 1 / zp, the z terms and the weights' coefficient.
__device__ __forceinline__ void tap_terms(const float (&fv)[9], int xi, int yi, double gw, double (&g)[3][3]) {
  OwnedTap T;
  owned_tap(fv, xi, yi, T);
  double q = 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++) q += T.c[a] / T.s / T.z[a];
  const double zp = 1.0 / q, zp2 = zp * zp;
  double G[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
  for (int a = 0; a < 3; a++) G[a][2] = gw * zp2 * (T.c[a] / T.s) / (T.z[a] * T.z[a]);
  weight_chain(T, [&](int a) { return -gw * zp2 * (1.0 / T.z[a] - q) / T.s / T.den; }, G);
  tap_unsort(G, T.order, g);
}
// the same for face f of an indexed mesh; vid[k] the vertex of corner k
__device__ __forceinline__ void tap_terms(const float4 *__restrict__ verts, const int *__restrict__ faces, int f, int xi,
                                          int yi, double gw, double (&g)[3][3], int (&vid)[3]) {
  float fv[9];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    vid[k] = faces[f * 3 + k];
    const float4 v = verts[vid[k]];
    fv[3 * k] = v.x; fv[3 * k + 1] = v.y; fv[3 * k + 2] = v.z;
  }
  tap_terms(fv, xi, yi, gw, g);
}

// The taps a backward sums over (fixed_point.h's Taps: the corners of the taps' faces are the accumulator points).
// MeshTaps: shr_mesh_depth_bwd's output pixels of the resampled depth, up to four bilinear owner taps each.
struct MeshTaps {
  const float4 *vertices;
  const int *faces;
  const int4 *owner;
  const float *grad_depth;
  int NV, src, S;
  static constexpr int kThreads = kBwdThreads, kBlockPix = kBwdBlockPix;
  static constexpr bool kRuns = false;
  __device__ __forceinline__ int points() const { return NV; }
  template <typename Fn>
  __device__ __forceinline__ void walk(Fn fn) const {
    const int b = blockIdx.y;
    const float4 *verts = vertices + (size_t)b * NV;
    const float scale = (float)src / (float)S;
    for (int k = 0; k < kBwdPix; k++) {
      const int i = blockIdx.x * kBwdBlockPix + k * kBwdThreads + threadIdx.x;
      if (i >= S * S) break;
      const int4 o = owner[(size_t)b * S * S + i];
      if ((o.x & o.y & o.z & o.w) < 0) continue;   // all four taps without an owner
      const float gd = grad_depth[(size_t)b * S * S + i];
      const int y = i / S, x = i - y * S;
      const Lin lx = lin_index(x, scale, src), ly = lin_index(y, scale, src);
      const int own[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int t = 0; t < 4; t++) {
        if (own[t] < 0) continue;
        const int sy = t >> 1, sx = t & 1;
        const double wt = (double)(sy ? ly.l1 : ly.l0) * (double)(sx ? lx.l1 : lx.l0);
        double g[3][3];
        int vid[3];
        tap_terms(verts, faces, own[t], sx ? lx.i1 : lx.i0, sy ? ly.i1 : ly.i0, (double)gd * wt, g, vid);
        fn(g, vid);
      }
    }
  }
};

// PixelTaps: the owner raster's W x H pixels (shr_tri_raster_bwd, shr_tri_raster_indexed_bwd), ONE tap of weight 1 at the
// integer pixel each -- the raster's own depth, no resampling.  The points: a face soup's corners (point 3 f + k of
// face_vertices[B][F][3][3], its gradient's own layout) or an indexed mesh's vertices[B][NV][4].  An owner outside
// [0, F) or a vertex index outside [0, NV) is skipped.  RUNS: fixed_point.h's PixelWalk (the accumulators in global
// memory: more than kBwdLdsVerts points, every hand-sized soup).
template <bool INDEXED, bool RUNS>
struct PixelTaps {
  const float *src;
  const int *faces;
  const int *owner;
  const float *grad_depth;
  int F, NV, W, H;
  static constexpr int kThreads = PixelWalk<RUNS>::kThreads, kBlockPix = PixelWalk<RUNS>::kBlockPix;
  static constexpr bool kRuns = RUNS;
  __device__ __forceinline__ int points() const { return INDEXED ? NV : 3 * F; }
  template <typename Fn>
  __device__ __forceinline__ void walk(Fn fn) const {
    const int b = blockIdx.y;
    const size_t npix = (size_t)W * H;
    for (int k = 0; k < PixelWalk<RUNS>::kPix; k++) {
      const size_t i = PixelWalk<RUNS>::pixel(k);
      if (i >= npix) break;
      const int f = owner[(size_t)b * npix + i];
      if ((unsigned)f >= (unsigned)F) continue;   // (background: -1)
      const float gd = grad_depth[(size_t)b * npix + i];
      if (gd == 0.f) continue;                    // (its terms are zeros or NaN: nothing to sum)
      const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
      float fv[9];
      int pid[3];
      if (INDEXED) {
        if (!tri_corners(reinterpret_cast<const float4 *>(src) + (size_t)b * NV, faces, NV, F, f, fv, pid)) continue;
      } else {
        const float *fp = src + ((size_t)b * F + f) * 9;
#pragma unroll
        for (int c = 0; c < 3; c++) pid[c] = 3 * f + c;
#pragma unroll
        for (int c = 0; c < 9; c++) fv[c] = fp[c];
      }
      double g[3][3];
      tap_terms(fv, x, y, (double)gd, g);
      fn(g, pid);
    }
  }
};

}  // namespace shr


extern "C" long long shr_mesh_depth_bwd_workspace_bytes(int B, int NV) { return fix_workspace_bytes(B, NV); }

extern "C" int shr_mesh_depth_bwd(const float *vertices, const int32_t *faces, const int32_t *owner, const float *grad_depth,
                                  int B, int NV, int F, int src_size, int S, float *grad_vertices, void *workspace,
                                  void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!vertices || !faces || !owner || !grad_depth || !grad_vertices || !workspace || B < 0 || NV <= 0 || F <= 0 ||
      src_size <= 0 || S <= 0)
    return SHR_EINVAL;
  if ((((uintptr_t)vertices | (uintptr_t)owner | (uintptr_t)grad_vertices | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  if (B > 65535 || src_size > 32767 || 2 * S > src_size || (long long)NV * 3 >= (1LL << 31)) return SHR_ETOOLARGE;
  const MeshTaps taps{reinterpret_cast<const float4 *>(vertices), faces, reinterpret_cast<const int4 *>(owner), grad_depth, NV,
                      src_size, S};
  // a vertex's accumulator takes at most twelve terms per output pixel: four taps x (at most) three corners of a tap's
  // face on that vertex -- 41 bits for every S <= 418, fewer above (fixed_point.h)
  return fixed_point_bwd<4>(taps, B, NV, (size_t)S * S, fix_term_bits(12, S, S), grad_vertices, workspace,
                            (hipStream_t)stream);
}

// The owner raster's backward.  A point's accumulator takes at most three terms per pixel (a face's three corners, one
// vertex each unless the face repeats one): fix_term_bits(3, W, H) -- 41 bits up to 640 x 640.

extern "C" long long shr_tri_raster_bwd_workspace_bytes(int B, int F) { return fix_workspace_bytes(B, 3LL * F); }
extern "C" long long shr_tri_raster_indexed_bwd_workspace_bytes(int B, int NV) { return fix_workspace_bytes(B, NV); }

extern "C" int shr_tri_raster_bwd(const float *face_vertices, const int32_t *owner, const float *grad_depth, int B, int F,
                                  int W, int H, float *grad_face_vertices, void *workspace, void *stream) {
  using namespace shr;
  if (B == 0 || F == 0) return SHR_OK;   // (no face: an empty gradient)
  if (!face_vertices || !owner || !grad_depth || !grad_face_vertices || !workspace || B < 0 || F < 0 || W <= 0 || H <= 0)
    return SHR_EINVAL;
  if (((uintptr_t)workspace & 15u) != 0) return SHR_EINVAL;
  if (B > 65535 || W > 65535 || H > 65535 || 3LL * F * 3 >= (1LL << 31)) return SHR_ETOOLARGE;
  return with_runs(3 * F, [&](auto runs) {
    return fixed_point_bwd<3>(PixelTaps<false, decltype(runs)::value>{face_vertices, nullptr, owner, grad_depth, F, 0, W, H}, B,
                              3 * F, (size_t)W * H, fix_term_bits(3, W, H), grad_face_vertices, workspace, (hipStream_t)stream);
  });
}

extern "C" int shr_tri_raster_indexed_bwd(const float *vertices, const int32_t *faces, const int32_t *owner,
                                          const float *grad_depth, int B, int NV, int F, int W, int H, float *grad_vertices,
                                          void *workspace, void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!vertices || (!faces && F > 0) || !owner || !grad_depth || !grad_vertices || !workspace || B < 0 || NV <= 0 || F < 0 ||
      W <= 0 || H <= 0)
    return SHR_EINVAL;
  if ((((uintptr_t)vertices | (uintptr_t)grad_vertices | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  if (B > 65535 || W > 65535 || H > 65535 || (long long)NV * 3 >= (1LL << 31)) return SHR_ETOOLARGE;
  return with_runs(NV, [&](auto runs) {
    return fixed_point_bwd<4>(PixelTaps<true, decltype(runs)::value>{vertices, faces, owner, grad_depth, F, NV, W, H}, B, NV,
                              (size_t)W * H, fix_term_bits(3, W, H), grad_vertices, workspace, (hipStream_t)stream);
  });
}
