// tri_tap.h -- what the differentiable triangle family's backwards share about ONE face at ONE pixel it owns, stated once
// for mesh_depth_bwd.hip (MeshTaps, PixelTaps), tri_interp.hip (the forward and its three walkers), tri_antialias.hip
// (pair_blend's front face), sil_cover.hip (CoverTaps) and mesh_d2m.hip (the face records, D2mTaps):
//   tri_corners     the checked gather of an indexed face's corners
//   face_points     the same for a unit that measures 3-D distances to the face (mesh_d2m.hip)
//   owned_tap       the forward's fp32 clamp decisions (tri_face.h) and the fp64 weights over the x-sorted corners
//   live_tap        the two together under the interpolation's rule for a live pixel
//   weight_chain    d w_a = (d n_a - w_a d den) / den: per-weight coefficients -> the sorted corners' (x, y) gradient
//   tap_sorted_ids, tap_unsort   between a face's own corner order and the sorted one
// The rule is mesh_depth_bwd.hip's: decisions in the forward's fp32 arithmetic, derivatives in fp64, a weight clamped
// strictly outside [0, 1] a constant (torch's clamp passes at 0 and 1).
#pragma once

#include "tri_face.h"

namespace shr {

// Face f of a crop whose vertices are verts[NV]: fv = x, y, z of its corners in the faces' own order, id[k] the vertex of
// corner k.  False -- and fv undefined -- when f is outside [0, F) or an id outside [0, NV): the caller skips the face.
__device__ __forceinline__ bool tri_corners(const float4 *__restrict__ verts, const int *__restrict__ faces, int NV, int F,
                                            int f, float (&fv)[9], int (&id)[3]) {
  if ((unsigned)f >= (unsigned)F) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    id[k] = faces[f * 3 + k];
    ok = ok && (unsigned)id[k] < (unsigned)NV;
  }
  if (!ok) return false;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float4 v = verts[id[k]];
    fv[3 * k] = v.x; fv[3 * k + 1] = v.y; fv[3 * k + 2] = v.z;
  }
  return true;
}

// The same gather for a unit that takes a face's corners as 3-D points and no owned tap (mesh_d2m.hip: the face records
// of the closest-point search and D2mTaps): the name says that nothing of the raster's pixel rule is implied.
__device__ __forceinline__ bool face_points(const float4 *__restrict__ verts, const int *__restrict__ faces, int NV, int F,
                                            int f, float (&fv)[9], int (&id)[3]) {
  return tri_corners(verts, faces, NV, F, f, fv, id);
}

// One owned pixel for a backward.  Everything is over the SORTED corners: sorted corner a is corner order[a] of fv.
struct OwnedTap {
  double px, py;                                 // the pixel
  double x[3], y[3], z[3], w[3], c[3], s, den;   // corners, unclamped weights, clamped ones, their sum, 2 x signed area
  bool pass[3];                                  // the fp32 weight lies inside [0, 1]
  int order[3];
};
// fv: a face's corners in their own order (tri_corners).  Returns the forward's fp32 sum of the clamped weights: whether
// the pixel is live is the caller's rule (the interpolation wrote a constant 0 unless 0 < sum <= 3e38; the depth does not
// test it -- a degenerate face's NaN terms are dropped by the sums).
__device__ __forceinline__ float owned_tap(const float (&fv)[9], int xi, int yi, OwnedTap &tap) {
  // the forward's sort by x and fp32 weights (tri_face.h): the clamp decisions
  float p[3][3], fi[9], w32[3], c32[3];
  face_sort(fv, p, tap.order);
  face_matrix(p, fi);
  const float s32 = pixel_weights(fi, (float)xi, (float)yi, w32, c32);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    tap.pass[a] = w32[a] >= 0.f && w32[a] <= 1.f;
    tap.x[a] = p[a][0]; tap.y[a] = p[a][1]; tap.z[a] = p[a][2];
  }
  // fp64 from here on
  tap.px = xi; tap.py = yi;
  tap.den = (tap.x[1] - tap.x[0]) * (tap.y[2] - tap.y[0]) - (tap.x[2] - tap.x[0]) * (tap.y[1] - tap.y[0]);
  tap.s = 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int b = (a + 1) % 3, e = (a + 2) % 3;
    tap.w[a] = ((tap.x[b] - tap.px) * (tap.y[e] - tap.py) - (tap.x[e] - tap.px) * (tap.y[b] - tap.py)) / tap.den;
    tap.c[a] = tap.pass[a] ? tap.w[a] : (double)c32[a];
    tap.s += tap.c[a];
  }
  return s32;
}

// Face f of an indexed mesh at pixel (xi, yi), for a walker whose pixel is not the one that reads the owner map
// (sil_cover.hip's CoverTaps: an observed pixel's tap lies at its nearest rendered pixel): the checked gather and the owned
// tap under the interpolation's rule for a live pixel, the fp32 sum of the clamped weights in (0, 3e38].  False -- and T
// undefined -- when the face, a vertex id or the sum fails: the caller skips the tap.  id[k]: the vertex of corner k.
__device__ __forceinline__ bool live_tap(const float4 *__restrict__ verts, const int *__restrict__ faces, int NV, int F, int f,
                                         int xi, int yi, OwnedTap &T, int (&id)[3]) {
  float fv[9];
  if (!tri_corners(verts, faces, NV, F, f, fv, id)) return false;
  const float s32 = owned_tap(fv, xi, yi, T);
  return s32 > 0.f && s32 <= 3.0e38f;
}

// With w_a = n_a / den, n_a = cross(P_b - P, P_e - P) and den = sum_a n_a: G[.][0..1] += sum over the weights that pass
// of coef(a) d n_a - (sum coef(a) w_a) d den, where coef(a) is (d loss / d w_a) / den.  coef is a callable and is
// evaluated only for a weight that passes (its fp64 divisions stay inside that branch).  G[.][2] is not touched.
template <typename Coef>
__device__ __forceinline__ void weight_chain(const OwnedTap &T, Coef coef, double (&G)[3][3]) {
  double kw = 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (!T.pass[a]) continue;
    const double k = coef(a);
    const int b = (a + 1) % 3, e = (a + 2) % 3;
    G[b][0] += k * (T.y[e] - T.py);
    G[b][1] -= k * (T.x[e] - T.px);
    G[e][0] -= k * (T.y[b] - T.py);
    G[e][1] += k * (T.x[b] - T.px);
    kw += k * T.w[a];
  }
  // - sum_a k_a w_a d den
  G[0][0] -= kw * (T.y[1] - T.y[2]); G[0][1] -= kw * (T.x[2] - T.x[1]);
  G[1][0] -= kw * (T.y[2] - T.y[0]); G[1][1] -= kw * (T.x[0] - T.x[2]);
  G[2][0] -= kw * (T.y[0] - T.y[1]); G[2][1] -= kw * (T.x[1] - T.x[0]);
}

// sorted corner a is corner order[a]: its vertex id, without dynamic indexing
__device__ __forceinline__ void tap_sorted_ids(const int (&id)[3], const int (&order)[3], int (&sid)[3]) {
#pragma unroll
  for (int a = 0; a < 3; a++) sid[a] = (order[a] == 0) ? id[0] : ((order[a] == 1) ? id[1] : id[2]);
}
// the other way: terms G_ over the sorted corners -> g over the face's own corners.  (Opaque copies, as in face_sort: the
// compiler otherwise turns the selects into loads from a select of addresses and pins the nine terms to scratch.)
__device__ __forceinline__ void tap_unsort(const double (&G_)[3][3], const int (&order)[3], double (&g)[3][3]) {
  double G[3][3];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int d = 0; d < 3; d++) { G[a][d] = G_[a][d]; asm("" : "+v"(G[a][d])); }
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int d = 0; d < 3; d++) g[k][d] = (order[0] == k) ? G[0][d] : ((order[1] == k) ? G[1][d] : G[2][d]);
}

}  // namespace shr
