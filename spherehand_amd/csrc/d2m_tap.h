// d2m_tap.h -- ONE observed data point on its saved face, in fp64: what shr_mesh_d2m_bwd (mesh_d2m.hip: D2mTaps) and the
// Gauss-Newton normal equations of the same distance (pose_icp.hip) both take from a pixel, stated once.
//   closest64     the seven regions in fp64, no clamp -> (v, w) of the closest point a + v ab + w ac
//   d2m_measured  the pixel rule on the forward's maps: a data point whose distance is neither zero nor saturated
//   d2m_closest   the checked gather of the saved face (tri_tap.h's face_points: every index from memory is checked before it
//                 indexes anything) and the closest point again: corner weights, e = p - c, n = |e|
#pragma once
#include "tri_tap.h"

namespace shr {

constexpr int kD2mMaxSide = 2048;

// The closest point of the triangle (a, a + ab, a + ac) to a + ap in fp64: the seven regions, (v, w) of a + v ab + w ac.
__device__ __forceinline__ void closest64(const double (&ab)[3], const double (&ac)[3], const double (&ap)[3], double &v,
                                          double &w) {
  auto dot = [](const double (&u)[3], const double (&t)[3]) { return (u[0] * t[0] + u[1] * t[1]) + u[2] * t[2]; };
  const double bp[3] = {ap[0] - ab[0], ap[1] - ab[1], ap[2] - ab[2]}, cp[3] = {ap[0] - ac[0], ap[1] - ac[1], ap[2] - ac[2]};
  const double d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const double e43 = d4 - d3, e56 = d5 - d6, den = (va + vb) + vc;
  if (d1 <= 0.0 && d2 <= 0.0) { v = 0.0; w = 0.0; }
  else if (d3 >= 0.0 && d4 <= d3) { v = 1.0; w = 0.0; }
  else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { v = d1 / (d1 - d3); w = 0.0; }
  else if (d6 >= 0.0 && d5 <= d6) { v = 0.0; w = 1.0; }
  else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { v = 0.0; w = d2 / (d2 - d6); }
  else if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) { w = e43 / (e43 + e56); v = 1.0 - w; }
  else { v = vb / den; w = vc / den; }
}

// observed value z and saved distance d of a pixel: a data point (a NaN is none) with 0 < d < max_dist (a zero or a
// saturated distance is a constant)
__device__ __forceinline__ bool d2m_measured(float z, float d, float fg_max, float max_dist) {
  return z < fg_max && d > 0.f && d < max_dist;
}

struct D2mClosest {
  double wk[3];     // the closest point's weights on the face's corners: (1 - v - w, v, w)
  double e[3], n;   // p - c and its length
  int pid[3];       // the corners' vertex ids
};

// Pixel i (row-major, W columns) with observed value z against face f of a crop whose vertices are verts[NV].  False: the
// face or one of its ids is out of range, or the point lies on the face, or n is not finite -- the pixel contributes nothing.
__device__ __forceinline__ bool d2m_closest(const float4 *__restrict__ verts, const int *__restrict__ faces, int NV, int F, int f,
                                            size_t i, int W, float ax, float bx, float ay, float by, float z, D2mClosest &t) {
  float fv[9];
  if (!face_points(verts, faces, NV, F, f, fv, t.pid)) return false;
  const int row = (int)(i / W), col = (int)(i - (size_t)row * W);
  const float px = ax * (float)col + bx, py = ay * (float)row + by;
  const double ab[3] = {(double)fv[3] - fv[0], (double)fv[4] - fv[1], (double)fv[5] - fv[2]};
  const double ac[3] = {(double)fv[6] - fv[0], (double)fv[7] - fv[1], (double)fv[8] - fv[2]};
  const double ap[3] = {(double)px - fv[0], (double)py - fv[1], (double)z - fv[2]};
  double v, w;
  closest64(ab, ac, ap, v, w);
#pragma unroll
  for (int c = 0; c < 3; c++) t.e[c] = ap[c] - (v * ab[c] + w * ac[c]);
  t.n = sqrt((t.e[0] * t.e[0] + t.e[1] * t.e[1]) + t.e[2] * t.e[2]);
  if (!(t.n > 0.0 && t.n <= 1.7976931348623157e308)) return false;        // (on the face, or not finite)
  t.wk[0] = (1.0 - v) - w; t.wk[1] = v; t.wk[2] = w;
  return true;
}

}  // namespace shr

// the common argument rules of the entries that take an observation and an indexed mesh (mesh_d2m.hip, pose_icp.hip)
static inline int d2m_check(int B, int NV, int F, int W, int H, float max_dist) {
  if (!(max_dist >= 0.f) || B < 0 || NV <= 0 || F < 0 || H < 1 || W < 1) return SHR_EINVAL;
  if (B > 65535 || H > shr::kD2mMaxSide || W > shr::kD2mMaxSide) return SHR_ETOOLARGE;
  if ((long long)NV * 3 >= (1LL << 31) || 3LL * F >= (1LL << 31)) return SHR_ETOOLARGE;
  return SHR_OK;
}
