// tri_aa_pair.h -- the pair decision of the antialias pass, shared by its two units (tri_antialias.hip: one plane of
// values; tri_antialias_maps.hip: C planes): the arguments, pair_blend -- the ONE restatement of a pair's front pixel,
// qualifying silhouette edge and crossing s that every kernel of the pass evaluates --, the walk over a pixel's four
// pairs, the fixed-point bit bound and the entries' argument check.  include/spherehand_hip.h states the contract.
#pragma once

#include "fixed_point.h"
#include "tri_face.h"

namespace shr {

struct AAArgs {
  const float *values, *depth;
  const int *owner;
  const float4 *verts;   // [B][NV]
  const int *faces, *edges;
  int NV, F, W, H;
};

struct PairBlend {
  bool ok;        // an edge qualifies
  bool front_p;   // the front pixel is the pair's first pixel p (else the second, q)
  float s;        // sigma (crossing - front pixel) along the pair's axis, in [0, 1]
  int t, k;       // the front face and its qualifying edge (corners k and (k + 1) % 3)
};

// face_sort's drawn test on corners already loaded: (x, y, z) of the face's corners in their original order
__device__ __forceinline__ bool aa_sorts(const float4 (&c)[3]) {
  float fv[9];
#pragma unroll
  for (int k = 0; k < 3; k++) { fv[3 * k] = c[k].x; fv[3 * k + 1] = c[k].y; fv[3 * k + 2] = c[k].z; }
  float p[3][3];
  int order[3];
  return face_sort(fv, p, order);
}

// the corners of face f of crop bi (false: f or one of its vertex ids out of range); id[k]: the vertex of corner k
__device__ __forceinline__ bool aa_corners(const AAArgs &A, int bi, int f, int (&id)[3], float4 (&c)[3]) {
  if ((unsigned)f >= (unsigned)A.F) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    id[k] = A.faces[f * 3 + k];
    ok = ok && (unsigned)id[k] < (unsigned)A.NV;
  }
  if (!ok) return false;
#pragma unroll
  for (int k = 0; k < 3; k++) c[k] = A.verts[(size_t)bi * A.NV + id[k]];
  return true;
}

// face f of crop bi is drawn: its ids are in range and face_sort accepts it (front-facing, x0 != x2)
__device__ __forceinline__ bool aa_drawn(const AAArgs &A, int bi, int f) {
  int id[3];
  float4 c[3];
  return aa_corners(A, bi, f, id, c) && aa_sorts(c);
}

// The pair (p, q) of crop bi, p = (x, y), q = p + (1, 0) (VERT false) or p + (0, 1) (VERT true), both inside the image,
// with owner(p) != owner(q).  ip, iq: their offsets in the crop.  The front face's corners are loaded once; the drawn
// tests run only for an edge whose crossing qualifies.
template <bool VERT>
__device__ __forceinline__ PairBlend pair_blend(const AAArgs &A, int bi, int x, int y, size_t ip, size_t iq) {
  PairBlend r;
  r.ok = false; r.front_p = true; r.s = 0.f; r.t = 0; r.k = 0;
  const size_t base = (size_t)bi * A.W * A.H;
  const int op = A.owner[base + ip], oq = A.owner[base + iq];
  const bool fp = op < 0 ? false : (oq < 0 ? true : !(A.depth[base + iq] < A.depth[base + ip]));   // equal bits: p
  const int t = fp ? op : oq;
  int id[3];
  float4 c[3];
  if (!aa_corners(A, bi, t, id, c)) return r;
  const float sigma = fp ? 1.f : -1.f;
  const float uf = (float)(VERT ? (fp ? y : y + 1) : (fp ? x : x + 1));   // the front pixel along the axis
  const float row = (float)(VERT ? x : y);                               // the pair's row (column) across it
  int t_drawn = -1;                                                       // -1: not yet tested
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float4 pa = c[k], pb = c[k == 2 ? 0 : k + 1];
    const float ua = VERT ? pa.y : pa.x, wa = VERT ? pa.x : pa.y;   // along the axis, across it
    const float ub = VERT ? pb.y : pb.x, wb = VERT ? pb.x : pb.y;
    const float du = ub - ua, dw = wb - wa;
    const bool steep = VERT ? fabsf(dw) > fabsf(du) : fabsf(dw) >= fabsf(du);
    if (!steep || dw == 0.f) continue;
    if (!(fminf(wa, wb) <= row && row <= fmaxf(wa, wb))) continue;
    const float uc = ua + ((row - wa) * du) / dw;
    const float s = sigma * (uc - uf);
    if (!(s >= 0.f && s <= 1.f)) continue;
    if (t_drawn < 0) t_drawn = aa_sorts(c) ? 1 : 0;
    if (!t_drawn) return r;                                 // an undrawn face has no silhouette edge
    const int n = A.edges[t * 3 + k];
    if ((unsigned)n < (unsigned)A.F && aa_drawn(A, bi, n)) continue;   // shared with a drawn face: not a silhouette
    r.ok = true; r.front_p = fp; r.s = s; r.t = t; r.k = k;
    return r;
  }
  return r;
}

// The four pairs of pixel (x, y) in the fixed order left, right, up, down: fn(pair, p_is_first, i_other) for each pair
// whose owners differ (i_other: the neighbour's offset in the crop).
template <typename Fn>
__device__ __forceinline__ void each_pair(const AAArgs &A, int bi, int x, int y, size_t i, int o, int ol, int orr, int ou,
                                          int od, Fn fn) {
  if (ol != o) fn(pair_blend<false>(A, bi, x - 1, y, i - 1, i), false, i - 1);
  if (orr != o) fn(pair_blend<false>(A, bi, x, y, i, i + 1), true, i + 1);
  if (ou != o) fn(pair_blend<true>(A, bi, x, y - 1, i - A.W, i), false, i - A.W);
  if (od != o) fn(pair_blend<true>(A, bi, x, y, i, i + A.W), true, i + A.W);
}

constexpr int kAAX = 64, kAAY = 4;   // a workgroup: 64 x 4 pixels, one wave per row segment

}  // namespace shr

// Each point's accumulator takes at most one term per coordinate per pair, and a crop has fewer than 2 W H pairs: the
// crop's largest term goes below 2^(62 - ceil(log2 2WH)), 2^41 at most -- no sum can wrap at any size.
static int aa_fix_bits(int W, int H) {
  const unsigned long long n = 2ull * (unsigned long long)W * (unsigned long long)H;
  int lg = 0;
  while ((1ull << lg) < n) lg++;
  return 62 - lg < shr::kFixBits ? 62 - lg : shr::kFixBits;
}

static int aa_check(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                    const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H) {
  if (!values || !depth || !owner || !vertices || (F > 0 && (!faces || !edges)) || B < 0 || NV <= 0 || F < 0 || W <= 0 ||
      H <= 0)
    return SHR_EINVAL;
  if (((uintptr_t)vertices & 15u) != 0) return SHR_EINVAL;
  if (B > 65535 || W > 65535 || H > 65535 || (long long)NV * 3 >= (1LL << 31) || 3LL * F >= (1LL << 31)) return SHR_ETOOLARGE;
  return SHR_OK;
}
