// tri_antialias.hip -- the antialias pass of the triangle raster (shr_tri_antialias_fwd / _bwd; include/spherehand_hip.h
// states the contract, DESIGN.md 4.4d the layout): values c[H,W] of one crop blended across the silhouette edges of the
// faces that own the pixels, by where the edge crosses between two pixel centres.  The hard raster is left as it is;
// the blend makes the output continuous in the vertices' x, y and carries a gradient to the edges' endpoints.
//
// Every kernel here evaluates ONE restatement of a pair's decision, pair_blend: the front pixel, the owner's first
// qualifying silhouette edge (face_sort of tri_face.h for the drawn test of the owner and of the face across), and the
// crossing s.  fp32 throughout (-ffp-contract=off): the forward, the value gradient and the vertex terms take the same
// decisions bit for bit.
//   forward       a per-pixel gather over the pixel's four pairs; a pixel whose owner equals its four neighbours' is a copy
//   grad values   the same gather of the upstream gradient (no atomics)
//   grad vertex   fixed_point.h's passes over AATaps: each pair once, at its first pixel -- two points x (x, y) per pair
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

// Forward (GRAD false): out = c + the gains of the pixel's pairs.  Value gradient (GRAD true): src = grad_out, out =
// grad_values = grad_out + sum over the pixel's qualifying pairs of grad_out[gaining pixel] * d gain / d c_pixel.
template <bool GRAD>
__global__ void __launch_bounds__(kAAX * kAAY)
aa_pixel_kernel(AAArgs A, const float *__restrict__ src, float *__restrict__ out) {
  const int x = blockIdx.x * kAAX + threadIdx.x, y = blockIdx.y * kAAY + threadIdx.y, bi = blockIdx.z;
  if (x >= A.W || y >= A.H) return;
  const size_t base = (size_t)bi * A.W * A.H, i = (size_t)y * A.W + x;
  const int *own = A.owner + base;
  const int o = own[i];
  const int ol = x > 0 ? own[i - 1] : o, orr = x + 1 < A.W ? own[i + 1] : o;
  const int ou = y > 0 ? own[i - A.W] : o, od = y + 1 < A.H ? own[i + A.W] : o;
  const float v = src[base + i];
  if (ol == o && orr == o && ou == o && od == o) {   // interior (or background): a copy
    out[base + i] = v;
    return;
  }
  float acc = v;
  each_pair(A, bi, x, y, i, o, ol, orr, ou, od, [&](const PairBlend &pb, bool p_first, size_t j) {
    if (!pb.ok) return;
    const bool me_front = p_first == pb.front_p;
    const bool o_gains = pb.s >= 0.5f;
    if (GRAD) {
      const float gr = (o_gains != me_front) ? v : src[base + j];   // grad_out of the gaining pixel
      acc = acc + gr * (me_front ? pb.s - 0.5f : 0.5f - pb.s);
    } else {
      if (o_gains == me_front) return;   // the other pixel gains
      const float cj = A.values[base + j];
      const float cf = me_front ? v : cj, co = me_front ? cj : v;
      acc = acc + (o_gains ? (pb.s - 0.5f) * (cf - co) : (0.5f - pb.s) * (co - cf));
    }
  });
  out[base + i] = acc;
}

// The vertex terms: every pair once, at its first pixel (right and down pairs), kBwdPix pixels per thread a workgroup's
// width apart.  A qualifying pair's two points get gw (d s / d (x, y)) of their vertex, gw = grad_out[gaining pixel] *
// (c_f - c_o) in fp64.
struct AATaps {
  AAArgs A;
  const float *grad_out;
  static constexpr int kThreads = kBwdThreads, kBlockPix = kBwdBlockPix;
  static constexpr bool kRuns = false;
  __device__ __forceinline__ int points() const { return A.NV; }
  template <bool VERT, typename Fn>
  __device__ __forceinline__ void pair(int bi, int x, int y, size_t i, size_t j, Fn &fn) const {
    const PairBlend pb = pair_blend<VERT>(A, bi, x, y, i, j);
    if (!pb.ok) return;
    const size_t base = (size_t)bi * A.W * A.H;
    const size_t f = pb.front_p ? i : j, o = pb.front_p ? j : i;
    const double gw = (double)grad_out[base + (pb.s >= 0.5f ? o : f)] *
                      ((double)A.values[base + f] - (double)A.values[base + o]);
    if (gw == 0.0) return;
    // the edge's endpoints, read again from the face (ids checked by pair_blend; ids carried out of pair_blend's unrolled
    // edge loop sent edge 2's terms to a wrong endpoint on the device)
    const int va = A.faces[pb.t * 3 + pb.k], vb = A.faces[pb.t * 3 + (pb.k + 1) % 3];
    const float4 pa = A.verts[(size_t)bi * A.NV + va], pc = A.verts[(size_t)bi * A.NV + vb];
    const double ua = VERT ? pa.y : pa.x, wa = VERT ? pa.x : pa.y, ub = VERT ? pc.y : pc.x, wb = VERT ? pc.x : pc.y;
    const double sg = pb.front_p ? 1.0 : -1.0;
    const double u = ((double)(VERT ? x : y) - wa) / (wb - wa), m = (ub - ua) / (wb - wa);
    const double d_ua = gw * sg * (1.0 - u), d_ub = gw * sg * u, d_wa = -gw * sg * m * (1.0 - u), d_wb = -gw * sg * m * u;
    double g[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    g[0][VERT ? 1 : 0] = d_ua; g[0][VERT ? 0 : 1] = d_wa;
    g[1][VERT ? 1 : 0] = d_ub; g[1][VERT ? 0 : 1] = d_wb;
    const int pid[3] = {va, vb, va};
    fn(g, pid);
  }
  template <typename Fn>
  __device__ __forceinline__ void walk(Fn fn) const {
    const int bi = blockIdx.y;
    const size_t npix = (size_t)A.W * A.H;
    const int *own = A.owner + (size_t)bi * npix;
    for (int k = 0; k < kBwdPix; k++) {
      const size_t i = (size_t)blockIdx.x * kBlockPix + k * kThreads + threadIdx.x;
      if (i >= npix) break;
      const int y = (int)(i / A.W), x = (int)(i - (size_t)y * A.W);
      const int o = own[i];
      if (x + 1 < A.W && own[i + 1] != o) pair<false>(bi, x, y, i, i + 1, fn);
      if (y + 1 < A.H && own[i + A.W] != o) pair<true>(bi, x, y, i, i + A.W, fn);
    }
  }
};

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

extern "C" int shr_tri_antialias_fwd(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                                     const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H,
                                     float *out, void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!out) return SHR_EINVAL;
  const int rc = aa_check(values, depth, owner, vertices, faces, edges, B, NV, F, W, H);
  if (rc != SHR_OK) return rc;
  const AAArgs A{values, depth, owner, reinterpret_cast<const float4 *>(vertices), faces, edges, NV, F, W, H};
  hipLaunchKernelGGL(aa_pixel_kernel<false>, dim3((unsigned)((W + kAAX - 1) / kAAX), (unsigned)((H + kAAY - 1) / kAAY),
                                                  (unsigned)B),
                     dim3(kAAX, kAAY), 0, (hipStream_t)stream, A, values, out);
  return (int)hipGetLastError();
}

extern "C" long long shr_tri_antialias_bwd_workspace_bytes(int B, int NV) { return fix_workspace_bytes(B, NV); }

extern "C" int shr_tri_antialias_bwd(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                                     const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H,
                                     const float *grad_out, float *grad_values, float *grad_vertices, void *workspace,
                                     void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!grad_out || (!grad_values && !grad_vertices) || (grad_vertices && !workspace)) return SHR_EINVAL;
  const int rc = aa_check(values, depth, owner, vertices, faces, edges, B, NV, F, W, H);
  if (rc != SHR_OK) return rc;
  if ((((uintptr_t)grad_vertices | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  const AAArgs A{values, depth, owner, reinterpret_cast<const float4 *>(vertices), faces, edges, NV, F, W, H};
  hipStream_t s = (hipStream_t)stream;
  if (grad_values) {
    hipLaunchKernelGGL(aa_pixel_kernel<true>, dim3((unsigned)((W + kAAX - 1) / kAAX), (unsigned)((H + kAAY - 1) / kAAY),
                                                   (unsigned)B),
                       dim3(kAAX, kAAY), 0, s, A, grad_out, grad_values);
    const int e = (int)hipGetLastError();
    if (e != 0 || !grad_vertices) return e;
  }
  return fixed_point_bwd<4>(AATaps{A, grad_out}, B, NV, (size_t)W * H, aa_fix_bits(W, H), grad_vertices, workspace, s);
}
