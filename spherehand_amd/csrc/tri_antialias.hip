// tri_antialias.hip -- the antialias pass of the triangle raster (shr_tri_antialias_fwd / _bwd: one plane of values;
// shr_tri_antialias_maps_fwd / _bwd: C planes; include/spherehand_hip.h states the contract, DESIGN.md 4.4d and 4.4f the
// layout): the planes values[C,H,W] of one crop, C >= 1 -- a clamped depth, or MeshAttributeRaster's part or
// correspondence maps -- blended across the silhouette edges of the faces that own the pixels, by where the edge crosses
// between two pixel centres.  The hard raster is left as it is; the blend makes the output continuous in the vertices'
// x, y and carries a gradient to the edges' endpoints.  ONE pass: the single-plane entries are its C = 1 case.
//
// Every kernel here evaluates ONE restatement of a pair's decision, pair_blend: the front pixel, the owner's first
// qualifying silhouette edge (tri_tap.h's checked gather of a face's corners, tri_face.h's face_sort for the drawn test of the
// owner and of the face across), and the
// crossing s.  It depends on depth, owner, vertices, faces and edges only, never on the values: a kernel takes it ONCE per
// pair and applies it to all channels.  fp32 throughout (-ffp-contract=off), per channel in one order: the forward, the
// value gradient and the vertex terms take the same decisions bit for bit, and plane ch of the output and of the value
// gradient has the bits of the pass on plane ch alone.
//   forward       per pixel: the four pairs once -> at most four (coefficient, neighbour) records, then the channel loop;
//                 a pixel whose owner equals its four neighbours' is a copy
//   grad values   the same records for the gather of the upstream gradient (no atomics)
//   grad vertex   fixed_point.h's passes over AATaps: each pair once, at its first pixel -- two points x (x, y) per pair
#include "fixed_point.h"
#include "tri_tap.h"

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
__device__ __forceinline__ bool aa_sorts(const float (&fv)[9]) {
  float p[3][3];
  int order[3];
  return face_sort(fv, p, order);
}

// face f of crop bi is drawn: its ids are in range (tri_tap.h's checked gather) and face_sort accepts it (front-facing,
// x0 != x2)
__device__ __forceinline__ bool aa_drawn(const AAArgs &A, int bi, int f) {
  int id[3];
  float fv[9];
  return tri_corners(A.verts + (size_t)bi * A.NV, A.faces, A.NV, A.F, f, fv, id) && aa_sorts(fv);
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
  float fv[9];   // (x, y, z of corner k at 3 k)
  if (!tri_corners(A.verts + (size_t)bi * A.NV, A.faces, A.NV, A.F, t, fv, id)) return r;
  const float sigma = fp ? 1.f : -1.f;
  const float uf = (float)(VERT ? (fp ? y : y + 1) : (fp ? x : x + 1));   // the front pixel along the axis
  const float row = (float)(VERT ? x : y);                               // the pair's row (column) across it
  int t_drawn = -1;                                                       // -1: not yet tested
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int ka = 3 * k, kb = k == 2 ? 0 : 3 * k + 3;
    const float ua = fv[ka + (VERT ? 1 : 0)], wa = fv[ka + (VERT ? 0 : 1)];   // along the axis, across it
    const float ub = fv[kb + (VERT ? 1 : 0)], wb = fv[kb + (VERT ? 0 : 1)];
    const float du = ub - ua, dw = wb - wa;
    const bool steep = VERT ? fabsf(dw) > fabsf(du) : fabsf(dw) >= fabsf(du);
    if (!steep || dw == 0.f) continue;
    if (!(fminf(wa, wb) <= row && row <= fmaxf(wa, wb))) continue;
    const float uc = ua + ((row - wa) * du) / dw;
    const float s = sigma * (uc - uf);
    if (!(s >= 0.f && s <= 1.f)) continue;
    if (t_drawn < 0) t_drawn = aa_sorts(fv) ? 1 : 0;
    if (!t_drawn) return r;                                 // an undrawn face has no silhouette edge
    const int n = A.edges[t * 3 + k];
    if ((unsigned)n < (unsigned)A.F && aa_drawn(A, bi, n)) continue;   // shared with a drawn face: not a silhouette
    r.ok = true; r.front_p = fp; r.s = s; r.t = t; r.k = k;
    return r;
  }
  return r;
}

constexpr int kAAX = 64, kAAY = 4;   // a workgroup: 64 x 4 pixels, one wave per row segment
constexpr int kAAMaxChannels = 64;   // shr_tri_interp_fwd's limit: the maps this pass takes are its output

// Forward (GRAD false): out[ch] = c[ch] + the gains of the pixel's pairs.  Value gradient (GRAD true): src = grad_out,
// out[ch] = grad_out[ch] + sum over the pixel's qualifying pairs of grad_out[ch][gaining pixel] * d gain / d c_pixel.
// A pair leaves one record, a coefficient w: the forward adds w * (c[neighbour] - c[pixel]) for a pair in which the pixel
// gains, w = s - 1/2 (the pixel is o) or 1/2 - s (it is f); the gradient adds src[gaining pixel] * w, w = s - 1/2 (the
// pixel is f) or 1/2 - s.  FIXED_C: the channel count at compile time, 0 for the run-time argument -- with the loop and
// its pointer steps folded away the single plane runs 3 % faster (256 crops @640^2: 1.61 against 1.66 ms forward), at 38
// VGPRs against 48.
template <bool GRAD, int FIXED_C>
__global__ void __launch_bounds__(kAAX * kAAY)
aa_pixel_kernel(AAArgs A, int runtime_C, const float *__restrict__ src, float *__restrict__ out) {
  const int x = blockIdx.x * kAAX + threadIdx.x, y = blockIdx.y * kAAY + threadIdx.y, bi = blockIdx.z;
  if (x >= A.W || y >= A.H) return;
  const int C = FIXED_C ? FIXED_C : runtime_C;
  const size_t npix = (size_t)A.W * A.H, i = (size_t)y * A.W + x;
  const int *own = A.owner + (size_t)bi * npix;
  const int o = own[i];
  const int ol = x > 0 ? own[i - 1] : o, orr = x + 1 < A.W ? own[i + 1] : o;
  const int ou = y > 0 ? own[i - A.W] : o, od = y + 1 < A.H ? own[i + A.W] : o;
  // the records, one slot per pair in the order left, right, up, down: m bit k -- slot k holds a record; bit 4 + k (GRAD)
  // -- the gaining pixel is this one, not the neighbour
  unsigned m = 0u;
  float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
  auto record = [&](const PairBlend &pb, bool p_first, unsigned slot, float &w) {
    if (!pb.ok) return;
    const bool me_front = p_first == pb.front_p;
    const bool o_gains = pb.s >= 0.5f;
    if (GRAD) {
      w = me_front ? pb.s - 0.5f : 0.5f - pb.s;
      m |= (o_gains != me_front ? 17u : 1u) << slot;   // grad_out of the gaining pixel
    } else {
      if (o_gains == me_front) return;                 // the other pixel gains
      w = o_gains ? pb.s - 0.5f : 0.5f - pb.s;
      m |= 1u << slot;
    }
  };
  // (the pairs whose owners differ: interior and background pixels have none)
  if (ol != o) record(pair_blend<false>(A, bi, x - 1, y, i - 1, i), false, 0u, w0);
  if (orr != o) record(pair_blend<false>(A, bi, x, y, i, i + 1), true, 1u, w1);
  if (ou != o) record(pair_blend<true>(A, bi, x, y - 1, i - A.W, i), false, 2u, w2);
  if (od != o) record(pair_blend<true>(A, bi, x, y, i, i + A.W), true, 3u, w3);
  const float *s = src + (size_t)bi * C * npix;
  float *d = out + (size_t)bi * C * npix;
  auto term = [&](float acc, float v, float w, size_t j, unsigned self) {
    if (GRAD) return acc + ((m & self) ? v : s[j]) * w;
    return acc + w * (s[j] - v);
  };
#pragma unroll 4
  for (int ch = 0; ch < C; ch++, s += npix, d += npix) {
    const float v = s[i];
    float acc = v;
    if (m & 15u) {
      if (m & 1u) acc = term(acc, v, w0, i - 1, 16u);
      if (m & 2u) acc = term(acc, v, w1, i + 1, 32u);
      if (m & 4u) acc = term(acc, v, w2, i - A.W, 64u);
      if (m & 8u) acc = term(acc, v, w3, i + A.W, 128u);
    }
    d[i] = acc;
  }
}

// The vertex terms: every pair once, at its first pixel (right and down pairs), fixed_point.h's PixelWalk without runs.
// A qualifying pair's two points get gw (d s / d (x, y)) of their vertex, gw = sum over the channels, ascending, of
// grad_out[ch][gaining pixel] * (c_f[ch] - c_o[ch]) in fp64 -- one term per coordinate per pair whatever C.
struct AATaps {
  AAArgs A;
  int C;
  const float *grad_out;
  static constexpr int kThreads = PixelWalk<false>::kThreads, kBlockPix = PixelWalk<false>::kBlockPix;
  static constexpr bool kRuns = false;
  __device__ __forceinline__ int points() const { return A.NV; }
  template <bool VERT, typename Fn>
  __device__ __forceinline__ void pair(int bi, int x, int y, size_t i, size_t j, Fn &fn) const {
    const PairBlend pb = pair_blend<VERT>(A, bi, x, y, i, j);
    if (!pb.ok) return;
    const size_t npix = (size_t)A.W * A.H;
    const size_t f = pb.front_p ? i : j, o = pb.front_p ? j : i, gp = pb.s >= 0.5f ? o : f;
    const float *c = A.values + (size_t)bi * C * npix, *g = grad_out + (size_t)bi * C * npix;
    double gw = 0.0;
    for (int ch = 0; ch < C; ch++, c += npix, g += npix) gw = gw + (double)g[gp] * ((double)c[f] - (double)c[o]);
    if (gw == 0.0) return;
    // the edge's endpoints, read again from the face (ids checked by pair_blend; ids carried out of pair_blend's unrolled
    // edge loop sent edge 2's terms to a wrong endpoint on the device)
    const int va = A.faces[pb.t * 3 + pb.k], vb = A.faces[pb.t * 3 + (pb.k + 1) % 3];
    const float4 pa = A.verts[(size_t)bi * A.NV + va], pc = A.verts[(size_t)bi * A.NV + vb];
    const double ua = VERT ? pa.y : pa.x, wa = VERT ? pa.x : pa.y, ub = VERT ? pc.y : pc.x, wb = VERT ? pc.x : pc.y;
    const double sg = pb.front_p ? 1.0 : -1.0;
    const double u = ((double)(VERT ? x : y) - wa) / (wb - wa), m = (ub - ua) / (wb - wa);
    const double d_ua = gw * sg * (1.0 - u), d_ub = gw * sg * u, d_wa = -gw * sg * m * (1.0 - u), d_wb = -gw * sg * m * u;
    double t[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    t[0][VERT ? 1 : 0] = d_ua; t[0][VERT ? 0 : 1] = d_wa;
    t[1][VERT ? 1 : 0] = d_ub; t[1][VERT ? 0 : 1] = d_wb;
    const int pid[3] = {va, vb, va};
    fn(t, pid);
  }
  template <typename Fn>
  __device__ __forceinline__ void walk(Fn fn) const {
    const int bi = blockIdx.y;
    const size_t npix = (size_t)A.W * A.H;
    const int *own = A.owner + (size_t)bi * npix;
    for (int k = 0; k < PixelWalk<false>::kPix; k++) {
      const size_t i = PixelWalk<false>::pixel(k);
      if (i >= npix) break;
      const int y = (int)(i / A.W), x = (int)(i - (size_t)y * A.W);
      const int o = own[i];
      if (x + 1 < A.W && own[i + 1] != o) pair<false>(bi, x, y, i, i + 1, fn);
      if (y + 1 < A.H && own[i + A.W] != o) pair<true>(bi, x, y, i, i + A.W, fn);
    }
  }
};

}  // namespace shr

// (C = 1: the single-plane entries)
static int aa_check(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                    const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H, int C) {
  if (!values || !depth || !owner || !vertices || (F > 0 && (!faces || !edges)) || B < 0 || NV <= 0 || F < 0 || W <= 0 ||
      H <= 0)
    return SHR_EINVAL;
  if (((uintptr_t)vertices & 15u) != 0) return SHR_EINVAL;
  if (B > 65535 || W > 65535 || H > 65535 || (long long)NV * 3 >= (1LL << 31) || 3LL * F >= (1LL << 31)) return SHR_ETOOLARGE;
  if (C <= 0) return SHR_EINVAL;
  return C > shr::kAAMaxChannels ? SHR_ETOOLARGE : SHR_OK;
}

// the forward (GRAD false) or the value gradient of src = grad_out (GRAD true) over B crops of C planes; one plane takes
// the kernel's compile-time instance
template <bool GRAD>
static int aa_pixels(const shr::AAArgs &A, int B, int C, const float *src, float *out, hipStream_t s) {
  using namespace shr;
  const dim3 grid((unsigned)((A.W + kAAX - 1) / kAAX), (unsigned)((A.H + kAAY - 1) / kAAY), (unsigned)B);
  if (C == 1) hipLaunchKernelGGL((aa_pixel_kernel<GRAD, 1>), grid, dim3(kAAX, kAAY), 0, s, A, C, src, out);
  else hipLaunchKernelGGL((aa_pixel_kernel<GRAD, 0>), grid, dim3(kAAX, kAAY), 0, s, A, C, src, out);
  return (int)hipGetLastError();
}

// Both backward entries.  Each point's accumulator takes at most one term per coordinate per pair, and a crop has fewer
// than 2 W H pairs: fix_term_bits(2, W, H).
static int aa_bwd(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                  const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H, int C,
                  const float *grad_out, float *grad_values, float *grad_vertices, void *workspace, void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!grad_out || (!grad_values && !grad_vertices) || (grad_vertices && !workspace)) return SHR_EINVAL;
  const int rc = aa_check(values, depth, owner, vertices, faces, edges, B, NV, F, W, H, C);
  if (rc != SHR_OK) return rc;
  if ((((uintptr_t)grad_vertices | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  const AAArgs A{values, depth, owner, reinterpret_cast<const float4 *>(vertices), faces, edges, NV, F, W, H};
  hipStream_t s = (hipStream_t)stream;
  if (grad_values) {
    const int e = aa_pixels<true>(A, B, C, grad_out, grad_values, s);
    if (e != 0 || !grad_vertices) return e;
  }
  return fixed_point_bwd<4>(AATaps{A, C, grad_out}, B, NV, (size_t)W * H, fix_term_bits(2, W, H), grad_vertices, workspace,
                            s);
}

extern "C" int shr_tri_antialias_fwd(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                                     const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H,
                                     float *out, void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!out) return SHR_EINVAL;
  const int rc = aa_check(values, depth, owner, vertices, faces, edges, B, NV, F, W, H, 1);
  if (rc != SHR_OK) return rc;
  const AAArgs A{values, depth, owner, reinterpret_cast<const float4 *>(vertices), faces, edges, NV, F, W, H};
  return aa_pixels<false>(A, B, 1, values, out, (hipStream_t)stream);
}

extern "C" int shr_tri_antialias_maps_fwd(const float *values, const float *depth, const int32_t *owner,
                                          const float *vertices, const int32_t *faces, const int32_t *edges, int B, int NV,
                                          int F, int W, int H, int C, float *out, void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!out) return SHR_EINVAL;
  const int rc = aa_check(values, depth, owner, vertices, faces, edges, B, NV, F, W, H, C);
  if (rc != SHR_OK) return rc;
  const uintptr_t bytes = (uintptr_t)B * C * W * H * sizeof(float), a = (uintptr_t)values, b = (uintptr_t)out;
  if (a < b + bytes && b < a + bytes) return SHR_EINVAL;   // gains are computed from the input values only
  const AAArgs A{values, depth, owner, reinterpret_cast<const float4 *>(vertices), faces, edges, NV, F, W, H};
  return aa_pixels<false>(A, B, C, values, out, (hipStream_t)stream);
}

extern "C" long long shr_tri_antialias_bwd_workspace_bytes(int B, int NV) { return fix_workspace_bytes(B, NV); }
extern "C" long long shr_tri_antialias_maps_bwd_workspace_bytes(int B, int NV) { return fix_workspace_bytes(B, NV); }

extern "C" int shr_tri_antialias_bwd(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                                     const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H,
                                     const float *grad_out, float *grad_values, float *grad_vertices, void *workspace,
                                     void *stream) {
  return aa_bwd(values, depth, owner, vertices, faces, edges, B, NV, F, W, H, 1, grad_out, grad_values, grad_vertices,
                workspace, stream);
}

extern "C" int shr_tri_antialias_maps_bwd(const float *values, const float *depth, const int32_t *owner,
                                          const float *vertices, const int32_t *faces, const int32_t *edges, int B, int NV,
                                          int F, int W, int H, int C, const float *grad_out, float *grad_values,
                                          float *grad_vertices, void *workspace, void *stream) {
  return aa_bwd(values, depth, owner, vertices, faces, edges, B, NV, F, W, H, C, grad_out, grad_values, grad_vertices,
                workspace, stream);
}
