// tri_antialias_maps.hip -- the antialias pass of the triangle raster over multi-channel maps
// (shr_tri_antialias_maps_fwd / _bwd; include/spherehand_hip.h states the contract, DESIGN.md 4.4f the layout): the C
// planes values[C,H,W] of one crop -- MeshAttributeRaster's part or correspondence maps -- blended across the silhouette
// edges exactly as tri_antialias.hip blends one plane.
//
// A pair's decision (tri_aa_pair.h's pair_blend: front pixel, qualifying silhouette edge, crossing s) depends on depth,
// owner, vertices, faces and edges only, never on the values: every kernel here takes it ONCE per pair and applies it to
// all channels.  Per channel the arithmetic is tri_antialias.hip's, fp32 with -ffp-contract=off, in the same order:
// plane ch of the output and of the value gradient has the bits of the single-plane pass on plane ch.
//   forward       per pixel: the four pairs once -> at most four (coefficient, neighbour) records, then the channel loop
//   grad values   the same records for the gather of the upstream gradient (no atomics)
//   grad vertex   fixed_point.h's passes over AAMapsTaps: AATaps with gw summed over the channels in fp64
#include "tri_aa_pair.h"

namespace shr {

// Forward (GRAD false): out[ch] = c[ch] + the gains of the pixel's pairs.  Value gradient (GRAD true): src = grad_out,
// out[ch] = grad_out[ch] + sum over the pixel's qualifying pairs of grad_out[ch][gaining pixel] * d gain / d c_pixel.
// A pair leaves one record, a coefficient w: the forward adds w * (c[neighbour] - c[pixel]) for a pair in which the pixel
// gains, w = s - 1/2 (the pixel is o) or 1/2 - s (it is f) -- aa_pixel_kernel's two expressions, which coincide term by
// term; the gradient adds src[gaining pixel] * w, w = s - 1/2 (the pixel is f) or 1/2 - s.
template <bool GRAD>
__global__ void __launch_bounds__(kAAX * kAAY)
aa_maps_pixel_kernel(AAArgs A, int C, const float *__restrict__ src, float *__restrict__ out) {
  const int x = blockIdx.x * kAAX + threadIdx.x, y = blockIdx.y * kAAY + threadIdx.y, bi = blockIdx.z;
  if (x >= A.W || y >= A.H) return;
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
  // (each_pair's four pairs, written out: a record's slot is its pair; interior and background pixels have none)
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

// The vertex terms: AATaps (tri_antialias.hip) with gw = sum over the channels, ascending, of grad_out[ch][gaining pixel]
// * (c_f[ch] - c_o[ch]) in fp64 -- still one term per coordinate per pair, so aa_fix_bits' bound holds as it is.
struct AAMapsTaps {
  AAArgs A;
  int C;
  const float *grad_out;
  static constexpr int kThreads = kBwdThreads, kBlockPix = kBwdBlockPix;
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
    // the edge's endpoints, read again from the face (ids checked by pair_blend)
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

constexpr int kAAMapsMaxChannels = 64;   // shr_tri_interp_fwd's limit: the maps this pass takes are its output

}  // namespace shr

static int aa_maps_check(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                         const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H, int C) {
  const int rc = aa_check(values, depth, owner, vertices, faces, edges, B, NV, F, W, H);
  if (rc != SHR_OK) return rc;
  if (C <= 0) return SHR_EINVAL;
  return C > shr::kAAMapsMaxChannels ? SHR_ETOOLARGE : SHR_OK;
}

extern "C" int shr_tri_antialias_maps_fwd(const float *values, const float *depth, const int32_t *owner,
                                          const float *vertices, const int32_t *faces, const int32_t *edges, int B, int NV,
                                          int F, int W, int H, int C, float *out, void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!out) return SHR_EINVAL;
  const int rc = aa_maps_check(values, depth, owner, vertices, faces, edges, B, NV, F, W, H, C);
  if (rc != SHR_OK) return rc;
  const uintptr_t bytes = (uintptr_t)B * C * W * H * sizeof(float), a = (uintptr_t)values, b = (uintptr_t)out;
  if (a < b + bytes && b < a + bytes) return SHR_EINVAL;   // gains are computed from the input values only
  const AAArgs A{values, depth, owner, reinterpret_cast<const float4 *>(vertices), faces, edges, NV, F, W, H};
  hipLaunchKernelGGL(aa_maps_pixel_kernel<false>, dim3((unsigned)((W + kAAX - 1) / kAAX), (unsigned)((H + kAAY - 1) / kAAY),
                                                       (unsigned)B),
                     dim3(kAAX, kAAY), 0, (hipStream_t)stream, A, C, values, out);
  return (int)hipGetLastError();
}

extern "C" long long shr_tri_antialias_maps_bwd_workspace_bytes(int B, int NV) { return fix_workspace_bytes(B, NV); }

extern "C" int shr_tri_antialias_maps_bwd(const float *values, const float *depth, const int32_t *owner,
                                          const float *vertices, const int32_t *faces, const int32_t *edges, int B, int NV,
                                          int F, int W, int H, int C, const float *grad_out, float *grad_values,
                                          float *grad_vertices, void *workspace, void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!grad_out || (!grad_values && !grad_vertices) || (grad_vertices && !workspace)) return SHR_EINVAL;
  const int rc = aa_maps_check(values, depth, owner, vertices, faces, edges, B, NV, F, W, H, C);
  if (rc != SHR_OK) return rc;
  if ((((uintptr_t)grad_vertices | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  const AAArgs A{values, depth, owner, reinterpret_cast<const float4 *>(vertices), faces, edges, NV, F, W, H};
  hipStream_t s = (hipStream_t)stream;
  if (grad_values) {
    hipLaunchKernelGGL(aa_maps_pixel_kernel<true>, dim3((unsigned)((W + kAAX - 1) / kAAX),
                                                        (unsigned)((H + kAAY - 1) / kAAY), (unsigned)B),
                       dim3(kAAX, kAAY), 0, s, A, C, grad_out, grad_values);
    const int e = (int)hipGetLastError();
    if (e != 0 || !grad_vertices) return e;
  }
  return fixed_point_bwd<4>(AAMapsTaps{A, C, grad_out}, B, NV, (size_t)W * H, aa_fix_bits(W, H), grad_vertices, workspace,
                            s);
}
