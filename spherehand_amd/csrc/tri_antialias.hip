// tri_antialias.hip -- the antialias pass of the triangle raster (shr_tri_antialias_fwd / _bwd; include/spherehand_hip.h
// states the contract, DESIGN.md 4.4d the layout): values c[H,W] of one crop blended across the silhouette edges of the
// faces that own the pixels, by where the edge crosses between two pixel centres.  The hard raster is left as it is;
// the blend makes the output continuous in the vertices' x, y and carries a gradient to the edges' endpoints.
//
// Every kernel here evaluates ONE restatement of a pair's decision, pair_blend (tri_aa_pair.h): the front pixel, the
// owner's first qualifying silhouette edge (face_sort of tri_face.h for the drawn test of the owner and of the face
// across), and the crossing s.  fp32 throughout (-ffp-contract=off): the forward, the value gradient and the vertex
// terms take the same decisions bit for bit.
//   forward       a per-pixel gather over the pixel's four pairs; a pixel whose owner equals its four neighbours' is a copy
//   grad values   the same gather of the upstream gradient (no atomics)
//   grad vertex   fixed_point.h's passes over AATaps: each pair once, at its first pixel -- two points x (x, y) per pair
#include "tri_aa_pair.h"

namespace shr {

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
