// tri_normals.hip -- area-weighted vertex normals of an indexed mesh and their backward (shr_tri_vertex_normals_fwd /
// _bwd), and the per-pixel unit normalisation of three-plane maps (shr_unit3_maps_fwd / _bwd).
// include/spherehand_hip.h states the contract and the tables, DESIGN.md 4.4g the layout.
//
//   forward        one thread per WELDED POINT of a crop: the point's faces gathered in ascending (face, corner) order
//                  from L2, one fp32 add per term, unit3 on the sum, and the result stored to every copy of the point --
//                  copies get identical bits because they get one evaluation.
//   backward       two gathers, no atomics.  (1) one thread per welded point: the fp32 sum again (the zero rule's
//                  decision) and the same sum in fp64, the copies' gradients added in ascending order, and
//                  G = (g - n (n . g)) / |N| written to the workspace [B][NP][3] fp64 -- every element, every call.
//                  (2) one thread per vertex: its own-id incidences in ascending order, H_f = (G_c0 + G_c1) + G_c2,
//                  the two cross products in fp64, one rounding to fp32.
//   unit3 maps     one thread per pixel (four with 16-byte aligned planes): one read and one write of the planes.
#include "common.h"
#include "unit3.h"   // unit3 and its zero rule

namespace shr {

constexpr int kNrmThreads = 256;

struct NormalTables {
  const int *faces;        // [F][3]
  const int *point;        // [NV]    vertex -> welded point
  const int *inc_start;    // [NP+1]  welded incidence: the corners 3 f + k whose welded point is p, ascending
  const int *inc;          // [NI]
  const int *copy_start;   // [NP+1]  the vertices whose welded point is p, ascending
  const int *copy;         // [NV]
  const int *own_start;    // [NV+1]  own-id incidence: the corners 3 f + k with faces[f,k] == v, ascending (backward)
  const int *own;          // [NO]
  int NV, F, NP, NI, NO;
};

// rows [lo, hi) of a CSR table whose entry array has n elements (a malformed table cannot index outside it)
__device__ __forceinline__ void csr_range(const int *start, int row, int n, int &lo, int &hi) {
  lo = max(start[row], 0);
  hi = min(start[row + 1], n);
}

// corner entry e = 3 f + k: the face's vertex ids; false when e or an id is out of range (the face contributes nothing)
__device__ __forceinline__ bool corner_face(const NormalTables &T, int e, int &f, int (&id)[3]) {
  if ((unsigned)e >= 3u * (unsigned)T.F) return false;
  f = e / 3;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    id[k] = T.faces[3 * f + k];
    ok = ok && (unsigned)id[k] < (unsigned)T.NV;
  }
  return ok;
}

// e1 = p1 - p0, e2 = p2 - p0 in R (fp32: the contract's operation order; fp64: exact differences of fp32 values)
template <typename R>
__device__ __forceinline__ void face_edges(const float4 *P, const int (&id)[3], R (&e1)[3], R (&e2)[3]) {
  const float4 a = P[id[0]], b = P[id[1]], c = P[id[2]];
  e1[0] = (R)b.x - (R)a.x; e1[1] = (R)b.y - (R)a.y; e1[2] = (R)b.z - (R)a.z;
  e2[0] = (R)c.x - (R)a.x; e2[1] = (R)c.y - (R)a.y; e2[2] = (R)c.z - (R)a.z;
}
template <typename R>
__device__ __forceinline__ void cross3(const R (&a)[3], const R (&b)[3], R (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// N of welded point p: its faces' normals in ascending (face, corner) order, one add per term from the first term on
// (WIDE: the same sum in fp64 next to it, for the backward)
template <bool WIDE>
__device__ __forceinline__ void point_sum(const NormalTables &T, const float4 *P, int p, float (&N)[3], double (&Nw)[3]) {
  int lo, hi;
  csr_range(T.inc_start, p, T.NI, lo, hi);
  bool first = true;
#pragma unroll
  for (int d = 0; d < 3; d++) { N[d] = 0.f; Nw[d] = 0.0; }
  for (int i = lo; i < hi; i++) {
    int f, id[3];
    if (!corner_face(T, T.inc[i], f, id)) continue;
    float e1[3], e2[3], n[3];
    face_edges<float>(P, id, e1, e2);
    cross3<float>(e1, e2, n);
#pragma unroll
    for (int d = 0; d < 3; d++) N[d] = first ? n[d] : N[d] + n[d];
    if (WIDE) {
      double w1[3], w2[3], nw[3];
      face_edges<double>(P, id, w1, w2);
      cross3<double>(w1, w2, nw);
#pragma unroll
      for (int d = 0; d < 3; d++) Nw[d] += nw[d];
    }
    first = false;
  }
}

template <bool RAW>
__global__ void __launch_bounds__(kNrmThreads)
vertex_normals_fwd_kernel(NormalTables T, const float4 *__restrict__ points, float4 *__restrict__ normals,
                          float4 *__restrict__ raw) {
  const int p = blockIdx.x * kNrmThreads + threadIdx.x, b = blockIdx.y;
  if (p >= T.NP) return;
  float N[3], n[3];
  double unused[3];
  point_sum<false>(T, points + (size_t)b * T.NV, p, N, unused);
  unit3(N, n);
  int lo, hi;
  csr_range(T.copy_start, p, T.NV, lo, hi);
  for (int i = lo; i < hi; i++) {
    const int v = T.copy[i];
    if ((unsigned)v >= (unsigned)T.NV) continue;
    normals[(size_t)b * T.NV + v] = make_float4(n[0], n[1], n[2], 0.f);
    if (RAW) raw[(size_t)b * T.NV + v] = make_float4(N[0], N[1], N[2], 0.f);
  }
}

// backward (1): G of every welded point -> ws[b][p][3]
__global__ void __launch_bounds__(kNrmThreads)
vertex_normals_point_grad_kernel(NormalTables T, const float4 *__restrict__ points, const float4 *__restrict__ grad_normals,
                                 double *__restrict__ ws) {
  const int p = blockIdx.x * kNrmThreads + threadIdx.x, b = blockIdx.y;
  if (p >= T.NP) return;
  float N[3], n32[3];
  double Nw[3];
  point_sum<true>(T, points + (size_t)b * T.NV, p, N, Nw);
  bool live = unit3(N, n32);
  const double s = (Nw[0] * Nw[0] + Nw[1] * Nw[1]) + Nw[2] * Nw[2];
  live = live && s > 0.0 && s <= 1.7976931348623157e308;
  double G[3] = {0.0, 0.0, 0.0};
  if (live) {
    int lo, hi;
    csr_range(T.copy_start, p, T.NV, lo, hi);
    double g[3] = {0.0, 0.0, 0.0};
    for (int i = lo; i < hi; i++) {
      const int v = T.copy[i];
      if ((unsigned)v >= (unsigned)T.NV) continue;
      const float4 gv = grad_normals[(size_t)b * T.NV + v];
      g[0] += (double)gv.x; g[1] += (double)gv.y; g[2] += (double)gv.z;
    }
    const double len = sqrt(s);
    const double n[3] = {Nw[0] / len, Nw[1] / len, Nw[2] / len};
    const double ng = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2];
#pragma unroll
    for (int d = 0; d < 3; d++) G[d] = (g[d] - n[d] * ng) / len;
  }
  double *o = ws + ((size_t)b * T.NP + p) * 3;
  o[0] = G[0]; o[1] = G[1]; o[2] = G[2];
}

// backward (2): the gradient of every vertex's position from the faces that read it
__global__ void __launch_bounds__(kNrmThreads)
vertex_normals_bwd_kernel(NormalTables T, const float4 *__restrict__ points, const double *__restrict__ ws,
                          float4 *__restrict__ grad_points) {
  const int v = blockIdx.x * kNrmThreads + threadIdx.x, b = blockIdx.y;
  if (v >= T.NV) return;
  const float4 *P = points + (size_t)b * T.NV;
  const double *G = ws + (size_t)b * T.NP * 3;
  int lo, hi;
  csr_range(T.own_start, v, T.NO, lo, hi);
  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = lo; i < hi; i++) {
    const int e = T.own[i];
    int f, id[3];
    if (!corner_face(T, e, f, id)) continue;
    const int k = e - 3 * f;
    const int q0 = T.point[id[0]], q1 = T.point[id[1]], q2 = T.point[id[2]];
    if ((unsigned)q0 >= (unsigned)T.NP || (unsigned)q1 >= (unsigned)T.NP || (unsigned)q2 >= (unsigned)T.NP) continue;
    double Hf[3], e1[3], e2[3], c1[3], c2[3];
#pragma unroll
    for (int d = 0; d < 3; d++) Hf[d] = (G[(size_t)q0 * 3 + d] + G[(size_t)q1 * 3 + d]) + G[(size_t)q2 * 3 + d];
    face_edges<double>(P, id, e1, e2);
    cross3<double>(e2, Hf, c1);   // d / d p1
    cross3<double>(Hf, e1, c2);   // d / d p2
#pragma unroll
    for (int d = 0; d < 3; d++) acc[d] += (k == 1) ? c1[d] : ((k == 2) ? c2[d] : -(c1[d] + c2[d]));
  }
  grad_points[(size_t)b * T.NV + v] = make_float4((float)acc[0], (float)acc[1], (float)acc[2], 0.f);
}

// ---- unit3 over maps[B][3][H][W] -------------------------------------------------------------------------------------
template <typename V> struct Lanes;
template <> struct Lanes<float> {
  static constexpr int n = 1;
  static __device__ __forceinline__ float get(const float &v, int) { return v; }
  static __device__ __forceinline__ void set(float &v, int, float x) { v = x; }
};
template <> struct Lanes<float4> {
  static constexpr int n = 4;
  static __device__ __forceinline__ float get(const float4 &v, int j) { return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w)); }
  static __device__ __forceinline__ void set(float4 &v, int j, float x) {
    if (j == 0) v.x = x; else if (j == 1) v.y = x; else if (j == 2) v.z = x; else v.w = x;
  }
};

// npix: pixels of a plane in units of V; one thread per unit
template <typename V>
__global__ void __launch_bounds__(kNrmThreads)
unit3_maps_fwd_kernel(const V *__restrict__ maps, V *__restrict__ out, size_t npix) {
  const size_t i = (size_t)blockIdx.x * kNrmThreads + threadIdx.x;
  if (i >= npix) return;
  const size_t base = (size_t)blockIdx.y * 3 * npix + i;
  const V m0 = maps[base], m1 = maps[base + npix], m2 = maps[base + 2 * npix];
  V o0, o1, o2;
#pragma unroll
  for (int j = 0; j < Lanes<V>::n; j++) {
    const float N[3] = {Lanes<V>::get(m0, j), Lanes<V>::get(m1, j), Lanes<V>::get(m2, j)};
    float n[3];
    unit3(N, n);
    Lanes<V>::set(o0, j, n[0]); Lanes<V>::set(o1, j, n[1]); Lanes<V>::set(o2, j, n[2]);
  }
  out[base] = o0; out[base + npix] = o1; out[base + 2 * npix] = o2;
}

template <typename V>
__global__ void __launch_bounds__(kNrmThreads)
unit3_maps_bwd_kernel(const V *__restrict__ maps, const V *__restrict__ grad_out, V *__restrict__ grad_maps, size_t npix) {
  const size_t i = (size_t)blockIdx.x * kNrmThreads + threadIdx.x;
  if (i >= npix) return;
  const size_t base = (size_t)blockIdx.y * 3 * npix + i;
  const V m0 = maps[base], m1 = maps[base + npix], m2 = maps[base + 2 * npix];
  const V g0 = grad_out[base], g1 = grad_out[base + npix], g2 = grad_out[base + 2 * npix];
  V o0, o1, o2;
#pragma unroll
  for (int j = 0; j < Lanes<V>::n; j++) {
    const float N[3] = {Lanes<V>::get(m0, j), Lanes<V>::get(m1, j), Lanes<V>::get(m2, j)};
    float n32[3];
    double r[3] = {0.0, 0.0, 0.0};
    if (unit3(N, n32)) {
      const double M[3] = {(double)N[0], (double)N[1], (double)N[2]};
      const double g[3] = {(double)Lanes<V>::get(g0, j), (double)Lanes<V>::get(g1, j), (double)Lanes<V>::get(g2, j)};
      const double len = sqrt((M[0] * M[0] + M[1] * M[1]) + M[2] * M[2]);   // positive: the fp32 sum of squares was
      const double n[3] = {M[0] / len, M[1] / len, M[2] / len};
      const double ng = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2];
#pragma unroll
      for (int d = 0; d < 3; d++) r[d] = (g[d] - n[d] * ng) / len;
    }
    Lanes<V>::set(o0, j, (float)r[0]); Lanes<V>::set(o1, j, (float)r[1]); Lanes<V>::set(o2, j, (float)r[2]);
  }
  grad_maps[base] = o0; grad_maps[base + npix] = o1; grad_maps[base + 2 * npix] = o2;
}

}  // namespace shr

static int normals_check(const float *points, const int32_t *faces, const int32_t *point, const int32_t *inc_start,
                         const int32_t *inc, const int32_t *copy_start, const int32_t *copy, int B, int NV, int F, int NP,
                         int NI) {
  if (!points || (F > 0 && !faces) || !point || !inc_start || (NI > 0 && !inc) || !copy_start || !copy || B < 0 ||
      NV <= 0 || F < 0 || NP <= 0 || NI < 0)
    return SHR_EINVAL;
  if ((((uintptr_t)points) & 15u) != 0) return SHR_EINVAL;
  if ((((uintptr_t)faces | (uintptr_t)point | (uintptr_t)inc_start | (uintptr_t)inc | (uintptr_t)copy_start |
        (uintptr_t)copy) & 3u) != 0)
    return SHR_EINVAL;
  if (B > 65535 || (long long)NV * 3 >= (1LL << 31) || 3LL * F >= (1LL << 31) || (long long)NP * 3 >= (1LL << 31))
    return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" int shr_tri_vertex_normals_fwd(const float *points, const int32_t *faces, const int32_t *point,
                                          const int32_t *inc_start, const int32_t *inc, const int32_t *copy_start,
                                          const int32_t *copy, int B, int NV, int F, int NP, int NI, float *normals,
                                          float *raw, void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!normals || (((uintptr_t)normals | (uintptr_t)raw) & 15u) != 0) return SHR_EINVAL;
  const int rc = normals_check(points, faces, point, inc_start, inc, copy_start, copy, B, NV, F, NP, NI);
  if (rc != SHR_OK) return rc;
  const NormalTables T{faces, point, inc_start, inc, copy_start, copy, nullptr, nullptr, NV, F, NP, NI, 0};
  const dim3 grid((unsigned)((NP + kNrmThreads - 1) / kNrmThreads), (unsigned)B);
  const float4 *P = reinterpret_cast<const float4 *>(points);
  if (raw)
    hipLaunchKernelGGL(vertex_normals_fwd_kernel<true>, grid, dim3(kNrmThreads), 0, (hipStream_t)stream, T, P,
                       reinterpret_cast<float4 *>(normals), reinterpret_cast<float4 *>(raw));
  else
    hipLaunchKernelGGL(vertex_normals_fwd_kernel<false>, grid, dim3(kNrmThreads), 0, (hipStream_t)stream, T, P,
                       reinterpret_cast<float4 *>(normals), static_cast<float4 *>(nullptr));
  return (int)hipGetLastError();
}

extern "C" long long shr_tri_vertex_normals_bwd_workspace_bytes(int B, int NP) {
  if (B < 0 || NP < 0) return -1;
  return (((long long)B * NP * 3 * 8) + 15) / 16 * 16;
}

extern "C" int shr_tri_vertex_normals_bwd(const float *points, const int32_t *faces, const int32_t *point,
                                          const int32_t *inc_start, const int32_t *inc, const int32_t *copy_start,
                                          const int32_t *copy, const int32_t *own_start, const int32_t *own, int B, int NV,
                                          int F, int NP, int NI, int NO, const float *grad_normals, float *grad_points,
                                          void *workspace, void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!grad_normals || !grad_points || !workspace || !own_start || (NO > 0 && !own) || NO < 0) return SHR_EINVAL;
  if ((((uintptr_t)grad_normals | (uintptr_t)grad_points | (uintptr_t)workspace) & 15u) != 0 ||
      (((uintptr_t)own_start | (uintptr_t)own) & 3u) != 0)
    return SHR_EINVAL;
  const int rc = normals_check(points, faces, point, inc_start, inc, copy_start, copy, B, NV, F, NP, NI);
  if (rc != SHR_OK) return rc;
  const NormalTables T{faces, point, inc_start, inc, copy_start, copy, own_start, own, NV, F, NP, NI, NO};
  const float4 *P = reinterpret_cast<const float4 *>(points);
  double *ws = reinterpret_cast<double *>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(vertex_normals_point_grad_kernel, dim3((unsigned)((NP + kNrmThreads - 1) / kNrmThreads), (unsigned)B),
                     dim3(kNrmThreads), 0, s, T, P, reinterpret_cast<const float4 *>(grad_normals), ws);
  hipLaunchKernelGGL(vertex_normals_bwd_kernel, dim3((unsigned)((NV + kNrmThreads - 1) / kNrmThreads), (unsigned)B),
                     dim3(kNrmThreads), 0, s, T, P, ws, reinterpret_cast<float4 *>(grad_points));
  return (int)hipGetLastError();
}

static bool ranges_overlap(const void *a, const void *b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

static int unit3_check(const float *maps, const float *other, int B, int W, int H) {
  if (!maps || !other || B < 0 || W <= 0 || H <= 0) return SHR_EINVAL;
  if ((((uintptr_t)maps | (uintptr_t)other) & 3u) != 0) return SHR_EINVAL;
  if (B > 65535 || W > 65535 || H > 65535) return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" int shr_unit3_maps_fwd(const float *maps, int B, int W, int H, float *out, void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  const int rc = unit3_check(maps, out, B, W, H);
  if (rc != SHR_OK) return rc;
  const size_t npix = (size_t)W * H;
  if (ranges_overlap(maps, out, (size_t)B * 3 * npix * sizeof(float))) return SHR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (npix % 4 == 0 && (((uintptr_t)maps | (uintptr_t)out) & 15u) == 0) {
    const size_t n = npix / 4;
    hipLaunchKernelGGL(unit3_maps_fwd_kernel<float4>, dim3((unsigned)((n + kNrmThreads - 1) / kNrmThreads), (unsigned)B),
                       dim3(kNrmThreads), 0, s, reinterpret_cast<const float4 *>(maps), reinterpret_cast<float4 *>(out), n);
  } else {
    hipLaunchKernelGGL(unit3_maps_fwd_kernel<float>, dim3((unsigned)((npix + kNrmThreads - 1) / kNrmThreads), (unsigned)B),
                       dim3(kNrmThreads), 0, s, maps, out, npix);
  }
  return (int)hipGetLastError();
}

extern "C" int shr_unit3_maps_bwd(const float *maps, const float *grad_out, int B, int W, int H, float *grad_maps,
                                  void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  const int rc = unit3_check(maps, grad_maps, B, W, H);
  if (rc != SHR_OK) return rc;
  if (!grad_out || (((uintptr_t)grad_out) & 3u) != 0) return SHR_EINVAL;
  const size_t npix = (size_t)W * H;
  if (ranges_overlap(maps, grad_maps, (size_t)B * 3 * npix * sizeof(float))) return SHR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (npix % 4 == 0 && (((uintptr_t)maps | (uintptr_t)grad_out | (uintptr_t)grad_maps) & 15u) == 0) {
    const size_t n = npix / 4;
    hipLaunchKernelGGL(unit3_maps_bwd_kernel<float4>, dim3((unsigned)((n + kNrmThreads - 1) / kNrmThreads), (unsigned)B),
                       dim3(kNrmThreads), 0, s, reinterpret_cast<const float4 *>(maps),
                       reinterpret_cast<const float4 *>(grad_out), reinterpret_cast<float4 *>(grad_maps), n);
  } else {
    hipLaunchKernelGGL(unit3_maps_bwd_kernel<float>, dim3((unsigned)((npix + kNrmThreads - 1) / kNrmThreads), (unsigned)B),
                       dim3(kNrmThreads), 0, s, maps, grad_out, grad_maps, npix);
  }
  return (int)hipGetLastError();
}
