// mesh_d2m.hip -- the mesh data-to-model distance: every observed 3-D point to its closest point on the triangles
// (shr_mesh_d2m_fwd / _bwd).  include/spherehand_hip.h states the contract -- the fp32 operation sequence of one
// point-triangle distance and the serial selection rule -- DESIGN.md 4.4j the layout, the cull's argument and the figures.
//
//   records    one thread per (crop, face): the checked gather (tri_tap.h's face_points) once, then 48 bytes to the
//              workspace: (a, R) (ab, 0) (ac, 0), R the inflated radius of a sphere about corner a that holds every point
//              a + v ab + w ac with v, w in [0, 1].  An invalid face: NaNs -- its distance is a NaN and is never taken.
//   search     a workgroup owns kD2mTilePix consecutive pixels of one crop, lists its data points in LDS in pixel order
//              (ballot + prefix: the order is fixed), and its lanes take one listed point each.  Per point two sweeps over
//              the faces, staged in chunks of kD2mChunk records in LDS (every lane reads the same record: a broadcast):
//                seed    the face whose corner a is nearest (a sub, a dot and a compare per face), then its exact distance:
//                        a finite first bound whatever order the faces come in
//                cull    for f ascending: skip when |ap|^2 > (S + R_f)^2, S the inflated root of the best distance so
//                        far; otherwise the exact distance, taken under the lexicographic minimum of (d2, f)
//              The result is the serial rule's: the minimum does not depend on the order, and the cull never skips a face
//              that rule would take (cull_root below).
//   backward   fixed_point.h's passes over D2mTaps: one tap per contributing pixel, on its saved face, the closest point
//              again in fp64.
#include "d2m_tap.h"
#include "fixed_point.h"

namespace shr {

constexpr int kD2mThreads = 256;      // search: four waves
constexpr int kD2mTilePix = 1024;     // ... pixels of a workgroup (a data point's offset fits 16 bits)
constexpr int kD2mSubs = kD2mTilePix / kD2mThreads;
constexpr int kD2mChunk = 256;        // ... face records staged together: 12 KB of LDS
constexpr int kD2mRecThreads = 256;
// The cull's margins.  With u = 2^-24: the fp32 |ap|^2, (S + R)^2 and the exact d2 are each within (1 + u)^5 of their real
// values, the record's R within (1 + u)^4 of |ab| + |ac|, the root of best within (1 + u): a relative 2^-16 on R and on S
// exceeds their sum (below 2^-20) many times over; 2^-60 absolute on each covers products that underflow (an error of at
// most 2^-149 each, 2^-74 after the root) and an |ab| whose square underflows.  DESIGN.md 4.4j has the chain.
constexpr float kD2mInflate = 1.0f + 1.0f / 65536.0f;
constexpr float kD2mSlack = 8.673617379884035e-19f;   // 2^-60

struct float3x { float x, y, z; };
__device__ __forceinline__ float dot3(const float3x &u, const float3x &v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }

// The contract's fp32 sequence: the squared distance from a + ap to the triangle (a, a + ab, a + ac).  Selects, no
// branches: the sequence is the same for every lane and the two divisions are the only ones.
__device__ __forceinline__ float tri_dist2(const float3x &ap, const float3x &ab, const float3x &ac) {
  const float3x bp = {ap.x - ab.x, ap.y - ab.y, ap.z - ab.z};
  const float3x cp = {ap.x - ac.x, ap.y - ac.y, ap.z - ac.z};
  const float d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  const float den = (va + vb) + vc;
  float nv = vb, dv = den, nw = vc, dw = den;                                             // in
  bool bc = false;
  if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) { nv = 0.f; dv = 1.f; nw = e43; dw = e43 + e56; bc = true; }   // BC
  if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { nv = 0.f; dv = 1.f; nw = d2; dw = d2 - d6; bc = false; }       // AC
  if (d6 >= 0.f && d5 <= d6) { nv = 0.f; dv = 1.f; nw = 1.f; dw = 1.f; bc = false; }                        // C
  if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { nv = d1; dv = d1 - d3; nw = 0.f; dw = 1.f; bc = false; }       // AB
  if (d3 >= 0.f && d4 <= d3) { nv = 1.f; dv = 1.f; nw = 0.f; dw = 1.f; bc = false; }                        // B
  if (d1 <= 0.f && d2 <= 0.f) { nv = 0.f; dv = 1.f; nw = 0.f; dw = 1.f; bc = false; }                       // A: the first
  float v = nv / dv, w = nw / dw;
  if (bc) v = 1.f - w;
  v = v > 1.f ? 1.f : v; v = v < 0.f ? 0.f : v;   // (a NaN passes both)
  w = w > 1.f ? 1.f : w; w = w < 0.f ? 0.f : w;
  const float3x e = {ap.x - (v * ab.x + w * ac.x), ap.y - (v * ab.y + w * ac.y), ap.z - (v * ab.z + w * ac.z)};
  return dot3(e, e);
}

// S of a best squared distance: a face is skipped when |ap|^2 > (S + R)^2.  Why that never skips a face the serial rule
// takes: the exact sequence measures e = ap - s with s = v ab + w ac, v and w in [0, 1], so |s| <= |ab| + |ac| <= R less
// its margin, and |e| >= |ap| - |s|; a skipped face has |ap| > S + R less the roundings of the comparison, hence
// |e| > root(best) and d2 > best -- with every rounding on the way covered by kD2mInflate and kD2mSlack.  best = +inf:
// S = +inf and nothing is skipped; a NaN |ap|^2 is not skipped either (its d2 is a NaN and is not taken).
__device__ __forceinline__ float cull_root(float best) { return sqrtf(best) * kD2mInflate + kD2mSlack; }

// rec[b][f][3]
__global__ void __launch_bounds__(kD2mRecThreads)
d2m_records_kernel(const float4 *__restrict__ vertices, const int *__restrict__ faces, int NV, int F,
                   float4 *__restrict__ rec) {
  const int f = blockIdx.x * kD2mRecThreads + threadIdx.x;
  if (f >= F) return;
  const int b = blockIdx.y;
  float fv[9];
  int id[3];
  const float nan = __int_as_float(0x7fc00000);
  float4 r0 = make_float4(nan, nan, nan, nan), r1 = r0, r2 = r0;
  if (face_points(vertices + (size_t)b * NV, faces, NV, F, f, fv, id)) {
    const float3x ab = {fv[3] - fv[0], fv[4] - fv[1], fv[5] - fv[2]}, ac = {fv[6] - fv[0], fv[7] - fv[1], fv[8] - fv[2]};
    const float R = (sqrtf(dot3(ab, ab)) + sqrtf(dot3(ac, ac))) * kD2mInflate + kD2mSlack;
    r0 = make_float4(fv[0], fv[1], fv[2], R);
    r1 = make_float4(ab.x, ab.y, ab.z, 0.f);
    r2 = make_float4(ac.x, ac.y, ac.z, 0.f);
  }
  float4 *out = rec + ((size_t)b * F + f) * 3;
  out[0] = r0; out[1] = r1; out[2] = r2;
}

__global__ void __launch_bounds__(kD2mThreads)
d2m_search_kernel(const float *__restrict__ observed, const float4 *__restrict__ rec, int F, int H, int W, float ax, float bx,
                  float ay, float by, float fg_max, float max_dist, float *__restrict__ dist, int *__restrict__ face) {
  __shared__ float4 s_rec[3 * kD2mChunk];          // [0]: (a, R), [1]: ab, [2]: ac -- planes of kD2mChunk
  __shared__ unsigned short s_list[kD2mTilePix];   // the tile's data points, ascending pixel
  __shared__ int s_count[kD2mSubs * (kD2mThreads / 64)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t npix = (size_t)H * W, base = (size_t)blockIdx.x * kD2mTilePix;
  const float *obs = observed + (size_t)blockIdx.y * npix;
  float *out_dist = dist + (size_t)blockIdx.y * npix;
  int *out_face = face + (size_t)blockIdx.y * npix;
  rec += (size_t)blockIdx.y * F * 3;

  // the list: sub-round k takes pixels base + k 256 + tid; a pixel that is no data point is finished here
  int before[kD2mSubs];
  unsigned flags = 0u;
#pragma unroll
  for (int k = 0; k < kD2mSubs; k++) {
    const size_t i = base + (size_t)(k * kD2mThreads + tid);
    const bool point = i < npix && obs[i] < fg_max;          // (NaN: not a data point)
    if (i < npix && !point) { out_dist[i] = 0.f; out_face[i] = -1; }
    const unsigned long long m = __ballot(point);
    before[k] = __popcll(m & ((1ull << lane) - 1ull));
    if (point) flags |= 1u << k;
    if (lane == 0) s_count[k * (kD2mThreads / 64) + wave] = __popcll(m);
  }
  __syncthreads();
  int n = 0;
#pragma unroll
  for (int k = 0; k < kD2mSubs; k++) {
#pragma unroll
    for (int w = 0; w < kD2mThreads / 64; w++) {
      if (w == wave && ((flags >> k) & 1u)) s_list[n + before[k]] = (unsigned short)(k * kD2mThreads + tid);
      n += s_count[k * (kD2mThreads / 64) + w];
    }
  }
  if (n == 0) return;                                        // (uniform)
  __syncthreads();

  const float inf = __int_as_float(0x7f800000);
  for (int first = 0; first < n; first += kD2mThreads) {
    const bool live = first + tid < n;
    const size_t i = base + (live ? s_list[first + tid] : 0);   // (a lane without a point: any pixel, nothing is stored)
    const int row = (int)(i / (size_t)W), col = (int)(i - (size_t)row * W);
    float3x p;
    p.x = ax * (float)col + bx;
    p.y = ay * (float)row + by;
    p.z = live ? obs[i] : 0.f;

    // seed: the nearest corner a
    float near2 = inf;
    int seed = -1;
    for (int c0 = 0; c0 < F; c0 += kD2mChunk) {
      const int cnt = min(kD2mChunk, F - c0);
      __syncthreads();
      for (int t = tid; t < cnt; t += kD2mThreads) s_rec[t] = rec[(size_t)(c0 + t) * 3];
      __syncthreads();
#pragma unroll 4
      for (int t = 0; t < cnt; t++) {
        const float4 a = s_rec[t];
        const float3x ap = {p.x - a.x, p.y - a.y, p.z - a.z};
        const float q = dot3(ap, ap);
        if (q < near2) { near2 = q; seed = c0 + t; }
      }
    }
    float best = inf;
    int bf = -1;
    if (live && seed >= 0) {
      const float4 a = rec[(size_t)seed * 3], ab = rec[(size_t)seed * 3 + 1], ac = rec[(size_t)seed * 3 + 2];
      const float d = tri_dist2({p.x - a.x, p.y - a.y, p.z - a.z}, {ab.x, ab.y, ab.z}, {ac.x, ac.y, ac.z});
      if (d < best) { best = d; bf = seed; }
    }
    float S = cull_root(best);

    for (int c0 = 0; c0 < F; c0 += kD2mChunk) {
      const int cnt = min(kD2mChunk, F - c0);
      __syncthreads();
      for (int t = tid; t < 3 * cnt; t += kD2mThreads) {
        const int plane = t / cnt, r = t - plane * cnt;
        s_rec[plane * kD2mChunk + r] = rec[(size_t)(c0 + r) * 3 + plane];
      }
      __syncthreads();
#pragma unroll 4
      for (int t = 0; t < cnt; t++) {
        const float4 a = s_rec[t];
        const float3x ap = {p.x - a.x, p.y - a.y, p.z - a.z};
        const float q = dot3(ap, ap);
        const float reach = S + a.w;
        if (live && !(q > reach * reach)) {
          const float4 ab = s_rec[kD2mChunk + t], ac = s_rec[2 * kD2mChunk + t];
          const float d = tri_dist2(ap, {ab.x, ab.y, ab.z}, {ac.x, ac.y, ac.z});
          const int f = c0 + t;
          if (d < best || (d == best && f < bf)) { best = d; bf = f; S = cull_root(best); }
        }
      }
    }
    if (live) {
      out_dist[i] = bf >= 0 ? fminf(sqrtf(best), max_dist) : 0.f;
      out_face[i] = bf;
    }
  }
}

// D2mTaps: the W x H pixels, ONE tap each (CoverTaps' pattern, sil_cover.hip) -- on the pixel's saved face.  face is
// checked in d2m_tap.h's d2m_closest, with the face's vertex ids: every index that comes from memory is checked before it
// indexes anything.
template <bool RUNS>
struct D2mTaps {
  const float *observed;
  const float4 *vertices;
  const int *faces;
  const float *dist;
  const int *face;
  const float *grad_dist;
  float ax, bx, ay, by, fg_max, max_dist;
  int F, NV, W, H;
  static constexpr int kThreads = PixelWalk<RUNS>::kThreads, kBlockPix = PixelWalk<RUNS>::kBlockPix;
  static constexpr bool kRuns = RUNS;
  __device__ __forceinline__ int points() const { return NV; }
  template <typename Fn>
  __device__ __forceinline__ void walk(Fn fn) const {
    const int b = blockIdx.y;
    const size_t npix = (size_t)W * H;
    for (int k = 0; k < PixelWalk<RUNS>::kPix; k++) {
      const size_t i = PixelWalk<RUNS>::pixel(k);
      if (i >= npix) break;
      const float z = observed[(size_t)b * npix + i];
      if (!(z < fg_max)) continue;                          // (d2m_measured's first test, here to save the other loads)
      const float d = dist[(size_t)b * npix + i];
      if (!d2m_measured(z, d, fg_max, max_dist)) continue;  // (zero or saturated: a constant)
      const float gd = grad_dist[(size_t)b * npix + i];
      if (gd == 0.f) continue;
      D2mClosest t;
      if (!d2m_closest(vertices + (size_t)b * NV, faces, NV, F, face[(size_t)b * npix + i], i, W, ax, bx, ay, by, z, t)) continue;
      double g[3][3];
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) g[a][c] = -(double)gd * t.wk[a] * (t.e[c] / t.n);
      fn(g, t.pid);
    }
  }
};

}  // namespace shr

// rec[B][F][3] float4
extern "C" long long shr_mesh_d2m_workspace_bytes(int B, int F) {
  if (B < 0 || F < 0) return -1;
  return (long long)B * F * 48;
}

extern "C" int shr_mesh_d2m_fwd(const float *observed, const float *vertices, const int32_t *faces, int B, int NV, int F,
                                int W, int H, float ax, float bx, float ay, float by, float fg_max, float max_dist, float *dist,
                                int32_t *face, void *workspace, void *stream) {
  using namespace shr;
  const int rc = d2m_check(B, NV, F, W, H, max_dist);
  if (rc != SHR_OK) return rc;
  if (B == 0) return SHR_OK;
  if (!observed || !vertices || (!faces && F > 0) || !dist || !face || (!workspace && F > 0)) return SHR_EINVAL;
  if ((((uintptr_t)observed | (uintptr_t)faces | (uintptr_t)dist | (uintptr_t)face) & 3u) != 0) return SHR_EINVAL;
  if ((((uintptr_t)vertices | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float4 *rec = reinterpret_cast<float4 *>(workspace);
  if (F > 0)
    hipLaunchKernelGGL(d2m_records_kernel, dim3((unsigned)((F + kD2mRecThreads - 1) / kD2mRecThreads), (unsigned)B),
                       dim3(kD2mRecThreads), 0, s, reinterpret_cast<const float4 *>(vertices), faces, NV, F, rec);
  const size_t npix = (size_t)H * W;
  hipLaunchKernelGGL(d2m_search_kernel, dim3((unsigned)((npix + kD2mTilePix - 1) / kD2mTilePix), (unsigned)B),
                     dim3(kD2mThreads), 0, s, observed, rec, F, H, W, ax, bx, ay, by, fg_max, max_dist, dist, face);
  return (int)hipGetLastError();
}

extern "C" long long shr_mesh_d2m_bwd_workspace_bytes(int B, int NV) { return fix_workspace_bytes(B, NV); }

// A vertex's accumulator takes at most three terms per pixel (its face's three corners): fix_term_bits(3, W, H).
extern "C" int shr_mesh_d2m_bwd(const float *observed, const float *vertices, const int32_t *faces, const float *dist,
                                const int32_t *face, const float *grad_dist, int B, int NV, int F, int W, int H, float ax,
                                float bx, float ay, float by, float fg_max, float max_dist, float *grad_vertices,
                                void *workspace, void *stream) {
  using namespace shr;
  const int rc = d2m_check(B, NV, F, W, H, max_dist);
  if (rc != SHR_OK) return rc;
  if (B == 0) return SHR_OK;
  if (!observed || !vertices || (!faces && F > 0) || !dist || !face || !grad_dist || !grad_vertices || !workspace)
    return SHR_EINVAL;
  if ((((uintptr_t)observed | (uintptr_t)faces | (uintptr_t)dist | (uintptr_t)face | (uintptr_t)grad_dist) & 3u) != 0)
    return SHR_EINVAL;
  if ((((uintptr_t)vertices | (uintptr_t)grad_vertices | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  return with_runs(NV, [&](auto runs) {
    return fixed_point_bwd<4>(D2mTaps<decltype(runs)::value>{observed, reinterpret_cast<const float4 *>(vertices), faces, dist,
                                                             face, grad_dist, ax, bx, ay, by, fg_max, max_dist, F, NV, W, H},
                              B, NV, (size_t)W * H, fix_term_bits(3, W, H), grad_vertices, workspace, (hipStream_t)stream);
  });
}
