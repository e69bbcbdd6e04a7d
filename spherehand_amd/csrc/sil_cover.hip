// sil_cover.hip -- the silhouette term's other half: the distance transform WITH its argument, the nearest site of every
// pixel (shr_dt_nearest_fwd), and the coverage distance of observed pixels to the rendered silhouette with its route to
// the vertices (shr_sil_cover_fwd / _bwd).  include/spherehand_hip.h states the contract, DESIGN.md 4.4i the layout and
// the figures.  The passes are this unit's own (dist_transform.hip's carry no argument); the site rule, the limits and
// the d2 bits are shr_dt_fwd's.
// dn_column_kernel is dt_column_kernel (dist_transform.hip) statement for statement except for dn_pick in the second
// sweep, and dn_row_kernel follows dt_row_kernel's search: that unit's source and code object are pinned by its tests, so
// the sweeps are written twice -- a fix to one of them belongs in the other too.
//
//   column pass    one lane per PAIR of adjacent columns, as dist_transform.hip's.  Sweep up: the distance to the nearest
//                  site at or below, 16 bits per column.  Sweep down: the lane reads its words back (0 = a site), compares
//                  with the distance to the nearest site at or above and stores g, the vertical distance to the column's
//                  nearest site, with bit 15 set when that site lies BELOW the pixel; an up / down tie goes to the site
//                  above (the smaller row).  g <= 2047 leaves the bit free; kDnNone: the column has no site.
//   row pass       one wave per row: per column the 64-bit key (g^2 << 22) | (site row * W + x') in LDS (a column without
//                  a site: (H H + W W) << 22), then a lane per pixel in segments of 64 consecutive x: the minimum over x'
//                  of key[x'] + ((x - x')^2 << 22) -- the pair (total, index) in lexicographic order as one integer --
//                  searched outward from x' = x while r^2 <= the best total so far (a term EQUAL to the best may still
//                  have a smaller index).  d2 = key >> 22, nearest = its low 22 bits, -1 when d2 is the empty value.
//                  Integers only: exact, whatever the launch shape.
//   cover forward  one thread per pixel.
//   cover backward fixed_point.h's passes over CoverTaps: one tap per contributing observed pixel p, at its nearest
//                  rendered pixel q, on q's owner face with the weights the depth used there (tri_tap.h), held fixed.
#include "fixed_point.h"
#include "tri_tap.h"

namespace shr {

constexpr int kDnMaxSide = 2048;      // d2 < 2^24, an index < 2^22, g < 2^15
constexpr unsigned kDnNone = 0xffffu; // g of a column with no site (in the direction swept so far)
constexpr unsigned kDnBelow = 0x8000u;   // the column's nearest site lies below the pixel
constexpr int kDnIndexBits = 22;      // H W <= 2^22
constexpr int kDnColThreads = 64;     // column pass: one wave of column pairs per workgroup
constexpr int kDnColRows = 8;         // ... rows requested together
constexpr int kDnRowWaves = 2;        // row pass: rows (waves) per workgroup -- 16 W bytes of LDS, 32 KB at the widest
constexpr int kDnRowStep = 4;         // ... distances searched per round
constexpr int kCoverThreads = 256;

__device__ __forceinline__ unsigned dn_step(unsigned dist, bool site) {
  return site ? 0u : (dist == kDnNone ? kDnNone : dist + 1u);
}
// the distances to the nearest site at or above and at or below -> g, bit 15 = below; a tie: above
__device__ __forceinline__ unsigned dn_pick(unsigned above, unsigned below) {
  return above <= below ? above : (below | kDnBelow);   // (both kDnNone: kDnNone)
}

// ws[b][i][pair]: low half column 2 pair, high half column 2 pair + 1 (a column >= W: kDnNone, never read back)
__global__ void __launch_bounds__(kDnColThreads)
dn_column_kernel(const float *__restrict__ depth, int H, int W, float fg_max, uint32_t *__restrict__ ws) {
  const int pairs = (W + 1) >> 1;
  const int pair = blockIdx.x * kDnColThreads + threadIdx.x;
  if (pair >= pairs) return;
  const int x0 = 2 * pair;
  const bool two = x0 + 1 < W;
  const float *img = depth + (size_t)blockIdx.y * H * W + x0;
  uint32_t *col = ws + (size_t)blockIdx.y * H * pairs + pair;
  unsigned d0 = kDnNone, d1 = kDnNone;
  for (int top = H; top > 0; top -= kDnColRows) {          // rows top - 1 down to top - kDnColRows
    float a[kDnColRows], b[kDnColRows];
#pragma unroll
    for (int k = 0; k < kDnColRows; k++) {
      const int i = top - 1 - k;
      a[k] = i >= 0 ? img[(size_t)i * W] : fg_max;
      b[k] = (i >= 0 && two) ? img[(size_t)i * W + 1] : fg_max;
    }
#pragma unroll
    for (int k = 0; k < kDnColRows; k++) {
      const int i = top - 1 - k;
      if (i < 0) break;
      d0 = dn_step(d0, a[k] < fg_max);                      // (NaN < fg_max is false: not a site)
      d1 = two ? dn_step(d1, b[k] < fg_max) : kDnNone;
      col[(size_t)i * pairs] = d0 | (d1 << 16);
    }
  }
  d0 = d1 = kDnNone;
  for (int top = 0; top < H; top += kDnColRows) {
    uint32_t up[kDnColRows];
#pragma unroll
    for (int k = 0; k < kDnColRows; k++) up[k] = top + k < H ? col[(size_t)(top + k) * pairs] : 0u;
#pragma unroll
    for (int k = 0; k < kDnColRows; k++) {
      if (top + k >= H) break;
      const unsigned u0 = up[k] & 0xffffu, u1 = up[k] >> 16;
      d0 = dn_step(d0, u0 == 0u);
      d1 = dn_step(d1, u1 == 0u);
      col[(size_t)(top + k) * pairs] = dn_pick(d0, u0) | (dn_pick(d1, u1) << 16);
    }
  }
}

// column x' of row i: its word -> (g^2 << 22) | (site row * W + x')
__device__ __forceinline__ long long dn_key(unsigned word, int i, int xs, int W, int none2) {
  if (word == kDnNone) return (long long)none2 << kDnIndexBits;
  const int g = (int)(word & (kDnBelow - 1u));
  const int row = (word & kDnBelow) ? i + g : i - g;
  return ((long long)(g * g) << kDnIndexBits) | (long long)(row * W + xs);
}

// dynamic LDS: kDnRowWaves rows of W keys
__global__ void __launch_bounds__(kDnRowWaves * 64)
dn_row_kernel(const uint32_t *__restrict__ ws, int H, int W, int32_t *__restrict__ d2, int32_t *__restrict__ nearest) {
  extern __shared__ long long dn_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kDnRowWaves + wave;
  const int pairs = (W + 1) >> 1;
  const int none2 = H * H + W * W;
  long long *key = dn_lds + (size_t)wave * W;
  if (i < H) {
    const uint32_t *row = ws + ((size_t)blockIdx.y * H + i) * pairs;
    for (int p = lane; p < pairs; p += 64) {
      const uint32_t w = row[p];
      key[2 * p] = dn_key(w & 0xffffu, i, 2 * p, W, none2);
      if (2 * p + 1 < W) key[2 * p + 1] = dn_key(w >> 16, i, 2 * p + 1, W, none2);
    }
  }
  __syncthreads();
  if (i >= H) return;
  const size_t at = ((size_t)blockIdx.y * H + i) * W;
  for (int x = lane; x < W; x += 64) {
    long long best = key[x];
    const int r_max = max(x, W - 1 - x);
    // kDnRowStep distances per round, their LDS reads requested together.  An index clamped into the row pairs an entry
    // with an r^2 LARGER than its own (x - x')^2: the same index at a larger total than the entry's own term, which was
    // offered before (its distance is smaller), so it never wins.  A round may run past the stopping distance: every
    // value offered is a term or loses to one, and every term with r^2 <= the best total is offered
    for (int r = 1; r <= r_max && r * r <= (int)(best >> kDnIndexBits); r += kDnRowStep) {
      long long a[kDnRowStep], b[kDnRowStep];
#pragma unroll
      for (int k = 0; k < kDnRowStep; k++) {
        a[k] = key[max(x - (r + k), 0)];
        b[k] = key[min(x + (r + k), W - 1)];
      }
#pragma unroll
      for (int k = 0; k < kDnRowStep; k++)
        best = min(best, min(a[k], b[k]) + ((long long)((r + k) * (r + k)) << kDnIndexBits));
    }
    const int total = (int)(best >> kDnIndexBits);
    d2[at + x] = total;
    nearest[at + x] = total >= none2 ? -1 : (int)(best & ((1ll << kDnIndexBits) - 1));
  }
}

__global__ void __launch_bounds__(kCoverThreads)
sil_cover_fwd_kernel(const float *__restrict__ observed, float obs_fg_max, const int32_t *__restrict__ d2, size_t n,
                     float max_dist, float *__restrict__ dist) {
  const size_t i = (size_t)blockIdx.x * kCoverThreads + threadIdx.x;
  if (i >= n) return;
  dist[i] = observed[i] < obs_fg_max ? fminf(sqrtf((float)d2[i]), max_dist) : 0.f;   // (NaN: not observed)
}

// CoverTaps: the W x H observed pixels, ONE tap each (PixelTaps' pattern, mesh_depth_bwd.hip) -- at the pixel's nearest
// rendered pixel q, on q's owner face.  nearest is checked here, owner and the face's vertex ids in tri_tap.h's live_tap:
// every index that comes from memory is checked before it indexes anything.
template <bool RUNS>
struct CoverTaps {
  const float *observed;
  const int *d2;
  const int *nearest;
  const int *owner;
  const float4 *vertices;
  const int *faces;
  const float *grad_dist;
  float obs_fg_max, max_dist;
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
      if (!(observed[(size_t)b * npix + i] < obs_fg_max)) continue;
      const int dd = d2[(size_t)b * npix + i];
      if (dd <= 0) continue;                               // (covered: the distance is at its minimum)
      if (!(sqrtf((float)dd) <= max_dist)) continue;        // (saturated: a constant)
      const float gd = grad_dist[(size_t)b * npix + i];
      if (gd == 0.f) continue;
      const int q = nearest[(size_t)b * npix + i];
      if ((unsigned)q >= (unsigned)npix) continue;         // (-1: the render is empty)
      const int f = owner[(size_t)b * npix + q];
      const int yq = q / W, xq = q - yq * W;
      OwnedTap T;
      int pid[3];
      if (!live_tap(vertices + (size_t)b * NV, faces, NV, F, f, xq, yq, T, pid)) continue;   // (checks f and the ids)
      const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
      const double d = sqrt((double)dd);
      double G[3][3], g[3][3];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double wg = -(double)gd * (T.c[a] / T.s);
        G[a][0] = wg * (double)(x - xq) / d;
        G[a][1] = wg * (double)(y - yq) / d;
        G[a][2] = 0.0;
      }
      tap_unsort(G, T.order, g);
      fn(g, pid);
    }
  }
};

}  // namespace shr

static int dn_check_image(int B, int H, int W) {
  if (B < 0 || H < 1 || W < 1) return SHR_EINVAL;
  if (B > 65535 || H > shr::kDnMaxSide || W > shr::kDnMaxSide) return SHR_ETOOLARGE;
  return SHR_OK;
}

// g[B][H][ceil(W/2)][2] uint16
extern "C" long long shr_dt_nearest_workspace_bytes(int B, int H, int W) {
  if (B < 0 || H < 0 || W < 0) return -1;
  return (((long long)B * H * ((W + 1) / 2) * 4) + 15) / 16 * 16;
}

extern "C" int shr_dt_nearest_fwd(const float *depth, int B, int H, int W, float fg_max, int32_t *d2, int32_t *nearest,
                                  void *workspace, void *stream) {
  using namespace shr;
  const int rc = dn_check_image(B, H, W);
  if (rc != SHR_OK) return rc;
  if (B == 0) return SHR_OK;
  if (!depth || !d2 || !nearest || !workspace) return SHR_EINVAL;
  if ((((uintptr_t)depth | (uintptr_t)d2 | (uintptr_t)nearest) & 3u) != 0 || (((uintptr_t)workspace) & 15u) != 0)
    return SHR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  uint32_t *ws = reinterpret_cast<uint32_t *>(workspace);
  const int pairs = (W + 1) / 2;
  hipLaunchKernelGGL(dn_column_kernel, dim3((unsigned)((pairs + kDnColThreads - 1) / kDnColThreads), (unsigned)B),
                     dim3(kDnColThreads), 0, s, depth, H, W, fg_max, ws);
  hipLaunchKernelGGL(dn_row_kernel, dim3((unsigned)((H + kDnRowWaves - 1) / kDnRowWaves), (unsigned)B),
                     dim3(kDnRowWaves * 64), (size_t)kDnRowWaves * W * sizeof(long long), s, ws, H, W, d2, nearest);
  return (int)hipGetLastError();
}

extern "C" int shr_sil_cover_fwd(const float *observed, float obs_fg_max, const int32_t *d2, int B, int H, int W,
                                 float max_dist, float *dist, void *stream) {
  using namespace shr;
  if (!(max_dist >= 0.f)) return SHR_EINVAL;
  const int rc = dn_check_image(B, H, W);
  if (rc != SHR_OK) return rc;
  if (B == 0) return SHR_OK;
  if (!observed || !d2 || !dist) return SHR_EINVAL;
  if ((((uintptr_t)observed | (uintptr_t)d2 | (uintptr_t)dist) & 3u) != 0) return SHR_EINVAL;
  const size_t n = (size_t)B * H * W;
  hipLaunchKernelGGL(sil_cover_fwd_kernel, dim3((unsigned)((n + kCoverThreads - 1) / kCoverThreads)), dim3(kCoverThreads), 0,
                     (hipStream_t)stream, observed, obs_fg_max, d2, n, max_dist, dist);
  return (int)hipGetLastError();
}

extern "C" long long shr_sil_cover_bwd_workspace_bytes(int B, int NV) { return fix_workspace_bytes(B, NV); }

// A vertex's accumulator takes at most three terms per observed pixel (its face's three corners, one vertex each unless
// the face repeats one): fix_term_bits(3, W, H).
extern "C" int shr_sil_cover_bwd(const float *observed, float obs_fg_max, const int32_t *d2, const int32_t *nearest,
                                 const int32_t *owner, const float *vertices, const int32_t *faces, const float *grad_dist,
                                 int B, int NV, int F, int W, int H, float max_dist, float *grad_vertices, void *workspace,
                                 void *stream) {
  using namespace shr;
  if (!(max_dist >= 0.f) || NV <= 0 || F < 0) return SHR_EINVAL;
  const int rc = dn_check_image(B, H, W);
  if (rc != SHR_OK) return rc;
  if ((long long)NV * 3 >= (1LL << 31) || 3LL * F >= (1LL << 31)) return SHR_ETOOLARGE;
  if (B == 0) return SHR_OK;
  if (!observed || !d2 || !nearest || !owner || !vertices || (!faces && F > 0) || !grad_dist || !grad_vertices || !workspace)
    return SHR_EINVAL;
  if ((((uintptr_t)observed | (uintptr_t)d2 | (uintptr_t)nearest | (uintptr_t)owner | (uintptr_t)faces |
        (uintptr_t)grad_dist) & 3u) != 0)
    return SHR_EINVAL;
  if ((((uintptr_t)vertices | (uintptr_t)grad_vertices | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  return with_runs(NV, [&](auto runs) {
    return fixed_point_bwd<4>(CoverTaps<decltype(runs)::value>{observed, d2, nearest, owner,
                                                               reinterpret_cast<const float4 *>(vertices), faces, grad_dist,
                                                               obs_fg_max, max_dist, F, NV, W, H},
                              B, NV, (size_t)W * H, fix_term_bits(3, W, H), grad_vertices, workspace, (hipStream_t)stream);
  });
}
