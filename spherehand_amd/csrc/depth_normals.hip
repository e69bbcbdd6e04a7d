// depth_normals.hip -- the unit normal map of a depth image by discontinuity-aware differences (shr_depth_normals_fwd)
// and its backward to the depth (shr_depth_normals_bwd).  include/spherehand_hip.h states the contract, DESIGN.md 4.4k
// the layout and the figures.
//
//   forward        one lane per pixel in tiles of 64 x 4 (a wave per row piece: every tap row is one coalesced request):
//                  the pixel and its four neighbours through dn_tap, the two differences, N, unit3, three plane stores.
//   backward       one lane per pixel, the same tiles: a gather in fixed order over the normals at the pixel and at its
//                  left, right, upper and lower neighbour.  Each of those pixels' fp32 decisions is made again by the
//                  forward's own function from its own five taps (13 distinct depths per lane, read through L1 / L2: the
//                  tile's rows are shared by its four waves), its G = (g - n (n . g)) / |N| evaluated in fp64 only when
//                  the pixel reads this one, and the sum rounded once.  A lane whose own pixel is no site stores 0 before
//                  any of that.  No LDS, no atomics, no workspace.
#include "common.h"
#include "unit3.h"

namespace shr {

constexpr int kDnTileW = 64;   // one wave per tile row
constexpr int kDnTileH = 4;
constexpr int kDnThreads = kDnTileW * kDnTileH;

struct DnArgs {
  int H, W;
  float fg_max, sx, sy, max_step;
};

// depth[i][j] of one crop; false (and pixel 0's value, never used) outside the image: no address outside it is formed
__device__ __forceinline__ bool dn_tap(const float *__restrict__ img, int H, int W, int i, int j, float &v) {
  const bool in = (unsigned)i < (unsigned)H && (unsigned)j < (unsigned)W;
  v = img[in ? (size_t)i * W + j : (size_t)0];
  return in;
}

// the discontinuity rule: a neighbour inside the image, foreground and within max_step of the centre (false on a NaN)
__device__ __forceinline__ bool dn_usable(bool in, float n, float c, const DnArgs &A) {
  return in && n < A.fg_max && fabsf(n - c) <= A.max_step;
}

// a pixel's fp32 decisions and differences; lo / hi are the neighbours at the smaller / larger index of each axis
struct DnPixel {
  float c, xl, xh, yl, yh;     // the taps: centre, left, right, upper, lower
  bool uxl, uxh, uyl, uyh;     // usable
  float dx, dy, wx, wy;
};

// false: the pixel has no normal (not a site, or an axis without a usable neighbour)
__device__ __forceinline__ bool dn_pixel(const float *__restrict__ img, int i, int j, const DnArgs &A, DnPixel &p) {
  dn_tap(img, A.H, A.W, i, j, p.c);
  const bool il = dn_tap(img, A.H, A.W, i, j - 1, p.xl), ih = dn_tap(img, A.H, A.W, i, j + 1, p.xh);
  const bool iu = dn_tap(img, A.H, A.W, i - 1, j, p.yl), id = dn_tap(img, A.H, A.W, i + 1, j, p.yh);
  p.uxl = dn_usable(il, p.xl, p.c, A);
  p.uxh = dn_usable(ih, p.xh, p.c, A);
  p.uyl = dn_usable(iu, p.yl, p.c, A);
  p.uyh = dn_usable(id, p.yh, p.c, A);
  p.dx = (p.uxl && p.uxh) ? p.xh - p.xl : (p.uxh ? p.xh - p.c : p.c - p.xl);
  p.dy = (p.uyl && p.uyh) ? p.yh - p.yl : (p.uyh ? p.yh - p.c : p.c - p.yl);
  p.wx = ((p.uxl && p.uxh) ? 2.f : 1.f) * A.sx;
  p.wy = ((p.uyl && p.uyh) ? 2.f : 1.f) * A.sy;
  return p.c < A.fg_max && (p.uxl || p.uxh) && (p.uyl || p.uyh);
}

// N = (dx wy, dy wx, -(wx wy)) and n = unit3(N); false under the zero rule
__device__ __forceinline__ bool dn_normal(const DnPixel &p, float (&n)[3]) {
  const float N[3] = {p.dx * p.wy, p.dy * p.wx, -(p.wx * p.wy)};
  return unit3(N, n);
}

// the pixel of lane threadIdx.x in tile blockIdx.x; false outside the image
__device__ __forceinline__ bool dn_lane_pixel(int H, int W, int &i, int &j) {
  const int tiles_x = (W + kDnTileW - 1) / kDnTileW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  i = ty * kDnTileH + (threadIdx.x / kDnTileW);
  j = tx * kDnTileW + (threadIdx.x % kDnTileW);
  return i < H && j < W;
}

__global__ void __launch_bounds__(kDnThreads)
depth_normals_fwd_kernel(const float *__restrict__ depth, DnArgs A, float *__restrict__ normals) {
  int i, j;
  if (!dn_lane_pixel(A.H, A.W, i, j)) return;
  const size_t plane = (size_t)A.H * A.W;
  DnPixel p;
  float n[3] = {0.f, 0.f, 0.f};
  if (dn_pixel(depth + blockIdx.y * plane, i, j, A, p)) dn_normal(p, n);
  float *out = normals + blockIdx.y * 3 * plane + (size_t)i * A.W + j;
  out[0] = n[0];
  out[plane] = n[1];
  out[2 * plane] = n[2];
}

// where q lies as seen from the pixel whose gradient is gathered
enum DnRole { kDnSelf, kDnLeft, kDnRight, kDnUp, kDnDown };

// d <grad_normals, normals> / d depth[p] through the normal at q = (qi, qj): 0 unless q lies in the image, has a normal
// and read depth[p]
template <DnRole ROLE>
__device__ __forceinline__ double dn_contribution(const float *__restrict__ img, const float *__restrict__ grad, size_t plane,
                                                  int qi, int qj, const DnArgs &A) {
  if ((unsigned)qi >= (unsigned)A.H || (unsigned)qj >= (unsigned)A.W) return 0.0;
  DnPixel q;
  if (!dn_pixel(img, qi, qj, A, q)) return 0.0;
  // the coefficient of depth[p] in q's dx and dy
  int cx = 0, cy = 0;
  if (ROLE == kDnSelf) {
    cx = (q.uxl && q.uxh) ? 0 : (q.uxh ? -1 : 1);
    cy = (q.uyl && q.uyh) ? 0 : (q.uyh ? -1 : 1);
  }
  if (ROLE == kDnLeft) cx = q.uxh ? 1 : 0;      // p is q's right neighbour
  if (ROLE == kDnRight) cx = q.uxl ? -1 : 0;    // ... left
  if (ROLE == kDnUp) cy = q.uyh ? 1 : 0;        // ... lower
  if (ROLE == kDnDown) cy = q.uyl ? -1 : 0;     // ... upper
  if (cx == 0 && cy == 0) return 0.0;
  float n32[3];
  if (!dn_normal(q, n32)) return 0.0;
  const double c = (double)q.c;
  const double dx = (q.uxl && q.uxh) ? (double)q.xh - (double)q.xl : (q.uxh ? (double)q.xh - c : c - (double)q.xl);
  const double dy = (q.uyl && q.uyh) ? (double)q.yh - (double)q.yl : (q.uyh ? (double)q.yh - c : c - (double)q.yl);
  const double wx = (double)q.wx, wy = (double)q.wy;
  const double M[3] = {dx * wy, dy * wx, -(wx * wy)};
  const double s = (M[0] * M[0] + M[1] * M[1]) + M[2] * M[2];
  if (!(s > 0.0 && s <= 1.7976931348623157e308)) return 0.0;
  const size_t at = (size_t)qi * A.W + qj;
  const double g[3] = {(double)grad[at], (double)grad[at + plane], (double)grad[at + 2 * plane]};
  // (one fp64 root and one division per pixel q: 1 / |N| multiplies where shr_unit3_maps_bwd divides five times -- a few
  // units of 2^-53 apart, far below the one rounding to fp32 -- since this lane pays for up to five pixels)
  const double inv = 1.0 / sqrt(s);
  const double n[3] = {M[0] * inv, M[1] * inv, M[2] * inv};
  const double ng = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2];
  const double Gx = (g[0] - n[0] * ng) * inv, Gy = (g[1] - n[1] * ng) * inv;
  return (Gx * wy) * (double)cx + (Gy * wx) * (double)cy;
}

__global__ void __launch_bounds__(kDnThreads)
depth_normals_bwd_kernel(const float *__restrict__ depth, const float *__restrict__ grad_normals, DnArgs A,
                         float *__restrict__ grad_depth) {
  int i, j;
  if (!dn_lane_pixel(A.H, A.W, i, j)) return;
  const size_t plane = (size_t)A.H * A.W;
  const float *img = depth + blockIdx.y * plane;
  const float *grad = grad_normals + blockIdx.y * 3 * plane;
  float *out = grad_depth + blockIdx.y * plane + (size_t)i * A.W + j;
  if (!(img[(size_t)i * A.W + j] < A.fg_max)) {   // no site: it has no normal and is usable to no neighbour
    *out = 0.f;
    return;
  }
  double acc = dn_contribution<kDnSelf>(img, grad, plane, i, j, A);
  acc += dn_contribution<kDnLeft>(img, grad, plane, i, j - 1, A);
  acc += dn_contribution<kDnRight>(img, grad, plane, i, j + 1, A);
  acc += dn_contribution<kDnUp>(img, grad, plane, i - 1, j, A);
  acc += dn_contribution<kDnDown>(img, grad, plane, i + 1, j, A);
  *out = (float)acc;
}

}  // namespace shr

static bool dn_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

static int dn_check(int B, int W, int H, float fg_max, float sx, float sy, float max_step) {
  if (B < 0 || W <= 0 || H <= 0) return SHR_EINVAL;
  if (!(sx > 0.f && sx <= shr::kNrmMaxFinite) || !(sy > 0.f && sy <= shr::kNrmMaxFinite)) return SHR_EINVAL;
  if (fg_max != fg_max || !(max_step >= 0.f)) return SHR_EINVAL;
  if (B > 65535 || W > 65535 || H > 65535) return SHR_ETOOLARGE;
  return SHR_OK;
}

static dim3 dn_grid(int B, int W, int H) {
  using namespace shr;
  return dim3((unsigned)(((W + kDnTileW - 1) / kDnTileW) * ((H + kDnTileH - 1) / kDnTileH)), (unsigned)B);
}

extern "C" int shr_depth_normals_fwd(const float *depth, int B, int W, int H, float fg_max, float sx, float sy,
                                     float max_step, float *normals, void *stream) {
  using namespace shr;
  const int rc = dn_check(B, W, H, fg_max, sx, sy, max_step);
  if (rc != SHR_OK) return rc;
  if (B == 0) return SHR_OK;
  if (!depth || !normals || (((uintptr_t)depth | (uintptr_t)normals) & 3u) != 0) return SHR_EINVAL;
  const size_t bytes = (size_t)B * H * W * sizeof(float);
  if (dn_overlap(depth, bytes, normals, 3 * bytes)) return SHR_EINVAL;
  const DnArgs A{H, W, fg_max, sx, sy, max_step};
  hipLaunchKernelGGL(depth_normals_fwd_kernel, dn_grid(B, W, H), dim3(kDnThreads), 0, (hipStream_t)stream, depth, A, normals);
  return (int)hipGetLastError();
}

extern "C" int shr_depth_normals_bwd(const float *depth, const float *grad_normals, int B, int W, int H, float fg_max,
                                     float sx, float sy, float max_step, float *grad_depth, void *stream) {
  using namespace shr;
  const int rc = dn_check(B, W, H, fg_max, sx, sy, max_step);
  if (rc != SHR_OK) return rc;
  if (B == 0) return SHR_OK;
  if (!depth || !grad_normals || !grad_depth ||
      (((uintptr_t)depth | (uintptr_t)grad_normals | (uintptr_t)grad_depth) & 3u) != 0)
    return SHR_EINVAL;
  const size_t bytes = (size_t)B * H * W * sizeof(float);
  if (dn_overlap(grad_depth, bytes, depth, bytes) || dn_overlap(grad_depth, bytes, grad_normals, 3 * bytes)) return SHR_EINVAL;
  const DnArgs A{H, W, fg_max, sx, sy, max_step};
  hipLaunchKernelGGL(depth_normals_bwd_kernel, dn_grid(B, W, H), dim3(kDnThreads), 0, (hipStream_t)stream, depth,
                     grad_normals, A, grad_depth);
  return (int)hipGetLastError();
}
