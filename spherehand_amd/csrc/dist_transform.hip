// dist_transform.hip -- the exact squared Euclidean distance transform of a depth image's foreground (shr_dt_fwd) and
// its bilinear sampler at points (shr_dt_sample_fwd / _bwd).  include/spherehand_hip.h states the contract, DESIGN.md
// 4.4h the layout and the figures.
//
//   column pass    one lane per PAIR of adjacent columns, lanes on consecutive pairs (a row read is one coalesced line per
//                  column of the pair).  Sweep up: the distance to the nearest site at or below, 16 bits per column, the
//                  pair packed into one 4-byte store to the workspace.  Sweep down: the lane reads its own words back (0 =
//                  the pixel is a site: the depth is read once), takes the minimum with the distance to the nearest site
//                  at or above, and stores g, the vertical distance to the column's nearest site (kDtNone: no site).
//   row pass       one wave per row: the row's g^2 in LDS (a column without a site: H H + W W), then a lane per pixel in
//                  segments of 64 consecutive x:  d2[x] = min over x' of (x - x')^2 + g^2[x'], searched outward from x' = x
//                  and stopped once r^2 >= the best so far (every later term is at least r^2).  Lanes of a segment read
//                  consecutive LDS words: no bank conflict.  Integers only: exact, whatever the launch shape.
//   sampler        one thread per point (forward), one per element of grad_points (backward): gathers, no reduction.
#include "common.h"

namespace shr {

constexpr int kDtMaxSide = 2048;      // d2 < 2^24: exact in fp32; g < kDtNone
constexpr unsigned kDtNone = 0xffffu; // g of a column with no site (in the direction swept so far)
constexpr int kDtColThreads = 64;     // column pass: one wave of column pairs per workgroup
constexpr int kDtColRows = 8;         // ... rows requested together
constexpr int kDtRowWaves = 4;        // row pass: rows (waves) per workgroup
constexpr int kDtRowStep = 4;         // ... distances searched per round
constexpr int kDtSampleThreads = 256;

__device__ __forceinline__ unsigned dt_step(unsigned dist, bool site) {
  return site ? 0u : (dist == kDtNone ? kDtNone : dist + 1u);
}

// ws[b][i][pair]: low half column 2 pair, high half column 2 pair + 1 (a column >= W: kDtNone, never read back as g)
__global__ void __launch_bounds__(kDtColThreads)
dt_column_kernel(const float *__restrict__ depth, int H, int W, float fg_max, uint32_t *__restrict__ ws) {
  const int pairs = (W + 1) >> 1;
  const int pair = blockIdx.x * kDtColThreads + threadIdx.x;
  if (pair >= pairs) return;
  const int x0 = 2 * pair;
  const bool two = x0 + 1 < W;
  const float *img = depth + (size_t)blockIdx.y * H * W + x0;
  uint32_t *col = ws + (size_t)blockIdx.y * H * pairs + pair;
  unsigned d0 = kDtNone, d1 = kDtNone;
  for (int top = H; top > 0; top -= kDtColRows) {          // rows top - 1 down to top - kDtColRows
    float a[kDtColRows], b[kDtColRows];
#pragma unroll
    for (int k = 0; k < kDtColRows; k++) {
      const int i = top - 1 - k;
      a[k] = i >= 0 ? img[(size_t)i * W] : fg_max;
      b[k] = (i >= 0 && two) ? img[(size_t)i * W + 1] : fg_max;
    }
#pragma unroll
    for (int k = 0; k < kDtColRows; k++) {
      const int i = top - 1 - k;
      if (i < 0) break;
      d0 = dt_step(d0, a[k] < fg_max);                      // (NaN < fg_max is false: not a site)
      d1 = two ? dt_step(d1, b[k] < fg_max) : kDtNone;
      col[(size_t)i * pairs] = d0 | (d1 << 16);
    }
  }
  d0 = d1 = kDtNone;
  for (int top = 0; top < H; top += kDtColRows) {
    uint32_t up[kDtColRows];
#pragma unroll
    for (int k = 0; k < kDtColRows; k++) up[k] = top + k < H ? col[(size_t)(top + k) * pairs] : 0u;
#pragma unroll
    for (int k = 0; k < kDtColRows; k++) {
      if (top + k >= H) break;
      const unsigned u0 = up[k] & 0xffffu, u1 = up[k] >> 16;
      d0 = dt_step(d0, u0 == 0u);
      d1 = dt_step(d1, u1 == 0u);
      col[(size_t)(top + k) * pairs] = min(d0, u0) | (min(d1, u1) << 16);
    }
  }
}

// dynamic LDS: kDtRowWaves rows of W ints
__global__ void __launch_bounds__(kDtRowWaves * 64)
dt_row_kernel(const uint32_t *__restrict__ ws, int H, int W, int32_t *__restrict__ d2) {
  extern __shared__ int dt_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kDtRowWaves + wave;
  const int pairs = (W + 1) >> 1;
  const int none2 = H * H + W * W;
  int *g2 = dt_lds + wave * W;
  if (i < H) {
    const uint32_t *row = ws + ((size_t)blockIdx.y * H + i) * pairs;
    for (int p = lane; p < pairs; p += 64) {
      const uint32_t w = row[p];
      const int lo = (int)(w & 0xffffu), hi = (int)(w >> 16);
      g2[2 * p] = lo == (int)kDtNone ? none2 : lo * lo;
      if (2 * p + 1 < W) g2[2 * p + 1] = hi == (int)kDtNone ? none2 : hi * hi;
    }
  }
  __syncthreads();
  if (i >= H) return;
  int32_t *out = d2 + ((size_t)blockIdx.y * H + i) * W;
  for (int x = lane; x < W; x += 64) {
    int best = g2[x];
    const int r_max = max(x, W - 1 - x);
    // kDtRowStep distances per round, their LDS reads requested together.  An index clamped into the row pairs an entry
    // with an r^2 at least its own (x - x')^2, and a round may run past the stopping distance: every value offered is
    // at least the term it stands for, and every term within the stopping distance is offered
    for (int r = 1; r * r < best && r <= r_max; r += kDtRowStep) {
      int a[kDtRowStep], b[kDtRowStep];
#pragma unroll
      for (int k = 0; k < kDtRowStep; k++) {
        a[k] = g2[max(x - (r + k), 0)];
        b[k] = g2[min(x + (r + k), W - 1)];
      }
#pragma unroll
      for (int k = 0; k < kDtRowStep; k++) best = min(best, (r + k) * (r + k) + min(a[k], b[k]));
    }
    out[x] = best;
  }
}

__device__ __forceinline__ bool dt_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // (false for NaN)

// xc = min(max(x, 0), n - 1), i0 = min(floor(xc), n - 2), f = xc - i0; returns whether x was clamped
__device__ __forceinline__ bool dt_cell(float x, int n, int &i0, float &f) {
  const float xc = fminf(fmaxf(x, 0.f), (float)(n - 1));
  const float x0 = fminf(floorf(xc), (float)(n - 2));
  i0 = (int)x0;
  f = xc - x0;
  return xc != x;
}

__global__ void __launch_bounds__(kDtSampleThreads)
dt_sample_fwd_kernel(const int32_t *__restrict__ d2, int H, int W, const float *__restrict__ points, int N, int C,
                     float max_dist, float *__restrict__ value, float *__restrict__ grad_xy) {
  const int n = blockIdx.x * kDtSampleThreads + threadIdx.x;
  if (n >= N) return;
  const size_t at = (size_t)blockIdx.y * N + n;
  const float x = points[at * C], y = points[at * C + 1];
  float v = 0.f, gx = 0.f, gy = 0.f;
  if (dt_finite(x) && dt_finite(y)) {
    int x0, y0;
    float fx, fy;
    const bool cx = dt_cell(x, W, x0, fx), cy = dt_cell(y, H, y0, fy);
    const int32_t *tap = d2 + ((size_t)blockIdx.y * H + y0) * W + x0;
    const float t00 = fminf(sqrtf((float)tap[0]), max_dist), t01 = fminf(sqrtf((float)tap[1]), max_dist);
    const float t10 = fminf(sqrtf((float)tap[W]), max_dist), t11 = fminf(sqrtf((float)tap[W + 1]), max_dist);
    const float ux = 1.f - fx, uy = 1.f - fy;
    const float top = t00 * ux + t01 * fx, bot = t10 * ux + t11 * fx;
    v = top * uy + bot * fy;
    gx = cx ? 0.f : (t01 - t00) * uy + (t11 - t10) * fy;
    gy = cy ? 0.f : bot - top;
  }
  value[at] = v;
  grad_xy[2 * at] = gx;
  grad_xy[2 * at + 1] = gy;
}

// one thread per element of grad_points[b][N][C]
__global__ void __launch_bounds__(kDtSampleThreads)
dt_sample_bwd_kernel(const float *__restrict__ grad_xy, const float *__restrict__ grad_value, int N, int C,
                     float *__restrict__ grad_points) {
  const size_t e = (size_t)blockIdx.x * kDtSampleThreads + threadIdx.x;
  if (e >= (size_t)N * C) return;
  const size_t n = e / (size_t)C, at = (size_t)blockIdx.y * N + n;
  const int c = (int)(e - n * C);
  grad_points[(size_t)blockIdx.y * N * C + e] = c < 2 ? grad_value[at] * grad_xy[2 * at + c] : 0.f;
}

}  // namespace shr

static int dt_check_image(int B, int H, int W) {
  if (B < 0 || H < 1 || W < 1) return SHR_EINVAL;
  if (B > 65535 || H > shr::kDtMaxSide || W > shr::kDtMaxSide) return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" long long shr_dt_workspace_bytes(int B, int H, int W) {
  if (B < 0 || H < 0 || W < 0) return -1;
  return (((long long)B * H * ((W + 1) / 2) * 4) + 15) / 16 * 16;
}

extern "C" int shr_dt_fwd(const float *depth, int B, int H, int W, float fg_max, int32_t *d2, void *workspace,
                          void *stream) {
  using namespace shr;
  const int rc = dt_check_image(B, H, W);
  if (rc != SHR_OK) return rc;
  if (B == 0) return SHR_OK;
  if (!depth || !d2 || !workspace) return SHR_EINVAL;
  if ((((uintptr_t)depth | (uintptr_t)d2) & 3u) != 0 || (((uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  uint32_t *ws = reinterpret_cast<uint32_t *>(workspace);
  const int pairs = (W + 1) / 2;
  hipLaunchKernelGGL(dt_column_kernel, dim3((unsigned)((pairs + kDtColThreads - 1) / kDtColThreads), (unsigned)B),
                     dim3(kDtColThreads), 0, s, depth, H, W, fg_max, ws);
  hipLaunchKernelGGL(dt_row_kernel, dim3((unsigned)((H + kDtRowWaves - 1) / kDtRowWaves), (unsigned)B),
                     dim3(kDtRowWaves * 64), (size_t)kDtRowWaves * W * sizeof(int), s, ws, H, W, d2);
  return (int)hipGetLastError();
}

static int dt_check_points(int B, int N, int C) {
  if (B < 0 || N < 0 || C < 2) return SHR_EINVAL;
  if (B > 65535 || (long long)N * C >= (1LL << 31)) return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" int shr_dt_sample_fwd(const int32_t *d2, int B, int H, int W, const float *points, int N, int C,
                                 float max_dist, float *value, float *grad_xy, void *stream) {
  using namespace shr;
  if (H < 2 || W < 2 || !(max_dist >= 0.f)) return SHR_EINVAL;
  int rc = dt_check_image(B, H, W);
  if (rc == SHR_OK) rc = dt_check_points(B, N, C);
  if (rc != SHR_OK) return rc;
  if (B == 0 || N == 0) return SHR_OK;
  if (!d2 || !points || !value || !grad_xy) return SHR_EINVAL;
  if ((((uintptr_t)d2 | (uintptr_t)points | (uintptr_t)value | (uintptr_t)grad_xy) & 3u) != 0) return SHR_EINVAL;
  hipLaunchKernelGGL(dt_sample_fwd_kernel, dim3((unsigned)((N + kDtSampleThreads - 1) / kDtSampleThreads), (unsigned)B),
                     dim3(kDtSampleThreads), 0, (hipStream_t)stream, d2, H, W, points, N, C, max_dist, value, grad_xy);
  return (int)hipGetLastError();
}

extern "C" int shr_dt_sample_bwd(const float *grad_xy, const float *grad_value, int B, int N, int C, float *grad_points,
                                 void *stream) {
  using namespace shr;
  const int rc = dt_check_points(B, N, C);
  if (rc != SHR_OK) return rc;
  if (B == 0 || N == 0) return SHR_OK;
  if (!grad_xy || !grad_value || !grad_points) return SHR_EINVAL;
  if ((((uintptr_t)grad_xy | (uintptr_t)grad_value | (uintptr_t)grad_points) & 3u) != 0) return SHR_EINVAL;
  const long long elems = (long long)N * C;
  hipLaunchKernelGGL(dt_sample_bwd_kernel, dim3((unsigned)((elems + kDtSampleThreads - 1) / kDtSampleThreads), (unsigned)B),
                     dim3(kDtSampleThreads), 0, (hipStream_t)stream, grad_xy, grad_value, N, C, grad_points);
  return (int)hipGetLastError();
}
