// fixed_point.h -- the deterministic gradient sums of the backward kernels (mesh_depth_bwd.hip, tri_antialias.hip,
// tri_interp.hip, sil_cover.hip, mesh_d2m.hip):
// clear, crop maxima, 64-bit fixed-point sums and the conversion to fp32, generic over a tap walker (Taps below).
//
// Sums: every (tap, corner, coordinate) term is a 64-bit FIXED-POINT integer in a per-crop power-of-two unit taken from
// the crop's largest term (a first pass over the taps, an order-independent maximum), so that the largest term is below
// 2^bits, a term is clamped to 2^bits besides, and any 2^(62 - bits) of them stay below 2^62.  bits is 41 while an
// accumulator can take at most 2^21 terms and 62 - ceil(log2(terms)) above that: EVERY entry states its terms per pixel
// and takes its bits from fix_term_bits(terms_per_pixel, W, H) below -- three for the owner raster and the interpolation
// (a face's corners), two for the antialias pairs, twelve for shr_mesh_depth_bwd (four taps x three corners; 41 bits
// up to S = 418) -- so no sum can wrap at any size an entry accepts.  Integer sums do not depend on order: the gradient
// is bitwise reproducible and independent of the batch and of the launch shape (data_to_model's fixed-point sums,
// d2m_search.h).  The unit is computed on the device: no host synchronisation, the backward can be captured into a graph.
//
// Taps: walk(fn) calls fn(g, pid) for every live tap of crop blockIdx.y in this workgroup's pixels, g its nine terms
// (three points x three coordinates; a zero term is skipped by the sums), pid[k] the accumulator point of g[k];
// points(): the accumulator points of a crop; kThreads, kBlockPix: the threads and pixels of a workgroup; kRuns: a
// thread's taps come in runs of one point triple (the sums merge a run in registers first).
//
// Host: fixed_point_bwd launches the four passes; with_runs picks a walker's RUNS instantiation from the point count, so
// that an entry writes its call of fixed_point_bwd once.  What the walkers share about one face at one owned pixel (the
// checked gather, the fp32 decisions and fp64 weights, the weights' chain to x, y) is tri_tap.h's.
#pragma once

#include <type_traits>

#include "common.h"

namespace shr {

constexpr int kBwdThreads = 1024;
constexpr int kBwdPix = 4;                            // output pixels per thread
constexpr int kBwdBlockPix = kBwdThreads * kBwdPix;   // output pixels per workgroup
constexpr int kBwdLdsVerts = 2048;                    // vertices whose accumulators fit LDS (2048 x 3 x 8 = 48 KB)
constexpr int kFixBits = 41;                          // the crop's largest term -> below 2^41 (fewer: fix_term_bits)

// The pixels of a tap walker over a W x H image, pixel(k) for k < kPix.  RUNS (the accumulators in global memory: more
// than kBwdLdsVerts points): a thread takes kPixRun CONSECUTIVE pixels of a row -- the hand's faces own runs of ~5 pixels
// of a row at 640 x 640, and a run's terms go to the same nine accumulators: summed in registers first, they cost one L2
// atomic each instead of one per pixel (256 soups @640^2: 10.1 -> 4.1 ms); 512 threads, so that the run's eighteen
// registers fit without spilling.  Without RUNS (LDS accumulators): 1024 threads, kBwdPix pixels each a workgroup's width
// apart (2.3 ms against 3.6 for consecutive pixels, 256 indexed hands @640^2).
constexpr int kPixRun = 8;
template <bool RUNS>
struct PixelWalk {
  static constexpr int kThreads = RUNS ? 512 : kBwdThreads, kPix = RUNS ? kPixRun : kBwdPix, kBlockPix = kThreads * kPix;
  static __device__ __forceinline__ size_t pixel(int k) {
    return RUNS ? ((size_t)blockIdx.x * kThreads + threadIdx.x) * kPix + k
                : (size_t)blockIdx.x * kBlockPix + k * kThreads + threadIdx.x;
  }
};

__device__ __forceinline__ double fix_unit(uint32_t max_bits, int bits) {   // 2^(bits - E), max < 2^E
  int e = 0;
  frexp((double)__uint_as_float(max_bits), &e);
  return ldexp(1.0, bits - e);
}
__device__ __forceinline__ long long to_fix(double v, double unit, int bits) {
  double t = v * unit;
  if (!(t == t)) return 0;
  const double lim = ldexp(1.0, bits);
  t = fmin(fmax(t, -lim), lim);
  return __double2ll_rn(t);
}

// pass 0: clear the workspace (a kernel rather than a memset node: the same launch sequence eager and in a graph)
static __global__ void __launch_bounds__(256)
mesh_bwd_clear_kernel(uint4 *__restrict__ ws, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x)
    ws[i] = make_uint4(0u, 0u, 0u, 0u);
}

// pass 1: the crop's largest |term| (float bits of non-negative numbers order like unsigned integers)
template <typename Taps>
__global__ void __launch_bounds__(Taps::kThreads)
mesh_bwd_max_kernel(Taps taps, uint32_t *__restrict__ crop_max) {
  __shared__ uint32_t s_max;
  if (threadIdx.x == 0) s_max = 0u;
  __syncthreads();
  float m = 0.f;
  taps.walk([&](const double (&g)[3][3], const int (&)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int d = 0; d < 3; d++) {
        const float a = (float)fabs(g[k][d]);
        if (a <= 3.0e38f) m = fmaxf(m, a);   // (NaN and inf: clamped / dropped by to_fix)
      }
  });
  if (m > 0.f) atomicMax(&s_max, __float_as_uint(m));
  __syncthreads();
  if (threadIdx.x == 0 && s_max != 0u) atomicMax(&crop_max[blockIdx.y], s_max);
}

// pass 2: the fixed-point sums, staged in LDS when the crop's accumulators fit, then added to acc[B][points][3]
template <typename Taps, bool LDS>
__global__ void __launch_bounds__(Taps::kThreads)
mesh_bwd_sum_kernel(Taps taps, const uint32_t *__restrict__ crop_max, int fix_bits, unsigned long long *__restrict__ acc) {
  __shared__ unsigned long long s_acc[LDS ? kBwdLdsVerts * 3 : 1];
  const int b = blockIdx.y, NP = taps.points();
  const uint32_t mb = crop_max[b];
  if (mb == 0u) return;   // (uniform: no term in this crop)
  const double unit = fix_unit(mb, fix_bits);
  unsigned long long *g_acc = acc + (size_t)b * NP * 3;
  if (LDS) {
    for (int i = threadIdx.x; i < NP * 3; i += Taps::kThreads) s_acc[i] = 0ull;
    __syncthreads();
  }
  auto add = [&](int p, int d, long long v) {
    if (v == 0) return;
    if (LDS) atomicAdd(&s_acc[p * 3 + d], (unsigned long long)v);
    else atomicAdd(&g_acc[(size_t)p * 3 + d], (unsigned long long)v);
  };
  // kRuns: the current run's points and sums (integers: merging first changes no bit of the result)
  int run_pid[3] = {-1, -1, -1};
  long long run[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  auto flush = [&]() {
    if (run_pid[0] < 0) return;
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int d = 0; d < 3; d++) add(run_pid[k], d, run[k][d]);
  };
  taps.walk([&](const double (&g)[3][3], const int (&pid)[3]) {
    if (Taps::kRuns && (pid[0] != run_pid[0] || pid[1] != run_pid[1] || pid[2] != run_pid[2])) {
      flush();
#pragma unroll
      for (int k = 0; k < 3; k++) {
        run_pid[k] = pid[k];
#pragma unroll
        for (int d = 0; d < 3; d++) run[k][d] = 0;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int d = 0; d < 3; d++) {
        const long long v = to_fix(g[k][d], unit, fix_bits);
        if (Taps::kRuns) run[k][d] += v;
        else add(pid[k], d, v);
      }
  });
  if (Taps::kRuns) flush();
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < NP * 3; i += Taps::kThreads) {
      const unsigned long long v = s_acc[i];
      if (v != 0ull) atomicAdd(&g_acc[i], v);
    }
  }
}

// pass 3: fixed point -> out[B][NP] = (du, dv, dz, 0) (STRIDE 4: vertices) or (du, dv, dz) (STRIDE 3: face corners)
template <int STRIDE>
__global__ void __launch_bounds__(256)
mesh_bwd_finish_kernel(const unsigned long long *__restrict__ acc, const uint32_t *__restrict__ crop_max, int B, int NP,
                       int fix_bits, float *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * NP) return;
  const int b = (int)(i / NP);
  const uint32_t mb = crop_max[b];
  float r[3] = {0.f, 0.f, 0.f};
  if (mb != 0u) {
    const double inv = 1.0 / fix_unit(mb, fix_bits);   // (a power of two: exact)
#pragma unroll
    for (int d = 0; d < 3; d++) r[d] = (float)((double)(long long)acc[i * 3 + d] * inv);
  }
  if (STRIDE == 4) reinterpret_cast<float4 *>(out)[i] = make_float4(r[0], r[1], r[2], 0.f);
  else { out[i * 3] = r[0]; out[i * 3 + 1] = r[1]; out[i * 3 + 2] = r[2]; }
}
}  // namespace shr

static size_t mesh_bwd_max_bytes(int B) { return (((size_t)B * 4) + 255) & ~(size_t)255; }
// crop maxima [B] u32 | accumulators [B][NP][3] i64
static long long fix_workspace_bytes(int B, long long NP) {
  if (B < 0 || NP < 0) return -1;
  return (long long)((mesh_bwd_max_bytes(B) + (size_t)B * NP * 3 * 8 + 15) & ~(size_t)15);
}

// The bits of a backward over a W x H image whose accumulators take at most `terms_per_pixel` terms per pixel: with
// N = terms_per_pixel W H terms the crop's largest term goes below 2^(62 - ceil(log2 N)), 2^41 at most -- no sum can wrap
// at any size.
static int fix_term_bits(int terms_per_pixel, int W, int H) {
  const unsigned long long n = (unsigned long long)terms_per_pixel * (unsigned long long)W * (unsigned long long)H;
  int lg = 0;
  while ((1ull << lg) < n) lg++;
  return 62 - lg < shr::kFixBits ? 62 - lg : shr::kFixBits;
}

// The four passes of a fixed-point backward over `taps` (clear, crop maxima, sums, conversion to out[B][NP][STRIDE]).
template <int STRIDE, typename Taps>
static int fixed_point_bwd(const Taps &taps, int B, int NP, size_t npix, int fix_bits, float *out, void *workspace,
                           hipStream_t s) {
  using namespace shr;
  uint32_t *crop_max = reinterpret_cast<uint32_t *>(workspace);
  unsigned long long *acc = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(workspace) + mesh_bwd_max_bytes(B));
  const size_t n16 = (size_t)fix_workspace_bytes(B, NP) / 16;
  const size_t clear_blocks = (n16 + 255) / 256;
  hipLaunchKernelGGL(mesh_bwd_clear_kernel, dim3((unsigned)(clear_blocks < 4096 ? clear_blocks : 4096)), dim3(256), 0, s,
                     reinterpret_cast<uint4 *>(workspace), n16);
  const dim3 grid((unsigned)((npix + Taps::kBlockPix - 1) / Taps::kBlockPix), (unsigned)B);
  hipLaunchKernelGGL(mesh_bwd_max_kernel<Taps>, grid, dim3(Taps::kThreads), 0, s, taps, crop_max);
  if (NP <= kBwdLdsVerts && !Taps::kRuns)
    hipLaunchKernelGGL((mesh_bwd_sum_kernel<Taps, !Taps::kRuns>), grid, dim3(Taps::kThreads), 0, s, taps, crop_max, fix_bits, acc);
  else
    hipLaunchKernelGGL((mesh_bwd_sum_kernel<Taps, false>), grid, dim3(Taps::kThreads), 0, s, taps, crop_max, fix_bits, acc);
  const size_t n = (size_t)B * NP;
  if (n > 0)
    hipLaunchKernelGGL(mesh_bwd_finish_kernel<STRIDE>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, acc, crop_max, B,
                       NP, fix_bits, out);
  return (int)hipGetLastError();
}

// A walker with a RUNS parameter takes it from the point count: fn(std::bool_constant<RUNS>{}) is called once, RUNS = the
// accumulators do not fit LDS.  fn is a generic lambda that names the instantiation (Taps<decltype(runs)::value>) and calls
// fixed_point_bwd -- the call and its arguments are written once.
template <typename Fn>
static int with_runs(long long NP, Fn fn) {
  return NP <= shr::kBwdLdsVerts ? fn(std::false_type{}) : fn(std::true_type{});
}
