// common.h -- shared device helpers for libspherehand_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spherehand_hip.h"

// Parity with the reference is defined on its fp32 operation sequence: one
// correctly rounded IEEE operation per written operator, no FMA contraction
// (build also passes -ffp-contract=off).
#pragma clang fp contract(off)

namespace shr {

constexpr int kWave = 64;  // CDNA4 wavefront

// Wave tile of the image rasterizers: 32 px wide x 8 px high; lane l owns the
// 4 consecutive pixels starting at column 4*(l&7) of row (l>>3): one 16-byte
// store per lane, eight lanes = one full 128-byte line per tile row.
constexpr int kTileW = 32;
constexpr int kTileH = 8;

// Image axis -> model-space millimetres, mesh/render.py:31-32:
//   (u - size/2) * 300.0 / size      (three fp32 ops: sub, mul, div)
// For a power-of-two size the division is an exact scaling, so
// round(t*300)/size == round(t*(300/size)) and the divide is skipped.
struct Axis {
  float half;   // size / 2
  float size;   // (float)size
  float mul;    // 300 / size   (used when pow2)
  int pow2;
};

__host__ __device__ inline Axis make_axis(int size) {
  Axis a;
  a.half = (float)((double)size / 2.0);
  a.size = (float)size;
  a.mul = 300.0f / (float)size;
  a.pow2 = (size & (size - 1)) == 0;
  return a;
}

// The same with 300 / size supplied by the launcher: the zbuf kernels take the two IEEE divisions of an image's axes
// (and the two of size / 300, the pixels per millimetre of the boxes) as launch constants -- sixteen waves per crop
// each spent ~45 VALU instructions on them (7 % of a crop's VALU work once the SIMDs are the contended resource).
struct AxisK { float mulx, muly, kx, ky; };   // 300 / W, 300 / H, W / 300, H / 300: fp32 divisions, host == device (IEEE)
inline AxisK make_axis_k(int W, int H) {
  AxisK k;
  k.mulx = 300.0f / (float)W;
  k.muly = 300.0f / (float)H;
  k.kx = (float)W / 300.0f;
  k.ky = (float)H / 300.0f;
  return k;
}
__device__ __forceinline__ Axis axis_of(int size, float mul) {
  Axis a;
  a.size = (float)size;
  a.half = a.size * 0.5f;   // exact (size < 2^24), == (float)((double)size / 2)
  a.mul = mul;
  a.pow2 = (size & (size - 1)) == 0;
  return a;
}

__device__ __forceinline__ float axis_coord(const Axis &a, int u) {
  const float t = (float)u - a.half;
  if (a.pow2) return t * a.mul;
  return (t * 300.0f) / a.size;
}

// ---- wave-level helpers ---------------------------------------------------
__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
  // lanes outside ROW_MASK (or whose DPP source is invalid) add 0
  const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false);
  return v + __int_as_float(moved);
}

// Sum of v over the 64 lanes of the wave, valid in lane 63.  Fixed association
// (butterfly inside each row of 16, then row 0->1, 2->3, {0,1}->{2,3}):
// deterministic for a given lane assignment.
__device__ __forceinline__ float wave_sum_lane63(float v) {
  v = dpp_add<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141, 0xF>(v);  // row_half_mirror
  v = dpp_add<0x140, 0xF>(v);  // row_mirror       -> every lane holds its row's sum
  v = dpp_add<0x142, 0xA>(v);  // row_bcast:15 into rows 1,3
  v = dpp_add<0x143, 0xC>(v);  // row_bcast:31 into rows 2,3
  return v;
}

// Four wave sums at once ("transposed" reduction): two quad exchanges leave ONE register
// whose lane l holds component l & 3 summed over its quad (9 ops for the 4 components),
// then the remaining four levels run on that single register -- row_shr:4, row_shr:8,
// and the gfx950 cross-row swaps (v_permlane16_swap / v_permlane32_swap: odd <-> even
// rows, upper <-> lower half).  15 VALU ops against 24 for four wave_sum_lane63, fixed
// association.  Lanes 12..15 of EVERY row return the totals of components 0..3; the
// other lanes return partial sums.
__device__ __forceinline__ float wave_sum4_transposed(float a0, float a1, float a2, float a3, int lane) {
  const bool odd = lane & 1, hi = lane & 2;
  const float k0 = odd ? a1 : a0, s0 = odd ? a0 : a1;
  const float k1 = odd ? a3 : a2, s1 = odd ? a2 : a3;
  const float b0 = k0 + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s0), 0xB1, 0xF, 0xF, false));
  const float b1 = k1 + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s1), 0xB1, 0xF, 0xF, false));
  const float k2 = hi ? b1 : b0, s2 = hi ? b0 : b1;
  float c = k2 + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s2), 0x4E, 0xF, 0xF, false));
  c = dpp_add<0x114, 0xF>(c);   // row_shr:4
  c = dpp_add<0x118, 0xF>(c);   // row_shr:8  -> lanes 12..15 of a row: the row's sums
  const auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(c), __float_as_uint(c), false, false);
  c = __uint_as_float(r16[0]) + __uint_as_float(r16[1]);   // rows 0+1 | 2+3
  const auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(c), __float_as_uint(c), false, false);
  return __uint_as_float(r32[0]) + __uint_as_float(r32[1]);
}

// min / max over the 64 lanes, broadcast to every lane (same DPP butterfly; lanes whose
// DPP source is invalid or masked combine with their own value)
template <int CTRL, int ROW_MASK, bool IS_MIN>
__device__ __forceinline__ float dpp_minmax(float v) {
  const float o = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
  return IS_MIN ? fminf(v, o) : fmaxf(v, o);
}
template <bool IS_MIN>
__device__ __forceinline__ float wave_minmax_all(float v) {
  v = dpp_minmax<0xB1, 0xF, IS_MIN>(v);
  v = dpp_minmax<0x4E, 0xF, IS_MIN>(v);
  v = dpp_minmax<0x141, 0xF, IS_MIN>(v);
  v = dpp_minmax<0x140, 0xF, IS_MIN>(v);
  v = dpp_minmax<0x142, 0xA, IS_MIN>(v);
  v = dpp_minmax<0x143, 0xC, IS_MIN>(v);
  return readlane_f(v, 63);
}

// Four wave minima at once, same scheme as wave_sum4_transposed: lanes 12..15 of every row
// return the minima of components 0..3 (fminf: a NaN operand is ignored).
__device__ __forceinline__ float wave_min4_transposed(float a0, float a1, float a2, float a3, int lane) {
  const bool odd = lane & 1, hi = lane & 2;
  const float k0 = odd ? a1 : a0, s0 = odd ? a0 : a1;
  const float k1 = odd ? a3 : a2, s1 = odd ? a2 : a3;
  const float b0 = fminf(k0, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(k0), __float_as_int(s0), 0xB1, 0xF, 0xF, false)));
  const float b1 = fminf(k1, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(k1), __float_as_int(s1), 0xB1, 0xF, 0xF, false)));
  const float k2 = hi ? b1 : b0, s2 = hi ? b0 : b1;
  float c = fminf(k2, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(k2), __float_as_int(s2), 0x4E, 0xF, 0xF, false)));
  c = dpp_minmax<0x114, 0xF, true>(c);   // row_shr:4 (lanes without a source keep their own value)
  c = dpp_minmax<0x118, 0xF, true>(c);   // row_shr:8  -> lanes 12..15 of a row: the row's minima
  const auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(c), __float_as_uint(c), false, false);
  c = fminf(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
  const auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(c), __float_as_uint(c), false, false);
  return fminf(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
}

// Correctly rounded fp32 square root for x in [0.01, 1e12] (sphere_zbuf.h documents the range and the
// exhaustive test).  One Newton step on the reciprocal-root estimate, the last operation a single FMA:
//   y = v_rsq_f32(x) (<= 1 ulp),  s = x y,  h = y / 2,  r = fma(-s, s, x),  result = fma(r, h, s).
// s is within ~1.5 ulp of the root and r = x - s^2 is exact (it fits 24 bits at that distance), so r h = sqrt(x) - s up
// to the relative error of h (2^-23) and the step's second-order term: the FMA rounds sqrt(x) + d ONCE, |d| <~ 2^-22 ulp.
// That is the correctly rounded root unless sqrt(x) lies within |d| of the midpoint of two neighbours; the closest an
// fp32 argument's root comes to one is ~2^-27 ulp (x = m (m + 1) in units of the root's ulp squared), so the bound
// alone does not prove exactness -- tests/test_sphere_raster_gpu.py::test_sqrt_rn_exhaustive does, on the hardware, for
// every fp32 value of the range, in the default GPU selection: the function is exact on gfx950 by measurement (its
// v_rsq_f32 is part of the result).  Another target needs the test re-run.
// Five VALU instructions, one of them quarter-rate, no vcc and no wait states; the form it replaces (v_sqrt_f32, one
// residual, two compares with carry-in increments) took eight and four wait states.  The plain-arithmetic variants
// measured on the way: s + r * h (two roundings) is exact on the range as well, one instruction more; v_sqrt_f32's
// estimate corrected with h = v_rcp_f32(s) / 2 fails at the 23 inputs prev(4^k).
// (An argument outside the range -- a lane that does not hit: zero, negative -- may give NaN; callers never store it.)
__device__ __forceinline__ float sqrt_rn(float x) {
  const float y = __builtin_amdgcn_rsqf(x);
  const float s = x * y, h = 0.5f * y;
  const float r = __builtin_fmaf(-s, s, x);
  return __builtin_fmaf(r, h, s);
}

int d2m_set_waves(int waves);        // data_to_model.hip: launch-shape hooks behind SHR_TUNE_D2M_WAVES /
int d2m_set_band_units(int units);  // SHR_TUNE_D2M_BAND_UNITS
int d2m_set_tiled(int on);          // SHR_TUNE_D2M_TILED
int tri_set_band(int rows);         // tri_raster.hip: SHR_TUNE_TRI_BAND
int mesh_set_band(int on);          // mesh_depth.hip: SHR_TUNE_MESH_BAND
int mesh_set_lattice(int on);       // mesh_depth.hip: SHR_TUNE_MESH_LATTICE
int tri_band_resize(const float *vertices, const int *faces, int B, int NV, int F, int src_size, int S, float clamp_max,
                    float *depth, hipStream_t s);   // tri_raster.hip: the band kernel with the clamp + resize epilogue (-1: not its problem)
// data_to_model.hip: the two halves of shr_data_to_model_compact (mutual_project.hip: shr_mv_project_compact)
int d2m_compact_check(const float *depth, int M, int H, int W, void *workspace, int **counts);
int d2m_compact_launch(const float *depth, int M, int H, int W, void *workspace, hipStream_t s);

// Linear blend skinning of one vertex for one sample, shared by lbs_project_kernel (lbs_project.hip) and the fused
// mesh_lattice_kernel (mesh_depth.hip): one (bone, weighted vertex) entry added to the four rows of the sum, and the
// sign flip + orthographic camera of mesh/render.py:320-329 on the finished sum.  M = the bone's 4 x 4 matrix.
__device__ __forceinline__ void lbs_add_entry(float (&acc)[4], const float *M, const float4 q) {
#pragma unroll
  for (int r = 0; r < 4; r++)
    acc[r] += ((M[4 * r] * q.x + M[4 * r + 1] * q.y) + M[4 * r + 2] * q.z) + M[4 * r + 3] * q.w;
}
__device__ __forceinline__ float4 lbs_finish(const float (&acc)[4], int right_hand, int project, float cx, float cy, float fx,
                                             float fy, bool has_rand, float rf) {
  float a0 = acc[0];
  if (right_hand) a0 = -a0;
  if (!project) return make_float4(a0, acc[1], acc[2], acc[3]);
  if (!has_rand) return make_float4(fx * a0 + cx * acc[3], fy * acc[1] + cy * acc[3], acc[2], acc[3]);
  return make_float4(a0 * rf * fx + cx, acc[1] * rf * fy + cy, acc[2], 1.0f);
}
// crops whose bone matrices a skinning workgroup stages in LDS (lbs_project.hip, pose_vertices.hip)
constexpr int kLbsCrops = 4;

// The skinning + camera backward of ONE bone by ONE wave, shared by lbs_project_bwd_kernel (lbs_project.hip) and the
// one-launch pose backward (pose_vertices.hip): a[4 r + c] = sum over the skin entries e of bone k of dacc_v(e)[r] *
// wv_e[c], dacc = d out / d acc of lbs_finish.  Lanes stride over the vertices (v = lane + 64 n), fp64 partial sums, the
// xor butterfly 32 .. 1: every lane returns the 16 totals, the same bits whatever the batch or the launch.
struct LbsCamera {
  int right_hand, project;
  float cx, cy, fx, fy;
  bool has_rand;
  float rf;                           // rand_f[b] (has_rand)
};
__device__ __forceinline__ void lbs_bone_grad_wave(double (&a)[16], int k, int lane, const float4 *__restrict__ gv, int NV,
                                                   const int *__restrict__ vstart, const int *__restrict__ sbone,
                                                   const float4 *__restrict__ swv, const LbsCamera cam) {
  const double sgn = cam.right_hand ? -1.0 : 1.0;
  const double rf = cam.has_rand ? (double)cam.rf : 1.0;
  const float cx = cam.cx, cy = cam.cy, fx = cam.fx, fy = cam.fy;
#pragma unroll
  for (int j = 0; j < 16; j++) a[j] = 0.0;
  for (int v = lane; v < NV; v += 64) {
    const int e0 = vstart[v], e1 = vstart[v + 1];
    int e = e0;
    while (e < e1 && sbone[e] != k) e++;
    if (e == e1) continue;
    const float4 g = gv[v];
    // d out / d acc (lbs_finish)
    double d[4];
    if (!cam.project) {
      d[0] = sgn * g.x; d[1] = g.y; d[2] = g.z; d[3] = g.w;
    } else if (!cam.has_rand) {
      d[0] = sgn * (double)fx * g.x; d[1] = (double)fy * g.y; d[2] = g.z;
      d[3] = (double)cx * g.x + (double)cy * g.y + (double)g.w;
    } else {
      d[0] = sgn * rf * (double)fx * g.x; d[1] = rf * (double)fy * g.y; d[2] = g.z; d[3] = 0.0;
    }
    for (; e < e1; e++) {
      if (sbone[e] != k) continue;
      const float4 q = swv[e];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        a[4 * r] += d[r] * q.x; a[4 * r + 1] += d[r] * q.y; a[4 * r + 2] += d[r] * q.z; a[4 * r + 3] += d[r] * q.w;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 16; j++) {
    double t = a[j];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
    a[j] = t;
  }
}
// entry `lane` (< 16) of the totals, rounded once to fp32
__device__ __forceinline__ float lbs_bone_grad_entry(const double (&a)[16], int lane) {
  double t = 0.0;
#pragma unroll
  for (int j = 0; j < 16; j++) t = (lane == j) ? a[j] : t;
  return (float)t;
}

// inclusive prefix sum over the 64 lanes (4 DPP steps inside each row of 16, then the row totals)
__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);
  const int r0s = __builtin_amdgcn_readlane(v, 15), r1s = __builtin_amdgcn_readlane(v, 31), r2s = __builtin_amdgcn_readlane(v, 47);
  const int row = lane >> 4;
  return v + (row >= 1 ? r0s : 0) + (row >= 2 ? r1s : 0) + (row >= 3 ? r2s : 0);
}
// Item k of a sequence cut into 64 consecutive runs whose inclusive ends the lanes hold (non-decreasing; `mine`: this
// lane's run exists): the run that holds k = the number of runs that END at or before k.  Those that end at or
// before k0 (wave-uniform, <= k) are counted by one ballot, the few that end inside [k0, k0 + 63] one by one.
__device__ __forceinline__ int run_of(int incl, bool mine, int k0, int k) {
  int run = __popcll(__ballot(mine && incl <= k0));
  unsigned long long inner = __ballot(mine && incl > k0 && incl <= k0 + 63);
  while (inner) {
    const int c = __builtin_ctzll(inner);
    inner &= inner - 1;
    run += (__builtin_amdgcn_readlane(incl, c) <= k) ? 1 : 0;
  }
  return run;
}


__device__ __forceinline__ bool is_aligned16(const void *p) { return (((uintptr_t)p) & 15u) == 0; }

// ATen area_pixel_compute_source_index (align_corners=False) for output index d:
// src = scale*(d+0.5)-0.5 clamped at 0; i0 = (int)src; i1 = i0 + (i0 < in-1); l1 = src - i0.
struct Lin { int i0, i1; float l0, l1; };
__device__ __forceinline__ Lin lin_index(int d, float scale, int in_size) {
  // (one rounding: ATen's GPU kernel is compiled with contraction, scale * (d + 0.5) - 0.5 is an FMA there;
  // the two forms differ by an ulp of the source index at non-dyadic ratios, 3e-5 of a pixel at 256)
  float src = __builtin_fmaf(scale, (float)d + 0.5f, -0.5f);
  if (src < 0.f) src = 0.f;
  Lin r;
  r.i0 = min((int)src, in_size - 1);
  r.i1 = r.i0 + ((r.i0 < in_size - 1) ? 1 : 0);
  r.l1 = src - (float)r.i0;
  r.l0 = 1.0f - r.l1;
  return r;
}

// ---- counter-based random numbers of the synthetic branch (HandSynthesizer: RandScale, focal jitter, DepthNoise) --------
// No state is carried between draws: a draw is a HASH of what it is for, so any launch geometry -- and a numpy
// restatement (spherehand_amd/synth_rng.py) -- produces the same numbers.
//   rng_hash        lowbias32 (C. Wellons' hash-prospector: xorshift-multiply, 2 rounds; bias 0.17 of an ideal hash)
//   rng_key         the stream word k of sample b in call `ctr` under `seed`: a chain of rng_hash over the six words
//   rng_uniform     the top 24 bits as a float in [0, 1) -- torch.rand's float32 construction
//   pixel p of a sample's noise field: h1 = rng_hash(key0 + p), h2 = rng_hash(key1 + p)  (mesh_depth.hip / synth_post.hip)
__host__ __device__ inline uint32_t rng_hash(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__host__ __device__ inline uint32_t rng_key(unsigned long long seed, unsigned long long ctr, uint32_t b, uint32_t k) {
  uint32_t h = rng_hash((uint32_t)seed ^ 0x9e3779b9u);
  h = rng_hash(h ^ (uint32_t)(seed >> 32));
  h = rng_hash(h ^ (uint32_t)ctr);
  h = rng_hash(h ^ (uint32_t)(ctr >> 32) ^ 0x85ebca6bu);
  h = rng_hash(h ^ b);
  return rng_hash(h ^ (k + 0x27d4eb2fu));
}
__host__ __device__ inline float rng_uniform(uint32_t h) { return (float)(h >> 8) * 5.9604644775390625e-8f; }   // 2^-24

// DepthNoise (network/util_modules.py:46-84) on pixel `p` of a sample whose stream keys are (key0, key1):
//   shift per axis  trunc(n * sigma_xy + 0.5), n ~ N(0, 1): a 16-bit uniform against the three cumulative thresholds
//                   thr = (P(shift < 0), P(shift < 1), P(shift < 2)) x 65536 -- shifts -1 .. +2; what lies beyond them
//                   (3e-7 at the reference's sigma 0.5) is folded into the outer two.  x: h1's high half, y: its low half.
//   depth noise     Box-Muller on h2's halves: sqrt(-2 ln u1) cos(2 pi u2), u1 = (hi + 0.5) / 65536, u2 = lo / 65536.
struct NoiseShift { int dx, dy; };
__device__ __forceinline__ NoiseShift noise_shift(uint32_t key0, uint32_t p, uint32_t t0, uint32_t t1, uint32_t t2) {
  const uint32_t h = rng_hash(key0 + p);
  const uint32_t ux = h >> 16, uy = h & 0xffffu;
  NoiseShift s;
  s.dx = -1 + (int)(ux >= t0) + (int)(ux >= t1) + (int)(ux >= t2);
  s.dy = -1 + (int)(uy >= t0) + (int)(uy >= t1) + (int)(uy >= t2);
  return s;
}
__device__ __forceinline__ float noise_normal(uint32_t key1, uint32_t p) {
  const uint32_t h = rng_hash(key1 + p);
  const float u1 = ((float)(h >> 16) + 0.5f) * 1.52587890625e-5f;    // (0, 1)
  const float u2 = (float)(h & 0xffffu) * 1.52587890625e-5f;         // [0, 1): v_cos_f32 takes revolutions
  const float r = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));   // -2 ln 2 * log2(u1)
  return r * __builtin_amdgcn_cosf(u2);
}

// ---- host side: what a launcher caches PER DEVICE -------------------------------------------------------------------
// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device function attribute and the CU count a per-device number:
// a process that launches on a second GPU must set / read them there too (ops._on() may launch on a non-current device).
constexpr int kMaxDevices = 64;
struct AttrDone { bool dev[kMaxDevices] = {}; };

// the opt-in to `bytes` of dynamic LDS for `kernel` on the CURRENT device, once per (kernel, device)
template <typename K>
inline hipError_t allow_dynamic_lds(K kernel, int bytes, AttrDone *done) {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) d = -1;
  if (d >= 0 && done->dev[d]) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess && d >= 0) done->dev[d] = true;
  return e;
}

// compute units of the current device (256 when it cannot be asked)
inline int device_cus() {
  static int cus[kMaxDevices] = {};
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) return 256;
  if (cus[d] == 0) {
    int v = 0;
    cus[d] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && v > 0) ? v : 256;
  }
  return cus[d];
}

}  // namespace shr
