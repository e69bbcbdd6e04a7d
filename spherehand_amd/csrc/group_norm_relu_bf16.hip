// group_norm_relu_bf16.hip -- group_norm_relu.hip's kernel pair for bf16 activations: x, y, dy and dx are bf16,
// everything else (pre_bias, gamma, beta, mean, rstd, every partial and parameter gradient) stays fp32, and so does
// all arithmetic.  A bf16 element is widened exactly (its 16 bits are the upper half of the fp32 pattern); the only
// rounding the fp32 kernels do not have is the final store of y and of dx, round-to-nearest-even (gn_bf16_pack).
//
// Thread layout: a lane owns 8 consecutive channels (one 16-byte access) of every 32nd pixel, 4 lanes per pixel,
// 128 threads (two waves) per (sample, block of 32 channels).  Why 8 channels and not the fp32 mapping with 8-byte
// accesses: on gfx950 an 8-byte global access runs at 0.54-0.70 of the 16-byte rate per byte, and the three passes
// over the slab are nothing but such accesses, so the narrower access would give back what the narrower type saves.
// (Measured, DESIGN.md 4.5: at the training batch neither pair is bound by bytes but by its one small workgroup per
// CU; the bf16 pair runs the 35 forward launches of a pass in 0.84 of the fp32 pair's time, the backward in the same.)
// Why 128 threads and not 256: the lane keeps the fp32 kernels'
// pixel walk (p0, p0 + 32, ...), so its lower and upper 4 channels ARE the fp32 kernels' channel-lanes 2k and
// 2k + 1, each with its own accumulators, and every sum below is taken in the fp32 kernels' order: pixels in the
// lane, the 8 pixel slots of an fp32 wave (xor 4, 8, 16 here for xor 8, 16, 32 there), the channel-lanes of a group
// (the two halves of the lane, then xor 1, 2 for xor 2, 4), the four fp32 waves in order through the LDS.  The value in
// front of the rounding is therefore the fp32 kernels' value on the widened input, bit for bit
// (tests/test_group_norm_bf16_gpu.py asserts it), and mean, rstd and the partials are theirs exactly.
// With C/G = 4 (GroupNorm(16, 64), layer1) the two halves of a lane lie in two groups: every per-group
// quantity (mean, rstd, the two backward group sums) is kept per half, and the halves are only combined from
// C/G = 8 on.
#include "group_norm_relu.h"

namespace shr {

constexpr int kGnBf16Threads = 128;
// A pass walks the lane's pixels kGnBf16Batch at a time: the batch's loads are issued together, then consumed in pixel
// order (the sums keep the fp32 kernels' order): four loads (backward: eight) in flight per lane instead of one, worth
// 5-10 % at 32 x 32 pixels, where a lane makes 32 rounds per pass and a CU holds one two-wave workgroup.  The loads
// carry no condition -- a pixel past the end reads the last pixel again (in bounds, unused) -- so that no branch, and
// no wait at its join, separates them.
constexpr int kGnBf16Batch = 4;
#define GN_BF16_LOADS(j, p, p_first) \
  _Pragma("unroll") for (int j = 0, p = min((p_first), HW - 1); j < kGnBf16Batch; j++, p = min((p_first) + 32 * (j), HW - 1))
#define GN_BF16_BATCH(j, p, p_first) \
  _Pragma("unroll") for (int j = 0, p = (p_first); j < kGnBf16Batch; j++, p += 32) if (p < HW)

// two fp32 -> two bf16 in one word, round to nearest even: gfx950's v_cvt_pk_bf16_f32 (what the conversion below
// compiles to).  An infinity stays one, a NaN stays one (quieted), a finite value above the largest bf16 rounds to
// infinity as IEEE says; tests/gn_bf16_ref.py's bf16_round restates it on bit patterns.
typedef __bf16 gn_bf16x2 __attribute__((ext_vector_type(2)));
typedef float gn_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t gn_bf16_pack(float lo, float hi) {
  const gn_f32x2 f = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, gn_bf16x2));
}

// 8 bf16 (one 16-byte load) -> the lane's two float4 halves, and back
__device__ __forceinline__ void gn_bf16_widen(const uint4 r, float4 &a, float4 &b) {
  a = make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                  __uint_as_float(r.y & 0xffff0000u));
  b = make_float4(__uint_as_float(r.z << 16), __uint_as_float(r.z & 0xffff0000u), __uint_as_float(r.w << 16),
                  __uint_as_float(r.w & 0xffff0000u));
}
__device__ __forceinline__ uint4 gn_bf16_narrow(const float4 a, const float4 b) {
  return make_uint4(gn_bf16_pack(a.x, a.y), gn_bf16_pack(a.z, a.w), gn_bf16_pack(b.x, b.y), gn_bf16_pack(b.z, b.w));
}

// the lane's pixel is tid >> 2: lanes with equal lane & 3 and equal lane >> 5 are the 8 pixel slots of one fp32 wave,
// whose number is tid >> 5
__device__ __forceinline__ float gn_bf16_slot_sum(float v) {
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 16);
  return v;
}

// gn_group_total of the fp32 unit for the two halves of a lane: both end up holding the total of THEIR group
__device__ __forceinline__ void gn_bf16_group_total(float &lo, float &hi, int cpg, float (*s_w)[8], int tid) {
  lo = gn_bf16_slot_sum(lo);
  hi = gn_bf16_slot_sum(hi);
  if (cpg >= 8) { const float t = lo + hi; lo = t; hi = t; }
  if (cpg >= 16) { lo += __shfl_xor(lo, 1); hi = lo; }
  if (cpg >= 32) { lo += __shfl_xor(lo, 2); hi = lo; }
  __syncthreads();   // s_w free
  if ((tid & 0x1c) == 0) { s_w[tid >> 5][2 * (tid & 3)] = lo; s_w[tid >> 5][2 * (tid & 3) + 1] = hi; }
  __syncthreads();
  const int k = 2 * (tid & 3);
  lo = ((s_w[0][k] + s_w[1][k]) + s_w[2][k]) + s_w[3][k];
  hi = ((s_w[0][k + 1] + s_w[1][k + 1]) + s_w[2][k + 1]) + s_w[3][k + 1];
}

__device__ __forceinline__ float4 gn_bf16_slot_sum4(float4 v) {
#pragma unroll
  for (int m = 4; m <= 16; m <<= 1) {
    v.x += __shfl_xor(v.x, m); v.y += __shfl_xor(v.y, m); v.z += __shfl_xor(v.z, m); v.w += __shfl_xor(v.w, m);
  }
  return v;
}

// gn_channel_total of the fp32 unit: per-CHANNEL totals of the lane's 8 channels, in every lane
__device__ __forceinline__ void gn_bf16_channel_total(float4 &lo, float4 &hi, float4 (*s_w4)[8], int tid) {
  lo = gn_bf16_slot_sum4(lo);
  hi = gn_bf16_slot_sum4(hi);
  __syncthreads();
  if ((tid & 0x1c) == 0) { s_w4[tid >> 5][2 * (tid & 3)] = lo; s_w4[tid >> 5][2 * (tid & 3) + 1] = hi; }
  __syncthreads();
  const int k = 2 * (tid & 3);
  lo = s_w4[0][k];
  hi = s_w4[0][k + 1];
#pragma unroll
  for (int w = 1; w < 4; w++) {
    const float4 a = s_w4[w][k], b = s_w4[w][k + 1];
    lo.x += a.x; lo.y += a.y; lo.z += a.z; lo.w += a.w;
    hi.x += b.x; hi.y += b.y; hi.z += b.z; hi.w += b.w;
  }
}

__device__ __forceinline__ float4 gn_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 gn_add4(float4 v, const float4 b) { v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; return v; }
__device__ __forceinline__ float gn_sum4(const float4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float gn_sumsq4(const float4 v, float mean) {
  const float a = v.x - mean, b = v.y - mean, cc = v.z - mean, d = v.w - mean;
  return (a * a + b * b) + (cc * cc + d * d);
}
__device__ __forceinline__ float4 gn_out4(const float4 v, float mean, const float4 sc, const float4 be) {
  return make_float4(fmaxf((v.x - mean) * sc.x + be.x, 0.f), fmaxf((v.y - mean) * sc.y + be.y, 0.f),
                     fmaxf((v.z - mean) * sc.z + be.z, 0.f), fmaxf((v.w - mean) * sc.w + be.w, 0.f));
}

__global__ void __launch_bounds__(kGnBf16Threads)
group_norm_relu_bf16_fwd_kernel(const uint16_t *__restrict__ x, const float *__restrict__ pre_bias,
                                const float *__restrict__ gamma, const float *__restrict__ beta, int C, int HW, int G,
                                float eps, uint16_t *__restrict__ y, float *__restrict__ mean_out,
                                float *__restrict__ rstd_out) {
  __shared__ float s_w[4][8];
  const int n = blockIdx.y, c0 = blockIdx.x * kGnBlockC;
  const int tid = threadIdx.x;
  const int k = tid & 3, p0 = tid >> 2;          // channel-lane (8 channels), first pixel
  const int cpg = C / G;
  const int c = c0 + 8 * k, g_lo = c / cpg, g_hi = (c + 4) / cpg;
  const uint4 *xs = reinterpret_cast<const uint4 *>(x + (size_t)n * HW * C + c);
  uint4 *ys = reinterpret_cast<uint4 *>(y + (size_t)n * HW * C + c);
  const int stride8 = C >> 3;                    // 16-byte units per pixel
  const float inv_m = 1.0f / (float)(cpg * HW);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 pb_lo = pre_bias ? gn_ld4(pre_bias + c) : zero, pb_hi = pre_bias ? gn_ld4(pre_bias + c + 4) : zero;

  float s_lo = 0.f, s_hi = 0.f;
  for (int first = p0; first < HW; first += 32 * kGnBf16Batch) {
    uint4 r[kGnBf16Batch];
    GN_BF16_LOADS(j, p, first) r[j] = xs[(size_t)p * stride8];
    GN_BF16_BATCH(j, p, first) {
      float4 a, b;
      gn_bf16_widen(r[j], a, b);
      s_lo += gn_sum4(gn_add4(a, pb_lo));
      s_hi += gn_sum4(gn_add4(b, pb_hi));
    }
  }
  gn_bf16_group_total(s_lo, s_hi, cpg, s_w, tid);
  const float mean_lo = s_lo * inv_m, mean_hi = s_hi * inv_m;
  float q_lo = 0.f, q_hi = 0.f;
  for (int first = p0; first < HW; first += 32 * kGnBf16Batch) {
    uint4 r[kGnBf16Batch];
    GN_BF16_LOADS(j, p, first) r[j] = xs[(size_t)p * stride8];
    GN_BF16_BATCH(j, p, first) {
      float4 a, b;
      gn_bf16_widen(r[j], a, b);
      q_lo += gn_sumsq4(gn_add4(a, pb_lo), mean_lo);
      q_hi += gn_sumsq4(gn_add4(b, pb_hi), mean_hi);
    }
  }
  gn_bf16_group_total(q_lo, q_hi, cpg, s_w, tid);
  const float rstd_lo = 1.0f / __builtin_sqrtf(q_lo * inv_m + eps), rstd_hi = 1.0f / __builtin_sqrtf(q_hi * inv_m + eps);
  if (tid < 4) {
    if ((c % cpg) == 0) { mean_out[(size_t)n * G + g_lo] = mean_lo; rstd_out[(size_t)n * G + g_lo] = rstd_lo; }
    if (((c + 4) % cpg) == 0) { mean_out[(size_t)n * G + g_hi] = mean_hi; rstd_out[(size_t)n * G + g_hi] = rstd_hi; }
  }
  const float4 ga_lo = gn_ld4(gamma + c), ga_hi = gn_ld4(gamma + c + 4);
  const float4 be_lo = gn_ld4(beta + c), be_hi = gn_ld4(beta + c + 4);
  const float4 sc_lo = make_float4(ga_lo.x * rstd_lo, ga_lo.y * rstd_lo, ga_lo.z * rstd_lo, ga_lo.w * rstd_lo);
  const float4 sc_hi = make_float4(ga_hi.x * rstd_hi, ga_hi.y * rstd_hi, ga_hi.z * rstd_hi, ga_hi.w * rstd_hi);
  for (int first = p0; first < HW; first += 32 * kGnBf16Batch) {
    uint4 r[kGnBf16Batch];
    GN_BF16_LOADS(j, p, first) r[j] = xs[(size_t)p * stride8];
    GN_BF16_BATCH(j, p, first) {
      float4 a, b;
      gn_bf16_widen(r[j], a, b);
      ys[(size_t)p * stride8] = gn_bf16_narrow(gn_out4(gn_add4(a, pb_lo), mean_lo, sc_lo, be_lo),
                                               gn_out4(gn_add4(b, pb_hi), mean_hi, sc_hi, be_hi));
    }
  }
}

// one half of a lane in the backward: xhat and the masked dy' of its 4 channels (the mask is decided on the fp32
// pre-activation recomputed from x, never on the rounded y)
struct GnHalf { float4 h, d; };
__device__ __forceinline__ GnHalf gn_bf16_half(float4 v, const float4 d, const float4 pb, float mean, float rstd,
                                               const float4 ga, const float4 be) {
  v = gn_add4(v, pb);
  GnHalf r;
  r.h = make_float4((v.x - mean) * rstd, (v.y - mean) * rstd, (v.z - mean) * rstd, (v.w - mean) * rstd);
  r.d = make_float4((r.h.x * ga.x + be.x > 0.f) ? d.x : 0.f, (r.h.y * ga.y + be.y > 0.f) ? d.y : 0.f,
                    (r.h.z * ga.z + be.z > 0.f) ? d.z : 0.f, (r.h.w * ga.w + be.w > 0.f) ? d.w : 0.f);
  return r;
}
__device__ __forceinline__ float4 gn_bf16_dx4(const GnHalf r, float rstd, const float4 ga, float m1, float m2) {
  return make_float4(rstd * (r.d.x * ga.x - (m1 + r.h.x * m2)), rstd * (r.d.y * ga.y - (m1 + r.h.y * m2)),
                     rstd * (r.d.z * ga.z - (m1 + r.h.z * m2)), rstd * (r.d.w * ga.w - (m1 + r.h.w * m2)));
}
__device__ __forceinline__ float gn_dot4(const float4 g, const float4 a) { return (g.x * a.x + g.y * a.y) + (g.z * a.z + g.w * a.w); }

// group_norm_relu_bwd_kernel's formulas; dpre_part sums the fp32 dx values before they are rounded
__global__ void __launch_bounds__(kGnBf16Threads)
group_norm_relu_bf16_bwd_kernel(const uint16_t *__restrict__ x, const float *__restrict__ pre_bias,
                                const uint16_t *__restrict__ dy, const float *__restrict__ gamma,
                                const float *__restrict__ beta, const float *__restrict__ mean_in,
                                const float *__restrict__ rstd_in, int C, int HW, int G, uint16_t *__restrict__ dx,
                                float *__restrict__ dgamma_part, float *__restrict__ dbeta_part,
                                float *__restrict__ dpre_part) {
  __shared__ float4 s_w4[4][8];
  const int n = blockIdx.y, c0 = blockIdx.x * kGnBlockC;
  const int tid = threadIdx.x;
  const int k = tid & 3, p0 = tid >> 2;
  const int cpg = C / G;
  const int c = c0 + 8 * k, g_lo = c / cpg, g_hi = (c + 4) / cpg;
  const size_t base = (size_t)n * HW * C + c;
  const uint4 *xs = reinterpret_cast<const uint4 *>(x + base);
  const uint4 *ds = reinterpret_cast<const uint4 *>(dy + base);
  uint4 *os = reinterpret_cast<uint4 *>(dx + base);
  const int stride8 = C >> 3;
  const float mean_lo = mean_in[(size_t)n * G + g_lo], rstd_lo = rstd_in[(size_t)n * G + g_lo];
  const float mean_hi = mean_in[(size_t)n * G + g_hi], rstd_hi = rstd_in[(size_t)n * G + g_hi];
  const float4 ga_lo = gn_ld4(gamma + c), ga_hi = gn_ld4(gamma + c + 4);
  const float4 be_lo = gn_ld4(beta + c), be_hi = gn_ld4(beta + c + 4);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 pb_lo = pre_bias ? gn_ld4(pre_bias + c) : zero, pb_hi = pre_bias ? gn_ld4(pre_bias + c + 4) : zero;

  float4 A_lo = zero, A_hi = zero, B_lo = zero, B_hi = zero;    // sum dy', sum dy' * xhat per channel
  for (int first = p0; first < HW; first += 32 * kGnBf16Batch) {
    uint4 rx[kGnBf16Batch], rd[kGnBf16Batch];
    GN_BF16_LOADS(j, p, first) { rx[j] = xs[(size_t)p * stride8]; rd[j] = ds[(size_t)p * stride8]; }
    GN_BF16_BATCH(j, p, first) {
      float4 va, vb, da, db;
      gn_bf16_widen(rx[j], va, vb);
      gn_bf16_widen(rd[j], da, db);
      const GnHalf l = gn_bf16_half(va, da, pb_lo, mean_lo, rstd_lo, ga_lo, be_lo);
      const GnHalf u = gn_bf16_half(vb, db, pb_hi, mean_hi, rstd_hi, ga_hi, be_hi);
      A_lo = gn_add4(A_lo, l.d);
      A_hi = gn_add4(A_hi, u.d);
      B_lo.x += l.d.x * l.h.x; B_lo.y += l.d.y * l.h.y; B_lo.z += l.d.z * l.h.z; B_lo.w += l.d.w * l.h.w;
      B_hi.x += u.d.x * u.h.x; B_hi.y += u.d.y * u.h.y; B_hi.z += u.d.z * u.h.z; B_hi.w += u.d.w * u.h.w;
    }
  }
  gn_bf16_channel_total(A_lo, A_hi, s_w4, tid);
  gn_bf16_channel_total(B_lo, B_hi, s_w4, tid);
  if (tid < 4) {
    *reinterpret_cast<float4 *>(dbeta_part + (size_t)n * C + c) = A_lo;
    *reinterpret_cast<float4 *>(dbeta_part + (size_t)n * C + c + 4) = A_hi;
    *reinterpret_cast<float4 *>(dgamma_part + (size_t)n * C + c) = B_lo;
    *reinterpret_cast<float4 *>(dgamma_part + (size_t)n * C + c + 4) = B_hi;
  }
  // group sums from the channel totals, per half; the halves share a group from C/G = 8 on
  float t1_lo = gn_dot4(ga_lo, A_lo), t1_hi = gn_dot4(ga_hi, A_hi);
  float t2_lo = gn_dot4(ga_lo, B_lo), t2_hi = gn_dot4(ga_hi, B_hi);
  if (cpg >= 8) { t1_lo += t1_hi; t1_hi = t1_lo; t2_lo += t2_hi; t2_hi = t2_lo; }
  if (cpg >= 16) { t1_lo += __shfl_xor(t1_lo, 1); t1_hi = t1_lo; t2_lo += __shfl_xor(t2_lo, 1); t2_hi = t2_lo; }
  if (cpg >= 32) { t1_lo += __shfl_xor(t1_lo, 2); t1_hi = t1_lo; t2_lo += __shfl_xor(t2_lo, 2); t2_hi = t2_lo; }
  const float inv_m = 1.0f / (float)(cpg * HW);
  const float m1_lo = t1_lo * inv_m, m2_lo = t2_lo * inv_m, m1_hi = t1_hi * inv_m, m2_hi = t2_hi * inv_m;
  float4 so_lo = zero, so_hi = zero;      // sum of the fp32 dx per channel = the producing convolution's bias gradient
  for (int first = p0; first < HW; first += 32 * kGnBf16Batch) {
    uint4 rx[kGnBf16Batch], rd[kGnBf16Batch];
    GN_BF16_LOADS(j, p, first) { rx[j] = xs[(size_t)p * stride8]; rd[j] = ds[(size_t)p * stride8]; }
    GN_BF16_BATCH(j, p, first) {
      float4 va, vb, da, db;
      gn_bf16_widen(rx[j], va, vb);
      gn_bf16_widen(rd[j], da, db);
      const float4 o_lo = gn_bf16_dx4(gn_bf16_half(va, da, pb_lo, mean_lo, rstd_lo, ga_lo, be_lo), rstd_lo, ga_lo, m1_lo, m2_lo);
      const float4 o_hi = gn_bf16_dx4(gn_bf16_half(vb, db, pb_hi, mean_hi, rstd_hi, ga_hi, be_hi), rstd_hi, ga_hi, m1_hi, m2_hi);
      os[(size_t)p * stride8] = gn_bf16_narrow(o_lo, o_hi);
      so_lo = gn_add4(so_lo, o_lo);
      so_hi = gn_add4(so_hi, o_hi);
    }
  }
  if (dpre_part) {                                   // (uniform)
    gn_bf16_channel_total(so_lo, so_hi, s_w4, tid);
    if (tid < 4) {
      *reinterpret_cast<float4 *>(dpre_part + (size_t)n * C + c) = so_lo;
      *reinterpret_cast<float4 *>(dpre_part + (size_t)n * C + c + 4) = so_hi;
    }
  }
}

}  // namespace shr

extern "C" int shr_group_norm_relu_bf16_fwd(const uint16_t *x, const float *pre_bias, const float *gamma, const float *beta,
                                            int N, int C, int HW, int G, float eps, uint16_t *y, float *mean, float *rstd,
                                            void *stream) {
  using namespace shr;
  if (N == 0) return SHR_OK;
  if (!x || !gamma || !beta || !y || !mean || !rstd || N < 0 || HW <= 0) return SHR_EINVAL;
  if (!gn_supported(C, G) ||
      ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)pre_bias)) & 15u))
    return SHR_EINVAL;
  if (N > 65535) return SHR_ETOOLARGE;
  hipLaunchKernelGGL(group_norm_relu_bf16_fwd_kernel, dim3((unsigned)(C / kGnBlockC), (unsigned)N), dim3(kGnBf16Threads),
                     0, (hipStream_t)stream, x, pre_bias, gamma, beta, C, HW, G, eps, y, mean, rstd);
  return (int)hipGetLastError();
}

extern "C" int shr_group_norm_relu_bf16_bwd(const uint16_t *x, const float *pre_bias, const uint16_t *dy, const float *gamma,
                                            const float *beta, const float *mean, const float *rstd, int N, int C, int HW,
                                            int G, uint16_t *dx, float *dgamma_partial, float *dbeta_partial,
                                            float *dpre_partial, float *dgamma, float *dbeta, float *dpre, void *stream) {
  using namespace shr;
  if (N == 0) return SHR_OK;
  if (!x || !dy || !gamma || !beta || !mean || !rstd || !dx || !dgamma_partial || !dbeta_partial || N < 0 || HW <= 0)
    return SHR_EINVAL;
  if (!gn_supported(C, G) ||
      ((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)dgamma_partial |
         (uintptr_t)dbeta_partial | (uintptr_t)pre_bias | (uintptr_t)dpre_partial)) & 15u))
    return SHR_EINVAL;
  if ((pre_bias != nullptr) != (dpre_partial != nullptr)) return SHR_EINVAL;
  if (N > 65535) return SHR_ETOOLARGE;
  hipLaunchKernelGGL(group_norm_relu_bf16_bwd_kernel, dim3((unsigned)(C / kGnBlockC), (unsigned)N), dim3(kGnBf16Threads),
                     0, (hipStream_t)stream, x, pre_bias, dy, gamma, beta, mean, rstd, C, HW, G, dx, dgamma_partial,
                     dbeta_partial, dpre_partial);
  if (dgamma && dbeta)
    gn_launch_param_grad(dgamma_partial, dbeta_partial, dpre_partial, N, C, dgamma, dbeta, dpre, (hipStream_t)stream);
  return (int)hipGetLastError();
}
