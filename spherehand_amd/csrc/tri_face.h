// tri_face.h -- the reference triangle kernel's per-face and per-pixel arithmetic, restated once for every mesh kernel
// (tri_raster.hip, mesh_depth.hip, and through tri_tap.h the backwards; capi.hip's division self-test).
//
// mesh/cuda_kernel/depth_rasterization_cuda_kernel.cu:25-110, operator for operator: fp32, one rounding per written
// operator (-ffp-contract=off), IEEE division -- the depth bits are the reference's.  The kernels compose these pieces
// and park what they keep in their own LDS layouts; a piece a caller does not use costs it nothing (the set-up's
// twelve divisions live in face_matrix and edge_slopes, apart from the culls and ranges).
#pragma once

#include "common.h"

namespace shr {

// CUDA double -> int32 conversion (cvt.rzi.s32.f64): truncate, saturate, NaN -> 0.
// The operands here are fp32 values promoted to double, so fp32 compares suffice.
__device__ __forceinline__ int cvt_rz_sat(float d) {
  if (d != d) return 0;
  if (d >= 2147483648.0f) return 2147483647;
  if (d <= -2147483648.0f) return (int)0x80000000;
  return (int)d;
}

// .cu:33-56: the back-face cull and the sort of the corners by x.  p: the corners sorted by x, sorted corner a is corner
// order[a] of f.  False for a back face (.cu:33) or one with x0 == x2 (.cu:54).
__device__ __forceinline__ bool face_sort(const float (&f_)[9], float (&p)[3][3], int (&order)[3]) {
  // (opaque copies: the compiler turns the selects of the sort below -- "vertex order[a] of three" -- into ONE load from a
  // select of addresses, which pins the nine values to a scratch array: 3 scratch stores and 9 dependent scratch loads per
  // set-up, ScratchSize 48, in every kernel that sets faces up; values that are no longer loads stay in registers)
  float f[9];
#pragma unroll
  for (int k = 0; k < 9; k++) { f[k] = f_[k]; asm("" : "+v"(f[k])); }
  bool live = !((f[7] - f[1]) * (f[3] - f[0]) < (f[4] - f[1]) * (f[6] - f[0]));   // :33 back face
  int p0, p2;
  if (f[0] < f[3]) { p0 = (f[6] < f[0]) ? 2 : 0; p2 = (f[3] < f[6]) ? 2 : 1; }
  else             { p0 = (f[6] < f[3]) ? 2 : 1; p2 = (f[0] < f[6]) ? 2 : 0; }
  int p1 = 0;
#pragma unroll
  for (int k = 0; k < 3; k++)
    if (p0 != k && p2 != k) p1 = k;
  order[0] = p0; order[1] = p1; order[2] = p2;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int d = 0; d < 3; d++) {
      // select without dynamic indexing (keeps everything in registers)
      const int o = order[a];
      p[a][d] = (o == 0) ? f[d] : ((o == 1) ? f[3 + d] : f[6 + d]);
    }
  if (p[0][0] == p[2][0]) live = false;   // :54
  return live;
}

// .cu:68-69: the face's pixel columns [xi_min, xi_max], and a conservative range [r_lo, r_hi] of the rows its columns'
// spans can hold -- no division.  x0, x2: the smallest and the largest x of face_sort; ya, yb, yc: the corners' y in
// any order (their minimum and maximum do not depend on it).  False when the column range is empty.
__device__ __forceinline__ bool face_ranges(float x0, float x2, float ya, float yb, float yc, int width, int height,
                                            int &xi_min, int &xi_max, int &r_lo, int &r_hi) {
  // max(ceil(x0), 0.) / min(x2, width - 1.)  (fmax/fmin drop a NaN operand)
  xi_min = cvt_rz_sat(fmaxf(ceilf(x0), 0.f));
  xi_max = cvt_rz_sat(fminf(x2, (float)width - 1.f));
  const float ylo = fminf(fminf(ya, yb), yc);
  const float yhi = fmaxf(fmaxf(ya, yb), yc);
  // (a face whose largest x lies in (-1, 0) still reaches column 0 -- the reference truncates x2 towards zero,
  // .cu:69 -- and the span there is an EXTRApolation of the edges: any row)
  const bool wild = !(fabsf(ylo) < 1e9f) || !(fabsf(yhi) < 1e9f) || x2 < 0.f;
  // A column's span ends are edge interpolations slope * (x - xa) + ya at an x inside the edge:
  // convex combinations of the vertices' y up to 4 roundings (<= 2.4e-7 * |y|); rows
  // [ceil(min), trunc(max)] (.cu:89-90; a span end in (-1, 0) truncates to row 0).
  const float yeps = 1e-5f * (fabsf(ylo) + fabsf(yhi)) + 1e-4f;
  r_lo = wild ? 0 : max(0, (int)ceilf(ylo - yeps));
  r_hi = wild ? height - 1 : min(height - 1, max(0, (int)floorf(yhi + yeps)));
  return xi_min <= xi_max;
}

// Order-preserving integer key of an fp32 depth (negative depths included, -0 below +0) and its inverse: the 32-bit
// slots of mesh_depth.hip and the high word of the 64-bit (key << 32 | face) owner slots.
__device__ __forceinline__ uint32_t mkey(float d) {
  const uint32_t b = __float_as_uint(d);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float mkey_inv(uint32_t k) {
  return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu));
}

// .cu:25-69 for one face.  Every field is computed for every face; a caller reads the ranges and corners of a live one only.
struct FaceSetup {
  float p[3][3];                    // corners sorted by x
  int xi_min, xi_max, r_lo, r_hi;   // face_ranges
  bool live;                        // front-facing, x0 != x2, and its columns meet the image
};
__device__ __forceinline__ FaceSetup face_setup(const float (&f)[9], int width, int height) {
  FaceSetup s;
  int order[3];
  const bool front = face_sort(f, s.p, order);
  const bool cols = face_ranges(s.p[0][0], s.p[2][0], s.p[0][1], s.p[1][1], s.p[2][1], width, height, s.xi_min, s.xi_max,
                                s.r_lo, s.r_hi);
  s.live = front && cols;
  return s;
}

// .cu:57-66: the inverse barycentric matrix over the sorted corners (nine IEEE divisions by the denominator)
__device__ __forceinline__ void face_matrix(const float (&p)[3][3], float (&fi)[9]) {
  fi[0] = p[1][1] - p[2][1]; fi[1] = p[2][0] - p[1][0]; fi[2] = p[1][0] * p[2][1] - p[2][0] * p[1][1];
  fi[3] = p[2][1] - p[0][1]; fi[4] = p[0][0] - p[2][0]; fi[5] = p[2][0] * p[0][1] - p[0][0] * p[2][1];
  fi[6] = p[0][1] - p[1][1]; fi[7] = p[1][0] - p[0][0]; fi[8] = p[0][0] * p[1][1] - p[1][0] * p[0][1];
  const float den = (p[2][0] * (p[0][1] - p[1][1]) + p[0][0] * (p[1][1] - p[2][1])) + p[1][0] * (p[2][1] - p[0][1]);
#pragma unroll
  for (int k = 0; k < 9; k++) fi[k] = fi[k] / den;
}

// .cu:75-85: the three edge slopes.  The reference divides per COLUMN, but the quotients depend on the face only: one
// IEEE division each in the set-up instead of two per column in the span test.
struct EdgeSlopes {
  float s01, s12, s02;   // (y1 - y0) / (x1 - x0), (y2 - y1) / (x2 - x1), (y2 - y0) / (x2 - x0)
  int flags;             // bit 0: x1 - x0 != 0, bit 1: x2 - x1 != 0 (else the span end is y1, .cu:77, :83)
};
__device__ __forceinline__ EdgeSlopes edge_slopes(const float (&p)[3][3]) {
  EdgeSlopes e;
  const bool d01 = p[1][0] - p[0][0] != 0.f, d12 = p[2][0] - p[1][0] != 0.f;
  e.s01 = d01 ? (p[1][1] - p[0][1]) / (p[1][0] - p[0][0]) : 0.f;
  e.s12 = d12 ? (p[2][1] - p[1][1]) / (p[2][0] - p[1][0]) : 0.f;
  e.s02 = (p[2][1] - p[0][1]) / (p[2][0] - p[0][0]);
  e.flags = (d01 ? 1 : 0) | (d12 ? 2 : 0);
  return e;
}

// .cu:72-90: the rows [yi_min, yi_max] of column xi's span of the face.  (x0, y0), (x1, y1): the first two corners
// sorted by x; the slopes and their flags from edge_slopes.
__device__ __forceinline__ void span_rows(float x0, float y0, float x1, float y1, float s01, float s12, float s02,
                                          int sflags, int xi, int height, int &yi_min, int &yi_max) {
  const float xf = (float)xi;
  float yi1;
  if (xf <= x1) yi1 = (sflags & 1) ? s01 * (xf - x0) + y0 : y1;
  else yi1 = (sflags & 2) ? s12 * (xf - x1) + y1 : y1;
  const float yi2 = s02 * (xf - x0) + y0;
  yi_min = cvt_rz_sat(fmaxf(0.f, ceilf(fminf(yi1, yi2))));
  yi_max = cvt_rz_sat(fminf(fmaxf(yi1, yi2), (float)height - 1.f));
}

// .cu:97-103: pixel (xf, yf)'s barycentric weights w and the same clamped to [0, 1], c; returns the sum of the c
__device__ __forceinline__ float pixel_weights(const float (&fi)[9], float xf, float yf, float (&w)[3], float (&c)[3]) {
  float c_sum = 0.f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    w[k] = (fi[3 * k + 0] * xf + fi[3 * k + 1] * yf) + fi[3 * k + 2];
    c[k] = fminf(fmaxf(w[k], 0.f), 1.f);
    c_sum += c[k];
  }
  return c_sum;
}

// ---- the triangle pixel's seven IEEE divisions (.cu:104-110) with the denominators' work shared -------------------------
// hipcc's fp32 division a / d (-fhip-fp32-correctly-rounded-divide-sqrt) is
//     ds = v_div_scale(d, d, a); as = v_div_scale(a, d, a); r = v_rcp(ds); e = fma(-ds, r, 1); r1 = fma(e, r, r);
//     q0 = as * r1; e1 = fma(-ds, q0, as); q1 = fma(e1, r1, q0); e2 = fma(-ds, q1, as); q = v_div_fmas(e2, r1, q1);
//     v_div_fixup(q, d, a)
// and v_div_scale leaves BOTH operands alone (ds = d, as = a, v_div_fmas = fma, v_div_fixup = identity up to the sign it
// would give anyway) when d is normal and below 2^126, a is zero or at least 2^-103, and the exponents differ by less than
// 96 upwards and 126 downwards.  Inside that domain r1 depends on d only: three divisions by one denominator share it
// (w[k] / w_sum), and a denominator that is a constant of the face (its corners' z) brings it from the set-up.  These are
// the compiler's own instructions on the compiler's own operands -- the quotients are the same bits (shr_selftest_division
// compares them over random and edge operands; every parity test of the triangle kernels runs through them).
__device__ __forceinline__ float div_rcp_refined(float d) {
  const float r = __builtin_amdgcn_rcpf(d);
  const float e = __builtin_fmaf(-d, r, 1.0f);
  return __builtin_fmaf(e, r, r);
}
__device__ __forceinline__ float div_with(float a, float d, float r1) {
  const float q0 = a * r1;
  const float e1 = __builtin_fmaf(-d, q0, a);
  const float q1 = __builtin_fmaf(e1, r1, q0);
  const float e2 = __builtin_fmaf(-d, q1, a);
  return __builtin_fmaf(e2, r1, q1);
}
// a corner depth whose reciprocal may be shared: 2^-40 <= |z| <= 2^40 (a hand's are within +-100 of the crop's centre; the
// sign rides through the same instructions as in the compiler's sequence, a zero quotient's included)
__device__ __forceinline__ bool div_tame_z(float z) { return fabsf(z) >= 0x1p-40f && fabsf(z) <= 0x1p40f; }
// The pixel: clamped barycentric weights w (each in [0, 1]), their sum, the corners' z and -- `tame`: all three
// div_tame_z -- their refined reciprocals rz.  Fast path when every weight is zero or at least 2^-60 (the sum is then
// within [2^-60, 3], w / w_sum zero or at least 2^-62, and that over z zero or at least 2^-102: all inside the domain
// above); the plain divisions otherwise (a constant `tame = false` leaves only those).
__device__ __forceinline__ float tri_pixel_depth(float w0, float w1, float w2, float w_sum, const float (&pz)[3],
                                                 const float (&rz)[3], bool tame) {
  // "every weight is zero or at least 2^-60" on the bit patterns of the non-negative weights: bits - 1 wraps a zero
  // to the top, so one unsigned minimum and one compare.  (The sum needs no test of its own: it is at least the largest
  // weight; all three zero or a NaN among them give NaN on either path, and the pixel is skipped.)  As a chain of && / ||
  // over float compares the test compiled into a branch per clause and cost what the shared reciprocals save: 256 crops
  // 284 us, 275 as one mask of compares, against 264 with no test of the weights at all.
  const uint32_t t = __float_as_uint(0x1p-60f) - 1u;
  const uint32_t m = min(min(__float_as_uint(w0) - 1u, __float_as_uint(w1) - 1u), __float_as_uint(w2) - 1u);
  const bool ok = tame & (m >= t);
  if (ok) {
    const float rs = div_rcp_refined(w_sum);
    const float u0 = div_with(div_with(w0, w_sum, rs), pz[0], rz[0]);
    const float u1 = div_with(div_with(w1, w_sum, rs), pz[1], rz[1]);
    const float u2 = div_with(div_with(w2, w_sum, rs), pz[2], rz[2]);
    return 1.0f / ((u0 + u1) + u2);
  }
  w0 = w0 / w_sum; w1 = w1 / w_sum; w2 = w2 / w_sum;
  return 1.0f / ((w0 / pz[0] + w1 / pz[1]) + w2 / pz[2]);
}

// .cu:97-110 for a pixel inside its column's span: the depth the reference offers to its atomicMin (NaN: none)
__device__ __forceinline__ float pixel_depth(const float (&fi)[9], float xf, float yf, const float (&pz)[3],
                                             const float (&rz)[3], bool tame) {
  float w[3], c[3];
  const float c_sum = pixel_weights(fi, xf, yf, w, c);
  return tri_pixel_depth(c[0], c[1], c[2], c_sum, pz, rz, tame);
}

}  // namespace shr
