// normal_eq.h -- the shape of the sphere fit's Gauss-Newton normal equations, stated once for every unit that builds them
// (sphere_icp_scan.h, sphere_render_icp.hip, sphere_prior.hip, sphere_collision.hip, sphere_temporal.hip, sphere_accel.hip,
// pose_vae.hip; icp_tile.h and pose_ik.hip take the constants and the entry map): A [B,26,26] symmetric, g [B,26] and
// cost [B] in fp64, one workgroup of 256 threads per sample or frame, every entry of A's lower triangle and of g with ONE
// owner thread, which sums its chain in a fixed order and then writes the entry or adds it to what the buffer holds.
//   constants    the parameter count, the triangle, the workgroup and the largest sphere count
//   entry map    idx 0 .. 350 -> (a, c), a >= c, of A's lower triangle, rows ascending; idx 351 + i -> g_i
//   ownership    the two entries thread t of a workgroup owns: t and t + 256
//   emission     one entry of A (lower triangle read, both triangles written), one of g, the cost: written or added
//   chains       the per-sphere contractions every term's A and g are made of; each returns the plain chain, the caller
//                spells its own sign and weight (-(+0) is -0 and 0.0 - (+0) is +0: the spelling is part of the bits)
//   entry checks the host side every entry repeats: a weight, the pointers' alignment, the launch limits
#pragma once
#include "common.h"

namespace shr {

constexpr int kNeqN = 26;                                  // pose parameters
constexpr int kNeqTri = kNeqN * (kNeqN + 1) / 2;           // 351
constexpr int kNeqThreads = 256;
constexpr int kNeqMaxJ = 64;

struct NeqEntry {
  int a, c;                                                // a >= c
};

// entry idx of A's lower triangle; `from`: a row known not to lie behind idx's (the search starts there)
constexpr __host__ __device__ inline NeqEntry neq_entry(int idx, int from = 0) {
  int a = from;
  while ((a + 1) * (a + 2) / 2 <= idx) a++;
  return NeqEntry{a, idx - a * (a + 1) / 2};
}

// entry idx = 351 + i of a thread's range is g_i
constexpr __host__ __device__ inline int neq_g_entry(int idx) { return idx - kNeqTri; }

constexpr bool neq_map_is_a_bijection() {
  int hits[kNeqN][kNeqN] = {};
  for (int idx = 0; idx < kNeqTri; idx++) {
    const NeqEntry e = neq_entry(idx);
    if (e.a < 0 || e.a >= kNeqN || e.c < 0 || e.c > e.a) return false;
    hits[e.a][e.c]++;
  }
  for (int a = 0; a < kNeqN; a++)
    for (int c = 0; c <= a; c++)
      if (hits[a][c] != 1) return false;
  return true;
}
static_assert(neq_entry(0).a == 0 && neq_entry(0).c == 0, "the first entry is (0, 0)");
static_assert(neq_entry(kNeqTri - 1).a == kNeqN - 1 && neq_entry(kNeqTri - 1).c == kNeqN - 1, "the last entry is (25, 25)");
static_assert(neq_entry(kNeqTri - 1, kNeqN - 1).a == kNeqN - 1 && neq_entry(27, 3).a == 6, "a search from a row before");
static_assert(neq_g_entry(kNeqTri) == 0 && neq_g_entry(kNeqTri + kNeqN - 1) == kNeqN - 1, "351 + i is g_i");
static_assert(neq_map_is_a_bijection(), "the 351 indices hit every (a >= c) once");
static_assert(kNeqTri + kNeqN <= 2 * kNeqThreads, "two entries per thread cover A's triangle and g");

// the entries thread tid of a workgroup owns: idx0 = tid is one of A's; idx1 = tid + 256 is one of A's (c1 >= 0), one of
// g's (own_g: g_a1), or none
struct NeqOwned {
  int a0, c0, a1, c1;
  bool own_g;
};

__device__ __forceinline__ NeqOwned neq_owned(int tid) {
  NeqOwned o;
  const NeqEntry e0 = neq_entry(tid);
  o.a0 = e0.a;
  o.c0 = e0.c;
  const int idx1 = tid + kNeqThreads;
  o.a1 = o.a0;
  o.c1 = -1;
  if (idx1 < kNeqTri) {
    const NeqEntry e1 = neq_entry(idx1, o.a0);
    o.a1 = e1.a;
    o.c1 = e1.c;
  } else if (idx1 < kNeqTri + kNeqN) {
    o.a1 = neq_g_entry(idx1);
  }
  o.own_g = idx1 >= kNeqTri && idx1 < kNeqTri + kNeqN;
  return o;
}

// What an entry does with A, g and cost: they are the term's; the term's are added to what the buffers hold; or they are
// left alone (a term without a weight on top of the others).  The caller returns before it emits in the last case; the
// emission below is told `add` and nothing else.
enum { kNeqWrite = 0, kNeqAdd = 1, kNeqKeep = 2 };

// A[b][a][c] (a >= c) = v, or what the lower triangle holds + v; the result goes to both triangles
__device__ __forceinline__ void neq_emit_A(double *__restrict__ A, int b, int a, int c, double v, bool add) {
  double *low = A + ((size_t)b * kNeqN + a) * kNeqN + c;
  const double out = add ? *low + v : v;
  *low = out;
  A[((size_t)b * kNeqN + c) * kNeqN + a] = out;
}

__device__ __forceinline__ void neq_emit_g(double *__restrict__ g, int b, int a, double v, bool add) {
  double *out = g + (size_t)b * kNeqN + a;
  *out = add ? *out + v : v;
}

__device__ __forceinline__ void neq_emit_cost(double *__restrict__ cost, int b, double v, bool add) {
  cost[b] = add ? cost[b] + v : v;
}

// The chain over the spheres, ascending, of q_a^T S q_c: mom holds kMom doubles per sphere, [S as uu^T (6: 00 01 02 11 12 22) |
// h (3) | . | rows | ..], jac the spheres' 3 x 26 fp32 Jacobians (both in LDS).  A sphere without a row adds nothing.
template <int kMom>
__device__ __forceinline__ double neq_moments_A(const double *mom, const float *jac, int J, int a, int c) {
  double acc = 0.0;
  for (int j = 0; j < J; j++) {
    const double *m = mom + j * kMom;
    if (m[10] == 0.0) continue;
    const float *q = jac + 3 * j * kNeqN;
    const double c0 = (double)q[c], c1 = (double)q[kNeqN + c], c2 = (double)q[2 * kNeqN + c];
    const double t0 = (m[0] * c0 + m[1] * c1) + m[2] * c2;
    const double t1 = (m[1] * c0 + m[3] * c1) + m[4] * c2;
    const double t2 = (m[2] * c0 + m[4] * c1) + m[5] * c2;
    acc += ((double)q[a] * t0 + (double)q[kNeqN + a] * t1) + (double)q[2 * kNeqN + a] * t2;
  }
  return acc;
}

// its counterpart for g: the chain of q_a^T h
template <int kMom>
__device__ __forceinline__ double neq_moments_g(const double *mom, const float *jac, int J, int a) {
  double acc = 0.0;
  for (int j = 0; j < J; j++) {
    const double *m = mom + j * kMom;
    if (m[10] == 0.0) continue;
    const float *q = jac + 3 * j * kNeqN;
    acc += ((double)q[a] * m[6] + (double)q[kNeqN + a] * m[7]) + (double)q[2 * kNeqN + a] * m[8];
  }
  return acc;
}

// The chain over the spheres with rows (act[j] != 0), ascending, of sum_axis x[3j + axis][r] y[3j + axis][c]: x and y are
// 3J x 26 fp32 Jacobians in LDS, of one frame or of two
__device__ __forceinline__ double neq_gram(const int *act, const float *x, const float *y, int r, int c, int J) {
  double acc = 0.0;
  for (int j = 0; j < J; j++) {
    if (!act[j]) continue;                                 // a sphere without rows adds nothing
    const float *q0 = x + 3 * j * kNeqN + r, *q1 = y + 3 * j * kNeqN + c;
    acc += ((double)q0[0] * (double)q1[0] + (double)q0[kNeqN] * (double)q1[kNeqN]) +
           (double)q0[2 * kNeqN] * (double)q1[2 * kNeqN];
  }
  return acc;
}

// its counterpart for g: the chain of sum_axis x[3j + axis][r] e[j][axis]
__device__ __forceinline__ double neq_gram_g(const int *act, const float *x, const double (*e)[3], int r, int J) {
  double acc = 0.0;
  for (int j = 0; j < J; j++) {
    if (!act[j]) continue;
    const float *q = x + 3 * j * kNeqN;
    acc += ((double)q[r] * e[j][0] + (double)q[kNeqN + r] * e[j][1]) + (double)q[2 * kNeqN + r] * e[j][2];
  }
  return acc;
}

// ---- the host side of an entry

// a term's weight: finite and >= 0 (a NaN is neither)
inline bool neq_weight_ok(float w) { return w >= 0.f && w <= 3.40282346638528859812e38f; }

// every pointer of a group is a multiple of `bytes` (a power of two); a null pointer is
template <class... P>
inline bool neq_aligned(unsigned bytes, P... p) {
  return ((... | (uintptr_t)p) & (uintptr_t)(bytes - 1)) == 0;
}

// a grid's y and z take at most 65535 samples and 65535 (sample, view) pairs; the LDS tables take kNeqMaxJ spheres
inline bool neq_too_large(int B, int V, int J) { return B > 65535 || (long long)B * V > 65535 || J > kNeqMaxJ; }

}  // namespace shr
