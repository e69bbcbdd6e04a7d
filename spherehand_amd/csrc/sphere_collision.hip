// sphere_collision.hip -- the term of the sphere model's Gauss-Newton fit against self-penetration
// (shr_sphere_collision_normal): every pair (a, b, m) of a table whose centres are closer than the pair's minimum
// distance m leaves the residual h = m - |c_a - c_b| and one row -u^T (Jc_a - Jc_b).  A row couples TWO spheres, so it
// does not fit the per-sphere moments of sphere_icp.hip's record: A and g are assembled per pair here.
//
// Inverts (reference file:line): HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by the
// key-point skinning of HandBallPrimitiveRender (mesh/render.py:65-88), under the pair table of CollisionLoss
// (mesh/render.py:145-176).  The reference's hinge relu(36 - |c_a - c_b|^2) is no square of a residual; the reference
// has no counterpart of the normal equations.
//
//   one workgroup of 256 threads (four wave64) per sample; the sample's 3J x 26 fp32 Jacobian and its centres live in
//   LDS beside the chunk's compacted pairs and the rows of 64 of them (43 552 bytes at the unit's J = 64).
//   per chunk of 256 pairs, one pair per thread:
//   decide    the pair is skipped (a bad index, a == b, m not > 0: nothing is read), inactive, or ACTIVE with
//             h = m - n; penetration[b, k] is written.
//   compact   ballot and prefix per wave, the waves' totals through LDS: the active pairs keep their ascending k.  The
//             list holds (h, u) and (a, b, rowed); u = 0 where the centres coincide.
//   add       the list is taken in groups of 64 pairs: the group's rows, 26 entries each, are formed once from the Jacobian
//             in LDS (one entry per thread and pass), and thread t, which owns entries t, t + 256 of A's 351 lower entries
//             and g's 26 (normal_eq.h's neq_owned), adds the group's pairs with rows to them in order: two barriers per
//             group, none per pair.  The last thread runs the cost chain.
//   The Jacobian is staged when the first pair with a row turns up: a sample without one (the common case) never reads it.
//   LDS banks: a pair's record is read at one address by all lanes (a broadcast).  In the add loop every lane reads
//   row[i][a] and row[i][c] of ONE pair: 26 consecutive doubles, 52 dwords of the 64 banks a ds_read_b64 sees, so distinct
//   entries are distinct banks and equal entries one address: no conflict.  Forming the rows, a wave's 64 lanes span up to
//   four pairs (26 entries each): their Jacobian reads fall into up to four rows of 26 consecutive dwords, at most a 4-way
//   conflict on the 32 banks of a ds_read_b32, in the pass that runs once per pair; the rows are written to consecutive
//   doubles.
#include "normal_eq.h"

namespace shr {

constexpr int kScnMaxK = 4096;
constexpr int kScnWaves = kNeqThreads / 64;
constexpr int kScnGroup = 64;                             // pairs whose rows are held in LDS at a time

struct ScnPair {
  double h, u0, u1, u2;
};

struct ScnLds {
  ScnPair pair[kNeqThreads];                               // the chunk's active pairs, k ascending
  double row[kScnGroup][kNeqN];                            // the rows of a group of the chunk's pairs
  float jac[kNeqMaxJ * 3 * kNeqN];
  float4 centre[kNeqMaxJ];
  int ab[kNeqThreads];                                     // a | b << 8 | (the pair has a row) << 16
  int wave_active[kScnWaves], wave_rows[kScnWaves];
};

// row_c of a pair = d h / d params_c: 0 - ((u0 D_0c + u1 D_1c) + u2 D_2c), D_ic = jac[3a + i, c] - jac[3b + i, c] in fp64
__device__ inline double scn_row(const float *jac, int a, int b, int c, double u0, double u1, double u2) {
  const float *qa = jac + 3 * a * kNeqN + c, *qb = jac + 3 * b * kNeqN + c;
  const double d0 = (double)qa[0] - (double)qb[0];
  const double d1 = (double)qa[kNeqN] - (double)qb[kNeqN];
  const double d2 = (double)qa[2 * kNeqN] - (double)qb[2 * kNeqN];
  return 0.0 - ((u0 * d0 + u1 * d1) + u2 * d2);
}

__global__ void __launch_bounds__(kNeqThreads)
sphere_collision_kernel(const float4 *__restrict__ centres, const float *__restrict__ jac, const int *__restrict__ pair_a,
                        const int *__restrict__ pair_b, const float *__restrict__ pair_min, double w, int J, int K, int mode,
                        int used, double *__restrict__ A, double *__restrict__ g, double *__restrict__ cost,
                        int *__restrict__ count, double *__restrict__ penetration) {
  __shared__ ScnLds s;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  if (tid < J) s.centre[tid] = centres[(size_t)b * J + tid];
  const NeqOwned own = neq_owned(tid);
  double acc0 = 0.0, acc1 = 0.0, C = 0.0;
  int rows = 0;
  bool staged = false;
  __syncthreads();
  for (int base = 0; base < K; base += kNeqThreads) {
    const int k = base + tid;
    bool active = false, rowed = false;
    double h = 0.0, u0 = 0.0, u1 = 0.0, u2 = 0.0;
    int pa = 0, pb = 0;
    if (k < K) {
      pa = pair_a[k];
      pb = pair_b[k];
      const float m = pair_min[k];
      if ((unsigned)pa < (unsigned)J && (unsigned)pb < (unsigned)J && pa != pb && m > 0.f) {     // (a NaN m: skipped)
        const float4 ca = s.centre[pa], cb = s.centre[pb];
        const double e0 = (double)ca.x - (double)cb.x, e1 = (double)ca.y - (double)cb.y, e2 = (double)ca.z - (double)cb.z;
        const double n = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
        active = n < (double)m;                            // a distance exactly m is not active; a NaN never fires
        if (active) {
          h = (double)m - n;
          rowed = n > 0.0;                                 // coincident centres pay m^2 and have no direction
          if (rowed) {
            u0 = e0 / n;
            u1 = e1 / n;
            u2 = e2 / n;
          }
        }
      }
      if (penetration) penetration[(size_t)b * K + k] = h;
    }
    const unsigned long long act = __ballot(active), row = __ballot(rowed);
    const int pos = __popcll(act & ((1ull << lane) - 1ull));
    if (lane == 0) {
      s.wave_active[wave] = __popcll(act);
      s.wave_rows[wave] = __popcll(row);
    }
    __syncthreads();
    int offset = 0, nact = 0, nrows = 0;
#pragma unroll
    for (int v = 0; v < kScnWaves; v++) {
      const int n = s.wave_active[v];
      offset += v < wave ? n : 0;
      nact += n;
      nrows += s.wave_rows[v];
    }
    rows += nrows;
    if (active) {
      ScnPair rec;
      rec.h = h;
      rec.u0 = u0;
      rec.u1 = u1;
      rec.u2 = u2;
      s.pair[offset + pos] = rec;
      s.ab[offset + pos] = pa | (pb << 8) | ((int)rowed << 16);
    }
    if (used && nrows > 0 && !staged) {                    // (uniform: every thread holds the same nrows)
      for (int idx = tid; idx < 3 * J * kNeqN; idx += kNeqThreads) s.jac[idx] = jac[(size_t)b * 3 * J * kNeqN + idx];
      staged = true;
    }
    __syncthreads();
    if (used) {
      if (tid == kNeqThreads - 1)                          // the cost: the active pairs, k ascending
        for (int i = 0; i < nact; i++) C += s.pair[i].h * s.pair[i].h;
      if (nrows > 0)                                       // (uniform, and so are the barriers inside)
        for (int first = 0; first < nact; first += kScnGroup) {
          const int ng = nact - first < kScnGroup ? nact - first : kScnGroup;
          for (int idx = tid; idx < ng * kNeqN; idx += kNeqThreads) {      // the group's rows, every entry once
            const int i = idx / kNeqN, c = idx - i * kNeqN;
            const int ab = s.ab[first + i];
            double r = 0.0;
            if (ab >> 16) {
              const ScnPair p = s.pair[first + i];
              r = scn_row(s.jac, ab & 255, (ab >> 8) & 255, c, p.u0, p.u1, p.u2);
            }
            s.row[i][c] = r;
          }
          __syncthreads();
          for (int i = 0; i < ng; i++) {
            if (!(s.ab[first + i] >> 16)) continue;        // no row (uniform)
            const double *r = s.row[i];
            acc0 += r[own.a0] * r[own.c0];
            if (own.c1 >= 0) acc1 += r[own.a1] * r[own.c1];
            else if (own.own_g) acc1 += s.pair[first + i].h * r[own.a1];
          }
          __syncthreads();                                 // the next group rewrites the rows
        }
    }
    __syncthreads();                                       // the next chunk rewrites the list
  }
  if (tid == 0) count[b] = rows;
  if (mode == kNeqKeep) return;
  const bool add = mode == kNeqAdd;
  if (tid == kNeqThreads - 1) neq_emit_cost(cost, b, used ? w * C : 0.0, add);
  neq_emit_A(A, b, own.a0, own.c0, used ? w * acc0 : 0.0, add);
  if (own.c1 >= 0) neq_emit_A(A, b, own.a1, own.c1, used ? w * acc1 : 0.0, add);
  else if (own.own_g) neq_emit_g(g, b, own.a1, used ? w * acc1 : 0.0, add);
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_sphere_collision_normal_workspace_bytes(int B, int J, int K) {
  if (B < 0 || J < 0 || K < 0) return -1;
  return 0;
}

extern "C" int shr_sphere_collision_normal(const float *centres, const float *jac, const int32_t *pair_a, const int32_t *pair_b,
                                           const float *pair_min, float weight, int B, int J, int K, int accumulate, double *A,
                                           double *g, double *cost, int32_t *count, double *penetration, void *workspace,
                                           void *stream) {
  if (B < 0 || J < 1 || K < 0 || (accumulate != 0 && accumulate != 1)) return SHR_EINVAL;
  if (!neq_weight_ok(weight)) return SHR_EINVAL;
  if ((pair_a == nullptr) != (pair_b == nullptr) || (pair_a == nullptr) != (pair_min == nullptr)) return SHR_EINVAL;
  if (K > 0 && !pair_a) return SHR_EINVAL;
  if (neq_too_large(B, 1, J) || K > kScnMaxK) return SHR_ETOOLARGE;
  if (B == 0) return SHR_OK;
  if (!centres || !jac || !A || !g || !cost || !count) return SHR_EINVAL;
  if (!neq_aligned(4, jac, pair_a, pair_b, pair_min, count) || !neq_aligned(8, A, g, cost, penetration) ||
      !neq_aligned(16, centres, workspace))
    return SHR_EINVAL;
  const int used = pair_a && K > 0 && weight > 0.f;
  const int mode = !accumulate ? kNeqWrite : (used ? kNeqAdd : kNeqKeep);
  hipLaunchKernelGGL(sphere_collision_kernel, dim3((unsigned)B), dim3(kNeqThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4 *>(centres), jac, pair_a, pair_b, pair_min, (double)weight, J,
                     pair_a ? K : 0, mode, used, A, g, cost, count, penetration);
  return (int)hipGetLastError();
}
