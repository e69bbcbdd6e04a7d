// sphere_accel.hip -- the constant-velocity term of the sphere model's sequence fit (shr_sphere_accel_normal): per triple of
// frames (k - 1, k, k + 1) and per sphere j the second difference a = (c_j(k - 1) + c_j(k + 1)) - 2 c_j(k) of the model-frame
// centres leaves three rows, +Jc_j(k - 1) in frame k - 1's columns, -2 Jc_j(k) in frame k's and +Jc_j(k + 1) in frame
// k + 1's.  A row couples THREE frames, so beside the diagonal blocks A, the gradient g and the first off-diagonal block E
// the term has a SECOND off-diagonal block F per frame: the normal equations of a sequence are block-pentadiagonal
// (lm_seq2.hip solves them).
//
// Inverts (reference file:line): nothing; the energy is of the family of ClampedL2lLoss / TemporalSmoothnessLoss
// (network/util_modules.py:349-381), one difference further.  The reference has no counterpart of the term or of the
// normal equations.
//
//   one workgroup of 256 threads (four wave64) PER FRAME b, t = b mod T its place in its sequence, as sphere_temporal_kernel:
//   one owner per output entry, nothing summed across threads, no second pass.  The frame belongs to up to three triples:
//   `prev` (centre t - 1, the frame is its last), `mid` (centre t) and `next` (centre t + 1, the frame is its first).  The
//   3J x 26 fp32 Jacobians of frames b, b + 1 (for E) and b + 2 (for F) live in LDS (3 x 19 968 bytes at the unit's J = 64)
//   beside the three triples' a, cost terms and flags: 66 816 bytes.
//   decide    thread 64 which + j decides (triple `which`, sphere j): a in fp64 from the fp32 centres of b - 2 ... b + 2, n2,
//             the cost term min(n2, cap2) and whether the sphere has rows (n2 < cap2; a NaN n2: no term at all).
//   add       thread t owns entries t, t + 256 of A's 351 lower entries and g's 26, and entries t, t + 256, t + 512 of E's and
//             F's 676 each: normal_eq.h's chains from 0 over the spheres with rows, ascending, a sphere's three axes summed first.  The
//             last thread runs prev's cost chain: the triple's cost is stored with its last frame.
//   A frame reads its neighbours' inputs and writes only its own outputs; a sequence does not see the other sequences.
//   LDS banks: in the add loops a wave's lanes read jac[3j + axis][r] and [c] of ONE sphere: 26 consecutive dwords, distinct
//   entries in distinct banks, equal entries one address; a, term and act are read at one address by all lanes.
#include "normal_eq.h"

namespace shr {

struct SanLds {
  float jac[3][kNeqMaxJ * 3 * kNeqN];                      // frame b's, b + 1's, b + 2's
  double a[3][kNeqMaxJ][3];                                // prev, mid, next: (c(k - 1) + c(k + 1)) - 2 c(k)
  double term[3][kNeqMaxJ];                                // min(n2, cap2); 0 where the sphere has no term
  int act[3][kNeqMaxJ];                                    // the sphere has rows
};

__global__ void __launch_bounds__(kNeqThreads)
sphere_accel_kernel(const float4 *__restrict__ centres, const float *__restrict__ jac, const float *__restrict__ triple_weight,
                    double aw, double cap2, int T, int J, int add, int add_E, int used, double *__restrict__ A,
                    double *__restrict__ g, double *__restrict__ E, double *__restrict__ F, double *__restrict__ cost,
                    int *__restrict__ count) {
  __shared__ SanLds s;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int t = b % T;
  // the centre of a triple is a frame 1 ... T - 2 of its sequence
  const bool has_p = t >= 2, has_m = t >= 1 && t <= T - 2, has_n = t <= T - 3;
  const float fp = !has_p ? 0.f : triple_weight ? triple_weight[b - 1] : 1.f;
  const float fm = !has_m ? 0.f : triple_weight ? triple_weight[b] : 1.f;
  const float fn = !has_n ? 0.f : triple_weight ? triple_weight[b + 1] : 1.f;
  const bool live_p = fp > 0.f, live_m = fm > 0.f, live_n = fn > 0.f;      // (a NaN weight: no term)
  const bool use_p = used && live_p, use_m = used && live_m, use_n = used && live_n;
  const double wp = use_p ? aw * (double)fp : 0.0, wm = use_m ? aw * (double)fm : 0.0, wn = use_n ? aw * (double)fn : 0.0;
  const int jsize = 3 * J * kNeqN;
  if (use_p || use_m || use_n)
    for (int idx = tid; idx < jsize; idx += kNeqThreads) s.jac[0][idx] = jac[(size_t)b * jsize + idx];
  if (use_m || use_n)                                      // (frame b + 1 is in the sequence: t <= T - 2)
    for (int idx = tid; idx < jsize; idx += kNeqThreads) s.jac[1][idx] = jac[(size_t)(b + 1) * jsize + idx];
  if (use_n)                                               // (frame b + 2 is in the sequence: t <= T - 3)
    for (int idx = tid; idx < jsize; idx += kNeqThreads) s.jac[2][idx] = jac[(size_t)(b + 2) * jsize + idx];
  if (tid < 3 * 64) {                                      // decide: wave 0 prev, wave 1 mid, wave 2 next
    const int which = tid >> 6, j = tid & 63;
    if (j < J) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, term = 0.0;
      int act = 0;
      if (which == 0 ? live_p : which == 1 ? live_m : live_n) {
        const size_t mid = (size_t)(b - 1 + which) * J + j;            // the triple's centre frame
        const float4 cm = centres[mid - J], c0 = centres[mid], cp = centres[mid + J];
        a0 = ((double)cm.x + (double)cp.x) - 2.0 * (double)c0.x;
        a1 = ((double)cm.y + (double)cp.y) - 2.0 * (double)c0.y;
        a2 = ((double)cm.z + (double)cp.z) - 2.0 * (double)c0.z;
        const double n2 = (a0 * a0 + a1 * a1) + a2 * a2;
        if (n2 == n2) {                                    // (a NaN: no term, no row)
          act = n2 < cap2;                                 // exactly the cap is saturated
          term = act ? n2 : cap2;
        }
      }
      s.a[which][j][0] = a0;
      s.a[which][j][1] = a1;
      s.a[which][j][2] = a2;
      s.term[which][j] = term;
      s.act[which][j] = act;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int rows = 0;
    for (int j = 0; j < J; j++) rows += s.act[0][j];
    count[b] = rows;
  }
  // F: always written; +0 where the frame is not the first of a weighted triple.  E: written, or added to what it holds
  for (int idx = tid; idx < kNeqN * kNeqN; idx += kNeqThreads) {
    const int r = idx / kNeqN, c = idx - r * kNeqN;
    F[(size_t)b * kNeqN * kNeqN + idx] = use_n ? wn * neq_gram(s.act[2], s.jac[0], s.jac[2], r, c, J) : 0.0;
    double *out = E + (size_t)b * kNeqN * kNeqN + idx;
    if (use_m || use_n) {
      const double XM = use_m ? neq_gram(s.act[1], s.jac[0], s.jac[1], r, c, J) : 0.0;
      const double XN = use_n ? neq_gram(s.act[2], s.jac[0], s.jac[1], r, c, J) : 0.0;
      const double mine = (0.0 - (2.0 * wm) * XM) - (2.0 * wn) * XN;
      *out = add_E ? *out + mine : mine;
    } else if (!add_E) {
      *out = 0.0;
    }
  }
  if (add && !use_p && !use_m && !use_n) return;           // nothing with a weight: A, g and cost are not touched
  if (tid == kNeqThreads - 1) {                            // the prev triple's cost: the spheres' terms ascending
    double C = 0.0;
    if (use_p)
      for (int j = 0; j < J; j++) C += s.term[0][j];
    if (!add || use_p) neq_emit_cost(cost, b, wp * C, add);
  }
  for (int idx = tid; idx < kNeqTri + kNeqN; idx += kNeqThreads) {
    double P = 0.0, M = 0.0, N = 0.0;
    if (idx < kNeqTri) {
      const NeqEntry e = neq_entry(idx);
      if (use_p) P = neq_gram(s.act[0], s.jac[0], s.jac[0], e.a, e.c, J);
      if (use_m) M = neq_gram(s.act[1], s.jac[0], s.jac[0], e.a, e.c, J);
      if (use_n) N = neq_gram(s.act[2], s.jac[0], s.jac[0], e.a, e.c, J);
      neq_emit_A(A, b, e.a, e.c, (wp * P + (4.0 * wm) * M) + wn * N, add);
    } else {
      const int r = neq_g_entry(idx);
      if (use_p) P = neq_gram_g(s.act[0], s.jac[0], s.a[0], r, J);
      if (use_m) M = neq_gram_g(s.act[1], s.jac[0], s.a[1], r, J);
      if (use_n) N = neq_gram_g(s.act[2], s.jac[0], s.a[2], r, J);
      // the centre of a triple is pulled against its ends
      neq_emit_g(g, b, r, (wp * P - (2.0 * wm) * M) + wn * N, add);
    }
  }
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_sphere_accel_normal_workspace_bytes(int B, int T, int J) {
  if (B < 0 || T < 0 || J < 0) return -1;
  return 0;
}

extern "C" int shr_sphere_accel_normal(const float *keypoints, const float *jac, const float *triple_weight, float accel_weight,
                                       float acc_max, int B, int T, int J, int accumulate, int accumulate_E, double *A, double *g,
                                       double *E, double *F, double *cost, int32_t *count, void *workspace, void *stream) {
  if (B < 0 || T < 1 || J < 1 || !(acc_max >= 0.f) || (accumulate != 0 && accumulate != 1)) return SHR_EINVAL;
  if (accumulate_E != 0 && accumulate_E != 1) return SHR_EINVAL;
  if (!neq_weight_ok(accel_weight) || B % T != 0) return SHR_EINVAL;
  if (neq_too_large(B, 1, J)) return SHR_ETOOLARGE;
  if (B == 0) return SHR_OK;
  if (!keypoints || !jac || !A || !g || !E || !F || !cost || !count) return SHR_EINVAL;
  if (!neq_aligned(4, jac, triple_weight, count) || !neq_aligned(8, A, g, E, F, cost) || !neq_aligned(16, keypoints, workspace))
    return SHR_EINVAL;
  const double cap = (double)acc_max;
  hipLaunchKernelGGL(sphere_accel_kernel, dim3((unsigned)B), dim3(kNeqThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4 *>(keypoints), jac, triple_weight, (double)accel_weight, cap * cap, T, J,
                     accumulate, accumulate_E, accel_weight > 0.f ? 1 : 0, A, g, E, F, cost, count);
  return (int)hipGetLastError();
}
