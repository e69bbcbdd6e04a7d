// sphere_temporal.hip -- the term of the sphere model's Gauss-Newton fit that ties consecutive frames of a sequence
// (shr_sphere_temporal_normal): per pair of frames (t, t + 1) and per sphere j the difference e = c_j(t + 1) - c_j(t) of the
// model-frame centres leaves three rows, +Jc_j(t + 1) in frame t + 1's columns and -Jc_j(t) in frame t's.  A row couples
// TWO frames, so beside the diagonal blocks A and the gradient g of every frame the term has an off-diagonal block E per
// frame: the normal equations of a sequence are block-tridiagonal (lm_seq.hip solves them).
//
// Inverts (reference file:line): HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by the
// key-point skinning of HandBallPrimitiveRender (mesh/render.py:65-88), under TemporalSmoothnessLoss
// (network/util_modules.py:360-381; ClampedL2lLoss, :349-358; weight 1.0 in MultiTaskLoss,
// create_network_and_criterion.py:242-245).  The reference detaches the previous frame; the rows here are symmetric.  The
// reference has no counterpart of the normal equations.
//
//   one workgroup of 256 threads (four wave64) PER FRAME b, t = b mod T its place in its sequence.  The frame belongs to up
//   to two pairs: `prev` (t - 1, t) and `next` (t, t + 1).  Its own 3J x 26 fp32 Jacobian and, for E, frame b + 1's live in LDS
//   (2 x 19 968 bytes at the unit's J = 64) beside both pairs' e, cost terms and flags: 44 544 bytes.
//   decide    thread j < J decides (prev, j), thread 64 + j decides (next, j): e in fp64 from the fp32 centres, n2, the
//             cost term min(n2, cap2) and whether the sphere has rows (n2 < cap2; a NaN n2: no term at all).
//   add       thread t owns entries t, t + 256 of A's 351 lower entries and g's 26 (normal_eq.h's entry map), and entries
//             t, t + 256, t + 512 of E's 676: normal_eq.h's chains from 0 over the spheres with rows, ascending, a sphere's
//             three axes summed first.  The last thread runs prev's cost chain: the pair's cost is stored with frame t + 1.
//   A frame reads its neighbours' inputs and writes only its own outputs: every entry has one owner thread, and a
//   sequence does not see the other sequences of the batch.
//   LDS banks: in the add loops a wave's lanes read jac[3j + axis][a] and [c] of ONE sphere: 26 consecutive dwords, distinct
//   entries in distinct banks, equal entries one address; e, term and act are read at one address by all lanes.
#include "normal_eq.h"

namespace shr {

struct StnLds {
  float jac[2][kNeqMaxJ * 3 * kNeqN];                      // frame b's, frame b + 1's
  double e[2][kNeqMaxJ][3];                                // prev: c(b) - c(b - 1); next: c(b + 1) - c(b)
  double term[2][kNeqMaxJ];                                // min(n2, cap2); 0 where the sphere has no term
  int act[2][kNeqMaxJ];                                    // the sphere has rows
};

// add: A, g and cost are added to what the buffers hold, and a frame none of whose pairs carries a weight is left alone

__global__ void __launch_bounds__(kNeqThreads)
sphere_temporal_kernel(const float4 *__restrict__ centres, const float *__restrict__ jac, const float *__restrict__ frame_weight,
                       double tw, double cap2, int T, int J, int add, int used, double *__restrict__ A, double *__restrict__ g,
                       double *__restrict__ E, double *__restrict__ cost, int *__restrict__ count) {
  __shared__ StnLds s;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int t = b % T;
  const bool has_prev = t > 0, has_next = t < T - 1;
  const float fwp = !has_prev ? 0.f : frame_weight ? frame_weight[b - 1] : 1.f;
  const float fwn = !has_next ? 0.f : frame_weight ? frame_weight[b] : 1.f;
  const bool live_p = fwp > 0.f, live_n = fwn > 0.f;       // (a NaN weight: no term)
  const bool use_p = used && live_p, use_n = used && live_n;
  const double wp = use_p ? tw * (double)fwp : 0.0, wn = use_n ? tw * (double)fwn : 0.0;
  const size_t jsize = (size_t)3 * J * kNeqN;
  if (use_p || use_n)
    for (int idx = tid; idx < 3 * J * kNeqN; idx += kNeqThreads) s.jac[0][idx] = jac[(size_t)b * jsize + idx];
  if (use_n)
    for (int idx = tid; idx < 3 * J * kNeqN; idx += kNeqThreads) s.jac[1][idx] = jac[(size_t)(b + 1) * jsize + idx];
  if (tid < 2 * 64) {                                      // decide: wave 0 the prev pair, wave 1 the next pair
    const int which = tid >> 6, j = tid & 63;
    if (j < J) {
      double e0 = 0.0, e1 = 0.0, e2 = 0.0, term = 0.0;
      int act = 0;
      if (which == 0 ? live_p : live_n) {
        const size_t late = (size_t)(which == 0 ? b : b + 1) * J + j;
        const float4 c1 = centres[late], c0 = centres[late - J];
        e0 = (double)c1.x - (double)c0.x;
        e1 = (double)c1.y - (double)c0.y;
        e2 = (double)c1.z - (double)c0.z;
        const double n2 = (e0 * e0 + e1 * e1) + e2 * e2;
        if (n2 == n2) {                                    // (a NaN: no term, no row)
          act = n2 < cap2;                                 // exactly the cap is saturated
          term = act ? n2 : cap2;
        }
      }
      s.e[which][j][0] = e0;
      s.e[which][j][1] = e1;
      s.e[which][j][2] = e2;
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
  // E: always written; +0 where the frame has no weighted next pair
  for (int idx = tid; idx < kNeqN * kNeqN; idx += kNeqThreads) {
    const int r = idx / kNeqN, c = idx - r * kNeqN;
    E[(size_t)b * kNeqN * kNeqN + idx] = use_n ? 0.0 - wn * neq_gram(s.act[1], s.jac[0], s.jac[1], r, c, J) : 0.0;
  }
  if (add && !use_p && !use_n) return;         // nothing with a weight: A, g and cost are not touched
  if (tid == kNeqThreads - 1) {                            // the prev pair's cost: the spheres' terms ascending
    double C = 0.0;
    if (use_p)
      for (int j = 0; j < J; j++) C += s.term[0][j];
    if (!add || use_p) neq_emit_cost(cost, b, wp * C, add);
  }
  for (int idx = tid; idx < kNeqTri + kNeqN; idx += kNeqThreads) {
    double P = 0.0, N = 0.0;
    if (idx < kNeqTri) {
      const NeqEntry e = neq_entry(idx);
      if (use_p) P = neq_gram(s.act[0], s.jac[0], s.jac[0], e.a, e.c, J);
      if (use_n) N = neq_gram(s.act[1], s.jac[0], s.jac[0], e.a, e.c, J);
      neq_emit_A(A, b, e.a, e.c, wp * P + wn * N, add);
    } else {
      const int a = neq_g_entry(idx);
      if (use_p) P = neq_gram_g(s.act[0], s.jac[0], s.e[0], a, J);
      if (use_n) N = neq_gram_g(s.act[1], s.jac[0], s.e[1], a, J);
      // the later frame of a pair is pulled back, the earlier one forward
      neq_emit_g(g, b, a, wp * P + wn * (0.0 - N), add);
    }
  }
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_sphere_temporal_normal_workspace_bytes(int B, int T, int J) {
  if (B < 0 || T < 0 || J < 0) return -1;
  return 0;
}

extern "C" int shr_sphere_temporal_normal(const float *keypoints, const float *jac, const float *frame_weight,
                                          float temporal_weight, float ts_max, int B, int T, int J, int accumulate, double *A,
                                          double *g, double *E, double *cost, int32_t *count, void *workspace, void *stream) {
  if (B < 0 || T < 1 || J < 1 || !(ts_max >= 0.f) || (accumulate != 0 && accumulate != 1)) return SHR_EINVAL;
  if (!neq_weight_ok(temporal_weight) || B % T != 0) return SHR_EINVAL;
  if (neq_too_large(B, 1, J)) return SHR_ETOOLARGE;
  if (B == 0) return SHR_OK;
  if (!keypoints || !jac || !A || !g || !E || !cost || !count) return SHR_EINVAL;
  if (!neq_aligned(4, jac, frame_weight, count) || !neq_aligned(8, A, g, E, cost) || !neq_aligned(16, keypoints, workspace))
    return SHR_EINVAL;
  const double cap = (double)ts_max;
  hipLaunchKernelGGL(sphere_temporal_kernel, dim3((unsigned)B), dim3(kNeqThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4 *>(keypoints), jac, frame_weight, (double)temporal_weight, cap * cap, T, J,
                     accumulate, temporal_weight > 0.f ? 1 : 0, A, g, E, cost, count);
  return (int)hipGetLastError();
}
