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
//   add       thread t owns entries t, t + 256 of A's 351 lower entries and g's 26, as sphere_prior_kernel does, and entries
//             t, t + 256, t + 512 of E's 676: chains from 0 over the spheres with rows, ascending, a sphere's three axes
//             summed first.  The last thread runs prev's cost chain: the pair's cost is stored with frame t + 1.
//   A frame reads its neighbours' inputs and writes only its own outputs: every entry has one owner thread, and a
//   sequence does not see the other sequences of the batch.
//   LDS banks: in the add loops a wave's lanes read jac[3j + axis][a] and [c] of ONE sphere: 26 consecutive dwords, distinct
//   entries in distinct banks, equal entries one address; e, term and act are read at one address by all lanes.
#include "common.h"

namespace shr {

constexpr int kStnThreads = 256;
constexpr int kStnMaxJ = 64;
constexpr int kStnN = 26;                                  // pose parameters
constexpr int kStnTri = kStnN * (kStnN + 1) / 2;           // 351

struct StnLds {
  float jac[2][kStnMaxJ * 3 * kStnN];                      // frame b's, frame b + 1's
  double e[2][kStnMaxJ][3];                                // prev: c(b) - c(b - 1); next: c(b + 1) - c(b)
  double term[2][kStnMaxJ];                                // min(n2, cap2); 0 where the sphere has no term
  int act[2][kStnMaxJ];                                    // the sphere has rows
};

// mode 0: A, g, cost = the term's; 1: they are added to what the buffers hold (A's lower triangle is read and the sum
// written to both triangles); a frame none of whose pairs carries a weight is left alone
enum { kStnWrite = 0, kStnAdd = 1 };

__global__ void __launch_bounds__(kStnThreads)
sphere_temporal_kernel(const float4 *__restrict__ centres, const float *__restrict__ jac, const float *__restrict__ frame_weight,
                       double tw, double cap2, int T, int J, int mode, int used, double *__restrict__ A, double *__restrict__ g,
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
  const size_t jsize = (size_t)3 * J * kStnN;
  if (use_p || use_n)
    for (int idx = tid; idx < 3 * J * kStnN; idx += kStnThreads) s.jac[0][idx] = jac[(size_t)b * jsize + idx];
  if (use_n)
    for (int idx = tid; idx < 3 * J * kStnN; idx += kStnThreads) s.jac[1][idx] = jac[(size_t)(b + 1) * jsize + idx];
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
  for (int idx = tid; idx < kStnN * kStnN; idx += kStnThreads) {
    double out = 0.0;
    if (use_n) {
      const int r = idx / kStnN, c = idx - r * kStnN;
      double acc = 0.0;
      for (int j = 0; j < J; j++) {
        if (!s.act[1][j]) continue;
        const float *q0 = s.jac[0] + 3 * j * kStnN + r, *q1 = s.jac[1] + 3 * j * kStnN + c;
        acc += ((double)q0[0] * (double)q1[0] + (double)q0[kStnN] * (double)q1[kStnN]) +
               (double)q0[2 * kStnN] * (double)q1[2 * kStnN];
      }
      out = 0.0 - wn * acc;
    }
    E[(size_t)b * kStnN * kStnN + idx] = out;
  }
  if (mode == kStnAdd && !use_p && !use_n) return;         // nothing with a weight: A, g and cost are not touched
  if (tid == kStnThreads - 1) {                            // the prev pair's cost: the spheres' terms ascending
    double C = 0.0;
    if (use_p)
      for (int j = 0; j < J; j++) C += s.term[0][j];
    const double c = wp * C;
    if (mode == kStnAdd) {
      if (use_p) cost[b] = cost[b] + c;
    } else {
      cost[b] = c;
    }
  }
  for (int idx = tid; idx < kStnTri + kStnN; idx += kStnThreads) {
    double P = 0.0, N = 0.0;
    if (idx < kStnTri) {
      int a = 0;
      while ((a + 1) * (a + 2) / 2 <= idx) a++;
      const int c = idx - a * (a + 1) / 2;                 // a >= c
      for (int which = 0; which < 2; which++) {
        if (!(which == 0 ? use_p : use_n)) continue;
        double acc = 0.0;
        for (int j = 0; j < J; j++) {
          if (!s.act[which][j]) continue;                  // a sphere without rows adds nothing
          const float *q = s.jac[0] + 3 * j * kStnN;
          acc += ((double)q[a] * (double)q[c] + (double)q[kStnN + a] * (double)q[kStnN + c]) +
                 (double)q[2 * kStnN + a] * (double)q[2 * kStnN + c];
        }
        if (which == 0) P = acc; else N = acc;
      }
      const double mine = wp * P + wn * N;
      double *low = A + ((size_t)b * kStnN + a) * kStnN + c;
      const double v = mode == kStnAdd ? *low + mine : mine;
      *low = v;
      A[((size_t)b * kStnN + c) * kStnN + a] = v;
    } else {
      const int a = idx - kStnTri;
      for (int which = 0; which < 2; which++) {
        if (!(which == 0 ? use_p : use_n)) continue;
        double acc = 0.0;
        for (int j = 0; j < J; j++) {
          if (!s.act[which][j]) continue;
          const float *q = s.jac[0] + 3 * j * kStnN;
          const double *e = s.e[which][j];
          acc += ((double)q[a] * e[0] + (double)q[kStnN + a] * e[1]) + (double)q[2 * kStnN + a] * e[2];
        }
        if (which == 0) P = acc; else N = acc;
      }
      const double mine = wp * P + wn * (0.0 - N);         // the later frame of a pair is pulled back, the earlier one forward
      double *out = g + (size_t)b * kStnN + a;
      *out = mode == kStnAdd ? *out + mine : mine;
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
  const float finite = 3.40282346638528859812e38f;
  if (B < 0 || T < 1 || J < 1 || !(ts_max >= 0.f) || (accumulate != 0 && accumulate != 1)) return SHR_EINVAL;
  if (!(temporal_weight >= 0.f) || !(temporal_weight <= finite) || B % T != 0) return SHR_EINVAL;
  if (B > 65535 || J > kStnMaxJ) return SHR_ETOOLARGE;
  if (B == 0) return SHR_OK;
  if (!keypoints || !jac || !A || !g || !E || !cost || !count) return SHR_EINVAL;
  if ((((uintptr_t)jac | (uintptr_t)frame_weight | (uintptr_t)count) & 3u) != 0) return SHR_EINVAL;
  if ((((uintptr_t)A | (uintptr_t)g | (uintptr_t)E | (uintptr_t)cost) & 7u) != 0) return SHR_EINVAL;
  if ((((uintptr_t)keypoints | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  const double cap = (double)ts_max;
  hipLaunchKernelGGL(sphere_temporal_kernel, dim3((unsigned)B), dim3(kStnThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4 *>(keypoints), jac, frame_weight, (double)temporal_weight, cap * cap, T, J,
                     accumulate ? kStnAdd : kStnWrite, temporal_weight > 0.f ? 1 : 0, A, g, E, cost, count);
  return (int)hipGetLastError();
}
