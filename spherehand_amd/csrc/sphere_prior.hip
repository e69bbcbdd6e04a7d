// sphere_prior.hip -- the two terms the sphere model's Gauss-Newton fit carries beside its image terms
// (shr_sphere_prior_normal): the predicted keypoints as soft anchors of the sphere centres, and hinge penalties at the
// joint limits.  Every (view, sphere) pair with a keypoint leaves three rows, one per axis of the view's frame, summed per
// sphere into the moments of sphere_icp.hip's record; A and g are formed from the moments and the centres' Jacobian, the
// limit term adds to the diagonal, and the result is written or, on request, added to what the image terms left.
//
// Inverts (reference file:line): HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by the
// key-point skinning of HandBallPrimitiveRender (mesh/render.py:65-88), against the key-points predicted per view (they
// ARE the sphere centres) and the support of the pose distribution of dataset/joint_angle.py:7-236.  The reference has
// no counterpart of the normal equations.
//
//   one workgroup of 256 threads (four wave64) per sample; the sample's 3J x 26 fp32 Jacobian and its J x 12 fp64 moments
//   live in LDS beside the 26 hinge values (26 320 bytes at the unit's J = 64).
//   phase 1   thread t owns the chains of moments t, t + 256, t + 512 of [J x 12]: for its (sphere, moment) it walks the
//             views in ascending order, forms e = k - c in fp64, decides the pair (a NaN keypoint, a confidence of 0 or NaN:
//             no term; n2 < kp_max^2: rows) and adds the pair's subtotal, the three axes' terms in ascending order.
//             Slot 10 counts the pairs with rows; slot 11, the record's spare, carries the sphere's cost chain sum_v w t
//             in LDS and is written as 0.  The moments are written contiguously (thread t to double t: no bank
//             conflict) and read as broadcasts, so the record needs no odd stride here.
//   phase 2   thread t owns entries t, t + 256 of A's 351 lower entries and g's 26 and sums normal_eq.h's chains of the
//             moments, spheres ascending.
//   phase 3   the owner of a diagonal entry (and of g_i) adds the limit term of parameter i; then weight and accumulate.
//             The last thread runs the cost: the spheres' chains ascending, then the limits.
#include "normal_eq.h"

namespace shr {

constexpr int kSpnMom = 12;                                // doubles per sphere: the layout of `moments`

struct SpnLds {
  double mom[kNeqMaxJ * kSpnMom];
  float jac[kNeqMaxJ * 3 * kNeqN];
  double h[kNeqN];                                         // the limit term's h_i (0: no row)
};

// h_i of the limit term: fp64 from the fp32 values; a comparison with a NaN never fires, a value ON a bound gives 0
__device__ inline double spn_hinge(float p, float lo, float hi) {
  return p > hi ? (double)p - (double)hi : (p < lo ? (double)p - (double)lo : 0.0);
}

__global__ void __launch_bounds__(kNeqThreads)
sphere_prior_kernel(const float4 *__restrict__ centres, const float *__restrict__ view, const float *__restrict__ jac,
                    const float *__restrict__ params, const float *__restrict__ keypoints,
                    const float *__restrict__ confidence, const float *__restrict__ lower, const float *__restrict__ upper,
                    double kw, double cap2, double lw, int V, int J, int mode, int use,
                    double *__restrict__ A, double *__restrict__ g, double *__restrict__ cost, int *__restrict__ count,
                    double *__restrict__ moments) {
  __shared__ SpnLds s;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int nmom = kSpnMom * J;
  const bool use_kp = use & 1, use_lim = use & 2, add = mode == kNeqAdd;
  if (tid < kNeqN) s.h[tid] = lower ? spn_hinge(params[b * kNeqN + tid], lower[tid], upper[tid]) : 0.0;
  if (use_kp)
    for (int idx = tid; idx < 3 * J * kNeqN; idx += kNeqThreads) s.jac[idx] = jac[(size_t)b * 3 * J * kNeqN + idx];
  // phase 1: the chains of (sphere, moment) over the views
  for (int idx = tid; idx < nmom; idx += kNeqThreads) {
    const int j = idx / kSpnMom, m = idx - j * kSpnMom;
    double acc = 0.0;
    if (keypoints) {
      for (int v = 0; v < V; v++) {
        const size_t pair = ((size_t)b * V + v) * J + j;
        const float *k = keypoints + pair * 3;
        const float k0 = k[0], k1 = k[1], k2 = k[2];
        const float wf = confidence ? confidence[pair] : 1.f;
        if (!(k0 == k0 && k1 == k1 && k2 == k2) || !(wf == wf) || wf == 0.f) continue;   // no term, no row
        const float4 c = centres[pair];
        const double e0 = (double)k0 - (double)c.x, e1 = (double)k1 - (double)c.y, e2 = (double)k2 - (double)c.z;
        const double n2 = (e0 * e0 + e1 * e1) + e2 * e2;
        const bool rowed = n2 < cap2;                      // (a NaN is saturated)
        const double w = (double)wf;
        if (m == 11) { acc += w * (rowed ? n2 : cap2); continue; }     // the truncated quadratic
        if (!rowed) continue;
        if (m == 10) { acc += 1.0; continue; }
        const float *rot = view + ((size_t)b * V + v) * 16;
        double sub = 0.0;                                  // the pair's subtotal: two identical views give exactly 2 x
#pragma unroll
        for (int a = 0; a < 3; a++) {                      // u = row a of R as given
          const double u0 = (double)rot[4 * a], u1 = (double)rot[4 * a + 1], u2 = (double)rot[4 * a + 2];
          const double ea = a == 0 ? e0 : (a == 1 ? e1 : e2);
          // S_pq += (w u_p) u_q; h_p += (w e_a) u_p; sum e^2 += (w e_a) e_a: every term is one x * y
          const double up = m < 3 ? u0 : (m < 5 ? u1 : u2);
          const double uq = (m == 0 || m == 6) ? u0 : ((m == 1 || m == 3 || m == 7) ? u1 : u2);
          const double x = m < 6 ? w * up : w * ea;
          const double y = m < 9 ? uq : ea;
          sub += x * y;
        }
        acc += sub;
      }
    }
    s.mom[idx] = acc;
    if (moments) moments[(size_t)b * nmom + idx] = m == 11 ? 0.0 : acc;
  }
  __syncthreads();
  if (tid == 0) {
    double rows = 0.0;                                     // (integers below 2^53: exact)
    for (int j = 0; j < J; j++) rows += s.mom[j * kSpnMom + 10];
    count[2 * b] = (int)rows;
  }
  if (tid == 1) {
    int rows = 0;
    for (int i = 0; i < kNeqN; i++) rows += s.h[i] != 0.0;
    count[2 * b + 1] = rows;
  }
  if (mode == kNeqKeep) return;
  if (tid == kNeqThreads - 1) {                            // the cost: the spheres' chains ascending, then the limits
    double kp_part = 0.0, lim_part = 0.0;
    if (use_kp) {
      double K = 0.0;
      for (int j = 0; j < J; j++) K += s.mom[j * kSpnMom + 11];
      kp_part = kw * K;
    }
    if (use_lim) {
      double L = 0.0;
      for (int i = 0; i < kNeqN; i++) L += s.h[i] * s.h[i];
      lim_part = lw * L;
    }
    neq_emit_cost(cost, b, kp_part + lim_part, add);
  }
  // phases 2 and 3: A's lower triangle and g from the moments and the Jacobian, the limit term on the diagonal
  for (int idx = tid; idx < kNeqTri + kNeqN; idx += kNeqThreads) {
    double acc = 0.0, lim = 0.0;
    if (idx < kNeqTri) {
      const NeqEntry e = neq_entry(idx);
      if (use_kp) acc = neq_moments_A<kSpnMom>(s.mom, s.jac, J, e.a, e.c);
      if (use_lim && e.a == e.c && s.h[e.a] != 0.0) lim = lw;
      neq_emit_A(A, b, e.a, e.c, (use_kp ? kw * acc : 0.0) + lim, add);
    } else {
      const int a = neq_g_entry(idx);
      if (use_kp) acc = neq_moments_g<kSpnMom>(s.mom, s.jac, J, a);
      if (use_lim && s.h[a] != 0.0) lim = lw * s.h[a];
      neq_emit_g(g, b, a, (use_kp ? kw * (0.0 - acc) : 0.0) + lim, add);
    }
  }
}

}  // namespace shr

using namespace shr;

extern "C" long long shr_sphere_prior_normal_workspace_bytes(int B, int V, int J) {
  if (B < 0 || V < 0 || J < 0) return -1;
  return 0;
}

extern "C" int shr_sphere_prior_normal(const float *view_centres, const float *view, const float *jac, const float *params,
                                       const float *keypoints, const float *confidence, float kp_weight, float kp_max,
                                       const float *lower, const float *upper, float limit_weight, int B, int V, int J,
                                       int accumulate, double *A, double *g, double *cost, int32_t *count, double *moments,
                                       void *workspace, void *stream) {
  if (B < 0 || V < 1 || J < 1 || !(kp_max >= 0.f) || (accumulate != 0 && accumulate != 1)) return SHR_EINVAL;
  if (!neq_weight_ok(kp_weight) || !neq_weight_ok(limit_weight)) return SHR_EINVAL;
  if ((lower == nullptr) != (upper == nullptr) || (confidence && !keypoints)) return SHR_EINVAL;
  if (neq_too_large(B, V, J)) return SHR_ETOOLARGE;
  if (B == 0) return SHR_OK;
  if (!view_centres || !view || !jac || !params || !A || !g || !cost || !count) return SHR_EINVAL;
  if (!neq_aligned(4, view, jac, params, keypoints, confidence, lower, upper, count) || !neq_aligned(8, A, g, cost, moments) ||
      !neq_aligned(16, view_centres, workspace))
    return SHR_EINVAL;
  const int use_kp = keypoints && kp_weight > 0.f, use_lim = lower && limit_weight > 0.f;
  const int mode = !accumulate ? kNeqWrite : ((use_kp || use_lim) ? kNeqAdd : kNeqKeep);
  const double cap = (double)kp_max;
  hipLaunchKernelGGL(sphere_prior_kernel, dim3((unsigned)B), dim3(kNeqThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4 *>(view_centres), view, jac, params, keypoints, confidence, lower, upper,
                     (double)kp_weight, cap * cap, (double)limit_weight, V, J, mode, use_kp | (use_lim << 1), A, g, cost, count,
                     moments);
  return (int)hipGetLastError();
}
