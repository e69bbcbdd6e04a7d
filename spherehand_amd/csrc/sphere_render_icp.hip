// sphere_render_icp.hip -- the model-to-data half of the sphere model's Gauss-Newton fit (shr_sphere_render_normal): the
// spheres are rendered the way the rasterizer renders them, the render is compared with the observed depth, and every
// model pixel leaves one row, summed per sphere into the moments of sphere_icp.hip's record; A and g are then formed from
// the moments and the centres' Jacobian, scaled by `weight` and, on request, added to what a preceding
// shr_sphere_icp_normal left.
//
// Inverts (reference file:line): HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by the
// key-point skinning and the render of HandBallPrimitiveRender (mesh/render.py:26-53, :65-89), against the observation of
// the fit's first term, MSELoss(render, observed) (mesh/multiview_utility.py:96-129).  The reference takes first-order
// steps on that term; it has no counterpart of the normal equations.
//
//   scan      sphere_icp_scan.h's pieces (the crop's spheres in LDS, the chains of the tile's J x 12 moments, the walk over
//             the round's live pixels with the cost as (hi, lo), the record's write-out) around this term's per-pixel
//             record: a thread runs its pixel's fp32 z-test over the J spheres in the rasterizer's operation sequence --
//             q = (r r - dx dx) - dy dy, a root only where q > 0.01f --, forms e = D - O', and for the owner alone recomputes
//             s = sqrt(r^2 - dx^2 - dy^2) in fp64, takes the gradient of the depth (-dx / s, -dy / s, 1) back to the model
//             frame and leaves [uu^T (6) | e u (3) | e^2 | 1 | 0 | min(|e|, max_resid)^2] in LDS, 13 doubles.
//   assemble  sphere_icp_scan.h's three pieces: one workgroup per sample adds the sample's V * tiles records in order and
//             writes moments and count (this term's own, unweighted); then A's lower triangle and g from the moments and
//             the Jacobian in LDS by normal_eq.h's chains, spheres ascending, and weight x them written -- or added to
//             the buffers.
#include "sphere_icp_scan.h"

namespace shr {

constexpr int kSrnMom = 12;                                // doubles per sphere: the layout of `moments`
constexpr float kSrnHitMin = 0.01f;                        // the rasterizer's hit rule: q > 0.01f

__global__ void __launch_bounds__(kNeqThreads, 4)
sphere_render_icp_scan_kernel(const float *__restrict__ observed, const float4 *__restrict__ centres,
                              const float *__restrict__ radii, const float *__restrict__ view, int J, int W, int H, float ax,
                              float bx, float ay, float by, float fg_max, float background, float max_resid,
                              double *__restrict__ part, float *__restrict__ depth, int *__restrict__ owner) {
  __shared__ SicpLds<kSrnMom> s;
  const int tid = threadIdx.x;
  const size_t crop = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
  const size_t npix = (size_t)H * W, base = (size_t)blockIdx.x * kSicpTilePix;
  float R[9];
  sicp_stage_crop(s, centres, radii, view, crop, J, R);
  SicpChains<kSrnMom> ch;
  sicp_chains_begin(ch, J);
  const double cap = (double)max_resid;
  __syncthreads();
#pragma unroll 1
  for (int r = 0; r < kSicpRounds; r++) {
    const size_t i = base + (size_t)(r * kNeqThreads + tid);
    int row = -1;
    double c2 = 0.0;
    double *rec = s.rec + tid * (kSrnMom + 1);
    if (i < npix) {
      const int pi = (int)(i / (size_t)W), pj = (int)(i - (size_t)pi * W);
      const float px = ax * (float)pj + bx, py = ay * (float)pi + by;
      // the rasterizer's z-test: the nearest hit, the first index among equal depths; a hit exactly AT the background is
      // the owner only while every lower sphere hit behind it (torch.min's first index over maps that hold the
      // background where a sphere misses)
      float best = background;
      int own = -1;
      bool behind = true;
      for (int j = 0; j < J; j++) {
        const float4 c = s.c[j];
        const float dx = px - c.x, dy = py - c.y;
        const float q = (c.w * c.w - dx * dx) - dy * dy;
        if (q > kSrnHitMin) {
          const float d = c.z - sqrtf(q);
          if (d < best) { best = d; own = j; }             // (a NaN is never taken)
          else if (own < 0 && behind && d == best) own = j;
          behind = behind && d > background;
        } else {
          behind = false;
        }
      }
      if (depth) depth[crop * npix + i] = best;
      if (owner) owner[crop * npix + i] = own;
      const float z = observed[crop * npix + i];
      if (z == z) {                                        // a NaN observation: no term, no row
        const float o = z < fg_max ? z : background;
        const double e = (double)best - (double)o, ae = fabs(e);
        const double cl = ae < cap ? ae : cap;             // the truncated quadratic
        c2 = cl * cl;
        if (own >= 0 && ae < cap) {
          const float4 c = s.c[own];
          const double dx = (double)px - (double)c.x, dy = (double)py - (double)c.y, rr = (double)c.w;
          const double sq = sqrt((rr * rr - dx * dx) - dy * dy);
          if (sq > 0.0 && sq <= 1.79769313486231570815e308) {   // finite and not zero: the gradient is defined
            const double v0 = -dx / sq, v1 = -dy / sq;     // grad_c D = (v0, v1, 1) in the view's frame
            // u = -R^T grad_c D: column j of R against the gradient, summed in index order
            const double u0 = -(((double)R[0] * v0 + (double)R[3] * v1) + (double)R[6]);
            const double u1 = -(((double)R[1] * v0 + (double)R[4] * v1) + (double)R[7]);
            const double u2 = -(((double)R[2] * v0 + (double)R[5] * v1) + (double)R[8]);
            rec[0] = u0 * u0; rec[1] = u0 * u1; rec[2] = u0 * u2; rec[3] = u1 * u1; rec[4] = u1 * u2; rec[5] = u2 * u2;
            rec[6] = e * u0; rec[7] = e * u1; rec[8] = e * u2; rec[9] = e * e;
            rec[10] = 1.0; rec[11] = 0.0;
            row = own;
          }
        }
      }
    }
    sicp_walk(s, ch, row, c2);
  }
  sicp_chains_store(ch, part, crop, J);
}

// mode (normal_eq.h): A, g, cost = weight x this term's, written or added; kept where weight == 0 on top of another term
__global__ void __launch_bounds__(kNeqThreads)
sphere_render_icp_assemble_kernel(const double *__restrict__ part, const float *__restrict__ jac, int J, int records,
                                  double weight, int mode, double *__restrict__ A, double *__restrict__ g,
                                  double *__restrict__ cost, int *__restrict__ count, double *__restrict__ moments) {
  __shared__ SicpAsmLds<kSrnMom> s;
  const int tid = threadIdx.x, b = blockIdx.x;
  const bool add = mode == kNeqAdd;
  sicp_sum_records(s, part, J, records, moments);
  if (tid == kNeqThreads - 1 && mode != kNeqKeep) neq_emit_cost(cost, b, weight * sicp_cost_total<kSrnMom>(part, J, records), add);
  sicp_stage_jacobian(s, jac, J, count);
  if (mode == kNeqKeep) return;
  for (int idx = tid; idx < kNeqTri + kNeqN; idx += kNeqThreads) {
    if (idx < kNeqTri) {
      const NeqEntry e = neq_entry(idx);
      neq_emit_A(A, b, e.a, e.c, weight * neq_moments_A<kSrnMom>(s.mom, s.jac, J, e.a, e.c), add);
    } else {
      const int a = neq_g_entry(idx);
      neq_emit_g(g, b, a, weight * -neq_moments_g<kSrnMom>(s.mom, s.jac, J, a), add);
    }
  }
}

}  // namespace shr

using namespace shr;

static int srn_check(int B, int V, int J, int W, int H, float background, float max_resid, float weight, int accumulate) {
  if (!(max_resid >= 0.f) || B < 0 || V < 1 || J < 1 || H < 1 || W < 1) return SHR_EINVAL;
  if (!neq_weight_ok(weight) || !(fabsf(background) <= 3.40282346638528859812e38f) || (accumulate != 0 && accumulate != 1))
    return SHR_EINVAL;
  if (neq_too_large(B, V, J) || H > kSicpMaxSide || W > kSicpMaxSide) return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" long long shr_sphere_render_normal_workspace_bytes(int B, int V, int J, int W, int H) {
  if (B < 0 || V < 0 || J < 0 || W < 0 || H < 0) return -1;
  return (long long)B * V * sicp_tiles(W, H) * sicp_stride<kSrnMom>(J) * 8;
}

extern "C" int shr_sphere_render_normal(const float *observed, const float *view_centres, const float *radii, const float *view,
                                        const float *jac, int B, int V, int J, int W, int H, float ax, float bx, float ay,
                                        float by, float fg_max, float background, float max_resid, float weight, int accumulate,
                                        double *A, double *g, double *cost, int32_t *count, double *moments, float *depth,
                                        int32_t *owner, void *workspace, void *stream) {
  if (int rc = srn_check(B, V, J, W, H, background, max_resid, weight, accumulate)) return rc;
  if (B == 0) return SHR_OK;
  if (!observed || !view_centres || !radii || !view || !jac || !A || !g || !cost || !count || !workspace) return SHR_EINVAL;
  if (!neq_aligned(4, observed, radii, view, jac, count, depth, owner) || !neq_aligned(8, A, g, cost, moments) ||
      !neq_aligned(16, view_centres, workspace))
    return SHR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (int)sicp_tiles(W, H);
  const int mode = !accumulate ? kNeqWrite : (weight == 0.f ? kNeqKeep : kNeqAdd);
  double *part = reinterpret_cast<double *>(workspace);
  hipLaunchKernelGGL(sphere_render_icp_scan_kernel, dim3((unsigned)tiles, (unsigned)V, (unsigned)B), dim3(kNeqThreads), 0, s,
                     observed, reinterpret_cast<const float4 *>(view_centres), radii, view, J, W, H, ax, bx, ay, by, fg_max,
                     background, max_resid, part, depth, owner);
  hipLaunchKernelGGL(sphere_render_icp_assemble_kernel, dim3((unsigned)B), dim3(kNeqThreads), 0, s, part, jac, J, V * tiles,
                     (double)weight, mode, A, g, cost, count, moments);
  return (int)hipGetLastError();
}
