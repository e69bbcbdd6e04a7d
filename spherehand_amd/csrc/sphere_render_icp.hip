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
//   scan      sphere_icp.hip's shape: one workgroup of 256 threads per (tile of 1024 pixels, view, sample), four rounds of
//             256 pixels, the crop's centres and radii in LDS (every lane reads the same sphere: a broadcast), the view's
//             rotation from a workgroup-uniform address.  Per round a thread runs its pixel's fp32 z-test over the J
//             spheres in the rasterizer's operation sequence -- q = (r r - dx dx) - dy dy, a root only where q > 0.01f --,
//             forms e = D - O', and for the owner alone recomputes s = sqrt(r^2 - dx^2 - dy^2) in fp64, takes the gradient
//             of the depth (-dx / s, -dy / s, 1) back to the model frame and leaves
//             [uu^T (6) | e u (3) | e^2 | 1 | 0 | min(|e|, max_resid)^2] in LDS, 13 doubles (an odd stride).  Each wave leaves
//             a ballot of the pixels that add to anything, and thread t continues the chains of entries t, t + 256, t + 512
//             of the tile's J x 12 moments over the set bits in ascending order; the first wave carries the cost as (hi, lo).
//   assemble  one workgroup per sample: thread t adds entries t, t + 256, .. of the sample's V * tiles records in order,
//             writes moments and count (this term's own, unweighted), then forms A's lower triangle and g from the moments
//             and the Jacobian in LDS, spheres ascending, and writes weight x them -- or adds weight x them to the buffers.
//
// The unit states its scan and its assembly itself: sphere_icp.hip is pinned byte for byte by its tests, and one assembly
// for both units is a later change.
#include "common.h"

namespace shr {

constexpr int kSrnThreads = 256;
constexpr int kSrnRounds = 4;
constexpr int kSrnTilePix = kSrnThreads * kSrnRounds;      // the unit of the summation order: part of the contract
constexpr int kSrnMaxJ = 64;
constexpr int kSrnMom = 12;                                // doubles per sphere: the layout of `moments`
constexpr int kSrnRec = 13;                                // a pixel's record in LDS: 12 moment terms and the cost's term
constexpr int kSrnChains = (kSrnMaxJ * kSrnMom + kSrnThreads - 1) / kSrnThreads;   // 3 moments per thread at J = 64
constexpr int kSrnN = 26;                                  // pose parameters
constexpr int kSrnTri = kSrnN * (kSrnN + 1) / 2;           // 351
constexpr int kSrnMaxSide = 2048;
constexpr int kSrnNone = kSrnMaxJ;                         // a chain beyond the record
constexpr float kSrnHitMin = 0.01f;                        // the rasterizer's hit rule: q > 0.01f

// doubles of a tile's record in the workspace: J x 12 moments, the cost as (hi, lo), 2 of padding (records stay 32-byte
// aligned)
__host__ __device__ inline int srn_stride(int J) { return kSrnMom * J + 4; }

struct SrnLds {
  float4 c[kSrnMaxJ];                                      // (centre in the view's frame, radius)
  double rec[kSrnThreads * kSrnRec];
  int owner[kSrnThreads];                                  // the sphere of the pixel's row, -1: no row
  unsigned long long live[kSrnThreads / kWave];            // per wave: the pixels that add to a chain (a row, or a cost term)
};

__global__ void __launch_bounds__(kSrnThreads, 4)
sphere_render_icp_scan_kernel(const float *__restrict__ observed, const float4 *__restrict__ centres,
                              const float *__restrict__ radii, const float *__restrict__ view, int J, int W, int H, float ax,
                              float bx, float ay, float by, float fg_max, float background, float max_resid,
                              double *__restrict__ part, float *__restrict__ depth, int *__restrict__ owner) {
  __shared__ SrnLds s;
  const int tid = threadIdx.x;
  const size_t crop = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
  const size_t npix = (size_t)H * W, base = (size_t)blockIdx.x * kSrnTilePix;
  if (tid < J) {
    const float4 c = centres[crop * J + tid];
    s.c[tid] = make_float4(c.x, c.y, c.z, radii[tid]);
  }
  const float *rot = view + crop * 16;                     // (uniform: scalar loads)
  float R[9];
#pragma unroll
  for (int q = 0; q < 9; q++) R[q] = rot[4 * (q / 3) + q % 3];
  // this thread's chains: moment idx = tid + 256 e of [J x 12]; the first wave also carries the cost, as (hi, lo)
  const int entries = kSrnMom * J;
  int cj[kSrnChains], cm[kSrnChains];
  double acc[kSrnChains], chi = 0.0, clo = 0.0;
#pragma unroll
  for (int e = 0; e < kSrnChains; e++) {
    const int idx = tid + kSrnThreads * e;
    acc[e] = 0.0;
    cj[e] = idx < entries ? idx / kSrnMom : kSrnNone;
    cm[e] = idx < entries ? idx % kSrnMom : 0;
  }
  const double cap = (double)max_resid;
  __syncthreads();
#pragma unroll 1
  for (int r = 0; r < kSrnRounds; r++) {
    const size_t i = base + (size_t)(r * kSrnThreads + tid);
    int row = -1;
    double c2 = 0.0;
    double *rec = s.rec + tid * kSrnRec;
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
    rec[kSrnRec - 1] = c2;
    s.owner[tid] = row;
    const unsigned long long mine = __ballot(row >= 0 || c2 != 0.0);   // (a NaN term is carried into the cost)
    if ((tid & (kWave - 1)) == 0) s.live[tid / kWave] = mine;
    __syncthreads();
    for (int w = 0; w < kSrnThreads / kWave; w++) {
      const unsigned long long m = s.live[w];
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m), hi = __builtin_amdgcn_readfirstlane((unsigned)(m >> 32));
      for (unsigned long long left = ((unsigned long long)hi << 32) | lo; left; left &= left - 1) {
        const int k = w * kWave + __builtin_ctzll(left);    // (ascending: the chains' order)
        const int o = s.owner[k];
        const double *rk = s.rec + k * kSrnRec;
        if (tid < kWave) {                                 // (hi, lo) += x: Knuth's two-sum, the error kept in lo
          const double x = rk[kSrnRec - 1], t = chi + x, bb = t - chi;
          clo += (chi - (t - bb)) + (x - bb);
          chi = t;
        }
#pragma unroll
        for (int e = 0; e < kSrnChains; e++)
          if (cj[e] == o) acc[e] += rk[cm[e]];
      }
    }
    __syncthreads();                                       // (the next round overwrites the records)
  }
  double *out = part + (crop * gridDim.x + blockIdx.x) * (size_t)srn_stride(J);
#pragma unroll
  for (int e = 0; e < kSrnChains; e++)
    if (cj[e] != kSrnNone) out[tid + kSrnThreads * e] = acc[e];
  if (tid == 0) { out[entries] = chi; out[entries + 1] = clo; }
}

struct SrnAsmLds {
  double mom[kSrnMaxJ * kSrnMom];
  float jac[kSrnMaxJ * 3 * kSrnN];
};

// mode 0: A, g, cost = weight x this term's; 1: they are added to what the buffers hold (A's lower triangle is read and
// the sum written to both triangles); 2: A, g and cost are left alone (weight == 0 on top of another term)
enum { kSrnWrite = 0, kSrnAdd = 1, kSrnKeep = 2 };

__global__ void __launch_bounds__(kSrnThreads)
sphere_render_icp_assemble_kernel(const double *__restrict__ part, const float *__restrict__ jac, int J, int records,
                                  double weight, int mode, double *__restrict__ A, double *__restrict__ g,
                                  double *__restrict__ cost, int *__restrict__ count, double *__restrict__ moments) {
  __shared__ SrnAsmLds s;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int nmom = kSrnMom * J, stride = srn_stride(J);
  const double *in = part + (size_t)b * records * stride;
  for (int idx = tid; idx < nmom; idx += kSrnThreads) {
    double acc = 0.0;
#pragma unroll 4
    for (int t = 0; t < records; t++) acc += in[(size_t)t * stride + idx];
    s.mom[idx] = acc;
    if (moments) moments[(size_t)b * nmom + idx] = acc;
  }
  if (tid == kSrnThreads - 1 && mode != kSrnKeep) {        // the records' (hi, lo) costs: two-sum of the hi, lo collects
    double hi = 0.0, lo = 0.0;
    for (int t = 0; t < records; t++) {
      const double x = in[(size_t)t * stride + nmom], t2 = hi + x, bb = t2 - hi;
      lo += ((hi - (t2 - bb)) + (x - bb)) + in[(size_t)t * stride + nmom + 1];
      hi = t2;
    }
    const double c = weight * (hi + lo);
    cost[b] = mode == kSrnAdd ? cost[b] + c : c;
  }
  for (int idx = tid; idx < 3 * J * kSrnN; idx += kSrnThreads) s.jac[idx] = jac[(size_t)b * 3 * J * kSrnN + idx];
  __syncthreads();
  if (tid == 0) {
    double rows = 0.0;                                     // (integers below 2^53: exact)
    for (int j = 0; j < J; j++) rows += s.mom[j * kSrnMom + 10];
    count[b] = (int)rows;
  }
  if (mode == kSrnKeep) return;
  for (int idx = tid; idx < kSrnTri + kSrnN; idx += kSrnThreads) {
    double acc = 0.0;
    if (idx < kSrnTri) {
      int a = 0;
      while ((a + 1) * (a + 2) / 2 <= idx) a++;
      const int c = idx - a * (a + 1) / 2;                 // a >= c
      for (int j = 0; j < J; j++) {
        const double *m = s.mom + j * kSrnMom;
        if (m[10] == 0.0) continue;                        // a sphere without a row adds nothing
        const float *q = s.jac + 3 * j * kSrnN;
        const double c0 = (double)q[c], c1 = (double)q[kSrnN + c], c2 = (double)q[2 * kSrnN + c];
        const double t0 = (m[0] * c0 + m[1] * c1) + m[2] * c2;
        const double t1 = (m[1] * c0 + m[3] * c1) + m[4] * c2;
        const double t2 = (m[2] * c0 + m[4] * c1) + m[5] * c2;
        acc += ((double)q[a] * t0 + (double)q[kSrnN + a] * t1) + (double)q[2 * kSrnN + a] * t2;
      }
      double *lower = A + ((size_t)b * kSrnN + a) * kSrnN + c;
      const double v = mode == kSrnAdd ? *lower + weight * acc : weight * acc;
      *lower = v;
      A[((size_t)b * kSrnN + c) * kSrnN + a] = v;
    } else {
      const int a = idx - kSrnTri;
      for (int j = 0; j < J; j++) {
        const double *m = s.mom + j * kSrnMom;
        if (m[10] == 0.0) continue;
        const float *q = s.jac + 3 * j * kSrnN;
        acc += ((double)q[a] * m[6] + (double)q[kSrnN + a] * m[7]) + (double)q[2 * kSrnN + a] * m[8];
      }
      const double v = weight * -acc;
      g[(size_t)b * kSrnN + a] = mode == kSrnAdd ? g[(size_t)b * kSrnN + a] + v : v;
    }
  }
}

static inline long long srn_tiles(int W, int H) { return ((long long)W * H + kSrnTilePix - 1) / kSrnTilePix; }

}  // namespace shr

using namespace shr;

static int srn_check(int B, int V, int J, int W, int H, float background, float max_resid, float weight, int accumulate) {
  if (!(max_resid >= 0.f) || B < 0 || V < 1 || J < 1 || H < 1 || W < 1) return SHR_EINVAL;
  if (!(weight >= 0.f) || !(weight <= 3.40282346638528859812e38f) || !(fabsf(background) <= 3.40282346638528859812e38f) ||
      (accumulate != 0 && accumulate != 1))
    return SHR_EINVAL;
  if (B > 65535 || (long long)B * V > 65535 || J > kSrnMaxJ || H > kSrnMaxSide || W > kSrnMaxSide) return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" long long shr_sphere_render_normal_workspace_bytes(int B, int V, int J, int W, int H) {
  if (B < 0 || V < 0 || J < 0 || W < 0 || H < 0) return -1;
  return (long long)B * V * srn_tiles(W, H) * srn_stride(J) * 8;
}

extern "C" int shr_sphere_render_normal(const float *observed, const float *view_centres, const float *radii, const float *view,
                                        const float *jac, int B, int V, int J, int W, int H, float ax, float bx, float ay,
                                        float by, float fg_max, float background, float max_resid, float weight, int accumulate,
                                        double *A, double *g, double *cost, int32_t *count, double *moments, float *depth,
                                        int32_t *owner, void *workspace, void *stream) {
  if (int rc = srn_check(B, V, J, W, H, background, max_resid, weight, accumulate)) return rc;
  if (B == 0) return SHR_OK;
  if (!observed || !view_centres || !radii || !view || !jac || !A || !g || !cost || !count || !workspace) return SHR_EINVAL;
  if ((((uintptr_t)observed | (uintptr_t)radii | (uintptr_t)view | (uintptr_t)jac | (uintptr_t)count | (uintptr_t)depth |
        (uintptr_t)owner) & 3u) != 0)
    return SHR_EINVAL;
  if ((((uintptr_t)A | (uintptr_t)g | (uintptr_t)cost | (uintptr_t)moments) & 7u) != 0) return SHR_EINVAL;
  if ((((uintptr_t)view_centres | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (int)srn_tiles(W, H);
  const int mode = !accumulate ? kSrnWrite : (weight == 0.f ? kSrnKeep : kSrnAdd);
  double *part = reinterpret_cast<double *>(workspace);
  hipLaunchKernelGGL(sphere_render_icp_scan_kernel, dim3((unsigned)tiles, (unsigned)V, (unsigned)B), dim3(kSrnThreads), 0, s,
                     observed, reinterpret_cast<const float4 *>(view_centres), radii, view, J, W, H, ax, bx, ay, by, fg_max,
                     background, max_resid, part, depth, owner);
  hipLaunchKernelGGL(sphere_render_icp_assemble_kernel, dim3((unsigned)B), dim3(kSrnThreads), 0, s, part, jac, J, V * tiles,
                     (double)weight, mode, A, g, cost, count, moments);
  return (int)hipGetLastError();
}
