// sphere_icp_scan.h -- the scan and the assembly of the sphere model's per-pixel normal equations, stated once for
// shr_sphere_icp_normal (sphere_icp.hip: kMom = 12 moments per sphere), shr_sphere_icp_radii_normal
// (sphere_icp_radii.hip: kMom = 16, the twelve and sum u (3), sum d for the radius columns) and shr_sphere_render_normal
// (sphere_render_icp.hip: kMom = 12, the render's rows): the tiles of 1024 pixels, the record, the chains and the summation
// order.  For the two data terms the per-pixel record is the same code too (sicp_scan_body): the fp32 owner search, the
// fp64 residual d = n - r and direction u = R^T u_v and the row rule, so the twelve moments, A, g, cost, count, dist and
// owner are the same bits.
//
//   scan      one workgroup of 256 threads per (tile of 1024 pixels, view, sample), four rounds of 256 pixels.
//     sicp_stage_crop     the crop's centres and radii to LDS (every lane reads the same sphere: a broadcast); the view's
//                         rotation is read from a workgroup-uniform address.
//     (the chains)        thread t takes the chains of entries t, t + 256, .. of the tile's J x kMom moments, from 0.
//     (the record)        per round a thread leaves its pixel's [uu^T (6) | d u (3) | d^2 | 1 | 0 (| u (3) | d)] and the
//                         cost's term in LDS, kMom + 1 doubles (an odd stride: the threads' records start in different
//                         banks).  The data term finds the pixel's owner in fp32 (41 candidates where the mesh search meets
//                         3 382 faces: search and row fit into one kernel) and recomputes residual and direction in fp64.
//     (the walk)          continues the chains over the round's pixels in ascending order: a row costs 10 accumulations
//                         instead of a 26-column row's 378, and nothing is summed across threads -- every entry has one
//                         owner thread, which is what makes the order fixed.  Only the pixels with a row or a cost term are
//                         walked: each wave leaves a ballot of them in LDS and the walk takes the set bits in order
//                         (workgroup-uniform; walking all 256 records paid an LDS round trip per pixel to find the seven in
//                         eight that add nothing: 541 us instead of 381 us at 256 crops @128^2, and 277 us instead of 34 us
//                         on an empty crop).  The cost, a sum of a thousand positive terms whose plain chain
//                         would be several ulps off, is carried by the first wave as (hi, lo) with the two-sum's error
//                         collected in lo: the same order, within an ulp of the exact sum.
//     (the write-out)     the tile's record to the workspace.
//     The chains, the walk and the write-out stand as the pieces sicp_chains_begin, sicp_walk and sicp_chains_store, which
//     the render term's scan composes around its record, AND inline in sicp_scan_body: composed of the pieces, the data
//     term's scan is the same operations under another register allocation and measured 0.4 % slower,
//     so it keeps the text that compiles to the instructions it had.  A change to one of the two is a change to both.
//   assemble  one workgroup per sample, three pieces and a loop.
//     sicp_sum_records    thread t adds entries t, t + 256, .. of the sample's V * tiles records in order (tiles ascending
//                         in a view, views ascending), leaves the moments in LDS and writes `moments`.
//     sicp_cost_total     the last thread's (hi, lo) sum of the records' costs.
//     sicp_stage_jacobian the Jacobian to LDS, the barrier, the row count.
//     then A's lower triangle and g from the moments and the Jacobian in LDS, spheres ascending, all 26 columns of every
//     sphere, by normal_eq.h's chains and emission: sicp_assemble_body for the data terms, the render term with its weight.
#pragma once
#include "normal_eq.h"

namespace shr {

constexpr int kSicpRounds = 4;
constexpr int kSicpTilePix = kNeqThreads * kSicpRounds;    // the unit of the summation order: part of the contract
constexpr int kSicpMaxSide = 2048;
constexpr int kSicpNone = kNeqMaxJ;                        // a chain beyond the record

// doubles of a tile's record in the workspace: J x kMom moments, the cost as (hi, lo), 2 of padding (records stay 32-byte
// aligned)
template <int kMom>
__host__ __device__ inline int sicp_stride(int J) { return kMom * J + 4; }

template <int kMom>
struct SicpLds {
  float4 c[kNeqMaxJ];                                      // (centre in the view's frame, radius)
  double rec[kNeqThreads * (kMom + 1)];                    // a pixel's record: kMom moment terms and the cost's term
  int owner[kNeqThreads];                                  // the sphere of the pixel's row, -1: no row
  unsigned long long live[kNeqThreads / kWave];            // per wave: the pixels that add to a chain (a row, or a cost term)
};

// this thread's chains: moment idx = tid + 256 e of [J x kMom]; the first wave also carries the cost, as (hi, lo)
template <int kMom>
struct SicpChains {
  static constexpr int kCount = (kNeqMaxJ * kMom + kNeqThreads - 1) / kNeqThreads;   // moments per thread at J = 64
  int cj[kCount], cm[kCount];
  double acc[kCount], chi, clo;
};

// The crop's spheres to s.c (the caller's barrier stands before their first read) and its view's rotation to R.  radii: the
// J radii of this crop's model.
template <int kMom>
__device__ __forceinline__ void sicp_stage_crop(SicpLds<kMom> &s, const float4 *__restrict__ centres,
                                                const float *__restrict__ radii, const float *__restrict__ view, size_t crop,
                                                int J, float (&R)[9]) {
  const int tid = threadIdx.x;
  if (tid < J) {
    const float4 c = centres[crop * J + tid];
    s.c[tid] = make_float4(c.x, c.y, c.z, radii[tid]);
  }
  const float *rot = view + crop * 16;                     // (uniform: scalar loads)
#pragma unroll
  for (int q = 0; q < 9; q++) R[q] = rot[4 * (q / 3) + q % 3];
}

template <int kMom>
__device__ __forceinline__ void sicp_chains_begin(SicpChains<kMom> &ch, int J) {
  const int tid = threadIdx.x, entries = kMom * J;
  ch.chi = 0.0;
  ch.clo = 0.0;
#pragma unroll
  for (int e = 0; e < SicpChains<kMom>::kCount; e++) {
    const int idx = tid + kNeqThreads * e;
    ch.acc[e] = 0.0;
    ch.cj[e] = idx < entries ? idx / kMom : kSicpNone;
    ch.cm[e] = idx < entries ? idx % kMom : 0;
  }
}

// One round: this thread's pixel has left its kMom moment terms in its record (where row >= 0: the sphere of its row);
// c2 is its cost term.  The round's live pixels are walked into the chains and the (hi, lo) cost, ascending.
template <int kMom>
__device__ __forceinline__ void sicp_walk(SicpLds<kMom> &s, SicpChains<kMom> &ch, int row, double c2) {
  constexpr int kRec = kMom + 1;
  const int tid = threadIdx.x;
  s.rec[tid * kRec + kRec - 1] = c2;
  s.owner[tid] = row;
  const unsigned long long mine = __ballot(row >= 0 || c2 != 0.0);   // (a NaN term is carried into the cost)
  if ((tid & (kWave - 1)) == 0) s.live[tid / kWave] = mine;
  __syncthreads();
  for (int w = 0; w < kNeqThreads / kWave; w++) {
    const unsigned long long m = s.live[w];
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m), hi = __builtin_amdgcn_readfirstlane((unsigned)(m >> 32));
    // (One pixel per turn.  Reading four pixels' records ahead of their sums, every thread its chains' terms whether it
    // takes them or not, measured 433 us where this takes 381 us at 256 crops @128^2: the conditional reads are few.)
    for (unsigned long long left = ((unsigned long long)hi << 32) | lo; left; left &= left - 1) {
      const int k = w * kWave + __builtin_ctzll(left);      // (ascending: the chains' order)
      const int o = s.owner[k];
      const double *rk = s.rec + k * kRec;
      if (tid < kWave) {                                   // (hi, lo) += x: Knuth's two-sum, the error kept in lo
        const double x = rk[kRec - 1], t = ch.chi + x, bb = t - ch.chi;
        ch.clo += (ch.chi - (t - bb)) + (x - bb);
        ch.chi = t;
      }
#pragma unroll
      for (int e = 0; e < SicpChains<kMom>::kCount; e++)
        if (ch.cj[e] == o) ch.acc[e] += rk[ch.cm[e]];
    }
  }
  __syncthreads();                                         // (the next round overwrites the records)
}

template <int kMom>
__device__ __forceinline__ void sicp_chains_store(const SicpChains<kMom> &ch, double *__restrict__ part, size_t crop, int J) {
  const int tid = threadIdx.x, entries = kMom * J;
  double *out = part + (crop * gridDim.x + blockIdx.x) * (size_t)sicp_stride<kMom>(J);
#pragma unroll
  for (int e = 0; e < SicpChains<kMom>::kCount; e++)
    if (ch.cj[e] != kSicpNone) out[tid + kNeqThreads * e] = ch.acc[e];
  if (tid == 0) { out[entries] = ch.chi; out[entries + 1] = ch.clo; }
}

// The data term's scan.  kMom: doubles per sphere, the layout of `moments` -- 12, or 16 with sum u and sum d behind the
// twelve.  radii: the J radii of this crop's model.
template <int kMom>
__device__ __forceinline__ void sicp_scan_body(SicpLds<kMom> &s, const float *__restrict__ observed,
                                               const float4 *__restrict__ centres, const float *__restrict__ radii,
                                               const float *__restrict__ view, int J, int W, int H, float ax, float bx, float ay,
                                               float by, float fg_max, float max_dist, double *__restrict__ part,
                                               float *__restrict__ dist, int *__restrict__ owner) {
  constexpr int kRec = kMom + 1;
  constexpr int kChains = (kNeqMaxJ * kMom + kNeqThreads - 1) / kNeqThreads;   // moments per thread at J = 64
  const int tid = threadIdx.x;
  const size_t crop = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
  const size_t npix = (size_t)H * W, base = (size_t)blockIdx.x * kSicpTilePix;
  float R[9];
  sicp_stage_crop(s, centres, radii, view, crop, J, R);
  // this thread's chains: moment idx = tid + 256 e of [J x kMom]; the first wave also carries the cost, as (hi, lo)
  const int entries = kMom * J;
  int cj[kChains], cm[kChains];
  double acc[kChains], chi = 0.0, clo = 0.0;
#pragma unroll
  for (int e = 0; e < kChains; e++) {
    const int idx = tid + kNeqThreads * e;
    acc[e] = 0.0;
    cj[e] = idx < entries ? idx / kMom : kSicpNone;
    cm[e] = idx < entries ? idx % kMom : 0;
  }
  __syncthreads();
#pragma unroll 1
  for (int r = 0; r < kSicpRounds; r++) {
    const size_t i = base + (size_t)(r * kNeqThreads + tid);
    int own = -1, row = -1;
    float d32 = 0.f;
    double *rec = s.rec + tid * kRec;
    if (i < npix) {
      const float z = observed[crop * npix + i];
      if (z < fg_max) {                                    // a data point (a NaN is none)
        const int pi = (int)(i / (size_t)W), pj = (int)(i - (size_t)pi * W);
        const float px = ax * (float)pj + bx, py = ay * (float)pi + by;
        float best = __builtin_inff();
        for (int j = 0; j < J; j++) {
          const float4 c = s.c[j];
          const float ex = px - c.x, ey = py - c.y, ez = z - c.z;
          const float n = sqrtf((ex * ex + ey * ey) + ez * ez);
          const float sj = fabsf(n - c.w);
          if (sj < best) { best = sj; own = j; }           // (a NaN is never taken, the first of equal ones stays)
        }
        if (own >= 0) {
          d32 = fminf(best, max_dist);
          if (best < max_dist) {
            const float4 c = s.c[own];
            const double ex = (double)px - (double)c.x, ey = (double)py - (double)c.y, ez = (double)z - (double)c.z;
            const double n = sqrt((ex * ex + ey * ey) + ez * ez);
            if (n > 0.0 && n <= 1.79769313486231570815e308) {   // finite and not zero: the direction is defined
              const double d = n - (double)c.w;
              const double v0 = ex / n, v1 = ey / n, v2 = ez / n;
              // u = R^T u_v: column j of R against u_v, summed in index order
              const double u0 = ((double)R[0] * v0 + (double)R[3] * v1) + (double)R[6] * v2;
              const double u1 = ((double)R[1] * v0 + (double)R[4] * v1) + (double)R[7] * v2;
              const double u2 = ((double)R[2] * v0 + (double)R[5] * v1) + (double)R[8] * v2;
              rec[0] = u0 * u0; rec[1] = u0 * u1; rec[2] = u0 * u2; rec[3] = u1 * u1; rec[4] = u1 * u2; rec[5] = u2 * u2;
              rec[6] = d * u0; rec[7] = d * u1; rec[8] = d * u2; rec[9] = d * d;
              rec[10] = 1.0; rec[11] = 0.0;
              if constexpr (kMom > 12) {                   // the radius column of the row is -1: sum u and sum d carry it
                rec[12] = u0; rec[13] = u1; rec[14] = u2; rec[15] = d;
              }
              row = own;
            }
          }
        }
      }
      if (dist) dist[crop * npix + i] = d32;
      if (owner) owner[crop * npix + i] = own;
    }
    const double c2 = (double)d32 * (double)d32;
    rec[kRec - 1] = c2;
    s.owner[tid] = row;
    const unsigned long long mine = __ballot(row >= 0 || c2 != 0.0);   // (a NaN dist^2 is carried into the cost)
    if ((tid & (kWave - 1)) == 0) s.live[tid / kWave] = mine;
    __syncthreads();
    for (int w = 0; w < kNeqThreads / kWave; w++) {
      const unsigned long long m = s.live[w];
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m), hi = __builtin_amdgcn_readfirstlane((unsigned)(m >> 32));
      // (One pixel per turn.  Reading four pixels' records ahead of their sums, every thread its chains' terms whether it
      // takes them or not, measured 433 us where this takes 381 us at 256 crops @128^2: the conditional reads are few.)
      for (unsigned long long left = ((unsigned long long)hi << 32) | lo; left; left &= left - 1) {
        const int k = w * kWave + __builtin_ctzll(left);    // (ascending: the chains' order)
        const int o = s.owner[k];
        const double *rk = s.rec + k * kRec;
        if (tid < kWave) {                                 // (hi, lo) += x: Knuth's two-sum, the error kept in lo
          const double x = rk[kRec - 1], t = chi + x, bb = t - chi;
          clo += (chi - (t - bb)) + (x - bb);
          chi = t;
        }
#pragma unroll
        for (int e = 0; e < kChains; e++)
          if (cj[e] == o) acc[e] += rk[cm[e]];
      }
    }
    __syncthreads();                                       // (the next round overwrites the records)
  }
  double *out = part + (crop * gridDim.x + blockIdx.x) * (size_t)sicp_stride<kMom>(J);
#pragma unroll
  for (int e = 0; e < kChains; e++)
    if (cj[e] != kSicpNone) out[tid + kNeqThreads * e] = acc[e];
  if (tid == 0) { out[entries] = chi; out[entries + 1] = clo; }
}

template <int kMom>
struct SicpAsmLds {
  double mom[kNeqMaxJ * kMom];
  float jac[kNeqMaxJ * 3 * kNeqN];
};

// The assembly's first part, three pieces in this order.  (1) The sample's records to moments in LDS (and to `moments`).
template <int kMom>
__device__ __forceinline__ void sicp_sum_records(SicpAsmLds<kMom> &s, const double *__restrict__ part, int J, int records,
                                                 double *__restrict__ moments) {
  const int tid = threadIdx.x, b = blockIdx.x;
  const int nmom = kMom * J, stride = sicp_stride<kMom>(J);
  const double *in = part + (size_t)b * records * stride;
  for (int idx = tid; idx < nmom; idx += kNeqThreads) {
    double acc = 0.0;
#pragma unroll 4
    for (int t = 0; t < records; t++) acc += in[(size_t)t * stride + idx];
    s.mom[idx] = acc;
    if (moments) moments[(size_t)b * nmom + idx] = acc;
  }
}

// (2) One thread: the records' (hi, lo) costs, the two-sum of the hi; lo collects the errors and the records' lo.
template <int kMom>
__device__ __forceinline__ double sicp_cost_total(const double *__restrict__ part, int J, int records) {
  const int nmom = kMom * J, stride = sicp_stride<kMom>(J);
  const double *in = part + (size_t)blockIdx.x * records * stride;
  double hi = 0.0, lo = 0.0;
  for (int t = 0; t < records; t++) {
    const double x = in[(size_t)t * stride + nmom], t2 = hi + x, bb = t2 - hi;
    lo += ((hi - (t2 - bb)) + (x - bb)) + in[(size_t)t * stride + nmom + 1];
    hi = t2;
  }
  return hi + lo;
}

// (3) The sample's Jacobian to LDS, the barrier behind which every thread may read it and the moments, and the row count.
template <int kMom>
__device__ __forceinline__ void sicp_stage_jacobian(SicpAsmLds<kMom> &s, const float *__restrict__ jac, int J,
                                                    int *__restrict__ count) {
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int idx = tid; idx < 3 * J * kNeqN; idx += kNeqThreads) s.jac[idx] = jac[(size_t)b * 3 * J * kNeqN + idx];
  __syncthreads();
  if (tid == 0) {
    double rows = 0.0;                                     // (integers below 2^53: exact)
    for (int j = 0; j < J; j++) rows += s.mom[j * kMom + 10];
    count[b] = (int)rows;
  }
}

// The data term's assembly.  void_all (kMom = 16's radius guard; false for kMom = 12): A = g = 0 and cost = +inf are
// written instead of the sums.
template <int kMom>
__device__ __forceinline__ void sicp_assemble_body(SicpAsmLds<kMom> &s, const double *__restrict__ part,
                                                   const float *__restrict__ jac, int J, int records, bool void_all,
                                                   double *__restrict__ A, double *__restrict__ g, double *__restrict__ cost,
                                                   int *__restrict__ count, double *__restrict__ moments) {
  const int tid = threadIdx.x, b = blockIdx.x;
  sicp_sum_records(s, part, J, records, moments);
  if (tid == kNeqThreads - 1) neq_emit_cost(cost, b, void_all ? __builtin_inf() : sicp_cost_total<kMom>(part, J, records), false);
  sicp_stage_jacobian(s, jac, J, count);
  for (int idx = tid; idx < kNeqTri + kNeqN; idx += kNeqThreads) {
    if (idx < kNeqTri) {
      const NeqEntry e = neq_entry(idx);
      const double acc = neq_moments_A<kMom>(s.mom, s.jac, J, e.a, e.c);
      neq_emit_A(A, b, e.a, e.c, void_all ? 0.0 : acc, false);
    } else {
      const int a = neq_g_entry(idx);
      const double acc = neq_moments_g<kMom>(s.mom, s.jac, J, a);
      neq_emit_g(g, b, a, void_all ? 0.0 : -acc, false);
    }
  }
}

static inline long long sicp_tiles(int W, int H) { return ((long long)W * H + kSicpTilePix - 1) / kSicpTilePix; }

static inline int sicp_check(int B, int V, int J, int W, int H, float max_dist) {
  if (!(max_dist >= 0.f) || B < 0 || V < 1 || J < 1 || H < 1 || W < 1) return SHR_EINVAL;
  if (neq_too_large(B, V, J) || H > kSicpMaxSide || W > kSicpMaxSide) return SHR_ETOOLARGE;
  return SHR_OK;
}

}  // namespace shr
