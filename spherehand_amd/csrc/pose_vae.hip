// pose_vae.hip -- the pose-VAE prior of the sphere model's Gauss-Newton fit (shr_pose_vae_normal): the residual
// r = c - 100 recon(c / 100) over the 41 sphere centres c (mm, model frame) and its exact Jacobian
// J_r = (I - D) J_c, D the 123 x 123 input Jacobian of the frozen network, which is never formed: the value and the 26 pose
// tangents pass through the MLP together as ONE 27-column matrix (forward mode), six small GEMMs per frame on
// v_mfma_f32_32x32x2_f32 with the GroupNorm and ReLU tangents between them.
//
// Inverts (reference file:line): PoseVae (network/pose_vae.py:11-99), the 123-256-256-32-256-256-123 MLP with
// GroupNorm(16, 256) behind --prior, on model-frame keypoints / 100 (network/pose_vae.py:169); z = mu (no
// reparameterisation draw, no logvar head).  The reference uses it as a first-order training term only
// (network/create_network_and_criterion.py:164, 238-243) and has no counterpart of the normal equations.
//
//   one workgroup of 256 threads (four wave64) per frame.  LDS (36 992 bytes): act[256][32] fp32, the layer's input M with
//   its column on the fast axis (column 0 the value, 1 .. 26 the tangents, 27 .. 31 zero), REUSED for the layer's output
//   (the accumulators wait in registers behind a barrier) and at the end for the fp64 rows [123][27]; lat[32][32] fp32,
//   mu and its tangents, the decoder's input and the latent rows; 32 mask words.
//   product   D[32 x 32] += W[32 out x 2 k] M[2 k x 32 columns] per MFMA: the A operand is the packed weight (lane l: output
//             l & 31 of the tile, k = k0 + (l >> 5)), one 8-byte load per lane and two k steps from L2; the B operand is
//             act[k0 + (l >> 5)][l & 31], 64 consecutive floats: no bank conflict.  Every output element is ONE fmaf chain
//             over k = 0 .. K - 1 ascending that starts from the bias (column 0) or from +0 (the other columns).
//             A wave owns two of a 256-wide layer's eight tiles (tiles 2 wave, 2 wave + 1) and one of the last layer's four.
//             The 256 -> 32 layer is ONE tile: wave v takes k = 64 v .. 64 v + 63 (wave 0's chain starts from the bias), the
//             four partial tiles go through act, and the sum is ((P0 + P1) + P2) + P3.
//   epilogue  in the C/D map (column l & 31; register r is row (r & 3) + 8 (r >> 2) + 4 (l >> 5)) GroupNorm group s of a
//             tile is registers 8 s .. 8 s + 7 of both lane halves: a group sum is eight adds and one exchange with
//             lane ^ 32.  The value column's entries reach the tangent columns by a read of lane l & 32.
//   rows      r_i = 100 ((double)x_i - (double)recon_i), J_r[i][c] = (double)jac[i][c] - (double)recon'[i][c]: the tangent
//             columns carry jac itself (the layers are linear in the tangent, so the 100 of x = c / 100 and the 100 of r
//             cancel) and the identity part is exact.
//   add       thread t owns entries t, t + 256 of A's 351 lower entries and g's 26 (normal_eq.h's neq_owned): fp64
//             chains over rows 0 .. 122, then the 32 latent rows; the last thread runs the cost chains.
#include "normal_eq.h"

namespace shr {

constexpr int kPvJ = 41;
constexpr int kPvIn = 3 * kPvJ;                            // 123
constexpr int kPvCols = kNeqN + 1;                          // 27: the value and the tangents
constexpr int kPvHidden = 256;
constexpr int kPvLatent = 32;
constexpr float kPvEps = 1e-5f;

// the blob: per linear layer the packed weight [K / 4][OUT][2][2] (element ((q OUT + o) 2 + h) 2 + s is W[o][4 q + 2 s + h],
// zero where o or k is padding), the bias [OUT], and behind a GroupNorm layer gamma [256] and beta [256]
constexpr int kPvK1 = 124, kPvOut6 = 128;
constexpr int kPvW1 = 0;
constexpr int kPvB1 = kPvW1 + kPvK1 * kPvHidden;
constexpr int kPvW2 = kPvB1 + 3 * kPvHidden;
constexpr int kPvB2 = kPvW2 + kPvHidden * kPvHidden;
constexpr int kPvW3 = kPvB2 + 3 * kPvHidden;
constexpr int kPvB3 = kPvW3 + kPvHidden * kPvLatent;
constexpr int kPvW4 = kPvB3 + kPvLatent;
constexpr int kPvB4 = kPvW4 + kPvLatent * kPvHidden;
constexpr int kPvW5 = kPvB4 + 3 * kPvHidden;
constexpr int kPvB5 = kPvW5 + kPvHidden * kPvHidden;
constexpr int kPvW6 = kPvB5 + 3 * kPvHidden;
constexpr int kPvB6 = kPvW6 + kPvHidden * kPvOut6;
constexpr int kPvBlob = kPvB6 + kPvOut6;                   // 215 200 floats

typedef float pv_acc __attribute__((ext_vector_type(16)));

struct PvLds {
  union {
    float act[kPvHidden * 32];
    double rows[kPvIn * kPvCols];
  };
  float lat[kPvLatent * 32];
  uint32_t mask[32];
};

__device__ __forceinline__ int pv_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// NT tiles (tile0 .. tile0 + NT - 1 of an OUT-wide layer) over k = 4 q0 .. 4 q1 - 1; !biased: every chain starts at +0
template <int OUT, int NT>
__device__ __forceinline__ void pv_gemm(const float *__restrict__ W, const float *__restrict__ bias, bool biased, const float *in,
                                        int tile0, int q0, int q1, int lane, pv_acc (&acc)[NT]) {
  const int col = lane & 31, half = lane >> 5;
  const bool first = biased && col == 0;
#pragma unroll
  for (int i = 0; i < NT; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float bv = bias[32 * (tile0 + i) + pv_row(r, half)];
      acc[i][r] = first ? bv : 0.f;
    }
  const float2 *w = reinterpret_cast<const float2 *>(W) + (size_t)(32 * tile0 + col) * 2 + half;
#pragma unroll 4
  for (int q = q0; q < q1; q++) {
    float2 a[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) a[i] = w[((size_t)q * OUT + 32 * i) * 2];
    const float b0 = in[(4 * q + half) * 32 + col], b1 = in[(4 * q + 2 + half) * 32 + col];
#pragma unroll
    for (int i = 0; i < NT; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b0, acc[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NT; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b1, acc[i], 0, 0, 0);
  }
}

// GroupNorm(16 groups of 16 channels, biased variance) and ReLU of one tile in place, value and tangents; -> the tile's 32
// ReLU decisions of the value column (bit = the tile's row), valid in every lane
__device__ __forceinline__ uint32_t pv_gn_relu(pv_acc &acc, const float *__restrict__ gamma, const float *__restrict__ beta,
                                               int tile, int lane) {
  const int col = lane & 31, half = lane >> 5;
  uint32_t bits = 0;
#pragma unroll
  for (int s = 0; s < 2; s++) {
    float hv[8];                                           // the value column's entries of this lane's rows
#pragma unroll
    for (int e = 0; e < 8; e++) hv[e] = __shfl(acc[8 * s + e], lane & 32, 64);
    float sum = hv[0];
#pragma unroll
    for (int e = 1; e < 8; e++) sum += hv[e];
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * 0.0625f;
    float d[8];
#pragma unroll
    for (int e = 0; e < 8; e++) d[e] = hv[e] - mean;
    float sq = d[0] * d[0];
#pragma unroll
    for (int e = 1; e < 8; e++) sq += d[e] * d[e];
    sq += __shfl_xor(sq, 32, 64);
    const float rs = 1.0f / sqrtf(sq * 0.0625f + kPvEps);
    float t1 = 0.f, t2 = 0.f;                              // the tangent's two group sums
#pragma unroll
    for (int e = 0; e < 8; e++) {
      d[e] = d[e] * rs;                                    // h^
      const float t = acc[8 * s + e];
      t1 = e == 0 ? t : t1 + t;
      t2 = e == 0 ? d[e] * t : t2 + d[e] * t;
    }
    t1 += __shfl_xor(t1, 32, 64);
    t2 += __shfl_xor(t2, 32, 64);
    const float m1 = t1 * 0.0625f, m2 = t2 * 0.0625f;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int ch = 32 * tile + pv_row(8 * s + e, half);
      const float ga = gamma[ch], be = beta[ch];
      const float y = d[e] * ga + be;
      const bool on = y > 0.f;
      const float yt = (ga * rs) * ((acc[8 * s + e] - m1) - d[e] * m2);
      acc[8 * s + e] = on ? (col == 0 ? y : yt) : 0.f;
      bits |= on ? 1u << pv_row(8 * s + e, half) : 0u;
    }
  }
  return bits | __shfl_xor(bits, 32, 64);
}

template <int NT>
__device__ __forceinline__ void pv_store(float *out, const pv_acc (&acc)[NT], int tile0, int lane) {
  const int col = lane & 31, half = lane >> 5;
#pragma unroll
  for (int i = 0; i < NT; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) out[(32 * (tile0 + i) + pv_row(r, half)) * 32 + col] = acc[i][r];
}

// one 256-wide layer with GroupNorm and ReLU: in (K rows) -> s.act; `layer` 0 .. 3 numbers the mask words
template <int K>
__device__ __forceinline__ void pv_hidden(PvLds &s, const float *__restrict__ blob, int w_at, int b_at, const float *in, int layer,
                                          int wave, int lane) {
  pv_acc acc[2];
  pv_gemm<kPvHidden, 2>(blob + w_at, blob + b_at, true, in, 2 * wave, 0, K / 4, lane, acc);
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const uint32_t bits = pv_gn_relu(acc[i], blob + b_at + kPvHidden, blob + b_at + 2 * kPvHidden, 2 * wave + i, lane);
    if (lane == 0) s.mask[8 * layer + 2 * wave + i] = bits;
  }
  __syncthreads();                                         // every wave has read the layer's input
  pv_store<2>(s.act, acc, 2 * wave, lane);
  __syncthreads();
}

__global__ void __launch_bounds__(kNeqThreads)
pose_vae_kernel(const float4 *__restrict__ kp, const float *__restrict__ jac, const float *__restrict__ blob, double w, double lw,
                int mode, double *__restrict__ A, double *__restrict__ g, double *__restrict__ cost,
                double *__restrict__ residual, double *__restrict__ latent, uint32_t *__restrict__ relu_mask) {
  __shared__ PvLds s;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const float *jb = jac + (size_t)b * kPvIn * kNeqN;
  // M0 = [x | jac], x = c / 100 (one IEEE division); row 123 and columns 27 .. 31 are +0
  for (int idx = tid; idx < kPvK1 * 32; idx += kNeqThreads) {
    const int i = idx >> 5, c = idx & 31;
    float v = 0.f;
    if (i < kPvIn) {
      if (c == 0) {
        const float4 p = kp[(size_t)b * kPvJ + i / 3];
        const int a = i - 3 * (i / 3);
        v = (a == 0 ? p.x : (a == 1 ? p.y : p.z)) / 100.0f;
      } else if (c < kPvCols) {
        v = jb[i * kNeqN + c - 1];
      }
    }
    s.act[idx] = v;
  }
  __syncthreads();
  pv_hidden<kPvK1>(s, blob, kPvW1, kPvB1, s.act, 0, wave, lane);
  pv_hidden<kPvHidden>(s, blob, kPvW2, kPvB2, s.act, 1, wave, lane);
  {                                                        // mu: one tile, K split over the waves
    pv_acc part[1];
    pv_gemm<kPvLatent, 1>(blob + kPvW3, blob + kPvB3, wave == 0, s.act, 0, 16 * wave, 16 * wave + 16, lane, part);
    __syncthreads();
    pv_store<1>(s.act + wave * 1024, part, 0, lane);
    __syncthreads();
    for (int idx = tid; idx < 1024; idx += kNeqThreads)
      s.lat[idx] = ((s.act[idx] + s.act[1024 + idx]) + s.act[2048 + idx]) + s.act[3072 + idx];
    __syncthreads();
  }
  pv_hidden<kPvLatent>(s, blob, kPvW4, kPvB4, s.lat, 2, wave, lane);
  pv_hidden<kPvHidden>(s, blob, kPvW5, kPvB5, s.act, 3, wave, lane);
  {                                                        // recon: tile `wave` of four, and the rows in fp64
    pv_acc acc[1];
    pv_gemm<kPvOut6, 1>(blob + kPvW6, blob + kPvB6, true, s.act, wave, 0, kPvHidden / 4, lane, acc);
    __syncthreads();
    const int col = lane & 31, half = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int i = 32 * wave + pv_row(r, half);
      if (i < kPvIn && col < kPvCols) {
        double v;
        if (col == 0) {
          const float4 p = kp[(size_t)b * kPvJ + i / 3];
          const int a = i - 3 * (i / 3);
          const float x = (a == 0 ? p.x : (a == 1 ? p.y : p.z)) / 100.0f;
          v = 100.0 * ((double)x - (double)acc[0][r]);
        } else {
          v = (double)jb[i * kNeqN + col - 1] - (double)acc[0][r];
        }
        s.rows[i * kPvCols + col] = v;
      }
    }
    __syncthreads();
  }
  if (residual)
    for (int i = tid; i < kPvIn; i += kNeqThreads) residual[(size_t)b * kPvIn + i] = s.rows[i * kPvCols];
  if (latent && tid < kPvLatent) latent[(size_t)b * kPvLatent + tid] = (double)s.lat[tid * 32];
  if (relu_mask && tid < 32) relu_mask[(size_t)b * 32 + tid] = s.mask[tid];
  if (mode == kNeqKeep) return;
  const NeqOwned own = neq_owned(tid);
  const int a0 = own.a0, c0 = own.c0, a1 = own.a1, c1 = own.c1;
  const bool add = mode == kNeqAdd;
  const bool with_latent = lw > 0.0;
  // the second entry's two columns of a row: A's (1 + a1, 1 + c1), g's (0, 1 + a1); a thread without one sums what it drops
  const int p1 = c1 >= 0 ? 1 + c1 : 0, q1 = 1 + a1;
  double acc0 = 0.0, acc1 = 0.0;
  for (int i = 0; i < kPvIn; i++) {
    const double *r = s.rows + i * kPvCols;
    acc0 += r[1 + a0] * r[1 + c0];
    acc1 += r[p1] * r[q1];
  }
  if (with_latent) {
    double l0 = 0.0, l1 = 0.0;
    for (int k = 0; k < kPvLatent; k++) {
      const float *r = s.lat + k * 32;
      l0 += (double)r[1 + a0] * (double)r[1 + c0];
      l1 += (double)r[p1] * (double)r[q1];
    }
    acc0 = acc0 + lw * l0;
    acc1 = acc1 + lw * l1;
  }
  if (tid == kNeqThreads - 1) {
    double C = 0.0;
    for (int i = 0; i < kPvIn; i++) C += s.rows[i * kPvCols] * s.rows[i * kPvCols];
    if (with_latent) {
      double L = 0.0;
      for (int k = 0; k < kPvLatent; k++) L += (double)s.lat[k * 32] * (double)s.lat[k * 32];
      C = C + lw * L;
    }
    neq_emit_cost(cost, b, w * C, add);
  }
  neq_emit_A(A, b, a0, c0, w * acc0, add);
  if (c1 >= 0) neq_emit_A(A, b, a1, c1, w * acc1, add);
  else if (own.own_g) neq_emit_g(g, b, a1, w * acc1, add);
}

}  // namespace shr

using namespace shr;

extern "C" int shr_pose_vae_blob_floats(void) { return kPvBlob; }

extern "C" long long shr_pose_vae_normal_workspace_bytes(int B, int J) {
  if (B < 0 || J < 0) return -1;
  return 0;
}

extern "C" int shr_pose_vae_normal(const float *kp, const float *jac, const float *blob, int blob_floats, float weight,
                                   float latent_weight, int B, int J, int accumulate, double *A, double *g, double *cost,
                                   double *residual, double *latent, uint32_t *relu_mask, void *workspace, void *stream) {
  if (B < 0 || J != kPvJ || (accumulate != 0 && accumulate != 1)) return SHR_EINVAL;
  if (!neq_weight_ok(weight) || !neq_weight_ok(latent_weight)) return SHR_EINVAL;
  if (blob_floats != kPvBlob) return SHR_EINVAL;
  if (neq_too_large(B, 1, J)) return SHR_ETOOLARGE;
  if (B == 0) return SHR_OK;
  const bool used = weight > 0.f;
  if (!kp || !jac || !blob || (used && (!A || !g || !cost))) return SHR_EINVAL;
  if (!neq_aligned(4, jac, relu_mask) || !neq_aligned(8, A, g, cost, residual, latent) || !neq_aligned(16, kp, blob, workspace))
    return SHR_EINVAL;
  if (!used && !residual && !latent && !relu_mask) return SHR_OK;     // nothing to write: no launch
  const int mode = !used ? kNeqKeep : (accumulate ? kNeqAdd : kNeqWrite);
  hipLaunchKernelGGL(pose_vae_kernel, dim3((unsigned)B), dim3(kNeqThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4 *>(kp), jac, blob, (double)weight, (double)latent_weight, mode, A, g, cost,
                     residual, latent, relu_mask);
  return (int)hipGetLastError();
}
