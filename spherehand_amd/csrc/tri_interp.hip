// tri_interp.hip -- vertex-attribute interpolation over the triangle raster's owner map (shr_tri_interp_fwd / _bwd;
// include/spherehand_hip.h states the contract, DESIGN.md 4.4e the layout): per-vertex attributes attr[NV,C] -> per-pixel
// maps out[B,C,H,W] with the clamped, normalised barycentric weights the raster's depth used at the pixel
// (tri_face.h: face_sort, face_matrix, pixel_weights), and the gradients to the attributes and to the vertices' x, y.
//
//   forward        one thread per pixel, 64 x 4 tiles: the owner's set-up in registers, the three weights kept while the
//                  channels loop; every channel plane is written coalesced.  fp32, one rounding per written operator.
//   grad vertex    fixed_point.h's passes over InterpVertexTaps: nine terms per owned pixel, mesh_depth_bwd.hip's rule
//                  (decisions in fp32, derivative in fp64; a weight clamped strictly outside [0, 1] is a constant) through
//                  the same statements: tri_tap.h's tri_corners, owned_tap and weight_chain
//   grad attr      C terms per corner: the channels go in groups of three, one group = the three coordinates of
//                  fixed_point.h's accumulator points, "crop" b * G + j for group j of crop b (G = ceil(C / 3)).  One
//                  walk over all channels finds the crop's largest term and gives every group of the crop that unit;
//                  fixed_point.h's sum kernel then runs per group, and a conversion of its own writes [B,NV,C].
#include "fixed_point.h"
#include "tri_tap.h"

namespace shr {

constexpr int kInterpMaxC = 64;   // channels per call (SHR_ETOOLARGE beyond)

struct InterpArgs {
  const int *owner;
  const float4 *verts;   // [B][NV]
  const int *faces;
  const float *attr;     // [B][NV][C], or [NV][C] with bstride 0
  long long bstride;     // floats between two crops' attributes
  int NV, F, W, H, C;
};

// face t of crop bi: tri_tap.h's checked gather
__device__ __forceinline__ bool interp_face(const InterpArgs &A, int bi, int t, float (&fv)[9], int (&id)[3]) {
  return tri_corners(A.verts + (size_t)bi * A.NV, A.faces, A.NV, A.F, t, fv, id);
}

constexpr int kIntX = 64, kIntY = 4;   // a workgroup: 64 x 4 pixels, one wave per row segment

// VEC4: C % 4 == 0 and 16-byte aligned attribute rows -- the three rows are read as float4
template <bool VEC4>
__global__ void __launch_bounds__(kIntX * kIntY)
interp_fwd_kernel(InterpArgs A, float *__restrict__ out) {
  const int x = blockIdx.x * kIntX + threadIdx.x, y = blockIdx.y * kIntY + threadIdx.y, bi = blockIdx.z;
  if (x >= A.W || y >= A.H) return;
  const size_t npix = (size_t)A.W * A.H, i = (size_t)y * A.W + x;
  float *o = out + (size_t)bi * A.C * npix + i;
  const int t = A.owner[(size_t)bi * npix + i];
  float fv[9], wh[3] = {0.f, 0.f, 0.f};
  int id[3], sid[3] = {0, 0, 0};
  bool live = interp_face(A, bi, t, fv, id);
  if (live) {
    float p[3][3], fi[9], w[3], c[3];
    int order[3];
    face_sort(fv, p, order);
    face_matrix(p, fi);
    const float s = pixel_weights(fi, (float)x, (float)y, w, c);
    live = s > 0.f && s <= 3.0e38f;   // (zero or not finite: the pixel gets 0)
    if (live) {
#pragma unroll
      for (int k = 0; k < 3; k++) wh[k] = c[k] / s;
      tap_sorted_ids(id, order, sid);
    }
  }
  if (!live) {
    for (int ch = 0; ch < A.C; ch++) o[(size_t)ch * npix] = 0.f;
    return;
  }
  const float *a0 = A.attr + (size_t)bi * A.bstride + (size_t)sid[0] * A.C;
  const float *a1 = A.attr + (size_t)bi * A.bstride + (size_t)sid[1] * A.C;
  const float *a2 = A.attr + (size_t)bi * A.bstride + (size_t)sid[2] * A.C;
  if (VEC4) {
    for (int ch = 0; ch < A.C; ch += 4) {
      const float4 u0 = *reinterpret_cast<const float4 *>(a0 + ch), u1 = *reinterpret_cast<const float4 *>(a1 + ch),
                   u2 = *reinterpret_cast<const float4 *>(a2 + ch);
      o[(size_t)ch * npix] = (wh[0] * u0.x + wh[1] * u1.x) + wh[2] * u2.x;
      o[(size_t)(ch + 1) * npix] = (wh[0] * u0.y + wh[1] * u1.y) + wh[2] * u2.y;
      o[(size_t)(ch + 2) * npix] = (wh[0] * u0.z + wh[1] * u1.z) + wh[2] * u2.z;
      o[(size_t)(ch + 3) * npix] = (wh[0] * u0.w + wh[1] * u1.w) + wh[2] * u2.w;
    }
  } else {
    for (int ch = 0; ch < A.C; ch++) o[(size_t)ch * npix] = (wh[0] * a0[ch] + wh[1] * a1[ch]) + wh[2] * a2[ch];
  }
}

// One owned pixel for the backward: tri_tap.h's owned_tap (the forward's fp32 decisions, the fp64 weights over the SORTED
// corners), the forward's liveness rule, the normalised weights wh = c / s and the sorted corners' vertex ids.
struct InterpTap : OwnedTap {
  double wh[3];
  int sid[3];
};
__device__ __forceinline__ bool interp_tap(const InterpArgs &A, int bi, int t, int xi, int yi, InterpTap &T) {
  float fv[9];
  int id[3];
  if (!interp_face(A, bi, t, fv, id)) return false;
  const float s32 = owned_tap(fv, xi, yi, T);
  if (!(s32 > 0.f && s32 <= 3.0e38f)) return false;   // the forward wrote a constant 0
  tap_sorted_ids(id, T.order, T.sid);
#pragma unroll
  for (int a = 0; a < 3; a++) T.wh[a] = T.c[a] / T.s;
  return true;
}

// grad_vertices: with g_k = sum_ch grad_out[ch] a_k[ch], d (sum_k g_k c_k / s) / d c_a = (g_a - sum_k g_k wh_k) / s, and
// d w_a = (d n_a - w_a d den) / den for the weights that pass.
template <bool RUNS>
struct InterpVertexTaps {
  InterpArgs A;
  const float *grad_out;
  static constexpr int kThreads = PixelWalk<RUNS>::kThreads, kBlockPix = PixelWalk<RUNS>::kBlockPix;
  static constexpr bool kRuns = RUNS;
  __device__ __forceinline__ int points() const { return A.NV; }
  template <typename Fn>
  __device__ __forceinline__ void walk(Fn fn) const {
    const int bi = blockIdx.y;
    const size_t npix = (size_t)A.W * A.H;
    for (int k = 0; k < PixelWalk<RUNS>::kPix; k++) {
      const size_t i = PixelWalk<RUNS>::pixel(k);
      if (i >= npix) break;
      const int t = A.owner[(size_t)bi * npix + i];
      if (t < 0) continue;
      const int yi = (int)(i / A.W), xi = (int)(i - (size_t)yi * A.W);
      InterpTap T;
      if (!interp_tap(A, bi, t, xi, yi, T)) continue;
      const float *go = grad_out + (size_t)bi * A.C * npix + i;
      const float *a0 = A.attr + (size_t)bi * A.bstride + (size_t)T.sid[0] * A.C;
      const float *a1 = A.attr + (size_t)bi * A.bstride + (size_t)T.sid[1] * A.C;
      const float *a2 = A.attr + (size_t)bi * A.bstride + (size_t)T.sid[2] * A.C;
      double gk[3] = {0.0, 0.0, 0.0};
      for (int ch = 0; ch < A.C; ch++) {
        const double g = go[(size_t)ch * npix];
        gk[0] += g * (double)a0[ch]; gk[1] += g * (double)a1[ch]; gk[2] += g * (double)a2[ch];
      }
      const double gbar = (gk[0] * T.wh[0] + gk[1] * T.wh[1]) + gk[2] * T.wh[2];
      double G[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
      weight_chain(T, [&](int a) { return (gk[a] - gbar) / T.s / T.den; }, G);
      fn(G, T.sid);
    }
  }
};

// grad_attr, channel group j = blockIdx.y % G of crop blockIdx.y / G: g[a][d] = wh_a * grad_out[3 j + d]
template <bool RUNS>
struct InterpAttrTaps {
  InterpArgs A;
  const float *grad_out;
  int G;
  static constexpr int kThreads = PixelWalk<RUNS>::kThreads, kBlockPix = PixelWalk<RUNS>::kBlockPix;
  static constexpr bool kRuns = RUNS;
  __device__ __forceinline__ int points() const { return A.NV; }
  template <typename Fn>
  __device__ __forceinline__ void walk(Fn fn) const {
    const int bi = blockIdx.y / G, ch0 = 3 * (blockIdx.y - bi * G);
    const size_t npix = (size_t)A.W * A.H;
    for (int k = 0; k < PixelWalk<RUNS>::kPix; k++) {
      const size_t i = PixelWalk<RUNS>::pixel(k);
      if (i >= npix) break;
      const int t = A.owner[(size_t)bi * npix + i];
      if (t < 0) continue;
      const float *go = grad_out + ((size_t)bi * A.C + ch0) * npix + i;
      double gd[3];
#pragma unroll
      for (int d = 0; d < 3; d++) gd[d] = ch0 + d < A.C ? (double)go[(size_t)d * npix] : 0.0;
      if (gd[0] == 0.0 && gd[1] == 0.0 && gd[2] == 0.0) continue;
      const int yi = (int)(i / A.W), xi = (int)(i - (size_t)yi * A.W);
      InterpTap T;
      if (!interp_tap(A, bi, t, xi, yi, T)) continue;
      double g[3][3];
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int d = 0; d < 3; d++) g[a][d] = T.wh[a] * gd[d];
      fn(g, T.sid);
    }
  }
};

// grad_attr's first pass: the crop's largest |term| over ALL channels, max_a wh_a x max_ch |grad_out[ch]| (the product
// of two non-negative doubles is monotone in both: this IS the largest product), given to each of the crop's G groups.
__global__ void __launch_bounds__(kBwdThreads)
interp_attr_max_kernel(InterpArgs A, const float *__restrict__ grad_out, int G, uint32_t *__restrict__ crop_max) {
  __shared__ uint32_t s_max;
  if (threadIdx.x == 0) s_max = 0u;
  __syncthreads();
  const int bi = blockIdx.y;
  const size_t npix = (size_t)A.W * A.H;
  float m = 0.f;
  for (int k = 0; k < kBwdPix; k++) {
    const size_t i = PixelWalk<false>::pixel(k);
    if (i >= npix) break;
    const int t = A.owner[(size_t)bi * npix + i];
    if (t < 0) continue;
    const float *go = grad_out + (size_t)bi * A.C * npix + i;
    float gm = 0.f;
    for (int ch = 0; ch < A.C; ch++) {
      const float a = fabsf(go[(size_t)ch * npix]);
      if (a <= 3.0e38f) gm = fmaxf(gm, a);
    }
    if (gm == 0.f) continue;
    const int yi = (int)(i / A.W), xi = (int)(i - (size_t)yi * A.W);
    InterpTap T;
    if (!interp_tap(A, bi, t, xi, yi, T)) continue;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float v = (float)fabs(T.wh[a] * (double)gm);
      if (v <= 3.0e38f) m = fmaxf(m, v);
    }
  }
  if (m > 0.f) atomicMax(&s_max, __float_as_uint(m));
  __syncthreads();
  if (s_max != 0u)
    for (int j = threadIdx.x; j < G; j += kBwdThreads) atomicMax(&crop_max[bi * G + j], s_max);
}

// grad_attr's last pass: acc[B][G][NV][3] fixed point -> grad_attr[B][NV][C]
__global__ void __launch_bounds__(256)
interp_attr_finish_kernel(const unsigned long long *__restrict__ acc, const uint32_t *__restrict__ crop_max, int B, int NV,
                          int C, int G, int fix_bits, float *__restrict__ grad_attr) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * NV * C) return;
  const int ch = (int)(i % C);
  const size_t bv = i / C;
  const int v = (int)(bv % NV), b = (int)(bv / NV);
  const int j = ch / 3, d = ch - 3 * j;
  const uint32_t mb = crop_max[b * G + j];
  float r = 0.f;
  if (mb != 0u)
    r = (float)((double)(long long)acc[(((size_t)b * G + j) * NV + v) * 3 + d] * (1.0 / fix_unit(mb, fix_bits)));
  grad_attr[i] = r;
}

}  // namespace shr

static int interp_groups(int C) { return (C + 2) / 3; }

static int interp_check(const int32_t *owner, const float *vertices, const int32_t *faces, const float *attr,
                        long long attr_batch_stride, int B, int NV, int F, int W, int H, int C) {
  if (!owner || !vertices || (F > 0 && !faces) || !attr || B < 0 || NV <= 0 || F < 0 || W <= 0 || H <= 0 || C <= 0)
    return SHR_EINVAL;
  if (attr_batch_stride != 0 && attr_batch_stride != (long long)NV * C) return SHR_EINVAL;
  if ((((uintptr_t)vertices) & 15u) != 0 || (((uintptr_t)attr) & 3u) != 0) return SHR_EINVAL;
  if (C > shr::kInterpMaxC || B > 65535 || W > 65535 || H > 65535 || (long long)NV * 3 >= (1LL << 31) ||
      3LL * F >= (1LL << 31) || (long long)NV * C >= (1LL << 31))
    return SHR_ETOOLARGE;
  return SHR_OK;
}

extern "C" int shr_tri_interp_fwd(const int32_t *owner, const float *vertices, const int32_t *faces, const float *attr,
                                  long long attr_batch_stride, int B, int NV, int F, int W, int H, int C, float *out,
                                  void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!out) return SHR_EINVAL;
  const int rc = interp_check(owner, vertices, faces, attr, attr_batch_stride, B, NV, F, W, H, C);
  if (rc != SHR_OK) return rc;
  const InterpArgs A{owner, reinterpret_cast<const float4 *>(vertices), faces, attr, attr_batch_stride, NV, F, W, H, C};
  const dim3 grid((unsigned)((W + kIntX - 1) / kIntX), (unsigned)((H + kIntY - 1) / kIntY), (unsigned)B);
  if (C % 4 == 0 && ((uintptr_t)attr & 15u) == 0)
    hipLaunchKernelGGL(interp_fwd_kernel<true>, grid, dim3(kIntX, kIntY), 0, (hipStream_t)stream, A, out);
  else
    hipLaunchKernelGGL(interp_fwd_kernel<false>, grid, dim3(kIntX, kIntY), 0, (hipStream_t)stream, A, out);
  return (int)hipGetLastError();
}

// vertex part (want_vertices): fixed_point.h's layout for B crops | attribute part (want_attr): the same for B * G
extern "C" long long shr_tri_interp_bwd_workspace_bytes(int B, int NV, int C, int want_attr, int want_vertices) {
  if (B < 0 || NV < 0 || C < 0) return -1;
  long long n = 0;
  if (want_vertices) n += fix_workspace_bytes(B, NV);
  if (want_attr) n += fix_workspace_bytes(B * interp_groups(C), NV);
  return n;
}

template <bool RUNS>
static int interp_attr_bwd(const shr::InterpArgs &A, const float *grad_out, int B, int fix_bits, float *grad_attr,
                           void *workspace, hipStream_t s) {
  using namespace shr;
  const int G = interp_groups(A.C), BG = B * G;
  const size_t npix = (size_t)A.W * A.H;
  uint32_t *crop_max = reinterpret_cast<uint32_t *>(workspace);
  unsigned long long *acc = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(workspace) + mesh_bwd_max_bytes(BG));
  const size_t n16 = (size_t)fix_workspace_bytes(BG, A.NV) / 16;
  const size_t clear_blocks = (n16 + 255) / 256;
  hipLaunchKernelGGL(mesh_bwd_clear_kernel, dim3((unsigned)(clear_blocks < 4096 ? clear_blocks : 4096)), dim3(256), 0, s,
                     reinterpret_cast<uint4 *>(workspace), n16);
  hipLaunchKernelGGL(interp_attr_max_kernel, dim3((unsigned)((npix + kBwdBlockPix - 1) / kBwdBlockPix), (unsigned)B),
                     dim3(kBwdThreads), 0, s, A, grad_out, G, crop_max);
  using Taps = InterpAttrTaps<RUNS>;
  const dim3 grid((unsigned)((npix + Taps::kBlockPix - 1) / Taps::kBlockPix), (unsigned)BG);
  hipLaunchKernelGGL((mesh_bwd_sum_kernel<Taps, !RUNS>), grid, dim3(Taps::kThreads), 0, s, Taps{A, grad_out, G}, crop_max,
                     fix_bits, acc);
  const size_t n = (size_t)B * A.NV * A.C;
  hipLaunchKernelGGL(interp_attr_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, acc, crop_max, B, A.NV,
                     A.C, G, fix_bits, grad_attr);
  return (int)hipGetLastError();
}

extern "C" int shr_tri_interp_bwd(const int32_t *owner, const float *vertices, const int32_t *faces, const float *attr,
                                  long long attr_batch_stride, int B, int NV, int F, int W, int H, int C,
                                  const float *grad_out, float *grad_attr, float *grad_vertices, void *workspace,
                                  void *stream) {
  using namespace shr;
  if (B == 0) return SHR_OK;
  if (!grad_out || (!grad_attr && !grad_vertices) || !workspace) return SHR_EINVAL;
  const int rc = interp_check(owner, vertices, faces, attr, attr_batch_stride, B, NV, F, W, H, C);
  if (rc != SHR_OK) return rc;
  if ((((uintptr_t)grad_vertices | (uintptr_t)workspace) & 15u) != 0) return SHR_EINVAL;
  if ((long long)B * interp_groups(C) > 65535) return SHR_ETOOLARGE;   // (one grid row per crop and channel group)
  const InterpArgs A{owner, reinterpret_cast<const float4 *>(vertices), faces, attr, attr_batch_stride, NV, F, W, H, C};
  hipStream_t s = (hipStream_t)stream;
  // an accumulator takes at most one term per corner per pixel: three per pixel
  const int bits = fix_term_bits(3, W, H);
  const size_t npix = (size_t)W * H;
  char *ws = reinterpret_cast<char *>(workspace);
  if (grad_vertices) {
    const int e = with_runs(NV, [&](auto runs) {
      return fixed_point_bwd<4>(InterpVertexTaps<decltype(runs)::value>{A, grad_out}, B, NV, npix, bits, grad_vertices, ws, s);
    });
    if (e != 0 || !grad_attr) return e;
    ws += fix_workspace_bytes(B, NV);
  }
  return with_runs(NV, [&](auto runs) {
    return interp_attr_bwd<decltype(runs)::value>(A, grad_out, B, bits, grad_attr, ws, s);
  });
}
