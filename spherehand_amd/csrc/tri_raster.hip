// tri_raster.hip -- triangle-mesh depth rasterizer (forward; the owner raster its backward needs).
//
// Replaces (reference file:line):
//   mesh/cuda_kernel/depth_rasterization_cuda_kernel.cu:18-113 `kernel` and :6-16
//   `atomicMin`, :115-134 depth_rasterization_cuda_forward  -> shr_tri_raster_fwd
//   the same plus the face that made each pixel's depth       -> shr_tri_raster_owner_fwd (backward: mesh_depth_bwd.hip)
//
// The reference launches one single-thread block per face that walks the face's
// pixel columns serially and CAS-loops a float min per pixel.  Here a wave takes
// 32 faces: lanes = faces for the set-up (cull, sort by x, inverse barycentric
// matrix), then lanes = the faces' pixel COLUMNS for the spans and lanes = the
// pixels inside the spans for the depth (raster_batch below).
// Every pixel repeats the reference's per-column span test and per-pixel
// arithmetic verbatim (fp32, one rounding per written operator, IEEE division; the
// `1. / x` the reference evaluates in fp64 and rounds to fp32 equals the fp32
// quotient exactly -- 53 >= 2*24+2 bits).  The float min is a native integer
// atomic on the fp32 bits (signed min / unsigned max by sign: order independent,
// hence deterministic); the image holds plain floats throughout: one fill pass,
// one raster pass.
#include "tri_face.h"

namespace shr {

typedef uint32_t v4u_t __attribute__((ext_vector_type(4)));

// Float min on the fp32 bits themselves, with native integer atomics: among non-negative
// floats the bits order like signed integers, among negative ones like unsigned integers
// reversed -- a signed MIN for a value whose sign bit is clear (an older negative entry is a
// smaller signed integer and stays), an unsigned MAX for one whose sign bit is set (it beats
// every non-negative entry, and the more negative of two negatives is the larger unsigned).
// The image holds plain floats at all times: no decode pass.  NaN is never offered.
__device__ __forceinline__ void zmin(float *cell, float v) {
  const uint32_t b = __float_as_uint(v);
  if (b >> 31) atomicMax(reinterpret_cast<unsigned int *>(cell), b);
  else atomicMin(reinterpret_cast<int *>(cell), (int)b);
}

// A wave sets up to 32 faces up with lanes = faces and parks each face's values in an LDS row (raster_batch below).
constexpr int kFaceRow = 28;          // x0 y0 x1 y1 x2 y2 s01 s12 | z0 z1 z2 fi[9] | x of column item 0, r_lo, r_hi, s02 | slope flags
constexpr int kFacesPerWave = 32;     // 4.5 KB of LDS per wave (rows, queue): eight waves per SIMD fit
// a wave's private scratch: face rows | pixel queue
constexpr int kScratchQueueBytes = 128 * 8;                                        // 1024
constexpr int kScratchMarkBytes = 64;                                               // start marks of a chunk's faces
constexpr int wave_scratch_bytes(int nf) { return nf * kFaceRow * 4 + kScratchQueueBytes + kScratchMarkBytes; }
constexpr int kWaveScratchBytes = wave_scratch_bytes(kFacesPerWave);               // 3584 + 1024

// One batch: lane l < 32 brings face set-up `s` (`have`: the lane holds a face; rows [s.r_lo, s.r_hi] already clipped
// to what the caller wants rasterized); every pixel inside its column's span goes to sink(xi, yi, depth, l) once, l the
// lane that brought its face.
// `scratch`: this wave's kWaveScratchBytes of LDS (16-byte aligned); nothing of it is live between two batches.
// One batch, the reference's own loop structure spread over a wave (.cu:70-111: for each column of the face its span
// of rows, for each row of the span a pixel):
//   columns  lanes = the COLUMNS of the batch's faces, 64 at a time whatever face they belong to: the column's span
//            (span_rows: two edge interpolations, the slopes divided once per face in the set-up), clipped to the
//            face's row range, and a prefix sum over the spans' lengths;
//   pixels   lanes = the pixels INSIDE those spans, 64 at a time, every lane with a pixel: queued as (face, x, y);
//   pass B   lanes = queued pixels, 64 at a time, every lane busy: the 7 divisions of the barycentric weights and the
//            perspective depth, then sink(x, y, depth).
// Rounds 1-4 walked every face's BOX (16-pixel groups; 8x8 patches of one face at a time for boxes above 256 pixels)
// with a span test per box pixel: three box pixels in four lie outside the spans, and the large boxes -- one face in
// six of the hand mesh, six tenths of its box pixels -- took 380 of the kernel's 630 us for 256 crops.
// NF = faces per batch (lanes 0 .. NF - 1 bring one each; `scratch` = wave_scratch_bytes(NF)).
// LEVELS: the pixels of a chunk of columns are queued LEVEL by level -- level t = row ylo + t of every column whose span
// is longer than t, compacted with a ballot -- instead of column after column: a level costs a ballot and a store where
// the pixel-order walk pays a run search and three shuffles per 64 pixels, and a drain's neighbouring lanes are then
// neighbouring columns at one height.  For an LDS sink (band kernel): 1 crop 54 -> 37 us.  NOT for the global atomics:
// 64 lanes in a few cache lines resolve slower in the L2 than 64 lanes in 64 lines (256 crops 461 -> 544 us;
// tools/exp_tri_level.py, EXPERIMENTS R3c).
// (tools/exp_tri_level.py builds this file with the two kernels' walks swapped: the measurements behind the defaults)
#ifndef SHR_TRI_ATOMIC_LEVELS
#define SHR_TRI_ATOMIC_LEVELS 0
#endif
#ifndef SHR_TRI_BAND_LEVELS
#define SHR_TRI_BAND_LEVELS 1
#endif
template <int NF, bool LEVELS, typename Sink>
__device__ __forceinline__ void raster_batch(const FaceSetup &s, bool have, int lane, unsigned char *scratch, int height,
                                             Sink &&sink) {
  float (*s_face)[kFaceRow] = reinterpret_cast<float (*)[kFaceRow]>(scratch);
  uint2 *s_queue = reinterpret_cast<uint2 *>(scratch + NF * kFaceRow * 4);
  unsigned char *s_mark = scratch + NF * kFaceRow * 4 + kScratchQueueBytes;
  float fi[9];
  face_matrix(s.p, fi);
  const EdgeSlopes e = edge_slopes(s.p);
  const int bw = s.xi_max - s.xi_min + 1, bh = s.r_hi - s.r_lo + 1;
  const bool alive = have && s.live && bh > 0 && bw > 0;
  const int ncol = alive ? bw : 0;                     // (<= 65535 columns each, 32 faces: 32 bits)
  const int fincl = wave_scan_incl(ncol, lane);        // lanes = faces: the face's columns end here
  const int ncols = __builtin_amdgcn_readlane(fincl, 63);
  if (lane < NF) {
    float *r = s_face[lane];
#pragma unroll
    for (int a = 0; a < 3; a++) { r[2 * a] = s.p[a][0]; r[2 * a + 1] = s.p[a][1]; r[8 + a] = s.p[a][2]; }
#pragma unroll
    for (int k = 0; k < 9; k++) r[11 + k] = fi[k];
    r[6] = e.s01; r[7] = e.s12;
    r[20] = __int_as_float(s.xi_min - (fincl - ncol));   // column item k of the face is pixel column k + this
    r[21] = __int_as_float(s.r_lo); r[22] = __int_as_float(s.r_hi); r[23] = e.s02;
    {   // the corners' z: their refined reciprocals for the pixels' divisions (tri_face.h tri_pixel_depth), bit 2: all tame
      const bool tame = div_tame_z(s.p[0][2]) && div_tame_z(s.p[1][2]) && div_tame_z(s.p[2][2]);
#pragma unroll
      for (int a = 0; a < 3; a++) r[25 + a] = tame ? div_rcp_refined(s.p[a][2]) : 0.f;
      r[24] = __int_as_float(e.flags | (tame ? 4 : 0));
    }
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);   // this wave's LDS writes (rows and queue are private to the wave)
  __builtin_amdgcn_wave_barrier();

  int qn = 0;   // queued pixels (wave-uniform)
  auto drain = [&](int take) {   // pass B on the last `take` queued pixels
    if (lane < take) {
      const uint2 e = s_queue[qn - take + lane];
      const float4 *r4 = reinterpret_cast<const float4 *>(s_face[e.x]);
      const float4 b2 = r4[2], b3 = r4[3], b4 = r4[4], b6 = r4[6];
      const float pz[3] = {b2.x, b2.y, b2.z};
      const float fi[9] = {b2.w, b3.x, b3.y, b3.z, b3.w, b4.x, b4.y, b4.z, b4.w};
      const float rz[3] = {b6.y, b6.z, b6.w};                                  // (row words 25 .. 27; word 24: the flags)
      const int xi = (int)(e.y & 0xffffu), yi = (int)(e.y >> 16);
      const float zp = pixel_depth(fi, (float)xi, (float)yi, pz, rz, (__float_as_int(b6.x) & 4) != 0);
      if (zp == zp) sink(xi, yi, zp, (int)e.x);  // fminf(NaN, old) = old
    }
    qn -= take;
  };
  for (int k0 = 0; k0 < ncols; k0 += 64) {
    const int k = k0 + lane;
    const bool colv = k < ncols;
    // the face of column item k: the faces whose first column lies in this chunk mark it (their number + 1: the numbers
    // rise with the position), a max-scan over the lanes spreads the marks, and the face that covers the chunk's first
    // column is one ballot (run_of's loop over the runs that end inside the chunk: ~5 of them here, ~25 on the lattice
    // of mesh_depth.hip, where this replaced 1 000 cycles per chunk)
    s_mark[lane] = 0;
    const int start = fincl - ncol;
    const unsigned long long before = __ballot(ncol > 0 && start < k0);
    if (ncol > 0 && start >= k0 && start < k0 + 64) s_mark[start - k0] = (unsigned char)(lane + 1);
    const int cover = before ? (int)(63 - __builtin_clzll(before)) : 0;       // the last face that starts before the chunk
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    int mk = (int)s_mark[lane];
    mk = max(mk, __builtin_amdgcn_update_dpp(0, mk, 0x111, 0xF, 0xF, false));   // row_shr:1
    mk = max(mk, __builtin_amdgcn_update_dpp(0, mk, 0x112, 0xF, 0xF, false));   // row_shr:2
    mk = max(mk, __builtin_amdgcn_update_dpp(0, mk, 0x114, 0xF, 0xF, false));   // row_shr:4
    mk = max(mk, __builtin_amdgcn_update_dpp(0, mk, 0x118, 0xF, 0xF, false));   // row_shr:8
    {
      const int m0 = __builtin_amdgcn_readlane(mk, 15), m1 = __builtin_amdgcn_readlane(mk, 31), m2 = __builtin_amdgcn_readlane(mk, 47);
      const int rowi = lane >> 4;
      mk = max(mk, rowi >= 1 ? m0 : 0);
      mk = max(mk, rowi >= 2 ? m1 : 0);
      mk = max(mk, rowi >= 3 ? m2 : 0);
    }
    const int face = mk > 0 ? mk - 1 : cover;
    __builtin_amdgcn_wave_barrier();   // (the marks are rewritten by the next chunk)
    const float4 *r4 = reinterpret_cast<const float4 *>(s_face[face]);
    const float4 a0 = r4[0], a1 = r4[1], i0 = r4[5];
    const int fl = __float_as_int(s_face[face][24]);
    const int xi = k + __float_as_int(i0.x);
    int ylo, yhi;
    span_rows(a0.x, a0.y, a0.z, a0.w, a1.z, a1.w, i0.w, fl, xi, height, ylo, yhi);
    ylo = max(ylo, __float_as_int(i0.y));
    yhi = min(yhi, __float_as_int(i0.z));
    const int cnt = (colv && yhi >= ylo) ? yhi - ylo + 1 : 0;   // (a span holds at most 65535 rows, a chunk 64 columns)
    if (LEVELS) {
      const unsigned packed = (unsigned)xi | ((unsigned)ylo << 16);   // (xi, yi < 65536)
      for (int t = 0;; t++) {
        const bool on = cnt > t;
        const unsigned long long m = __ballot(on);
        if (m == 0ull) break;
        if (on) {
          const int pos = qn + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
          s_queue[pos] = make_uint2((unsigned)face, packed + ((unsigned)t << 16));
        }
        qn += __popcll(m);
        if (qn >= 64) drain(64);
      }
    } else {
      const int cincl = wave_scan_incl(cnt, lane);
      const int ctotal = __builtin_amdgcn_readlane(cincl, 63), cexcl = cincl - cnt;
      const int packed = face | (xi << 8);                          // (face < 32, xi < 65536)
      for (int p0 = 0; p0 < ctotal; p0 += 64) {
        const int p = p0 + lane;
        const int col = min(run_of(cincl, colv, p0, p), 63);       // (empty columns among the runs count too)
        const int cy = __shfl(ylo, col), ce = __shfl(cexcl, col), fx = __shfl(packed, col);
        const bool inside = p < ctotal;
        const unsigned long long m = __ballot(inside);
        if (inside) {
          const int pos = qn + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
          s_queue[pos] = make_uint2((unsigned)(fx & 0xff), (unsigned)(fx >> 8) | ((unsigned)(cy + (p - ce)) << 16));
        }
        qn += __popcll(m);
        if (qn >= 64) drain(64);
      }
    }
  }
  if (qn > 0) drain(qn);
  __builtin_amdgcn_s_waitcnt(0xc07f);   // the queue's and the rows' last reads: the next batch rewrites them
  __builtin_amdgcn_wave_barrier();
}

template <bool INDEXED>
__device__ __forceinline__ void load_face(const float *__restrict__ src, const int *__restrict__ faces, int b, int F, int NV,
                                          int fidx, float f[9]) {
  if (INDEXED) {  // vertices [B,NV,4] + faces [F,3]: the gather of mesh/render.py:308-309 fused
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float4 v = reinterpret_cast<const float4 *>(src)[(size_t)b * NV + faces[fidx * 3 + k]];
      f[3 * k] = v.x; f[3 * k + 1] = v.y; f[3 * k + 2] = v.z;
    }
  } else {
    const float *fp = src + ((size_t)b * F + fidx) * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = fp[k];
  }
}

// ---- the global-atomic kernel (any size) --------------------------------------------------------------------------
// A wave takes 32 faces and offers every covered pixel to the image with a native integer atomic on the fp32 bits
// (zmin), after one fill pass: 256 hand crops @640x640 (a 419-MB image) 630 us in rounds 1-4, 440-480 us since
// raster_batch walks column spans instead of boxes.
// OWNER (the owner raster's second pass where the band kernel does not fit): zbuf holds the finished depth image; a face
// whose offered depth has the pixel's bits takes an unsigned minimum of its index on owner (all -1 before): the smallest
// of the faces that tie -- the 64-bit (key << 32 | face) minimum of the band kernel, in two passes.
template <bool INDEXED, bool OWNER = false>
__global__ void __launch_bounds__(256)
tri_raster_kernel(const float *__restrict__ src, const int *__restrict__ faces, int B, int F, int NV, int width,
                  int height, float *__restrict__ zbuf, int *__restrict__ owner = nullptr) {
  const int lane = threadIdx.x & 63;
  const int wave_global = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int groups = (F + kFacesPerWave - 1) / kFacesPerWave;
  const int b = wave_global / groups;
  if (b >= B) return;
  const int fbase = (wave_global - b * groups) * kFacesPerWave, fidx = fbase + lane;
  float f[9];
  const bool have = lane < kFacesPerWave && fidx < F;
  if (have) {
    load_face<INDEXED>(src, faces, b, F, NV, fidx, f);
  } else {
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = 0.f;
  }
  const FaceSetup s = face_setup(f, width, height);
  float *zimg = zbuf + (size_t)b * width * height;
  __shared__ __attribute__((aligned(16))) unsigned char s_scratch[4][kWaveScratchBytes];
  int *oimg = OWNER ? owner + (size_t)b * width * height : nullptr;
  raster_batch<kFacesPerWave, SHR_TRI_ATOMIC_LEVELS != 0>(s, have, lane, s_scratch[threadIdx.x >> 6], height,
               [&](int xi, int yi, float zp, int slot) {
                 const size_t i = (size_t)yi * width + xi;
                 if (!OWNER) zmin(zimg + i, zp);
                 else if (__float_as_uint(zp) == __float_as_uint(zimg[i]))
                   atomicMin(reinterpret_cast<unsigned int *>(oimg + i), (unsigned)(fbase + slot));
               });
}

// ---- the band kernel (round 5) ----------------------------------------------------------------------------------
// The image is produced in BANDS of R rows held in LDS: every covered pixel is an LDS integer minimum, every image
// pixel is written to HBM exactly once with full-line stores -- no fill pass, no L2 atomics, and the float image is
// the reference's bit for bit (a minimum does not depend on the order it is taken in).
//   grid = (B, segments), block = 16 waves, dynamic LDS = row ranges [F] u32 | band's faces [F] u16 | band [R x W] f32 |
//   16 wave scratches.
//   phase 1  lanes = faces, once per workgroup: the reference's culls (.cu:33, :54, :68-69) and the conservative row
//            range of the face's spans -> s_range[f] = r_lo | r_hi << 16 (0xFFFF: culled), and the number of faces that
//            reach each band;
//   phase 2  per band of the segment: a band no face reaches is 1000.0 straight from registers; otherwise the band is
//            initialised in LDS, every wave walks its share of the ranges (one LDS word per face), collects the faces
//            that reach the band and rasterizes them 32 at a time (raster_batch, rows clipped to the band) with an LDS
//            minimum per covered pixel, and the band is streamed out.
constexpr int kBandWaves = 16;
constexpr int kBandFaces = 16;            // faces per batch: a wave's share of a band's faces is about that, and sixteen rows of
                                          // scratch less per wave are eleven more rows of band (2.8 instead of 4.5 KB per wave)
constexpr int kBandScratchBytes = wave_scratch_bytes(kBandFaces);
constexpr int kBandMaxBands = 512;        // per-band face counters in LDS
constexpr uint32_t kFillBits = 0x447A0000u;   // 1000.0f, .cu:122

// the culls and the row range of face_setup without its divisions (face_matrix, edge_slopes) and without sorting the
// corners' y (face_ranges takes them in any order)
__device__ __forceinline__ uint32_t face_row_range(const float (&f)[9], int width, int height) {
  float p[3][3];
  int order[3], xi_min, xi_max, r_lo, r_hi;
  bool live = face_sort(f, p, order);
  live &= face_ranges(p[0][0], p[2][0], f[1], f[4], f[7], width, height, xi_min, xi_max, r_lo, r_hi);
  return live && r_hi >= r_lo ? ((uint32_t)r_lo | ((uint32_t)r_hi << 16)) : 0xFFFFu;
}

// RESIZE (DepthRasterization.forward's tail, mesh/render.py:286, :311, for sizes the lattice kernel does not take -- S = 256
// from 640): the band never leaves LDS as a 640 x 640 image; its stream-out IS clamp(max) + ATen's bilinear resize to
// S x S.  With src / S = p_src / p_out in lowest terms, output rows [k p_out, (k + 1) p_out) take their two source rows
// from [k p_src, (k + 1) p_src) (down-sampling: scale > 1), so bands of a multiple of p_src rows hold every tap of their
// own output rows: zbuf = out [B][S][S], R % p_src == 0, square images.  The rasterized values are the full-resolution
// kernel's (same code), the epilogue is mesh_depth_kernel's formula: the same bits as raster -> clamp -> F.interpolate.
// OWNER (shr_tri_raster_owner_fwd): the band's cells are 64-bit minima (mkey(depth) << 32 | face), mesh_depth_tile's
// OWNER slots: the same depth bits, plus owner[B][H][W] = the face of the smallest offered depth, ties to the smaller
// face index, -1 where no face offered one (the fill's face word is 0xFFFFFFFF).  Twice the LDS per band row.
template <bool INDEXED, bool RESIZE = false, bool OWNER = false>
__global__ void __launch_bounds__(kBandWaves * 64)
tri_band_kernel(const float *__restrict__ src, const int *__restrict__ faces, int B, int F, int NV, int width, int height,
                float *__restrict__ zbuf, int R, int nbands, int S = 0, int p_src = 1, int p_out = 1, float clamp_max = 0.f,
                int *__restrict__ owner = nullptr) {
  static_assert(!(RESIZE && OWNER), "the owner raster is full-size");
  constexpr int kCell = OWNER ? 8 : 4;
  constexpr unsigned long long kFillSlot = ((unsigned long long)(kFillBits ^ 0x80000000u) << 32) | 0xFFFFFFFFull;   // mkey(1000), no face
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Fpad = (F + 7) & ~7;
  uint32_t *s_range = reinterpret_cast<uint32_t *>(smem);
  uint16_t *s_pend = reinterpret_cast<uint16_t *>(smem + (size_t)Fpad * 4);          // the faces that reach the current band
  float *s_band = reinterpret_cast<float *>(smem + (size_t)Fpad * 6);
  unsigned long long *s_band64 = reinterpret_cast<unsigned long long *>(smem + (size_t)Fpad * 6);   // (OWNER; Fpad * 6 % 16 == 0)
  // (the band rounded up to 16 bytes: the scratch is read through float4 / uint2 -- odd widths would leave it 4-byte aligned)
  unsigned char *s_scr = smem + (size_t)Fpad * 6 + (((size_t)R * width * kCell + 15) & ~(size_t)15);
  __shared__ int s_bandcnt[kBandMaxBands];
  __shared__ int s_npend;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // workgroup y of a crop takes bands y, y + gridDim.y, ...: interleaved, so that every workgroup of a crop gets its
  // share of the hand's rows and of the empty ones (consecutive bands: the top and bottom segments were nearly free)
  const int band_first = blockIdx.y, band_step = gridDim.y;
  float *zimg = RESIZE ? zbuf + (size_t)b * S * S : zbuf + (size_t)b * width * height;
  int *oimg = OWNER ? owner + (size_t)b * width * height : nullptr;
  const bool counted = nbands <= kBandMaxBands;
  for (int i = tid; i < min(nbands, kBandMaxBands); i += kBandWaves * 64) s_bandcnt[i] = 0;
  __syncthreads();
  // ---- phase 1: row ranges -------------------------------------------------------------------------------------
  const float rinv = 1.0f / (float)R;
  for (int fidx = tid; fidx < F; fidx += kBandWaves * 64) {
    float f[9];
    load_face<INDEXED>(src, faces, b, F, NV, fidx, f);
    const uint32_t rw = face_row_range(f, width, height);
    s_range[fidx] = rw;
    if (counted && rw != 0xFFFFu) {
      // (band numbers through a float quotient: a band too many on either side only costs that band its shortcut)
      const int ba = max(0, (int)((float)(rw & 0xffffu) * rinv) - 1), bb = min(nbands - 1, (int)((float)(rw >> 16) * rinv) + 1);
      for (int k = ba; k <= bb; k++)
        if ((int)(rw & 0xffffu) <= min(height, (k + 1) * R) - 1 && (int)(rw >> 16) >= k * R) atomicAdd(&s_bandcnt[k], 1);
    }
  }
  __syncthreads();
  // ---- phase 2: the bands ----------------------------------------------------------------------------------------
  const bool vec4 = (width & 3) == 0;
  unsigned char *scratch = s_scr + (size_t)wave * kBandScratchBytes;
  const int nchunks = (F + 63) >> 6;
  for (int band = band_first; band < nbands; band += band_step) {
    const int lo = band * R, hi = min(height, lo + R) - 1, rows = hi - lo + 1;
    const int npix = rows * width;
    // RESIZE: the band's output rows [oy_lo, oy_lo + orows)
    const int oy_lo = RESIZE ? (lo / p_src) * p_out : 0, orows = RESIZE ? (rows / p_src) * p_out : 0;
    float *gout = RESIZE ? zimg + (size_t)oy_lo * S : zimg + (size_t)lo * width;
    int *oout = OWNER ? oimg + (size_t)lo * width : nullptr;
    if (counted && s_bandcnt[band] == 0) {          // no face reaches the band (workgroup-uniform)
      if (OWNER) {
        for (int i = tid; i < npix; i += kBandWaves * 64) { gout[i] = __uint_as_float(kFillBits); oout[i] = -1; }
      } else
      if (RESIZE) {                                 // every tap is the clamped background: min(1000, clamp_max) exactly
        const float bgv = fminf(__uint_as_float(kFillBits), clamp_max);
        for (int i = tid; i < orows * S; i += kBandWaves * 64) gout[i] = bgv;
      } else
      if (vec4) {
        const v4u_t t = {kFillBits, kFillBits, kFillBits, kFillBits};
        for (int i = tid; i < (npix >> 2); i += kBandWaves * 64)
          asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(reinterpret_cast<float4 *>(gout) + i), "v"(t) : "memory");
      } else {
        for (int i = tid; i < npix; i += kBandWaves * 64) gout[i] = __uint_as_float(kFillBits);
      }
      continue;
    }
    // the faces that reach the band, collected by ALL waves into one list (face numbers cluster: a wave's own chunks
    // hold all of a band's faces or none), then dealt out in equal shares
    if (tid == 0) s_npend = 0;
    if (OWNER) {
      for (int i = tid; i < npix; i += kBandWaves * 64) s_band64[i] = kFillSlot;
    } else
    if (vec4) {
      const float4 fv = make_float4(__uint_as_float(kFillBits), __uint_as_float(kFillBits), __uint_as_float(kFillBits),
                                    __uint_as_float(kFillBits));
      for (int i = tid; i < (npix >> 2); i += kBandWaves * 64) reinterpret_cast<float4 *>(s_band)[i] = fv;
    } else {
      for (int i = tid; i < npix; i += kBandWaves * 64) s_band[i] = __uint_as_float(kFillBits);
    }
    __syncthreads();
    for (int c = wave; c < nchunks; c += kBandWaves) {
      const int fidx = (c << 6) + lane;
      const uint32_t rw = fidx < F ? s_range[fidx] : 0xFFFFu;
      const bool reach = (int)(rw & 0xffffu) <= hi && (int)(rw >> 16) >= lo;
      const unsigned long long m = __ballot(reach);
      if (m == 0ull) continue;
      int base = 0;
      if (lane == 0) base = atomicAdd(&s_npend, __popcll(m));
      base = __builtin_amdgcn_readfirstlane(base);
      if (reach)
        s_pend[base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = (uint16_t)fidx;
    }
    __syncthreads();
    float *cells = s_band - (size_t)lo * width;      // cell of pixel (yi, xi) = cells[yi * width + xi]
    unsigned long long *cells64 = s_band64 - (size_t)lo * width;
    {
      // equal shares of the list, 16 faces at a time.  (Drawing batches of 16 from a counter instead -- a face costs what
      // its box holds -- measured 1022 us against 634 for 256 crops: a batch costs its LATENCY, the gather of its
      // vertices and the set-up's chain of divisions, whatever it holds; fewer, fuller batches win.)
      // The shares are STRIDED (wave w takes entries w, w + 16, ...): the list is in face order, neighbouring faces are
      // neighbours on the hand and of one size -- a contiguous share was all palm or all finger tips, and the band
      // waited for the wave with the palm.
      const int n = s_npend;
      const int mine = (n - wave + kBandWaves - 1) / kBandWaves;            // entries wave, wave + 16, ... below n
      for (int at = 0; at < mine; at += kBandFaces) {
        const int count = min(kBandFaces, mine - at);
        float f[9];
        const bool have = lane < count;
        if (have) {
          load_face<INDEXED>(src, faces, b, F, NV, (int)s_pend[wave + kBandWaves * (at + lane)], f);
        } else {
#pragma unroll
          for (int k = 0; k < 9; k++) f[k] = 0.f;
        }
        FaceSetup fs = face_setup(f, width, height);
        fs.r_lo = max(fs.r_lo, lo);
        fs.r_hi = min(fs.r_hi, hi);
        auto sink = [&](int xi, int yi, float zp, int slot) {
          if (OWNER) {   // (the face that lane `slot` brought: entry wave + 16 (at + slot) of the list)
            const uint32_t face = s_pend[wave + kBandWaves * (at + slot)];
            atomicMin(cells64 + yi * width + xi, ((unsigned long long)mkey(zp) << 32) | face);
            return;
          }
          float *cell = cells + yi * width + xi;
          const uint32_t bits = __float_as_uint(zp);
          if (bits >> 31) atomicMax(reinterpret_cast<unsigned int *>(cell), bits);   // (zmin's rule on an LDS cell)
          else atomicMin(reinterpret_cast<int *>(cell), (int)bits);
        };
        raster_batch<kBandFaces, SHR_TRI_BAND_LEVELS != 0>(fs, have, lane, scratch, height, sink);
      }
    }
    __syncthreads();
    // stream the band out
    if (OWNER) {
      for (int i = tid; i < npix; i += kBandWaves * 64) {
        const unsigned long long v = s_band64[i];
        gout[i] = mkey_inv((uint32_t)(v >> 32));
        oout[i] = (int)(uint32_t)v;
      }
    } else
    if (RESIZE) {
      const float scale = (float)height / (float)S;
      for (int i = tid; i < orows * S; i += kBandWaves * 64) {
        const int r = i / S, ox = i - r * S;
        const Lin ly = lin_index(oy_lo + r, scale, height), lx = lin_index(ox, scale, width);
        const float *r0 = cells + ly.i0 * width, *r1 = cells + min(ly.i1, hi) * width;   // (i1 <= hi whenever scale > 1)
        const float v00 = fminf(r0[lx.i0], clamp_max), v01 = fminf(r0[lx.i1], clamp_max);
        const float v10 = fminf(r1[lx.i0], clamp_max), v11 = fminf(r1[lx.i1], clamp_max);
        gout[i] = ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
      }
    } else
    if (vec4) {
      for (int i = tid; i < (npix >> 2); i += kBandWaves * 64) {
        const uint4 v = reinterpret_cast<const uint4 *>(s_band)[i];
        const v4u_t t = {v.x, v.y, v.z, v.w};
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(reinterpret_cast<float4 *>(gout) + i), "v"(t) : "memory");
      }
    } else {
      for (int i = tid; i < npix; i += kBandWaves * 64) gout[i] = s_band[i];
    }
    __syncthreads();                                  // the band's cells are re-initialised next
  }
}

__global__ void zbuf_fill_kernel(uint4 *__restrict__ z, size_t n4, uint32_t key, uint32_t *__restrict__ tail,
                                 int ntail) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const v4u_t v = {key, key, key, key};
  for (; i < n4; i += stride) asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(z + i), "v"(v) : "memory");
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = key;
}

}  // namespace shr

using namespace shr;

static int g_tri_band = -1;   // SHR_TUNE_TRI_BAND: -1 = by batch size (below), 0 = never (the global-atomic kernel), n > 0 = always, bands of <= n rows
int shr::tri_set_band(int v) { g_tri_band = v; return SHR_OK; }

// resize_S > 0: the band kernel with the clamp + resize epilogue (RESIZE above; depth = [B][S][S]); -1 when it does not fit.
// owner != nullptr: the owner raster (OWNER above; owner = [B][H][W]).
static int tri_raster_common(bool indexed, const float *src, const int *faces, int B, int F, int NV, int W, int H,
                             float *depth, hipStream_t s, int resize_S = 0, float clamp_max = 0.f, int *owner = nullptr) {
  int p_src = 1, p_out = 1;
  if (resize_S > 0) {
    if (W != H || resize_S >= H) return -1;   // (scale 1: the second tap, weight 0, is the NEXT period's first row)
    int a = H, c = resize_S;
    while (c) { const int t = a % c; a = c; c = t; }
    p_src = H / a; p_out = resize_S / a;
  }
  // The band kernel: the row ranges of all faces (4 F bytes) + sixteen wave scratches + a band of at least 8 rows
  // in one CU's LDS, 16-bit face numbers and row numbers.  (The owner raster's cells are 8 bytes: half the rows.)
  constexpr int kLds = 160 * 1024;
  const int cell = owner ? 8 : 4;
  const long long fixed = (long long)((F + 7) & ~7) * 6 + (long long)kBandWaves * kBandScratchBytes + 4096 + 16;   // (+ the static arrays: band counters, pending faces; + the band's rounding to 16 bytes)
  long long Rmax = (kLds - fixed) / ((long long)cell * W);
  if (Rmax > H) Rmax = H;
  Rmax -= Rmax % p_src;                                  // (resize: whole periods of source rows per band)
  if (resize_S > 0 && (Rmax < p_src || g_tri_band == 0 || !(F > 0 && F <= 65535 && H <= 65535))) return -1;
  // Which kernel: the band kernel wherever it fits (round 5, after raster_batch's level walk: hand mesh @640x640,
  // tools/exp_tri_band.py -- 1 crop 20.8 us against 78 for the atomic kernel, 48 crops 142 against 173, 256 crops 348
  // against 461); the atomic kernel for what does not (more than 65535 faces, rows too wide for 8 of them in LDS).
  // SHR_TUNE_TRI_BAND: 0 forces the atomic kernel, n > 0 bands of at most n rows.
  if (g_tri_band != 0 && F > 0 && F <= 65535 && (Rmax >= 8 || resize_S > 0) && H <= 65535 && W <= 65535) {
    const int cus = device_cus();   // (per device: common.h)
    // Rows per band and workgroups per crop.  A band costs a fixed part -- one batch's latency: the gather of its faces,
    // the set-up's chain of divisions, three barriers -- worth ~24 rows of raster and stream-out (256 crops: 8.8 us per
    // band of 8 rows, 13.4 per band of 25), a workgroup its pass over all faces' row ranges (~10 rows' worth), and a
    // workgroup has the CU's LDS: what does not fit the CUs at once waits for a CU.  The plan minimises
    //     rounds x (10 + bands per workgroup x (24 + R)),   rounds = 1 if B x segs <= cus, else B x segs / cus + 1/2
    // over R and the workgroups per crop (their bands interleaved): a crop per CU -> the tallest band, one workgroup
    // per crop; few crops -> cus / B workgroups per crop at the height that leaves each the fewest rows; somewhat more
    // crops than CUs -> several workgroups per crop again, so that the second round is not a whole crop long (288
    // crops: 517 -> see EXPERIMENTS R3c).
    int R = (int)Rmax, segs = 1;
    if (g_tri_band > 0) {
      if (g_tri_band < R) R = g_tri_band;
      R = R < p_src ? p_src : R - R % p_src;
      const int nb = (H + R - 1) / R;
      segs = B >= cus ? 1 : (cus + B - 1) / B;
      if (segs > nb) segs = nb;
    } else {
      float best = -1.f;
      const int lo = (int)(Rmax < 8 ? Rmax : 8);
      for (int r = (int)Rmax; r >= lo; r -= p_src) {
        const int nb = (H + r - 1) / r;
        // far fewer crops than CUs: cus / B workgroups per crop, all resident at once; from half a crop per CU on: up to
        // 8 per crop (200 crops as 200 workgroups leave 56 CUs idle for a whole crop's time)
        int sg_lo = B >= cus ? 1 : cus / B, sg_hi = 2 * B > cus ? 8 : cus / B;
        if (sg_lo > nb) sg_lo = nb;
        if (sg_hi > nb) sg_hi = nb;
        for (int sg = sg_lo; sg <= sg_hi; sg++) {
          const int per = (nb + sg - 1) / sg;
          if (sg > sg_lo && (nb + sg - 2) / (sg - 1) == per) continue;      // (one workgroup fewer does the same)
          const float load = (float)B * (float)sg / (float)cus;
          const float rounds = load <= 1.f ? 1.f : load + 0.5f;
          const float cost = rounds * (10.f + (float)per * (float)(24 + r));
          if (best < 0.f || cost < best) { best = cost; R = r; segs = sg; }
        }
      }
    }
    const int nbands = (H + R - 1) / R;
    if (segs > nbands) segs = nbands;
    if (segs > 65535) segs = 65535;
    const size_t lds = (size_t)((F + 7) & ~7) * 6 + (((size_t)R * W * cell + 15) & ~(size_t)15) + (size_t)kBandWaves * kBandScratchBytes;
    static AttrDone attr_done[6];   // per (kernel, device)
    auto launch = [&](auto kernel, int which) -> int {
      const hipError_t e = allow_dynamic_lds(kernel, kLds - 4096, &attr_done[which]);   // (the static arrays take the rest)
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(kernel, dim3((unsigned)B, (unsigned)segs), dim3(kBandWaves * 64), lds, s, src, faces, B, F, NV, W, H,
                         depth, R, nbands, resize_S, p_src, p_out, clamp_max, owner);
      return (int)hipGetLastError();
    };
    if (resize_S > 0) return indexed ? launch(tri_band_kernel<true, true>, 2) : launch(tri_band_kernel<false, true>, 3);
    if (owner) return indexed ? launch(tri_band_kernel<true, false, true>, 4) : launch(tri_band_kernel<false, false, true>, 5);
    return indexed ? launch(tri_band_kernel<true>, 0) : launch(tri_band_kernel<false>, 1);
  }
  if (resize_S > 0) return -1;
  const size_t n = (size_t)B * W * H;
  uint32_t *z = reinterpret_cast<uint32_t *>(depth);
  const size_t n4 = n / 4;
  const int ntail = (int)(n - n4 * 4);
  // (16384 workgroups at most: 4096 left the fill of 256 crops at 74 us, 16384 at ~60 -- torch's fill of the same bytes
  // takes 64; write-through / non-temporal stores change nothing, tools/exp_tri_fill.sh in round 5)
  const size_t want_blocks = (n4 + 255) / 256;
  const unsigned fill_blocks = (unsigned)(want_blocks > 16384 ? 16384 : (want_blocks ? want_blocks : 1));
  hipLaunchKernelGGL(zbuf_fill_kernel, dim3(fill_blocks), dim3(256), 0, s, reinterpret_cast<uint4 *>(z), n4,
                     0x447A0000u /* 1000.0f, .cu:122 */, z + n4 * 4, ntail);
  if (owner) {   // (-1: no face; the depth's layout, 16-byte aligned)
    uint32_t *o = reinterpret_cast<uint32_t *>(owner);
    hipLaunchKernelGGL(zbuf_fill_kernel, dim3(fill_blocks), dim3(256), 0, s, reinterpret_cast<uint4 *>(o), n4, 0xFFFFFFFFu,
                       o + n4 * 4, ntail);
  }
  if (F > 0) {
    const long long waves = (long long)B * ((F + kFacesPerWave - 1) / kFacesPerWave);
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    if (indexed)
      hipLaunchKernelGGL(tri_raster_kernel<true>, dim3(blocks), dim3(256), 0, s, src, faces, B, F, NV, W, H, depth, nullptr);
    else
      hipLaunchKernelGGL(tri_raster_kernel<false>, dim3(blocks), dim3(256), 0, s, src, faces, B, F, NV, W, H, depth, nullptr);
    if (owner && indexed)   // the second pass: the finished depth -> the faces that offered it
      hipLaunchKernelGGL((tri_raster_kernel<true, true>), dim3(blocks), dim3(256), 0, s, src, faces, B, F, NV, W, H, depth, owner);
    else if (owner)
      hipLaunchKernelGGL((tri_raster_kernel<false, true>), dim3(blocks), dim3(256), 0, s, src, faces, B, F, NV, W, H, depth, owner);
  }
  return (int)hipGetLastError();
}

// shr_mesh_depth_fwd's non-lattice sizes (mesh_depth.hip): vertices + faces -> clamp + resize of the 640 x 640 raster as
// ONE band-kernel launch; -1 when the band kernel does not take the problem
int shr::tri_band_resize(const float *vertices, const int *faces, int B, int NV, int F, int src_size, int S, float clamp_max,
                         float *depth, hipStream_t s) {
  return tri_raster_common(true, vertices, faces, B, F, NV, src_size, src_size, depth, s, S, clamp_max);
}

// The four forward entries' sizes, after an entry's own null-pointer line and before its alignment line (the order of
// the return codes: SHR_EINVAL for a size that is no size, then SHR_ETOOLARGE, then the alignment's SHR_EINVAL).
static int tri_raster_limits(int B, int F, int W, int H) {
  if (B < 0 || F < 0 || W <= 0 || H <= 0) return SHR_EINVAL;
  if ((long long)B * W * H > (1LL << 40) || (long long)B * ((F + 31) / 32) > (1LL << 31) || W > 65535 || H > 65535)
    return SHR_ETOOLARGE;   // (pixel coordinates travel in 16 bits)
  return SHR_OK;
}

extern "C" int shr_tri_raster_fwd(const float *face_vertices, int B, int F, int W, int H, float *depth,
                                  void *stream) {
  if (B == 0) return SHR_OK;
  if (!depth || (!face_vertices && F > 0)) return SHR_EINVAL;
  if (const int rc = tri_raster_limits(B, F, W, H)) return rc;
  if (((uintptr_t)depth & 15u) != 0) return SHR_EINVAL;
  return tri_raster_common(false, face_vertices, nullptr, B, F, 0, W, H, depth, (hipStream_t)stream);
}

extern "C" int shr_tri_raster_indexed_fwd(const float *vertices, const int32_t *faces, int B, int NV, int F, int W,
                                          int H, float *depth, void *stream) {
  if (B == 0) return SHR_OK;
  if (!depth || !vertices || (!faces && F > 0) || NV <= 0) return SHR_EINVAL;
  if (const int rc = tri_raster_limits(B, F, W, H)) return rc;
  if ((((uintptr_t)depth | (uintptr_t)vertices) & 15u) != 0) return SHR_EINVAL;
  return tri_raster_common(true, vertices, faces, B, F, NV, W, H, depth, (hipStream_t)stream);
}

extern "C" int shr_tri_raster_owner_fwd(const float *face_vertices, int B, int F, int W, int H, float *depth, int32_t *owner,
                                        void *stream) {
  if (B == 0) return SHR_OK;
  if (!depth || !owner || (!face_vertices && F > 0)) return SHR_EINVAL;
  if (const int rc = tri_raster_limits(B, F, W, H)) return rc;
  if ((((uintptr_t)depth | (uintptr_t)owner) & 15u) != 0) return SHR_EINVAL;
  return tri_raster_common(false, face_vertices, nullptr, B, F, 0, W, H, depth, (hipStream_t)stream, 0, 0.f, owner);
}

extern "C" int shr_tri_raster_indexed_owner_fwd(const float *vertices, const int32_t *faces, int B, int NV, int F, int W,
                                                int H, float *depth, int32_t *owner, void *stream) {
  if (B == 0) return SHR_OK;
  if (!depth || !owner || !vertices || (!faces && F > 0) || NV <= 0) return SHR_EINVAL;
  if (const int rc = tri_raster_limits(B, F, W, H)) return rc;
  if ((((uintptr_t)depth | (uintptr_t)owner | (uintptr_t)vertices) & 15u) != 0) return SHR_EINVAL;
  return tri_raster_common(true, vertices, faces, B, F, NV, W, H, depth, (hipStream_t)stream, 0, 0.f, owner);
}
