/* spherehand_hip.h -- C ABI of libspherehand_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the rasterize-and-fit hot path of melonwan/sphereHand.
 * Plain pointers and sizes only: no torch / ATen types cross this boundary.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *   - buffers are caller-allocated, contiguous, row-major fp32 unless noted;
 *     outputs are fully overwritten (no accumulate-into semantics);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *     kernels are enqueued on it and the call returns without synchronising;
 *     nothing is allocated, freed or synchronised inside the library;
 *   - return value: 0 (SHR_OK) or a negative SHR_E* code; a positive value is
 *     a hipError_t reported by the launch.  shr_error_string() names either.
 *   - image grid: pixel (v,u) has model-space coordinates
 *       xg = (u - W/2)*300/W , yg = (v - H/2)*300/H            (mm)
 *     (reference mesh/render.py:31-32).
 *
 * Each entry point cites the reference interface it replaces
 * (file:line relative to the reference repo root).
 */
#ifndef SPHEREHAND_HIP_H
#define SPHEREHAND_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHR_OK 0
#define SHR_EINVAL (-1)     /* null pointer / non-positive size / misaligned */
#define SHR_ETOOLARGE (-2)  /* size beyond what the kernels index (see each fn) */
#define SHR_ENODEVICE (-3)  /* no gfx950 device visible to the process */

#define SHR_MAX_SPHERES 64  /* spheres per crop (reference: 41) */
#define SHR_ARGMIN_NONE 255 /* argmin value of a pixel no sphere owns */

/* Library / device introspection ------------------------------------------ */
int shr_abi_version(void);               /* bumps on any signature change */
const char *shr_error_string(int code);  /* static string, never NULL */
/* 0 if a gfx950 device is current; fills name (<= name_len bytes, may be NULL),
 * compute-unit count and peak HBM clock-independent info are for logging only */
int shr_device_info(char *name_host, int name_len, int *num_cu_host);

/* Launch-shape tuning / test hooks (process-wide, not thread-safe; results never
 * depend on them).  *_LDS_BYTES cap the LDS a workgroup of the z-buffer kernels
 * may take (decides rows per region and workgroups per CU; FWD_LDS_BYTES 0 = the
 * default); FORCE_GENERAL = 1
 * routes every call to the general tile kernels. */
#define SHR_TUNE_FWD_LDS_BYTES 1
#define SHR_TUNE_FWD_OWNER_LDS_BYTES 2
#define SHR_TUNE_BWD_LDS_BYTES 3
#define SHR_TUNE_FORCE_GENERAL 4
#define SHR_TUNE_FWD_WAVES 5  /* waves per forward workgroup, 1..16 */
/* Shares of a crop's work list given to the four wave age groups of a 16-wave
 * workgroup (waves 0-3, 4-7, 8-11, 12-15; the SIMD arbitration favours the oldest):
 * one byte per group, oldest in the low byte, any scale (normalised internally). */
#define SHR_TUNE_FWD_SHARES 6
#define SHR_TUNE_BWD_SHARES 7
#define SHR_TUNE_D2M_WAVES 8       /* waves per workgroup of the data->model kernel: 0 = by batch size, 4, 8 or 16 */
#define SHR_TUNE_PERSISTENT 10     /* sphere rasterizer launches over more crops than the device holds: 0 = one workgroup per
                                    * crop, 1 = persistent workgroups (default), > 1 = that many workgroups */
#define SHR_TUNE_D2M_BAND_UNITS 9  /* 256-pixel units per band handed to a wave: 0 = by crop size */
#define SHR_TUNE_BWD_WAVES 12      /* waves per backward workgroup: 0 = by launch size (8 with half of a CU's LDS when the
                                    * launch has two workgroups per CU, else 16), 8, 16 */
#define SHR_TUNE_MSE_BOX 13        /* fused render-and-compare with the box z-buffer (two workgroups per CU): -1 = by launch
                                    * size, 0 = never, 1 = always (power-of-two images >= 32 wide), > 1 = with that many bytes
                                    * of LDS per workgroup */
#define SHR_TUNE_FWD_ZBUF_BYTES 11  /* forward z-buffer bytes per workgroup: 0 = by launch size (half of a CU's LDS when the
                                    * launch has two workgroups per CU, else one pass for any box); a box that exceeds
                                    * it is rasterized in passes over row bands */
#define SHR_TUNE_FWD_RUN_TABLE 14   /* forward, whole-crop workgroups on power-of-two images: runs on a sphere start from a
                                    * per-(sphere, lane) LDS table built by the idle waves: -1 = when it fits (default),
                                    * 0 = never, 1 = same as -1 */
#define SHR_TUNE_D2M_TILED 15        /* data->model kernel: 1 = units are 32 x 8-pixel tiles and a search is bounded by its
                                    * points' own box (needs W % 4 == 0 and 16-byte aligned images), 0 = 256 consecutive
                                    * pixels per unit and strip bounds (round 2's kernel), -1 = tiles from 192 x 192 pixels
                                    * on (default) */
#define SHR_TUNE_TRI_BAND 16         /* shr_tri_raster_fwd: -1 = the LDS band kernel wherever it fits (default: band height
                                    * and workgroups per crop planned per launch), 0 = always the global-atomic kernel,
                                    * n > 0 = the band kernel with bands of at most n rows */
#define SHR_TUNE_MESH_BAND 17        /* shr_mesh_depth_fwd / shr_mesh_render_fwd at sizes without a lattice kernel whose resize
                                    * samples at least half of the source pixels (S = 256 from 640): 1 = the triangle band
                                    * kernel with clamp + resize as its stream-out (default), 0 = the tile kernel */
#define SHR_TUNE_MESH_LATTICE 18     /* shr_mesh_depth_fwd / shr_mesh_render_fwd / shr_mesh_render_post_fwd at integer resize
                                    * ratios whose sampled pixels fit a 128 x 128 lattice (S = 128 / 64 / 32 from 640): 1 =
                                    * the one-workgroup-per-crop lattice kernel (default), 0 = never (the tile kernel; the
                                    * *_one_launch queries answer 0 and shr_hand_synth_fwd SHR_EINVAL) */
int shr_set_tuning(int key, int value);
/* Self-test: adds to *mismatches (device, caller-zeroed u64) the number of fp32
 * bit patterns in [lo_bits, hi_bits) where the rasterizer's internal square root
 * differs from the correctly rounded one. */
int shr_selftest_sqrt(unsigned lo_bits, unsigned hi_bits,
                      unsigned long long *mismatches, void *stream);
/* Self-test: adds to *mismatches the number of pseudo-random (weights, corner depths) cases -- 4096 x 256 threads x
 * per_thread of them -- for which the triangle kernels' pixel depth with shared reciprocals (tri_face.h tri_pixel_depth)
 * differs in any bit from the reference's seven plain IEEE divisions (.cu:97-110). */
int shr_selftest_division(unsigned seed, unsigned per_thread, unsigned long long *mismatches, void *stream);
/* Measurement hook (bench.py `roofline.launch_floor`, not part of the path): N workgroups of 1024 threads with
 * lds_bytes of dynamic LDS -- the sphere forward's launch shape at one crop per CU -- that only move the forward's
 * bytes: read spheres[N,J,4], write depth[N,H,W] (background) and the owner bytes of rows [row0, row1) of every crop
 * (argmin may be NULL), full-line 16-byte stores.  W % 16 == 0, buffers 16-byte aligned. */
int shr_selftest_launch_floor(const float *spheres, int N, int J, int H, int W, int row0, int row1,
                              float *depth, uint8_t *argmin, int lds_bytes, void *stream);

/* Sphere-set depth rasterizer ------------------------------------------------
 * Replaces BallRender.forward + the min over the sphere axis:
 *   mesh/render.py:26-53 (BallRender), :87-89 (HandBallPrimitiveRender),
 *   mesh/multiview_utility.py:72-76 (MutualProjection).
 * spheres[N,J,4] = (x, y, z, r) per sphere in the TARGET view's frame, mm.
 * depth[N,H,W]   = min_j ( hit_j ? z_j - sqrt(q_j) : 100 ),
 *                  q_j = (r*r - (xg-x)^2) - (yg-y)^2 , hit_j <=> q_j > 0.01f.
 * argmin[N,H,W] (uint8, may be NULL): index of the owning sphere, 255 where
 * the pixel is background.  J <= SHR_MAX_SPHERES.  With J == 1 this IS
 * BallRender.forward (one map per sphere).
 * Bit-exact with the reference's fp32 operation sequence (no FMA contraction,
 * IEEE sqrt). */
int shr_sphere_raster_fwd(const float *spheres, int N, int J, int H, int W,
                          float *depth, uint8_t *argmin, void *stream);
/* The same with `flags` (0 = shr_sphere_raster_fwd).
 * SHR_RASTER_OWNER_TOUCHED_ROWS: argmin is written only on the rows some sphere's pixel box touches; the
 * owner bytes of the other rows (background whatever the depths, half of a hand crop) are left as they were.
 * shr_sphere_raster_bwd never reads them -- it derives the same rows from the same records -- so the
 * autograd pair that replaces mesh/render.py:26-53 + :89 saves a tenth of the forward's stores; a caller that
 * wants the full owner map (the public `argmin` contract above) passes 0.  depth is always complete. */
#define SHR_RASTER_OWNER_TOUCHED_ROWS 1
int shr_sphere_raster_fwd_ex(const float *spheres, int N, int J, int H, int W,
                             float *depth, uint8_t *argmin, int flags, void *stream);

/* Analytic backward of the above (the reference gets it from autograd of
 * mesh/render.py:37-52 + torch.min): for upstream grad_depth[N,H,W],
 *   grad_spheres[N,J,4] = sum over the pixels sphere j owns of
 *     g * ( -(xg-x)/sqrt(q), -(yg-y)/sqrt(q), 1, -r/sqrt(q) ).
 * argmin: the owner map the forward wrote for the SAME spheres (fast path), or
 * NULL to recompute the owners (slower, no saved state needed).
 * Deterministic: fixed-order in-wave reductions, no float atomics. */
int shr_sphere_raster_bwd(const float *spheres, const float *grad_depth,
                          const uint8_t *argmin, int N, int J, int H, int W,
                          float *grad_spheres, void *stream);

/* Data-to-model loss ------------------------------------------------------------
 * Replaces DataToModelLoss.forward (mesh/render.py:123-142) and its autograd
 * backward in ONE pass.  depth[N,H,W] observed depth (background > 99),
 * centres[N,J,3], radii[J].  Per pixel with depth <= 99:
 *   e = min_j | ||(xg,yg,depth) - c_j|| - r_j | , clamped to [0,50].
 * loss_sum[N]: sum of e over the crop's pixels (the reference's scalar is
 *   sum(loss_sum) / (N*H*W)).
 * grad_centres[N,J,3] (may be NULL): d loss_sum[n] / d c_j; the caller scales it
 *   by upstream/(N*H*W).  Deterministic (no atomics). */
int shr_data_to_model(const float *depth, const float *centres, const float *radii,
                      int N, int J, int H, int W, float *loss_sum,
                      float *grad_centres, void *stream);
/* Same, crop n reading the depth image depth + depth_index[n]*H*W: the V*V view pairs
 * of mesh/multiview_utility.py:98-105 share V observed images, the reference's
 * expand().reshape() copy (9x the images) is not needed. */
int shr_data_to_model_indexed(const float *depth, const int32_t *depth_index,
                              const float *centres, const float *radii,
                              int N, int J, int H, int W, float *loss_sum,
                              float *grad_centres, void *stream);
/* The same in `parts` PARTIAL results per crop (1, 2 or 4): crop n's loss sum is
 * loss_parts[n*parts] + ... + loss_parts[n*parts + parts-1], likewise grad_parts[N*parts][J][3] -- large crops
 * are split over several workgroups on different CUs, and the caller adds the partials (fixed order:
 * deterministic).  shr_data_to_model_parts() returns the split this library prefers for a problem size
 * (1 below 192 x 192 pixels, else 2).  depth_index may be NULL (crop n reads image n).  The sums are accumulated
 * as fixed-point integers inside the kernel: a crop's result is bit-reproducible and does not depend on the
 * launch shape. */
int shr_data_to_model_parts(int N, int H, int W);
/* centre_stride: floats between consecutive centres (3, or 4 to read the rasterizer's (x, y, z, r) records in place). */
int shr_data_to_model_partial(const float *depth, const int32_t *depth_index,
                              const float *centres, int centre_stride, const float *radii,
                              int N, int J, int H, int W, int parts, float *loss_parts,
                              float *grad_parts, void *stream);

/* The same loss in TWO STEPS (round 4), for callers that compare one observed image with several sphere sets (the V*V
 * view pairs of mesh/multiview_utility.py:98-105 share V images) -- or that just want the faster path:
 *   shr_data_to_model_compact      every image of depth[M,H,W] once: its foreground pixels (<= 99) as 8-byte (v << 16 | u, depth)
 *                                  records sorted by 16 x 16-pixel tile, into `workspace`
 *                                  (shr_data_to_model_points_bytes(M, H, W) bytes, 16-byte aligned; 0 = image not
 *                                  taken: W % 4 != 0 or more than 2^28 pixels -- use the calls above);
 *   shr_data_to_model_from_points  crop n (sphere set n) against the points of image depth_index[n] (or n; then
 *                                  M == N): loss_parts [N*parts], grad_parts [N*parts][J][3] (may be NULL) exactly
 *                                  as shr_data_to_model_partial returns them, 1 <= parts <= 64.
 * The per-point search is the same code (csrc/d2m_search.h) with a tighter -- still conservative -- bound; the sums
 * are fixed-point integers: for parts = 1 the results are bit-identical to shr_data_to_model's and bit-reproducible.
 * (With parts > 1 a part owns every parts-th group of 256 points of the image's list, whose order follows the arrival
 * of the compaction's workgroups: the PARTIAL sums then vary from run to run, their total only to a float rounding.) */
long long shr_data_to_model_points_bytes(int M, int H, int W);
int shr_data_to_model_compact(const float *depth, int M, int H, int W, void *workspace, void *stream);
int shr_data_to_model_from_points(const void *workspace, int M, const int32_t *depth_index,
                                  const float *centres, int centre_stride, const float *radii,
                                  int N, int J, int H, int W, int parts, float *loss_parts,
                                  float *grad_parts, void *stream);
/* The same with crop n searching with record set centre_index[n] of `centres` (NULL: n): the V same-view pairs of a
 * [B,V,V] batch of projections without gathering their records first (MutualProjectionLoss with is_mv = False,
 * mesh/multiview_utility.py:107-127). */
int shr_data_to_model_from_points_indexed(const void *workspace, int M, const int32_t *depth_index,
                                          const int32_t *centre_index, const float *centres, int centre_stride,
                                          const float *radii, int N, int J, int H, int W, int parts,
                                          float *loss_parts, float *grad_parts, void *stream);

/* The same search in another LAUNCH ORDER: `order` is a permutation of the N record sets, workgroup w searches for set
 * order[w] against image depth_index[w] (the caller permutes that array alike) and writes that set's slots -- the
 * results of shr_data_to_model_from_points bit for bit.  What it is for: XCD placement -- workgroups w, w + 8, ... share
 * an L2, and the V pairs of a multi-view batch that read one image's list belong on one of them, one after the other. */
int shr_data_to_model_from_points_ordered(const void *workspace, int M, const int32_t *depth_index,
                                          const int32_t *order, const float *centres, int centre_stride,
                                          const float *radii, int N, int J, int H, int W, int parts,
                                          float *loss_parts, float *grad_parts, void *stream);

/* Fused render-and-compare: the model->data term of mesh/multiview_utility.py:98-101 and
 * :107-113 (MSELoss(BallRender(...).min(), observed)) with its whole backward, one
 * launch: e = raster(spheres[n]) - target[target_index ? target_index[n] : n],
 *   sse_partial[n*R + r]              = sum of e*e over region r of crop n,
 *   grad_spheres_partial[(n*R+r)*J+j] = d(sum e*e)/d(x, y, z, radius) of sphere j,
 *   depth[N,H,W] (optional, may be NULL) = the rendered depth.
 * R = shr_sphere_raster_mse_regions(H, W) row regions per crop (1 up to 128x128; 0 = image
 * rows too wide for the kernel); the caller sums the R partials (fixed order: deterministic)
 * and applies MSELoss's 1/(N*H*W) and its weights.  Requires W % 4 == 0 and 16-byte
 * aligned spheres / target / depth / grad buffers (SHR_EINVAL otherwise: compose
 * shr_sphere_raster_fwd and _bwd).  Results equal that composition: bit-identical depth,
 * gradients and sums to fp32 summation order. */
int shr_sphere_raster_mse_regions(int H, int W);
int shr_sphere_raster_mse(const float *spheres, int N, int J, int H, int W,
                          const float *target, const int32_t *target_index,
                          float *depth, float *sse_partial,
                          float *grad_spheres_partial, void *stream);
/* The same over a SELECTION of the batch: workgroup n (0 <= n < N) renders crop c = crop_index[n] (NULL: n) -- records
 * spheres[c], observed image target_index[c] (or c), depth[c] when depth is given -- and reports into slot n of
 * sse_partial / grad_spheres_partial ([N][R], [N][R][J][4]).  The same-view pairs of MutualProjectionLoss with
 * is_mv = False (mesh/multiview_utility.py:107-113) out of the [B,V,V] projections, no gather in front. */
int shr_sphere_raster_mse_indexed(const float *spheres, const int32_t *crop_index, int N, int J, int H, int W,
                                  const float *target, const int32_t *target_index, float *depth,
                                  float *sse_partial, float *grad_spheres_partial, void *stream);

/* shr_sphere_raster_mse in another LAUNCH ORDER: `order` is a permutation of the N crops, workgroup w renders crop
 * order[w] and writes that crop's slots of depth / sse_partial / grad_spheres_partial -- the same results bit for bit;
 * the caller places the crops that compare against one observed image on one XCD (workgroups w, w + 8, ...). */
int shr_sphere_raster_mse_ordered(const float *spheres, const int32_t *order, int N, int J, int H, int W,
                                  const float *target, const int32_t *target_index, float *depth,
                                  float *sse_partial, float *grad_spheres_partial, void *stream);

/* CollisionLoss and BoneLengthLoss (mesh/render.py:145-206) on M samples of J sphere centres (sample m at
 * joints + m*sample_stride floats, [J][3]) with their gradients, one launch.  Collision pairs: spheres
 * 0..num_palm-1 (palm) against every finger sphere, and finger spheres of different fingers (finger f =
 * spheres num_palm + f*per_finger ...); hinge relu(min_dist_sq - |c_a - c_b|^2).  Bone pairs (bone_a[k],
 * bone_b[k]), k < K: relu(bone_min_sq[k] - d^2) and relu(d^2 - bone_max_sq[k]).  Outputs per sample: the three
 * sums [M] and the three UNIT gradients [M][J][3]; the caller applies the reference's sum / means and weights. */
int shr_pair_losses(const float *joints, long long sample_stride, int M, int J, int num_palm, int per_finger,
                    float min_dist_sq, const int32_t *bone_a, const int32_t *bone_b,
                    const float *bone_min_sq, const float *bone_max_sq, int K,
                    float *coll_sum, float *bone_lo_sum, float *bone_hi_sum,
                    float *grad_coll, float *grad_bone_lo, float *grad_bone_hi, void *stream);

/* MultiviewConsistencyLoss (mesh/multiview_utility.py:138-167, hm_weight = None) with its gradient: cam [B,V,4,4]
 * (canonical = R joint + t, t in COLUMN 3), joints [B,V,J,3], V <= 8.  loss_sum[b] = sum over views, joints and
 * coordinates of (canonical - median over the views)^2 with torch.median's lower median; grad_joints [B,V,J,3]
 * (may be NULL) = d loss_sum[b] / d joints, the median's gradient routed to the view it was taken from.  The
 * caller applies MSELoss's 1/(B*V*J*3) and the weight. */
int shr_mv_consistency(const float *cam, const float *joints, int B, int V, int J, float *loss_sum,
                       float *grad_joints, void *stream);

/* DepthResample.forward (network/util_modules.py:10-43) on N scaled depth crops: pixels whose uniform[N][H][W]
 * draw exceeds sample_ratio become 1.0, then the module's fixed 3x3 or 5x5 Gaussian with zero padding
 * (out must not alias depth). */
int shr_depth_resample(const float *depth, const float *uniform, int N, int H, int W, float sample_ratio,
                       int kernel_size, float *out, void *stream);

/* Soft-argmax read-out of the network's heat-maps (network/util_modules.py:164-201), forward and
 * backward: hm[N][2J][h][w] fp32 with element (n, c, y, x) at n*stride_n + c*stride_c + (y*w + x)*stride_px
 * (NCHW: stride_c = h*w, stride_px = 1; channels-last: stride_c = 1, stride_px = 2J).  Channels 0..J-1 are
 * the uv heat-maps, J..2J-1 the depth heat-maps.  xyz[N][J][3] = ((u - cx)/fx, (v - cy)/fy, d * depth_scale_inv)
 * with u, v the softmax(20 * uv) expectation of the pixel grid and d the relu-normalised depth.  The backward
 * writes grad_hm in the input's layout (same strides).  _supported: the 2J maps of a sample fit LDS. */
int shr_soft_argmax_supported(int J, int h, int w);
int shr_soft_argmax_fwd(const float *hm, long long stride_n, long long stride_c, long long stride_px,
                        int N, int J, int h, int w, float cx, float cy, float fx, float fy,
                        float depth_scale_inv, float *xyz, void *stream);
int shr_soft_argmax_bwd(const float *hm, long long stride_n, long long stride_c, long long stride_px,
                        int N, int J, int h, int w, float cx, float cy, float fx, float fy,
                        float depth_scale_inv, const float *grad_xyz, float *grad_hm, void *stream);

/* Pointwise tail of the synthetic branch (network/util_modules.py:104-122), forward only.
 * shr_heatmap_paint: HeatmapRender.forward (mesh/render.py:226-248) for BJ = B*J key-points
 *   uvd[BJ][4] = (u, v, depth, w): uv_hm = uv_scale * exp(-0.5*sigma*((u-uj)^2+(v-vj)^2)) on the S x S
 *   grid, d_hm = d_scale * (depth where the Gaussian > 0.05, else 0), and xyz[BJ][4] = K^-1 uvd
 *   (mesh/pointTransformation.py:102-124; a00,a03 / a11,a13 = the non-trivial entries of rows 0 / 1
 *   of K^-1).
 * shr_depth_noise: DepthNoise.forward (network/util_modules.py:46-84): per pixel a rounded source
 *   shift and depth noise on foreground pixels from normal3[3][B][H][W] standard-normal draws
 *   (out must not alias depth). */
int shr_heatmap_paint(const float *uvd, int BJ, int S, float sigma, float uv_scale, float d_scale,
                      float a00, float a03, float a11, float a13,
                      float *uv_hm, float *d_hm, float *xyz, void *stream);
int shr_depth_noise(const float *depth, const float *normal3, int B, int H, int W,
                    float sigma_xy, float sigma_z, float *out, void *stream);

/* HandSynthesizer.forward (network/util_modules.py:104-122) as THREE launches, capturable in a hipGraph -- no host
 * random numbers, no torch launches in between:
 *   shr_synth_pose_fwd        forward kinematics (shr_fk_fwd) + RandScale (mesh/pointTransformation.py:128-148:
 *                             diag(s) T, s_k = rand * rand_scale + 0.90 - rand_scale / 2) + the sample's draws
 *                             draws[6][B] = s_x, s_y, s_z, the focal jitter rand * 0.2 + 0.9 (:110), and the two uint32
 *                             keys of the sample's pixel-noise stream (as float bits);
 *   shr_mesh_render_post_fwd  DepthRender (shr_mesh_render_fwd) + `* depth_scale` + DepthNoise (:46-84) in the
 *                             rasterizer's epilogue; advances the generator's call counter;
 *   shr_heatmap_render_fwd    Hand3DHeatmapRender (mesh/render.py:274-279): key-point skinning + heat-map camera
 *                             (shr_lbs_project on the key-point CSR table kp_start[J+1], kp_bone, kp_wv) + shr_heatmap_paint.
 * Random numbers: rng_state[3] = (seed, call counter, ticket) in device memory; a draw is a hash of (seed, counter, sample,
 * word) and, per pixel, of (sample key, pixel index) -- csrc/common.h rng_*, restated in numpy by
 * spherehand_amd/synth_rng.py.  Parity with the reference's torch generator is in distribution (as for any RNG-
 * dependent step); with the noise off and the same draws the images are the reference chain's bit for bit.
 * One launch at a time per rng_state: launches that share a state must be ordered (one stream, or events) -- the
 * counter is read by every workgroup and advanced by the last one to finish. */
int shr_synth_pose_fwd(const float *params, int B, const float *offset, const float *offset_inv,
                       const unsigned long long *rng_state, float rand_scale, float *T, float *draws, void *stream);
int shr_mesh_render_post_fwd(const float *T, int B, int NB, int NV, const int32_t *skin_vertex_start,
                             const int32_t *skin_bone, const float *skin_wv, int right_hand, float cx, float cy,
                             float fx, float fy, const float *rand_f, const int32_t *faces, int F, int src_size,
                             int S, float clamp_max, float depth_scale, const uint32_t *noise_keys,
                             float sigma_xy, float sigma_z, unsigned long long *rng_state, float *vertices_ws,
                             float *depth_ws, float *depth, void *stream);
int shr_mesh_render_one_launch(int NB, int NV, int F, int src_size, int S);   /* 1: no workspaces needed by the two above */
/* ... and as ONE launch where shr_hand_synth_one_launch() returns 1 (integer resize ratio with a lattice of at most
 * 128 x 128 sampled pixels -- S = 128, 64, 32 from 640 --, NB = 17, J <= 64 key-points, a power-of-two heat-map side):
 * every workgroup runs its crop's forward kinematics + RandScale + draws, skins, rasterizes, scales, noises and paints its
 * heat-maps.  The same bits as the three entries above.  rng_state: uint64 [3] = (seed, call counter, ticket = 0 between
 * launches); noise: 0 / 1; uv_hm = NULL: depth only.  draws[6][B] receives the samples' draws. */
int shr_hand_synth_one_launch(int NB, int NV, int F, int src_size, int S, int J, int hm);
int shr_hand_synth_fwd(const float *params, int B, const float *offset, const float *offset_inv,
                       unsigned long long *rng_state, float rand_scale, int NV,
                       const int32_t *skin_vertex_start, const int32_t *skin_bone, const float *skin_wv,
                       int right_hand, float cx, float cy, float fx, float fy, const int32_t *faces, int F,
                       int src_size, int S, float clamp_max, float depth_scale, int noise, float sigma_xy,
                       float sigma_z, int J, const int32_t *kp_start, const int32_t *kp_bone, const float *kp_wv,
                       int hm, float hcx, float hcy, float hfx, float hfy, float hm_sigma, float uv_scale,
                       float d_scale, float a00, float a03, float a11, float a13, float *draws, float *depth,
                       float *uv_hm, float *d_hm, float *xyz, void *stream);
int shr_heatmap_render_fwd(const float *T, int B, int NB, int J, const int32_t *kp_start, const int32_t *kp_bone,
                           const float *kp_wv, int right_hand, float cx, float cy, float fx, float fy,
                           const float *rand_f, int S, float sigma, float uv_scale, float d_scale, float a00,
                           float a03, float a11, float a13, float *uv_hm, float *d_hm, float *xyz, void *stream);

/* y = relu(GroupNorm(x)) for channels-last (NHWC) fp32 activations x[N][HW][C], forward and
 * backward: the `F.relu(self.bnK(x))` pairs of network/hourglass.py:28-31 without the NCHW
 * round trips of torch's GroupNorm.  G groups of C/G consecutive channels, biased variance,
 * eps inside the root (torch.nn.GroupNorm).  mean / rstd are [N][G] (saved for the backward).
 * The backward returns dx, PER-SAMPLE partials dgamma_partial / dbeta_partial [N][C] and, when
 * dgamma / dbeta [C] are not NULL, their sums over the samples (in order: deterministic).
 * shr_group_norm_relu_supported: C % 32 == 0 and C/G in
 * {4, 8, 16, 32}; buffers 16-byte aligned. */
int shr_group_norm_relu_supported(int C, int G);
/* pre_bias [C] (may be NULL): the bias of the convolution that produced x, added on the fly (y = relu(GN(x +
 * pre_bias))): the convolution then runs without its bias-add pass and the backward returns that bias's
 * gradient (dpre [C], per-sample partials dpre_partial [N][C]; both NULL when pre_bias is) with dx, instead of
 * a separate reduction over dx. */
int shr_group_norm_relu_fwd(const float *x, const float *pre_bias, const float *gamma, const float *beta,
                            int N, int C, int HW, int G, float eps,
                            float *y, float *mean, float *rstd, void *stream);
int shr_group_norm_relu_bwd(const float *x, const float *pre_bias, const float *dy, const float *gamma,
                            const float *beta, const float *mean, const float *rstd,
                            int N, int C, int HW, int G, float *dx,
                            float *dgamma_partial, float *dbeta_partial, float *dpre_partial,
                            float *dgamma, float *dbeta, float *dpre, void *stream);
/* The same pair for bf16 activations: x, y, dy and dx are bf16 (uint16_t: the upper half of the fp32 pattern),
 * x[N][HW][C] channels-last; pre_bias, gamma, beta, mean, rstd and every partial and parameter gradient stay fp32.
 * Every element is widened exactly and all arithmetic is the fp32 entries', in their order; the one added rounding
 * is the store of y and of dx, round-to-nearest-even.  Same supported (C, G) set, same argument rules and codes
 * (SHR_EINVAL: NULL, unsupported (C, G), a buffer off 16 bytes; SHR_ETOOLARGE: N > 65535). */
int shr_group_norm_relu_bf16_fwd(const uint16_t *x, const float *pre_bias, const float *gamma, const float *beta,
                                 int N, int C, int HW, int G, float eps,
                                 uint16_t *y, float *mean, float *rstd, void *stream);
int shr_group_norm_relu_bf16_bwd(const uint16_t *x, const float *pre_bias, const uint16_t *dy, const float *gamma,
                                 const float *beta, const float *mean, const float *rstd,
                                 int N, int C, int HW, int G, uint16_t *dx,
                                 float *dgamma_partial, float *dbeta_partial, float *dpre_partial,
                                 float *dgamma, float *dbeta, float *dpre, void *stream);


/* View-to-view projection of the sphere centres ---------------------------------
 * Replaces MutualTransformation + the projection in MutualProjection.forward
 * (mesh/multiview_utility.py:13-30, :62-72).  cam, inv_cam [B,V,4,4] (row-major,
 * p' = R p + t with t in COLUMN 3, as the reference reads them), joints [B,V,J,3],
 * radii [J].  spheres[B,V,V,J,4]: entry (b,i,j,k) = view-i joint k expressed in
 * view j, with its radius: the sphere records the rasterizer takes (N = B*V*V). */
int shr_mutual_project_fwd(const float *cam, const float *inv_cam, const float *joints,
                           const float *radii, int B, int V, int J, float *spheres,
                           void *stream);
/* The two preparations of MutualProjectionLoss (mesh/multiview_utility.py:90-105) in TWO launches instead of three:
 * shr_mutual_project_fwd (which also clears the point lists' fill counters) followed by the compaction of
 * shr_data_to_model_compact(depth[M,H,W] -> workspace) without its memset.  Same results as the two calls. */
int shr_mv_project_compact(const float *cam, const float *inv_cam, const float *joints,
                           const float *radii, int B, int V, int J, float *spheres,
                           const float *depth, int M, int H, int W, void *workspace, void *stream);
/* Assembly of MutualProjectionLoss (mesh/multiview_utility.py:98-129) and of its backward from the partial results
 * of shr_sphere_raster_mse (sse_part [N][Rm], grad_spheres_part [N][Rm][J][4], N = B*V*V pairs) and of
 * shr_data_to_model_partial (d2m_part [E][Rd], grad_d2m_part [E][Rd][J][3]; E = N pairs when is_mv, else the B*V
 * same-view pairs, entry b*V+i):
 *   loss[0] = 9 MSE + d2m_weight * 9 d2m over all pairs (is_mv), or 3 x the same over the V same-view pairs,
 *   grad_joints[B,V,J,3] (may be NULL) = d loss / d joints (both sphere gradients weighted, added and pulled back
 *   through the detached view transforms).  fp64 accumulation of the scalar in a fixed order: deterministic.
 * is_mv: 1 = all pairs; 0 = the same-view pairs, picked out of sse_part / grad_spheres_part of all N pairs; 2 = the
 * same-view pairs with sse_part [B*V][Rm] / grad_spheres_part [B*V][Rm][J][4] holding those pairs only (entry b*V+i:
 * the caller ran shr_sphere_raster_mse on them alone) -- same values as 0.
 * Limits: V <= 8 (the pairs of a view are summed by a 4- or 8-lane butterfly; SHR_ETOOLARGE beyond -- the reference
 * runs V = 3, mesh/multiview_utility.py:107), 4*B*V*V*J*max(Rm,Rd) below 2^31 (SHR_ETOOLARGE). */
int shr_mv_loss_combine(const float *cam, const float *inv_cam, const float *sse_part,
                        const float *grad_spheres_part, int Rm, const float *d2m_part,
                        const float *grad_d2m_part, int Rd, int B, int V, int J, int H, int W, int is_mv,
                        float d2m_weight, float *loss, float *grad_joints, void *stream);
/* grad_joints[B,V,J,3] = sum_j R(b,i,j)^T grad_spheres[b,i,j,k].xyz (the view
 * transforms are constants: detached at mesh/multiview_utility.py:68). */
int shr_mutual_project_bwd(const float *cam, const float *inv_cam, const float *grad_spheres,
                           int B, int V, int J, float *grad_joints, void *stream);

/* Triangle-mesh depth rasterizer (forward only) -----------------------------------
 * Replaces depth_rasterization.forward(width, height, vertices)
 * (mesh/cuda_kernel/depth_rasterization_cuda.cpp:15-25 ->
 *  depth_rasterization_cuda_kernel.cu:115-134, kernel :18-113).
 * face_vertices[B,F,3,3] = pixel-space (x, y, z) of each face's three vertices;
 * depth[B,H,W] is initialised to 1000 and receives, per covered pixel, the
 * minimum over faces of the 1/z-interpolated depth.  Coverage (back-face cull,
 * per-column spans with their truncation quirks) and arithmetic follow the
 * reference kernel; the result is order independent (integer atomics on the fp32
 * bits).  depth 16-byte aligned; W, H <= 65535 (SHR_ETOOLARGE beyond). */
int shr_tri_raster_fwd(const float *face_vertices, int B, int F, int W, int H,
                       float *depth, void *stream);
/* Same, with the face gather of DepthRasterization.forward (mesh/render.py:308-309)
 * fused: vertices[B,NV,4] (x,y,z,w) + faces[F,3] vertex indices (winding already
 * swapped for the right hand, mesh/render.py:298-300). */
int shr_tri_raster_indexed_fwd(const float *vertices, const int32_t *faces, int B,
                               int NV, int F, int W, int H, float *depth, void *stream);

/* Fused DepthRender back end: raster + clamp(max) + bilinear resize src_size -> S, touching
 * only the source pixels the resize reads.  Replaces the chain
 * DepthRasterizationFunction.apply(640,640,...) / clamp / F.interpolate of
 * mesh/render.py:284-287, :310-311.  vertices[B,NV,4] in src_size pixel space, faces[F,3]
 * (winding already swapped for the right hand).  depth[B,S,S].  Needs S <= src_size
 * (no up-sampling; S == src_size is the clamped raster itself). */
int shr_mesh_depth_fwd(const float *vertices, const int32_t *faces, int B, int NV, int F,
                       int src_size, int S, float clamp_max, float *depth, void *stream);

/* Skinning + orthographic camera -----------------------------------------------------
 * Replaces LinearBlendSkinning.forward (mesh/pointTransformation.py:39-46) and
 * OthographicalProjection.forward (:84-99).  T[B,NB,4,4]; the skin table is CSR by
 * vertex (skin_vertex_start[NV+1], skin_bone[NS], skin_wv[NS,4] = fp32(weight *
 * vertex) as the reference stores it, :31), bones ascending within a vertex.
 * right_hand: negate x (:44-45).  project: 0 = skinned points only; 1 = apply the
 * camera u = fx*x + cx*w, v = fy*y + cy*w (rand_f NULL, :88-89) or
 * u = x*rand_f[b]*fx + cx, ..., w = 1 (rand_f given, :91-97).  out[B,NV,4]. */
int shr_lbs_project(const float *T, int B, int NB, int NV, const int32_t *skin_vertex_start,
                    const int32_t *skin_bone, const float *skin_wv, int right_hand,
                    int project, float cx, float cy, float fx, float fy,
                    const float *rand_f, float *out, void *stream);

/* DepthRender.forward (mesh/render.py:315-331: LinearBlendSkinning -> OthographicalProjection -> DepthRasterization ->
 * clamp -> resize) in ONE launch where the resize ratio src_size / S is an integer and the sampled source pixels form a
 * lattice of at most 128 x 128 (S = 128, 64, 32 from 640): every workgroup skins and projects its crop's vertices into
 * LDS (shr_lbs_project's arguments and arithmetic, project = 1) and rasterizes from there (shr_mesh_depth_fwd's
 * arguments).  Any other size: the two launches through vertices_ws[B,NV,4] (16-byte aligned; may be NULL when the
 * caller knows the fused kernel applies -- SHR_EINVAL otherwise).  The images are the same bits either way. */
int shr_mesh_render_fwd(const float *T, int B, int NB, int NV, const int32_t *skin_vertex_start,
                        const int32_t *skin_bone, const float *skin_wv, int right_hand, float cx, float cy,
                        float fx, float fy, const float *rand_f, const int32_t *faces, int F, int src_size,
                        int S, float clamp_max, float *vertices_ws, float *depth, void *stream);

/* Differentiable DepthRender / DepthRasterization (the reference defines no backward for the mesh path,
 * mesh/render.py:282-287).  The gradient routes to each bilinear tap's OWNER face and holds coverage fixed, as the sphere
 * backward does: no edge, silhouette or visibility terms.  Square S <= src_size / 2 only (SHR_ETOOLARGE otherwise).
 *   shr_mesh_depth_owner_fwd   shr_mesh_depth_fwd's arguments and depth[B,S,S] bits, plus owner[B,S,S,4] int32 (16-byte
 *                              aligned): the face of each of the output pixel's four ATen taps (y0x0, y0x1, y1x0, y1x1) --
 *                              the smallest offered depth at that source pixel of the raster (.cu:97-110), ties to the
 *                              smallest face index; -1 for background, zero-weight taps and taps whose raw depth is above
 *                              clamp_max (mesh/render.py:286: torch's clamp passes the gradient at equality).
 *   shr_mesh_depth_bwd         grad_depth[B,S,S] + the owners + vertices[B,NV,4] (the forward's) -> grad_vertices[B,NV,4] =
 *                              (d/du, d/dv, d/dz, 0): per tap, bilinear weight x d zp / d (the owner's three corners) of
 *                              .cu:57-110 (a weight clamped strictly outside [0, 1] contributes nothing).  64-bit
 *                              fixed-point sums in a per-crop unit computed on the device: bitwise reproducible,
 *                              independent of the batch, no host synchronisation.  workspace: 16-byte aligned,
 *                              shr_mesh_depth_bwd_workspace_bytes(B, NV) bytes, cleared by the call itself.
 *   shr_lbs_project_bwd        shr_lbs_project's backward (project = 1, mesh/pointTransformation.py:39-46, :84-99):
 *                              grad_vertices[B,NV,4] -> grad_T[B,NB,4,4]; rand_f gets no gradient.  Fixed summation
 *                              order (bitwise reproducible, independent of the batch). */
int shr_mesh_depth_owner_fwd(const float *vertices, const int32_t *faces, int B, int NV, int F, int src_size, int S,
                             float clamp_max, float *depth, int32_t *owner, void *stream);
long long shr_mesh_depth_bwd_workspace_bytes(int B, int NV);
int shr_mesh_depth_bwd(const float *vertices, const int32_t *faces, const int32_t *owner, const float *grad_depth, int B,
                       int NV, int F, int src_size, int S, float *grad_vertices, void *workspace, void *stream);
int shr_lbs_project_bwd(const float *grad_vertices, int B, int NB, int NV, const int32_t *skin_vertex_start,
                        const int32_t *skin_bone, const float *skin_wv, int right_hand, float cx, float cy, float fx,
                        float fy, const float *rand_f, float *grad_T, void *stream);

/* Differentiable triangle raster at its own resolution: depth_rasterization.forward(width, height, face_vertices)
 * (mesh/cuda_kernel/depth_rasterization_cuda.cpp:15-25 -> depth_rasterization_cuda_kernel.cu:115-134, kernel :18-113),
 * which the reference ships forward-only, with a backward at any W x H.  The contract is shr_mesh_depth_bwd's: each
 * pixel's gradient goes to the face that OWNS its raw depth, coverage held fixed (no edge, silhouette or visibility
 * terms).  Callers clamp in torch (mesh/render.py:286-287).
 *   shr_tri_raster_owner_fwd / shr_tri_raster_indexed_owner_fwd
 *       shr_tri_raster_fwd's / shr_tri_raster_indexed_fwd's arguments, limits and depth[B,H,W] bits, plus owner[B,H,W]
 *       int32 (16-byte aligned): the face with the smallest offered depth at the pixel (.cu:97-110), ties to the smaller
 *       face index; -1 where no face offered a depth (the background, 1000).
 *   shr_tri_raster_bwd            grad_depth[B,H,W] + the owners + face_vertices[B,F,3,3] (the forward's) ->
 *                                 grad_face_vertices[B,F,3,3]: d/d(x, y, z) of every corner.
 *   shr_tri_raster_indexed_bwd    the same for vertices[B,NV,4] + faces[F,3] -> grad_vertices[B,NV,4] = (d/du, d/dv, d/dz, 0).
 *       Per owned pixel, d zp / d (the owner's three corners) of .cu:57-110 at the integer pixel (a weight clamped strictly
 *       outside [0, 1] contributes nothing), shr_mesh_depth_bwd's arithmetic with one tap of weight 1.  64-bit fixed-point
 *       sums in a per-crop unit computed on the device: bitwise reproducible, independent of the batch, no host
 *       synchronisation.  workspace: 16-byte aligned, shr_tri_raster_bwd_workspace_bytes(B, F) /
 *       shr_tri_raster_indexed_bwd_workspace_bytes(B, NV) bytes, cleared by the call itself.  Owners outside [0, F) are
 *       skipped.  B <= 65535 (SHR_ETOOLARGE beyond). */
int shr_tri_raster_owner_fwd(const float *face_vertices, int B, int F, int W, int H, float *depth, int32_t *owner,
                             void *stream);
int shr_tri_raster_indexed_owner_fwd(const float *vertices, const int32_t *faces, int B, int NV, int F, int W, int H,
                                     float *depth, int32_t *owner, void *stream);
long long shr_tri_raster_bwd_workspace_bytes(int B, int F);
long long shr_tri_raster_indexed_bwd_workspace_bytes(int B, int NV);
int shr_tri_raster_bwd(const float *face_vertices, const int32_t *owner, const float *grad_depth, int B, int F, int W,
                       int H, float *grad_face_vertices, void *workspace, void *stream);
int shr_tri_raster_indexed_bwd(const float *vertices, const int32_t *faces, const int32_t *owner, const float *grad_depth,
                               int B, int NV, int F, int W, int H, float *grad_vertices, void *workspace, void *stream);

/* Antialias pass of the triangle raster (a capability the reference does not have; the edge-blending step of modular
 * differentiable rasterizers): a crop's values blended across the silhouette edges of the faces that own its pixels, so
 * that the output is continuous in the vertices' x, y and has a gradient at the outline.  The hard raster is unchanged.
 * Pixel (x, y) is sampled at integer (x, y), x = column, y = row; smaller depth is nearer.  Per crop b:
 *   values c[B,H,W]       what is antialiased (e.g. clamp(raw, max=100) or a 0/1 coverage mask)
 *   depth d[B,H,W], owner[B,H,W]   the raw depth and owners of shr_tri_raster_indexed_owner_fwd (-1: background)
 *   vertices[B,NV,4]      pixel-space (x, y, z, -), 16-byte aligned; faces[F,3] as the raster took them
 *   edges[F,3]            edge k of face f joins corners k and (k + 1) % 3; edges[f,k] is the other face that shares this
 *                         undirected edge (corners matched on welded ids), -1 when none or when three or more share it.
 *                         Values outside [0, F) count as -1.  (ops.tri_edge_table builds it on the host.)
 * A face is DRAWN when face_sort accepts it: front-facing by the reference's cull (.cu:33) and x0 != x2 (.cu:54), its
 * vertex ids inside [0, NV).  Edge k of a drawn face t is a SILHOUETTE edge when edges[t,k] == -1 or the face across it
 * is not drawn.
 * PAIRS: every 4-neighbour pair inside the image, (p, p + (1, 0)) and (p, p + (0, 1)), with owner(p) != owner(q):
 *   1. the front pixel f is the one with owner >= 0 and the smaller raw depth (equal depth bits: p); o is the other,
 *      sigma = +-1 the sign of the step from f to o along the pair's axis, t = owner(f) (outside [0, F): no blend).
 *   2. edge A -> B of t qualifies when it is a silhouette edge, and, for a horizontal pair at row y:
 *      |y_B - y_A| >= |x_B - x_A|, y_A != y_B, min(y_A, y_B) <= y <= max(y_A, y_B), and the crossing
 *          x_c = x_A + ((y - y_A) * (x_B - x_A)) / (y_B - y_A)            (fp32, in this order)
 *      gives s = sigma (x_c - x_f) with 0 <= s <= 1.  A vertical pair at column x: the same with x and y swapped and the
 *      strict |x_B - x_A| > |y_B - y_A|, so that each edge blends along one axis only.  The smallest qualifying k wins.
 *   3. with a qualifying edge: s >= 1/2: o gains (s - 1/2)(c_f - c_o); s < 1/2: f gains (1/2 - s)(c_o - c_f).  Gains
 *      are computed from the input values only.
 *   out[p] = (((c[p] + gain_left) + gain_right) + gain_up) + gain_down in fp32, over the pairs (p - (1, 0), p),
 *   (p, p + (1, 0)), (p - (0, 1), p), (p, p + (0, 1)) in which p gains; a pixel that gains nothing is a bitwise copy.
 *   shr_tri_antialias_fwd   -> out[B,H,W] (not aliasing values)
 *   shr_tri_antialias_bwd   grad_out[B,H,W] -> grad_values[B,H,W] and grad_vertices[B,NV,4] = (d/dx, d/dy, 0, 0); either
 *       output may be NULL (not both).  Both branches of 3. give d gain / d s = c_f - c_o; for a horizontal pair, with
 *       u = (y - y_A) / (y_B - y_A) and m = (x_B - x_A) / (y_B - y_A), ds/dx_A = sigma (1 - u), ds/dx_B = sigma u,
 *       ds/dy_A = -sigma m (1 - u), ds/dy_B = -sigma m u (vertical pairs: x and y swapped); no gradient to depth, owner
 *       or z.  grad_values is a per-pixel gather in the forward's order: grad_out[p] + sum over p's qualifying pairs of
 *       grad_out[gaining pixel] * (p == f ? s - 1/2 : 1/2 - s).  The vertex terms go to faces[t,k] and faces[t,(k+1)%3]
 *       in shr_tri_raster_indexed_bwd's 64-bit fixed point (a per-crop unit computed on the device): bitwise
 *       reproducible, independent of the batch, no host synchronisation.  workspace: 16-byte aligned,
 *       shr_tri_antialias_bwd_workspace_bytes(B, NV) bytes (only with grad_vertices), cleared by the call itself.
 *   B, W, H <= 65535 (SHR_ETOOLARGE beyond). */
int shr_tri_antialias_fwd(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                          const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H, float *out,
                          void *stream);
long long shr_tri_antialias_bwd_workspace_bytes(int B, int NV);
int shr_tri_antialias_bwd(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                          const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H,
                          const float *grad_out, float *grad_values, float *grad_vertices, void *workspace, void *stream);

/* The antialias pass over multi-channel maps: values[B,C,H,W] (shr_tri_interp_fwd's maps) -> out[B,C,H,W], every channel
 * plane blended as shr_tri_antialias_fwd blends one plane.  depth, owner, vertices, faces and edges as there.  The
 * PAIRS, the front pixel, the silhouette edges, the qualifying edge and s are word for word shr_tri_antialias_fwd's:
 * they do not depend on the values, so there is one decision per pair, shared by all channels.
 *   shr_tri_antialias_maps_fwd   for every channel ch, out[b,ch] is shr_tri_antialias_fwd's output for values[b,ch]:
 *       the same fp32 expression in the same order (left, right, up, down), gains computed from the input values only
 *       (out must not overlap values: SHR_EINVAL); a pixel that gains nothing is a bitwise copy in every channel.
 *   shr_tri_antialias_maps_bwd   grad_out[B,C,H,W] -> grad_values[B,C,H,W] and grad_vertices[B,NV,4] = (d/dx, d/dy, 0,
 *       0); either output may be NULL (not both).  grad_values[b,ch] is shr_tri_antialias_bwd's gather of grad_out[b,ch].
 *       The vertex terms are shr_tri_antialias_bwd's with
 *           gw = sum_ch grad_out[b,ch,gaining pixel] * (c_f[ch] - c_o[ch])        (fp64, ch ascending)
 *       in place of the single plane's product (at C = 1 the same bits): one term per coordinate per pair to
 *       faces[t,k] and faces[t,(k+1)%3], in the same 64-bit fixed point with the same bit bound -- bitwise
 *       reproducible, independent of the batch, no host synchronisation.  No gradient to depth, owner or z.
 *       workspace: 16-byte aligned, shr_tri_antialias_maps_bwd_workspace_bytes(B, NV) bytes (only with grad_vertices;
 *       equal to shr_tri_antialias_bwd_workspace_bytes(B, NV)), cleared by the call itself.
 *   1 <= C <= 64 as shr_tri_interp_fwd (C <= 0: SHR_EINVAL; beyond 64: SHR_ETOOLARGE); B, W, H <= 65535
 *   (SHR_ETOOLARGE beyond); B == 0 is a no-op; NULLs and misaligned vertices / grad_vertices / workspace: SHR_EINVAL. */
int shr_tri_antialias_maps_fwd(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                               const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H, int C,
                               float *out, void *stream);
long long shr_tri_antialias_maps_bwd_workspace_bytes(int B, int NV);
int shr_tri_antialias_maps_bwd(const float *values, const float *depth, const int32_t *owner, const float *vertices,
                               const int32_t *faces, const int32_t *edges, int B, int NV, int F, int W, int H, int C,
                               const float *grad_out, float *grad_values, float *grad_vertices, void *workspace,
                               void *stream);

/* Vertex-attribute interpolation over the owner map (a capability the reference does not have; the interpolation step
 * of modular differentiable rasterizers): per-vertex attributes -> per-pixel maps through the faces that own the
 * pixels, with the weights the raster's depth used there.  Per crop b:
 *   owner[B,H,W]        shr_tri_raster_indexed_owner_fwd's owners (-1: background)
 *   vertices[B,NV,4]    pixel-space (x, y, z, -), 16-byte aligned; faces[F,3] as the raster took them
 *   attr                [B,NV,C] with attr_batch_stride = NV * C, or [NV,C] shared by all crops with
 *                       attr_batch_stride = 0 (any other stride: SHR_EINVAL).  1 <= C <= 64 (SHR_ETOOLARGE beyond).
 * Pixel (x, y), sampled at integer (x, y), with t = owner >= 0, t < F and face t's vertex ids inside [0, NV) (anything
 * else counts as background), in fp32 with one rounding per written operator:
 *   1. the reference's set-up on face t's corners in the faces' own order (.cu:33-66, :97-103): the corners sorted by
 *      x -> p[0..2], sorted corner k being corner order[k] of the face; fi = the inverse barycentric matrix of p (nine
 *      IEEE divisions by den); w_k = (fi[3k] * x + fi[3k+1] * y) + fi[3k+2]; c_k = min(max(w_k, 0), 1) (a NaN clamps
 *      to 0); s = (c_0 + c_1) + c_2 -- exactly the values the raster's depth used at this pixel.
 *   2. wh_k = c_k / s (IEEE division, the raster's w / w_sum).
 *   3. out[b,ch,y,x] = (wh_0 * a_0[ch] + wh_1 * a_1[ch]) + wh_2 * a_2[ch], a_k the attribute row of vertex
 *      faces[t, order[k]].  Background pixels, and pixels where s is 0 or not finite, get 0.
 * These are the screen-linear weights, not the raster's 1 / sum_k wh_k / z_k form: the camera is orthographic.
 *   shr_tri_interp_fwd   -> out[B,C,H,W]; no workspace.
 *   shr_tri_interp_bwd   grad_out[B,C,H,W] -> grad_attr[B,NV,C] (per crop also for shared attributes: the caller sums
 *       over b) and grad_vertices[B,NV,4] = (d/dx, d/dy, 0, 0); either output may be NULL (not both).
 *       shr_mesh_depth_bwd's rule: the clamp decisions are step 1's fp32 values, a weight strictly outside [0, 1] is a
 *       constant, coverage and owner are held fixed; no gradient to z or owner.  With the weights re-evaluated in fp64
 *       from the fp32 corners (c_k = w_k where the fp32 w_k lies inside [0, 1], else the fp32 c_k):
 *         grad_attr[b, faces[t,order[k]], ch] += wh_k * grad_out[b,ch,y,x];
 *         grad_vertices: with g_k = sum_ch grad_out[ch] * a_k[ch] (ch ascending), the derivative of sum_k g_k wh_k with
 *         respect to the three corners' x, y:  d / d c_a = (g_a - sum_k g_k wh_k) / s,  d w_a = (d n_a - w_a d den) / den.
 *       Both sums are 64-bit fixed point in a per-crop unit computed on the device from the crop's largest term (one
 *       unit for the vertex part, one for the attribute part; at most 3 W H terms per accumulator): bitwise
 *       reproducible, independent of the batch and of the launch shape, no host synchronisation.  workspace: 16-byte
 *       aligned, shr_tri_interp_bwd_workspace_bytes(B, NV, C, want_attr, want_vertices) bytes for the requested parts
 *       (-1 on a negative size), cleared by the call itself.
 *   B, W, H <= 65535 and, for the backward, B * ceil(C / 3) <= 65535 (SHR_ETOOLARGE beyond). */
int shr_tri_interp_fwd(const int32_t *owner, const float *vertices, const int32_t *faces, const float *attr,
                       long long attr_batch_stride, int B, int NV, int F, int W, int H, int C, float *out, void *stream);
long long shr_tri_interp_bwd_workspace_bytes(int B, int NV, int C, int want_attr, int want_vertices);
int shr_tri_interp_bwd(const int32_t *owner, const float *vertices, const int32_t *faces, const float *attr,
                       long long attr_batch_stride, int B, int NV, int F, int W, int H, int C, const float *grad_out,
                       float *grad_attr, float *grad_vertices, void *workspace, void *stream);

/* Vertex normals of an indexed mesh and unit normalisation of three-plane maps (a capability the reference does not
 * have; with shr_tri_interp_fwd they give a normal map).  Per crop b:
 *   points[B,NV,4]   fp32 (x, y, z, -), 16-byte aligned: the raster's vertex layout (shr_lbs_project's output as it is);
 *                    the fourth component is ignored and gets zero gradient
 *   faces[F,3]       as the raster takes them (after the right hand's winding swap)
 *   the tables       built once on the host (ops.tri_vertex_tables), all int32; a CORNER is the integer 3 f + k, corner k
 *                    of face f; faces with a vertex id outside [0, NV) appear in no table
 *     point[NV]                        vertex -> welded point id in [0, NP)
 *     inc_start[NP+1], inc[NI]         welded incidence (CSR by point): the corners whose vertex welds to the point, ascending
 *     copy_start[NP+1], copy[NV]       the copies of each point (CSR by point): the vertices that weld to it, ascending
 *     own_start[NV+1], own[NO]         own-id incidence (CSR by vertex): the corners with faces[f,k] == v, ascending
 *   Without welding NP = NV, point and copy are the identity and inc == own.  Entries out of range are skipped.
 * In fp32 with one rounding per written operator (no contraction):
 *   1. face normal, area-weighted, corners p0, p1, p2 in the order of faces[f]:  e1 = p1 - p0, e2 = p2 - p0,
 *      n_f = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x).
 *   2. N_v = sum of n_f over the corners of inc for v's point, in ascending corner order (a face with two corners on the
 *      point counts twice): one add per term, starting FROM the first term; no corner: N = 0.  The sum is evaluated once
 *      per point and stored to its copies: copies of a point get identical bits.
 *   3. unit3:  s = (Nx Nx + Ny Ny) + Nz Nz;  s > 0 and finite:  n = N / sqrt(s), the IEEE square root and three IEEE
 *      divisions;  otherwise n = (0, 0, 0) and nothing flows back through it (the ZERO RULE).  NaN and infinite inputs
 *      give 0 (n) or NaN / inf (N), never a fault.
 *   shr_tri_vertex_normals_fwd   -> normals[B,NV,4] = (n, 0) and, when raw is not NULL, raw[B,NV,4] = (N, 0); both
 *       16-byte aligned.  No flip: the normals are those of the faces' own winding.  The raster's cull (.cu:33) draws a
 *       face when (y2 - y0)(x1 - x0) >= (y1 - y0)(x2 - x0), which is n_f.z >= 0: drawn faces point AWAY from the camera
 *       in this convention (smaller depth is nearer).  render.MeshNormalRaster turns them by building its tables from
 *       the faces with corners 1 and 2 exchanged, which negates every n_f exactly (a b - c d = -(c d - a b) in IEEE).
 *   shr_tri_vertex_normals_bwd   grad_normals[B,NV,4] (the fourth component is not read) -> grad_points[B,NV,4] =
 *       (d/dx, d/dy, d/dz, 0): the exact derivative of 1 .. 3 with the zero rule's fp32 decision held fixed, evaluated in
 *       fp64 from the fp32 points by two gathers in fixed order, no atomics:
 *         per welded point p:  g = sum of grad_normals over copy (ascending);  N, n = N / |N| in fp64 (N summed as in 2.);
 *             G_p = (g - n (n . g)) / |N|   (0 under the zero rule, or when the fp64 |N|^2 is 0 or not finite)
 *         per vertex v:  over own (ascending), with H_f = (G_point(c0) + G_point(c1)) + G_point(c2):
 *             corner 1: e2 x H_f;  corner 2: H_f x e1;  corner 0: -(both);  one rounding to fp32 at the end.
 *       The gradients land on faces[f,k], the positions that were read.  Bitwise reproducible, independent of B and of
 *       the launch shape, no host synchronisation.  workspace: 16-byte aligned,
 *       shr_tri_vertex_normals_bwd_workspace_bytes(B, NP) bytes (-1 on a negative size), fully written by the call.
 *   shr_unit3_maps_fwd   maps[B,3,H,W] -> out[B,3,H,W]: step 3 on every pixel's three planes (the same device function;
 *       a background pixel, all planes 0, stays 0).  One read and one write of the planes.  out must not overlap maps
 *       (SHR_EINVAL).
 *   shr_unit3_maps_bwd   grad_out[B,3,H,W] -> grad_maps[B,3,H,W] = (g - o (o . g)) / |m|, o = m / |m| in fp64 from the
 *       fp32 m, one rounding; 0 under the zero rule.  grad_maps must not overlap maps (it may be grad_out).
 *   B, W, H <= 65535 (SHR_ETOOLARGE beyond); B == 0 is a no-op; NULLs and misaligned points / normals / raw / gradients /
 *   workspace: SHR_EINVAL. */
int shr_tri_vertex_normals_fwd(const float *points, const int32_t *faces, const int32_t *point, const int32_t *inc_start,
                               const int32_t *inc, const int32_t *copy_start, const int32_t *copy, int B, int NV, int F,
                               int NP, int NI, float *normals, float *raw, void *stream);
long long shr_tri_vertex_normals_bwd_workspace_bytes(int B, int NP);
int shr_tri_vertex_normals_bwd(const float *points, const int32_t *faces, const int32_t *point, const int32_t *inc_start,
                               const int32_t *inc, const int32_t *copy_start, const int32_t *copy, const int32_t *own_start,
                               const int32_t *own, int B, int NV, int F, int NP, int NI, int NO, const float *grad_normals,
                               float *grad_points, void *workspace, void *stream);
int shr_unit3_maps_fwd(const float *maps, int B, int W, int H, float *out, void *stream);
int shr_unit3_maps_bwd(const float *maps, const float *grad_out, int B, int W, int H, float *grad_maps, void *stream);

/* Silhouette distance: the exact squared Euclidean distance transform of an image's foreground, and its bilinear
 * sampler at points (a capability the reference does not have: a term that pulls a model point towards the observed
 * silhouette from any distance).  Pixel (row i, column j) is the point (x = j, y = i): the sample points the triangle
 * raster tests (tri_face.h: span_rows evaluates column xi at xf = (float)xi, pixel_weights row yi at yf = (float)yi), so
 * projected vertices, sphere centres and key points are sampled as they are.
 *   shr_dt_fwd   depth[B,H,W] fp32 -> d2[B,H,W] int32.  A pixel is a SITE iff depth < fg_max (a NaN depth is not a site;
 *       a NaN fg_max makes none).  d2[b,i,j] = min over the sites (i', j') of image b of (i - i')^2 + (j - j')^2; an image
 *       without a site gets H H + W W everywhere, above the largest real value (H-1)^2 + (W-1)^2 and finite.  Integer
 *       arithmetic only: exact, independent of B and of the launch shape; no atomics, no host synchronisation, no
 *       allocation.  1 <= H, W <= 2048 (every d2 < 2^24 converts to fp32 exactly) and B <= 65535: SHR_ETOOLARGE beyond.
 *       workspace: 16-byte aligned, shr_dt_workspace_bytes(B, H, W) bytes (-1 on a negative size), every element that is
 *       read is written by the call first.  It holds g[B][H][ceil(W/2)][2] uint16, the vertical distance of each pixel to
 *       its column's nearest site (0xffff: the column has none).  B == 0 is a no-op; NULL or misaligned depth / d2 /
 *       workspace: SHR_EINVAL.
 *   shr_dt_sample_fwd   points[B,N,C] fp32, C >= 2, (x, y) first ([B,NV,4] vertices pass as they are); H, W >= 2;
 *       max_dist >= 0, +inf allowed (SHR_EINVAL otherwise).  Per point, in fp32 with one rounding per written operation:
 *         1. x or y not finite:  value 0, gradient (0, 0).
 *         2. xc = min(max(x, 0), W-1);  x0 = min(floor(xc), W-2);  fx = xc - x0;  the same for y with H.
 *         3. taps t = min(sqrt((float)d2), max_dist) (the IEEE root) at (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1).
 *         4. top = t00 (1-fx) + t01 fx;  bot = t10 (1-fx) + t11 fx;  value = top (1-fy) + bot fy.
 *         5. gx = (t01-t00) (1-fy) + (t11-t10) fy;  gy = bot - top.
 *         6. a component whose coordinate was clamped in 2. (xc != x) gets gradient 0.
 *       -> value[B,N] and grad_xy[B,N,2], the derivative of value with respect to (x, y) inside the cell.
 *   shr_dt_sample_bwd   grad_points[B,N,C] = (grad_value grad_xy[0], grad_value grad_xy[1], 0, ...): every element is
 *       written.
 *   The sampler is a gather with no reduction: bitwise reproducible.  B <= 65535, N C < 2^31 (SHR_ETOOLARGE beyond);
 *   B == 0 or N == 0 is a no-op; NULL or misaligned pointers: SHR_EINVAL. */
long long shr_dt_workspace_bytes(int B, int H, int W);
int shr_dt_fwd(const float *depth, int B, int H, int W, float fg_max, int32_t *d2, void *workspace, void *stream);
int shr_dt_sample_fwd(const int32_t *d2, int B, int H, int W, const float *points, int N, int C, float max_dist,
                      float *value, float *grad_xy, void *stream);
int shr_dt_sample_bwd(const float *grad_xy, const float *grad_value, int B, int N, int C, float *grad_points,
                      void *stream);

/* Silhouette coverage, the other half of the silhouette term: the distance from every OBSERVED pixel to the RENDERED
 * silhouette, and its gradient to the vertices -- a pull on the model over observed pixels it does not cover (the
 * sampler above pulls model points that lie outside the observation; a model inside it gets nothing from that half).
 *   shr_dt_nearest_fwd   shr_dt_fwd with its argument.  depth[B,H,W] -> d2[B,H,W] int32, the bits of shr_dt_fwd, and
 *       nearest[B,H,W] int32.  The site rule (depth < fg_max, a NaN is not a site), the limits (1 <= H, W <= 2048,
 *       B <= 65535: H W <= 2^22, an index fits), the error codes, the alignment rules and the B == 0 no-op are
 *       shr_dt_fwd's.  nearest[b,i,j] = i' W + j' of a site (i', j') of image b with (i - i')^2 + (j - j')^2 == d2[b,i,j];
 *       among several such sites the one with the SMALLEST i' W + j'; -1 everywhere in an image without a site; a site
 *       is its own nearest.  Integer arithmetic only, no atomics: exact, independent of B and of the launch shape; no
 *       host synchronisation, no allocation.  Two passes: per column the vertically nearest site (an up / down tie:
 *       the smaller row), then per row the lexicographic minimum of (total, index).
 *       workspace: 16-byte aligned, shr_dt_nearest_workspace_bytes(B, H, W) bytes (-1 on a negative size), every element
 *       that is read is written by the call first.  It holds g[B][H][ceil(W/2)][2] uint16: bits 0..14 the vertical
 *       distance of each pixel to its column's nearest site, bit 15 set when that site lies below the pixel (a larger
 *       row); 0xffff: the column has none.
 *   shr_sil_cover_fwd   observed[B,H,W] fp32 (a pixel is OBSERVED iff observed < obs_fg_max; NaN: not observed), d2 the
 *       transform of the rendered depth -> dist[B,H,W] = fminf(sqrtf((float)d2), max_dist) at an observed pixel, 0
 *       elsewhere.  fp32, the IEEE root; every element is written; a gather with no reduction: bitwise reproducible.
 *       max_dist >= 0, +inf allowed (SHR_EINVAL otherwise).
 *   shr_sil_cover_bwd   d2, nearest: the transform of the rendered depth; owner[B,H,W], vertices[B,NV,4], faces[F,3]: as
 *       shr_tri_raster_indexed_owner_fwd gave and took them; grad_dist[B,H,W] -> grad_vertices[B,NV,4] = (du, dv, 0, 0),
 *       every element written.  Pixel p = (x = j, y = i) contributes iff it is observed, d2 > 0,
 *       sqrtf((float)d2) <= max_dist, grad_dist != 0, q = nearest lies in [0, H W), f = owner[q] lies in [0, F), the
 *       face's vertex ids lie in [0, NV), and the fp32 sum of the clamped weights of f at q = (xq, yq) is > 0 and
 *       <= 3e38 (shr_tri_interp_fwd's rule for a live pixel).  It adds to the face's x-sorted corner a
 *         (-grad_dist (c_a / s) (x - xq) / d,  -grad_dist (c_a / s) (y - yq) / d,  0),   d = sqrt((double)d2) in fp64,
 *       c_a / s the weights the depth and the attribute maps use at q (shr_tri_interp_bwd's rule: fp32 clamp decisions,
 *       fp64 values), HELD FIXED -- the envelope rule: q is a material point of face f with weights c / s, and moving it
 *       by delta changes |p - q| by -u . delta, u = (p - q) / d.  The gradient is the attribute gradient of
 *       shr_tri_interp_bwd for the attribute (x, y) under the map G[b,:,q] = sum over the pixels p with nearest(p) = q
 *       of -grad_dist(p) u(p).  No gradient to z, to the weights, or through the choice of q.  An image whose render is
 *       empty (nearest = -1 everywhere) gets a zero gradient.  The sums are 64-bit fixed point in a per-crop unit
 *       computed on the device (at most 3 W H terms per accumulator): bitwise reproducible, independent of the batch
 *       and of the launch shape, no host synchronisation.  workspace: 16-byte aligned,
 *       shr_sil_cover_bwd_workspace_bytes(B, NV) bytes (-1 on a negative size), cleared by the call itself.
 *   1 <= H, W <= 2048, B <= 65535 (SHR_ETOOLARGE beyond); B == 0 is a no-op; NULLs (faces may be NULL when F == 0) and
 *   misaligned pointers (4 bytes; vertices, grad_vertices and workspace 16): SHR_EINVAL. */
long long shr_dt_nearest_workspace_bytes(int B, int H, int W);
int shr_dt_nearest_fwd(const float *depth, int B, int H, int W, float fg_max, int32_t *d2, int32_t *nearest,
                       void *workspace, void *stream);
int shr_sil_cover_fwd(const float *observed, float obs_fg_max, const int32_t *d2, int B, int H, int W, float max_dist,
                      float *dist, void *stream);
long long shr_sil_cover_bwd_workspace_bytes(int B, int NV);
int shr_sil_cover_bwd(const float *observed, float obs_fg_max, const int32_t *d2, const int32_t *nearest,
                      const int32_t *owner, const float *vertices, const int32_t *faces, const float *grad_dist, int B,
                      int NV, int F, int W, int H, float max_dist, float *grad_vertices, void *workspace, void *stream);

/* Mesh data-to-model distance: every observed 3-D point to its closest point on the triangles, at any distance and in
 * x, y and z -- the ICP term of a mesh fit, the direction DataToModelLoss (mesh/render.py:93-142) runs for spheres.
 *   shr_mesh_d2m_fwd   observed[B,H,W] fp32; vertices[B,NV,4] fp32 (x, y, z in model space, the 4th float ignored,
 *       16-byte aligned); faces[F,3] int32 as given (the distance does not depend on winding; `face` indexes these
 *       rows); ax, bx, ay, by; fg_max; max_dist >= 0, +inf allowed (SHR_EINVAL otherwise).
 *       Points.  Pixel (row i, column j) is a DATA POINT iff observed < fg_max (a NaN is none: shr_dt_fwd's site rule).
 *       Its point is p = (ax (float)j + bx, ay (float)i + by, observed), one rounding per written operation.
 *       (1, 0, 1, 0) is the raster's pixel space (tri_face.h), (300/W, -150, 300/H, -150) the reference's millimetre
 *       grid, (5, 0, 5, 0) puts a 128 x 128 observation over the 640 x 640 raster.
 *       Per point and face with corners a, b, c (the vertices of faces[f,0..2]), all fp32, one correctly rounded
 *       operation per written operator, dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z:
 *         ab = b - a;  ac = c - a;  ap = p - a;  bp = ap - ab;  cp = ap - ac
 *         d1 = dot(ab, ap);  d2 = dot(ac, ap);  d3 = dot(ab, bp);  d4 = dot(ac, bp);  d5 = dot(ab, cp);  d6 = dot(ac, cp)
 *         vc = d1 d4 - d3 d2;  vb = d5 d2 - d1 d6;  va = d3 d6 - d5 d4;  e43 = d4 - d3;  e56 = d5 - d6
 *       The FIRST of the seven regions whose test holds gives (nv, dv, nw, dw):
 *         A    d1 <= 0 and d2 <= 0                     (0, 1, 0, 1)
 *         B    d3 >= 0 and d4 <= d3                    (1, 1, 0, 1)
 *         AB   vc <= 0 and d1 >= 0 and d3 <= 0         (d1, d1 - d3, 0, 1)
 *         C    d6 >= 0 and d5 <= d6                    (0, 1, 1, 1)
 *         AC   vb <= 0 and d2 >= 0 and d6 <= 0         (0, 1, d2, d2 - d6)
 *         BC   va <= 0 and e43 >= 0 and e56 >= 0       (0, 1, e43, e43 + e56), and v below is 1 - w instead
 *         in   otherwise                               (vb, (va + vb) + vc, vc, (va + vb) + vc)
 *         v = nv / dv;  w = nw / dw;  (BC: v = 1 - w);  v = v > 1 ? 1 : v;  v = v < 0 ? 0 : v;  the same for w
 *         e = ap - (v ab + w ac) per component (two products, their sum, the difference);  d2 = dot(e, e)
 *       The closest point is a + v ab + w ac with v, w in [0, 1] whatever the roundings decided (a NaN passes the
 *       two selects).  A zero-area face falls into a vertex or an edge region: it gives the distance to its segment or
 *       point, or -- where the edge's denominator is 0, as with two coincident corners -- 0 / 0, a NaN d2; a NaN
 *       operand gives a NaN d2, an infinite one a NaN or +inf.  Neither is ever taken.
 *       Selection.  best = +inf, face = -1; for f ascending, face f is taken iff its three ids lie in [0, NV) and
 *       d2 < best.  A NaN d2 is never taken, equal distances keep the smallest f.  However the kernels split the
 *       faces, the result is that of this serial rule: partial results combine by the lexicographic minimum of
 *       (d2, f).  The kernels skip a face whose bounding sphere cannot beat the current best (DESIGN.md 4.4j states
 *       the margin); the outputs are bit-identical with and without that.
 *       -> dist[B,H,W] fp32 = fminf(sqrtf(best), max_dist) at a data point with a face, 0 at a pixel that is no data
 *       point and at a data point for which no face was taken; face[B,H,W] int32, -1 where dist has no face.  Every
 *       element is written.  No reduction over memory: bitwise reproducible, independent of B and the launch shape.
 *       workspace: 16-byte aligned, shr_mesh_d2m_workspace_bytes(B, F) bytes (-1 on a negative size): 48 bytes per
 *       (crop, face), written by the call before it is read.
 *   shr_mesh_d2m_bwd   dist, face: the forward's maps (or any maps: every index is checked); grad_dist[B,H,W] ->
 *       grad_vertices[B,NV,4] = (d/dx, d/dy, d/dz, 0) of sum grad_dist dist, every element written.  A pixel
 *       contributes iff it is a data point, f = face lies in [0, F), the ids of faces[f] lie in [0, NV),
 *       grad_dist != 0 and 0 < dist < max_dist (a saturated or a zero distance is a constant).  In fp64 from the fp32
 *       p (computed as above) and corners: the seven regions above decided in fp64 (A, B, AB, C, AC, BC, in; no
 *       clamp), the closest point c = (1 - v - w) a + v b + w c as ap - (v ab + w ac) = p - c, n = |p - c|; n == 0 or
 *       not finite: nothing.  Corner k with weight w_k = (1 - v - w, v, w) takes -grad_dist w_k (p - c) / n: the
 *       closest point is continuous across the regions, so the fp64 decisions need not agree with the fp32 ones.
 *       The sums are 64-bit fixed point in a per-crop unit computed on the device (at most 3 W H terms per
 *       accumulator): bitwise reproducible, independent of the batch and of the launch shape, no host
 *       synchronisation.  workspace: 16-byte aligned, shr_mesh_d2m_bwd_workspace_bytes(B, NV) bytes (-1 on a negative
 *       size), cleared by the call itself.
 *   1 <= H, W <= 2048, B <= 65535, 3 NV and 3 F < 2^31 (SHR_ETOOLARGE beyond); NV >= 1, F >= 0 (F == 0: every dist 0,
 *   every face -1); B == 0 is a no-op; NULLs (faces may be NULL when F == 0) and misaligned pointers (4 bytes;
 *   vertices, grad_vertices and workspace 16): SHR_EINVAL. */
long long shr_mesh_d2m_workspace_bytes(int B, int F);
int shr_mesh_d2m_fwd(const float *observed, const float *vertices, const int32_t *faces, int B, int NV, int F, int W,
                     int H, float ax, float bx, float ay, float by, float fg_max, float max_dist, float *dist,
                     int32_t *face, void *workspace, void *stream);
long long shr_mesh_d2m_bwd_workspace_bytes(int B, int NV);
int shr_mesh_d2m_bwd(const float *observed, const float *vertices, const int32_t *faces, const float *dist,
                     const int32_t *face, const float *grad_dist, int B, int NV, int F, int W, int H, float ax,
                     float bx, float ay, float by, float fg_max, float max_dist, float *grad_vertices, void *workspace,
                     void *stream);

/* Normal map of a depth image, and its backward to the depth (a capability the reference does not have: the data side
 * of an orientation term -- render.MeshNormalRaster is its model side -- and, through the backward, an orientation term
 * for any rendered depth, the spheres' included).
 *   shr_depth_normals_fwd   depth[B,H,W] fp32 -> normals[B,3,H,W].  In fp32 with one rounding per written operator (no
 *       contraction), for pixel (row i, column j) with c = depth[i,j]:
 *         1. SITE iff c < fg_max (shr_dt_fwd's rule: a NaN is no site).  A pixel that is no site gets (0, 0, 0).
 *         2. a neighbour value n is USABLE iff it lies inside the image, n < fg_max and fabsf(n - c) <= max_step (the
 *            discontinuity rule; a NaN difference is not usable; max_step = +inf keeps every foreground neighbour).
 *         3. horizontal difference, l = depth[i,j-1], r = depth[i,j+1]:  both usable: dx = r - l, hx = 2;  only r:
 *            dx = r - c, hx = 1;  only l: dx = c - l, hx = 1;  neither: the pixel has no normal, (0, 0, 0).
 *         4. vertical difference, u = depth[i-1,j], d = depth[i+1,j]: the same rule; both usable: dy = d - u, hy = 2.
 *         5. wx = hx sx, wy = hy sy: the widths of the two differences in model units (exact: h is 1 or 2).
 *            N = (dx wy, dy wx, -(wx wy)): the cross product of the tangents (wx, 0, dx) and (0, wy, dy), turned towards
 *            the camera.  On z = a x + b y + c it is proportional to (a, b, -1): MeshNormalRaster's orientation, z <= 0.
 *         6. n = unit3(N): step 3 of shr_tri_vertex_normals_fwd, the same device function, with its ZERO RULE.
 *       W == 1 or H == 1 is legal and gives zeros everywhere.  normals must not overlap depth.
 *   shr_depth_normals_bwd   grad_normals[B,3,H,W] -> grad_depth[B,H,W]: the exact derivative of 1 .. 6 with every fp32
 *       decision held fixed (site, usable, the case of each axis, the zero rule), evaluated in fp64 from the fp32 depths
 *       and rounded to fp32 once per element.  A gather, no atomics: grad_depth[p] is the fp64 sum, in this order, of the
 *       contributions of the normals at p, at its left, right, upper and lower neighbour -- those inside the image that
 *       have a normal.  For such a pixel q:  N, n = N / |N| in fp64;  G = (g - n (n . g)) / |N| (as shr_unit3_maps_bwd; 0
 *       when the fp64 |N|^2 is 0 or not finite);  d/d dx = G_x wy,  d/d dy = G_y wx;  dx and dy hand these on to l, r, c
 *       (u, d, c) with the signs of q's case in 3. and 4.  Every element of grad_depth is written, 0 where nothing
 *       contributes (every pixel that is no site).  grad_depth must not overlap depth or grad_normals.  Bitwise
 *       reproducible, independent of B and of the launch shape; no workspace, no host synchronisation.
 *   sx, sy finite and > 0; fg_max and max_step not NaN, max_step >= 0 (+inf allowed): SHR_EINVAL otherwise.  1 <= W, H
 *   and B, W, H <= 65535 (SHR_ETOOLARGE beyond); B == 0 is a no-op; NULL, misaligned (4 bytes) or overlapping pointers:
 *   SHR_EINVAL. */
int shr_depth_normals_fwd(const float *depth, int B, int W, int H, float fg_max, float sx, float sy, float max_step,
                          float *normals /* [B,3,H,W] */, void *stream);
int shr_depth_normals_bwd(const float *depth, const float *grad_normals /* [B,3,H,W] */, int B, int W, int H,
                          float fg_max, float sx, float sy, float max_step, float *grad_depth /* [B,H,W] */, void *stream);

/* Key-point skinning -> sphere records -----------------------------------------------------
 * Replaces, inside HandBallPrimitiveRender (mesh/render.py:65-88), the LinearBlendSkinning of the key-points (each
 * bound to ONE bone with weight 1: mesh/pointTransformation.py:39-46 reduces to p = T[bone[j]] @ wv[j], x -> -x for
 * the right hand) and the cat with the radii:  spheres[B,J,4] = (+-p.x, p.y, p.z, radii[j]).
 * T[B,NB,4,4]; bone[J] (bone of key-point j), wv[J,4] = fp32(weight * key-point) as the reference stores it (:31). */
int shr_keypoint_spheres_fwd(const float *T, int B, int NB, int J, const int32_t *bone, const float *wv,
                             const float *radii, int right_hand, float *spheres, void *stream);
/* Its autograd backward: grad_T[B,NB,4,4] = d<grad_spheres, spheres>/dT (the radii are buffers in the reference and
 * get no gradient, the homogeneous row gets none).  bone_start[NB+1], bone_points[J]: the key-points of every bone
 * (CSR, ascending: the sums run in index order). */
int shr_keypoint_spheres_bwd(const float *grad_spheres, int B, int NB, int J, const int32_t *bone_start,
                             const int32_t *bone_points, const float *wv, int right_hand, float *grad_T, void *stream);

/* Forward kinematics -------------------------------------------------------------------
 * Replaces HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177)
 * and its autograd backward.  params[B,26] (palm Euler xyz, palm translation, 5 x
 * (abduct, flex1, flex2, flex3)); offset, offset_inv [17,4,4] = the bones' offset
 * matrices and their inverses (16-byte aligned; AFFINE: last row 0 0 0 1, as every bone
 * offset matrix and its inverse is -- the kernels never read that row);
 * T[B,17,4,4] (bones 0 and 1 = palm transform). */
int shr_fk_fwd(const float *params, int B, const float *offset, const float *offset_inv,
               float *T, void *stream);
/* grad_params[B,26] = d<grad_T, T>/d params (analytic reverse mode; the homogeneous row of
 * T is constant and takes no gradient). */
int shr_fk_bwd(const float *params, int B, const float *offset, const float *offset_inv,
               const float *grad_T, float *grad_params, void *stream);

/* Pose -> sphere records in one launch per direction ---------------------------------------
 * shr_fk_fwd followed by shr_keypoint_spheres_fwd without T visiting HBM: the fit chain
 * HandBallPrimitiveRender(HandTransformationMat(pose)) of mesh/render.py:81-88 over
 * mesh/kinematicsTransformation.py:169-177.  Same arithmetic as the two entries, same bits.
 * bone[J] < 17, wv[J,4], radii[J] as for shr_keypoint_spheres_fwd; spheres[B,J,4];
 * T: NULL, or [B,17,4,4] to receive the bone transforms as well. */
int shr_pose_spheres_fwd(const float *params, int B, const float *offset, const float *offset_inv, int J,
                         const int32_t *bone, const float *wv, const float *radii, int right_hand,
                         float *spheres, float *T, void *stream);
/* grad_params[B,26] = d<grad_spheres, spheres>/d params: shr_keypoint_spheres_bwd and
 * shr_fk_bwd in one launch (bone_start[18], bone_points[J]: CSR as there). */
int shr_pose_spheres_bwd(const float *params, int B, const float *offset, const float *offset_inv, int J,
                         const int32_t *bone_start, const int32_t *bone_points, const float *wv,
                         int right_hand, const float *grad_spheres, float *grad_params, void *stream);

/* Differentiable skinning of the mesh: bone transforms or pose -> vertices, and back ---------
 * The backward of LinearBlendSkinning.forward (mesh/pointTransformation.py:39-46) and OthographicalProjection.forward
 * (:84-99) in both modes of shr_lbs_project, and the chain HandTransformationMat.forward
 * (mesh/kinematicsTransformation.py:157-177) -> skinning -> camera as one launch per direction.  The skin table and the
 * camera arguments are shr_lbs_project's; rand_f and the table get no gradient.
 *   shr_lbs_vertices_bwd   grad_vertices[B,NV,4] -> grad_T[B,NB,4,4], shr_lbs_project_bwd's arguments plus `project`.
 *                          project = 1: shr_lbs_project_bwd's result bit for bit (the same kernel).  project = 0: the
 *                          derivative of the skinned points, d acc = (+-g.x, g.y, g.z, g.w) (- for the right hand); cx, cy,
 *                          fx, fy and rand_f are ignored.  Summation order (the contract): one wave per bone, lane l takes
 *                          the vertices l + 64 n in ascending order and a vertex's entries of the bone in table order, fp64
 *                          partial sums, the xor butterfly 32, 16 .. 1 over the lanes, one rounding to fp32: bitwise
 *                          reproducible, independent of the batch.  A bone without an entry gets zeros.
 *   shr_pose_vertices_fwd  params[B,26] -> vertices[B,NV,4]: the bits of shr_fk_fwd followed by shr_lbs_project, the bone
 *                          transforms formed in LDS by every workgroup for its crops.  NB is the hand's 17 (offset,
 *                          offset_inv [17,4,4] as for shr_fk_fwd); a bone number of the table outside [0, 17) is clamped
 *                          into it.  T: NULL, or [B,17,4,4] (16-byte aligned) to receive shr_fk_fwd's bits as well,
 *                          written by one workgroup per group of crops.
 *   shr_pose_vertices_bwd  grad_vertices[B,NV,4] -> grad_params[B,26]: the bits of shr_lbs_vertices_bwd followed by
 *                          shr_fk_bwd, one workgroup per crop: the skinning sums above (rows 0..2 of each bone, rounded to
 *                          fp32) stay in LDS and one wave runs shr_fk_bwd's reverse row chain on them.
 * skin_wv, vertices, grad_vertices 16-byte aligned, grad_params 8-byte aligned, NULL pointers: SHR_EINVAL.  B * NV above
 * 2^30, B above 2^24 (shr_lbs_vertices_bwd: 2^30): SHR_ETOOLARGE.  B == 0 or NV == 0: SHR_OK, nothing is launched and
 * nothing written. */
int shr_lbs_vertices_bwd(const float *grad_vertices, int B, int NB, int NV, const int32_t *skin_vertex_start,
                         const int32_t *skin_bone, const float *skin_wv, int right_hand, int project, float cx, float cy,
                         float fx, float fy, const float *rand_f, float *grad_T, void *stream);
int shr_pose_vertices_fwd(const float *params, int B, const float *offset, const float *offset_inv, int NV,
                          const int32_t *skin_vertex_start, const int32_t *skin_bone, const float *skin_wv,
                          int right_hand, int project, float cx, float cy, float fx, float fy, const float *rand_f,
                          float *vertices, float *T /* may be NULL */, void *stream);
int shr_pose_vertices_bwd(const float *params, int B, const float *offset, const float *offset_inv, int NV,
                          const int32_t *skin_vertex_start, const int32_t *skin_bone, const float *skin_wv,
                          int right_hand, int project, float cx, float cy, float fx, float fy, const float *rand_f,
                          const float *grad_vertices, float *grad_params, void *stream);

/* Pose from keypoints: the inverse of shr_pose_spheres_fwd, as a refinement from a start pose ---------
 * Inverts HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by the key-point skinning of
 * HandBallPrimitiveRender (mesh/render.py:65-88); the reference has no counterpart.  offset, offset_inv [17,4,4], bone[J],
 * wv[J,4] and right_hand are shr_pose_spheres_fwd's (a bone number outside [0, 17) is clamped into it, as there);
 * 1 <= J <= 64.  Keypoints, targets and the Jacobian are in the frame shr_pose_spheres_fwd outputs: model millimetres, x
 * negated for the right hand.  One wave per crop, no workspace, no host synchronisation: capturable in a hipGraph.
 *   shr_pose_keypoints_jacobian  params[B,26] -> keypoints[B,J,4] = (shr_pose_spheres_fwd's xyz bit for bit, 1) and
 *                          jac[B,3J,26], row 3 j + c = d keypoint j component c / d params, fp32.
 *   shr_pose_ik_fwd        Levenberg-Marquardt on cost(p) = sum_j w_j |k_j(p) - target_j|^2 + sum_i mu_i (p_i - params0_i)^2
 *                          from p = params0.  target[B,J,3]; weights: NULL (all 1), [J] (weight_stride 0) or [B,J]
 *                          (weight_stride J), each >= 0; stiffness: NULL (all 0) or mu[26], each >= 0; iters >= 0,
 *                          lambda0 > 0.  Each iteration forms A = J^T W J + diag(mu) and g = J^T W r + mu (p - params0),
 *                          solves (A + lambda diag(A)) delta = -g by Cholesky, evaluates the cost at p + delta and accepts
 *                          iff it is lower; lambda <- 0.3 lambda on accept, 10 lambda on reject, clamped to [1e-9, 1e6].  A
 *                          pivot that is not positive, or a trial cost that is not finite, is a rejected step.  Always
 *                          `iters` iterations.  Outputs params[B,26], cost0[B] (at params0) and cost[B] (at params);
 *                          iters = 0: params = params0 and cost = cost0.  Arithmetic: keypoints, residuals and the
 *                          Jacobian fp32; A, g, the factor, the solves, lambda and the costs fp64 (the costs leave rounded to
 *                          fp32).  Every sum runs in a fixed order: bitwise reproducible, and a crop's result does not
 *                          depend on the batch it is in.
 *   shr_pose_ik_bwd        the implicit-function gradient at the returned pose in Gauss-Newton form:
 *                          grad_target[B,J,3] = w_j J_j(params) (J^T W J + diag(mu))^-1 grad_params (exact where the residual
 *                          is 0).  A crop whose matrix is not positive definite gets zeros.  params0, the weights and the
 *                          stiffness get no gradient.
 * wv and keypoints 16-byte aligned, every other array 4-byte aligned, NULL pointers (other than weights, stiffness), J < 1,
 * iters < 0, lambda0 <= 0, a weight_stride other than 0 or J: SHR_EINVAL.  J above 64, B above 2^24: SHR_ETOOLARGE.  B == 0:
 * SHR_OK, nothing is launched and nothing written. */
int shr_pose_keypoints_jacobian(const float *params, int B, const float *offset, const float *offset_inv, int J,
                                const int32_t *bone, const float *wv, int right_hand, float *keypoints, float *jac,
                                void *stream);
int shr_pose_ik_fwd(const float *target, const float *params0, int B, const float *offset, const float *offset_inv, int J,
                    const int32_t *bone, const float *wv, int right_hand, const float *weights /* may be NULL */,
                    int weight_stride, const float *stiffness /* may be NULL */, int iters, float lambda0, float *params,
                    float *cost0, float *cost, void *stream);
int shr_pose_ik_bwd(const float *params, const float *grad_params, int B, const float *offset, const float *offset_inv,
                    int J, const int32_t *bone, const float *wv, int right_hand, const float *weights /* may be NULL */,
                    int weight_stride, const float *stiffness /* may be NULL */, float *grad_target, void *stream);

/* Pose from observed depth points: Gauss-Newton / Levenberg-Marquardt ICP on the mesh ---------------
 * Inverts HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by LinearBlendSkinning.forward
 * (mesh/pointTransformation.py:39-46), against the observation of DataToModelLoss (mesh/render.py:93-142) taken to the
 * triangles by shr_mesh_d2m_fwd; the reference has no counterpart.  One evaluation of a fit is
 *   shr_pose_vertices_fwd(trial, project = 0) -> shr_mesh_d2m_fwd -> shr_pose_icp_normal -> shr_pose_lm_step
 * on one stream, without a host synchronisation: capturable in a hipGraph.
 *   shr_pose_icp_normal    the normal equations of 1/2 sum dist^2 over the contributing data points with respect to the
 *       26 pose parameters.  observed, vertices, faces, dist, face, ax .. max_dist: shr_mesh_d2m_bwd's, with its meaning and
 *       checks (dist and face the forward's maps, or any maps: every index is checked); params[B,26], offset, offset_inv
 *       [17,4,4]: shr_fk_fwd's; skin_vertex_start[NV+1], skin_bone, skin_wv, right_hand: shr_pose_vertices_fwd's table (a
 *       bone number outside [0, 17) is clamped into it).  vertices MUST be those shr_pose_vertices_fwd(params, project = 0)
 *       writes for this table: this is NOT checked, and other vertices give the equations of no function.
 *       A pixel contributes a row under shr_mesh_d2m_bwd's rule without its grad_dist test: a data point, its face in
 *       [0, F) with ids in [0, NV), 0 < dist < max_dist, and the recomputed distance d finite and not zero.  On the saved
 *       face, as there (the same device code): the fp64 regions without a clamp give the corner weights w_k, e = p - c,
 *       d = |e|, u = e / d.  With the weights held (the envelope theorem), row J = d d / d params =
 *       -u^T sum_k w_k d v_k / d params, where a vertex is the sum over its table entries of T_bone wv: the palm angles
 *       by omega x (T_bone wv - wv.w t) about the palm translation t, omega = P e_x, Rz e_y, e_z, the translation by wv.w,
 *       a finger angle by the forward-mode tangent of T_bone (shr_pose_keypoints_jacobian's columns); component x of the
 *       right hand negated.  No assumption about which fingers a point touches: every entry of every corner adds to the
 *       columns of its own bone.  Transforms, tangents and the entries of J are fp32; w_k, u, d and every sum are fp64.
 *       -> A[B,26,26] fp64 = sum J^T J, both triangles written from one sum (bit-symmetric); g[B,26] fp64 = sum d J, the
 *       gradient of 1/2 sum dist^2; cost[B] fp64 = sum dist^2 over ALL pixels of the fp32 map `dist`, each promoted to
 *       fp64 before it is squared (a saturated point counts max_dist^2: a truncated quadratic); count[B] int32, the rows.
 *       A crop without a row gets A = 0, g = 0, count = 0.
 *       Summation order (the contract): the pixels of a crop in row-major order form tiles of 1024; within a tile every
 *       entry is one fp64 chain from 0 over the tile's pixels in ascending order (fma(J_a, J_c, .) for A, fma(d, J_a, .)
 *       for g, a sum for cost); the tiles' values are then added from 0 in ascending tile order.  Bitwise reproducible;
 *       a crop's result does not depend on the batch it is in or on the launch shape.
 *       workspace: 16-byte aligned, shr_pose_icp_normal_workspace_bytes(B, W, H) bytes (-1 on a negative size): 3072
 *       bytes per (crop, tile), written by the call before it is read.
 *       Argument rules: shr_mesh_d2m_bwd's and shr_pose_vertices_fwd's -- 1 <= H, W <= 2048, B <= 65535, 3 NV and 3 F <
 *       2^31, B NV <= 2^30 (SHR_ETOOLARGE beyond); NV >= 1, F >= 0; B == 0 is a no-op; NULLs (faces may be NULL when
 *       F == 0) and misaligned pointers (4 bytes; A, g, cost 8; vertices, offset, offset_inv, skin_wv, workspace 16):
 *       SHR_EINVAL.
 *   shr_pose_lm_begin, shr_pose_lm_step   the Levenberg-Marquardt bookkeeping of shr_pose_ik_fwd's iteration, kept on the
 *       device; `state`: shr_pose_lm_state_bytes(B) bytes (-1 for B < 0), 8-byte aligned, per crop the accepted pose, its
 *       total cost, its A and g, params0, lambda, and counters of accepted and rejected steps: 760 doubles per crop --
 *       A [0, 676), g [676, 702), the pose [702, 728), params0 [728, 754), cost 754, lambda 755, 756: no step since
 *       begin, 757: a step has been accepted since begin, 758 and 759: the accepted and the rejected steps.
 *       begin(params0[B,26], lambda0 > 0): pose <- params0, cost <- +inf, lambda <- lambda0, A and g <- 0, the counters
 *       <- 0, and trial[B,26] <- params0: the pose to evaluate first.
 *       step(A, g, cost_data of the pose `trial`; prior[B,26] or NULL = params0; stiffness mu[26] >= 0 or NULL = 0):
 *         total = cost_data + mu_0 (trial_0 - prior_0)^2 + ... + mu_25 (trial_25 - prior_25)^2, added in this order;
 *         the trial is ACCEPTED iff total is finite and below the state's cost; the state then takes trial, A, g, total;
 *         lambda <- 0.3 lambda on an accepted step -- except the first accepted one after begin, which leaves it as it
 *         is -- and 10 lambda on a rejected one; then lambda is clamped to [1e-9, 1e6];
 *         params[B,26] <- the accepted pose, cost[B] <- its total (fp32; +inf while nothing has been accepted), and on
 *         the first step after begin cost0[B] <- total (fp32), accepted or not;
 *         solve != 0: with p, A, g the accepted pose's and M = A + diag(mu), the step solves
 *         (M + lambda diag M) delta = -(g + mu (p - prior)) by Cholesky and writes trial_out[B,26] = fp32(p + delta); a
 *         pivot that is not positive and finite writes trial_out = p (evaluated next, it costs the same, is rejected, and
 *         lambda rises: no special case).  solve == 0 writes no trial_out (it may be NULL).  trial_out may be trial.
 *       All arithmetic fp64, every sum in index order, one wave per crop, the factor and the substitutions those of
 *       shr_pose_ik_fwd: bitwise reproducible, a crop does not depend on its batch.
 *       NULLs (other than prior, stiffness), lambda0 <= 0, misaligned pointers (state, A, g, cost_data 8; others 4):
 *       SHR_EINVAL.  B above 2^24: SHR_ETOOLARGE.  B == 0: SHR_OK, nothing is launched and nothing written. */
long long shr_pose_icp_normal_workspace_bytes(int B, int W, int H);
int shr_pose_icp_normal(const float *observed, const float *vertices, const int32_t *faces, const float *dist,
                        const int32_t *face, const float *params, const float *offset, const float *offset_inv,
                        const int32_t *skin_vertex_start, const int32_t *skin_bone, const float *skin_wv, int right_hand,
                        int B, int NV, int F, int W, int H, float ax, float bx, float ay, float by, float fg_max,
                        float max_dist, double *A, double *g, double *cost, int32_t *count, void *workspace, void *stream);
long long shr_pose_lm_state_bytes(int B);
int shr_pose_lm_begin(const float *params0, int B, float lambda0, void *state, float *trial, void *stream);
int shr_pose_lm_step(void *state, const double *A, const double *g, const double *cost_data, const float *trial,
                     const float *prior /* may be NULL */, const float *stiffness /* may be NULL */, int solve, int B,
                     float *trial_out, float *params, float *cost, float *cost0, void *stream);

/* One pose fitted to several depth views: multi-view ICP on the mesh ---------------
 * One pose per sample in the model frame, V observed depth images per sample, one rigid transform per view: view[B,V,4,4]
 * fp32, row-major, maps the model frame to view v's frame, x_v = R x + t (the top-left 3 x 3 and the last column; the
 * fourth row is not read).  With camera poses as MutualTransformation takes them (mesh/multiview_utility.py:13-30),
 * view[:, v] = inv_camera_poses[:, v] @ camera_poses[:, ref]: its (ref, v) entry.  All views share W, H, ax .. by, fg_max
 * and max_dist.  An iteration is one Levenberg-Marquardt step on the sum of all views' point-to-mesh costs:
 *   shr_pose_vertices_fwd(trial, project = 0) -> shr_view_vertices_fwd -> shr_mesh_d2m_fwd (B V crops)
 *   -> shr_pose_icp_normal_views -> shr_pose_lm_step
 * on one stream, without a host synchronisation: capturable in a hipGraph.  The reference has no counterpart.
 *   shr_view_vertices_fwd  vertices[B,NV,4] in model space (shr_pose_vertices_fwd's with project = 0) and view -> out
 *       [B,V,NV,4] fp32: out.x = ((R00 x + R01 y) + R02 z) + t0, and y, z alike with rows 1 and 2 -- the three products and
 *       the sums in exactly this association, each operation rounded to fp32 once (no fused multiply-add); the 4th float is
 *       copied.  For the identity view, out holds the bits of its input (a -0 becomes +0).
 *   shr_pose_icp_normal_views  shr_pose_icp_normal's equations, summed over the views.  observed, dist, face: [B,V,H,W],
 *       crop b V + v being view v of sample b; view_vertices[B,V,NV,4]: shr_view_vertices_fwd's (as for `vertices` there:
 *       they MUST be those of params under view, which is NOT checked); dist, face: shr_mesh_d2m_fwd's maps of the B V
 *       crops; params[B,26], offset, offset_inv, the skin table, right_hand, faces, ax .. max_dist: shr_pose_icp_normal's.
 *       The top-left 3 x 3 of a view is read as a rotation: it is NOT checked to be orthonormal, and another matrix gives
 *       the equations of no function.
 *       Row rule: a pixel of view v gives a row under shr_pose_icp_normal's rule (a data point, its face in [0, F) with ids
 *       in [0, NV), 0 < dist < max_dist, the recomputed distance finite and not zero); its closest point is recomputed in
 *       fp64 on the VIEW-frame vertices, on the saved face: corner weights w_k, e = p - c, d = |e|, u_v = e / d; the unit
 *       direction is taken back to the model frame in fp64, u_j = (R0j u_v0 + R1j u_v1) + R2j u_v2 (u = R^T u_v: a distance
 *       does not change under a rigid map, so the row with respect to the pose needs nothing else of the view); from there
 *       the row is shr_pose_icp_normal's with this u, the same device code: the cross products for the palm angles, w_k u
 *       for the translation, the finger tangents, component x negated for the right hand.
 *       -> A[B,26,26], g[B,26], cost[B] fp64 and count[B] int32 as there, over all pixels of all views: cost = sum dist^2
 *       over the B V maps.  A view without a data point (a missing camera: an all-background image) adds nothing.
 *       Summation order (the contract): pixels ascending inside a tile of 1024 (one fp64 chain from 0, as there), tiles
 *       ascending inside a view, views ascending: the V tiles values of a sample are added from 0 in this order.  Bitwise
 *       reproducible; a sample's result does not depend on the batch it is in or on the launch shape.  For V = 1 and the
 *       identity view it is shr_pose_icp_normal's result bit for bit.
 *       workspace: 16-byte aligned, shr_pose_icp_normal_views_workspace_bytes(B, V, W, H) bytes (-1 on a negative size):
 *       3072 bytes per (sample, view, tile), written by the call before it is read.
 *   Argument rules (both entries): shr_pose_icp_normal's limits, alignments (view, view_vertices, out: 16 bytes) and error
 *   codes; V < 1: SHR_EINVAL; B V above 65535 or B V NV above 2^30: SHR_ETOOLARGE; B == 0 is a no-op. */
int shr_view_vertices_fwd(const float *vertices, const float *view, int B, int V, int NV, float *out, void *stream);
long long shr_pose_icp_normal_views_workspace_bytes(int B, int V, int W, int H);
int shr_pose_icp_normal_views(const float *observed, const float *view_vertices, const int32_t *faces, const float *dist,
                              const int32_t *face, const float *view, const float *params, const float *offset,
                              const float *offset_inv, const int32_t *skin_vertex_start, const int32_t *skin_bone,
                              const float *skin_wv, int right_hand, int B, int V, int NV, int F, int W, int H, float ax,
                              float bx, float ay, float by, float fg_max, float max_dist, double *A, double *g, double *cost,
                              int32_t *count, void *workspace, void *stream);

/* Pose from observed depth points through the SPHERE model: Gauss-Newton / Levenberg-Marquardt ICP on the spheres -------
 * Inverts HandTransformationMat.forward (mesh/kinematicsTransformation.py:157-177) followed by the key-point skinning of
 * HandBallPrimitiveRender (mesh/render.py:65-88), against the observation of DataToModelLoss (mesh/render.py:93-142), whose
 * distance min_j | |p - c_j| - r_j | this is.  The reference has no counterpart.  One evaluation of a fit is
 *   shr_pose_keypoints_jacobian(trial) -> shr_view_vertices_fwd (NV := J) -> shr_sphere_icp_normal -> shr_pose_lm_step
 * on one stream, without a host synchronisation: capturable in a hipGraph.  The search has J <= 64 candidates per point, so
 * search, residual and row are ONE entry: there are no saved maps to hand in.
 *   shr_sphere_icp_normal   the normal equations of 1/2 sum d^2, d = |p - c_owner| - r_owner, over the rows of all views
 *       with respect to the 26 pose parameters.  observed[B,V,H,W] fp32, crop b V + v being view v of sample b;
 *       view_centres[B,V,J,4]: shr_view_vertices_fwd of shr_pose_keypoints_jacobian's keypoints under view (the 4th float is
 *       not read; they MUST be those of the pose jac belongs to, which is NOT checked); radii[J]; view[B,V,4,4] as for
 *       shr_pose_icp_normal_views: only its top-left 3 x 3 is read, as a rotation, and it is NOT checked to be orthonormal;
 *       jac[B,3J,26]: shr_pose_keypoints_jacobian's.  ax, bx, ay, by, fg_max, max_dist: shr_mesh_d2m_fwd's.
 *       Data points.  shr_mesh_d2m_fwd's: pixel (row i, column j) of a view is a DATA POINT iff observed < fg_max (a NaN is
 *       none); p = (ax (float)j + bx, ay (float)i + by, observed), one rounding per written operation.
 *       Owner.  All fp32, one correctly rounded operation per written operator, nothing contracted.  best = +inf,
 *       owner = -1; for j ascending with c_j = view_centres[b,v,j,0..2], r_j = radii[j]:
 *         e = p - c_j;  n2 = (e.x e.x + e.y e.y) + e.z e.z;  n = sqrt(n2) correctly rounded;  s_j = |n - r_j|
 *       sphere j is taken iff s_j < best: a NaN s is never taken (nor is +inf), equal distances keep the smallest j -- the
 *       reference's min_j | |p - c_j| - r_j | with the first index on ties.  The kernel prunes nothing: every data point meets
 *       every sphere.
 *       -> dist[B,V,H,W] fp32 (or NULL) = fminf(s_owner, max_dist) at a data point with an owner, 0 at every other pixel;
 *       owner[B,V,H,W] int32 (or NULL), -1 where dist has no owner.  Every element of a map that is given is written.
 *       Row.  A data point gives a row iff it has an owner, s_owner < max_dist and, recomputed in fp64 from the fp32 p, c, r
 *       of the owner, n = sqrt((e.x e.x + e.y e.y) + e.z e.z) is finite and > 0 (a point exactly on a centre has no
 *       direction: no row).  Then d = n - r, signed: negative inside the sphere; u_v = e / n; the direction is taken back
 *       to the model frame in fp64 with shr_pose_icp_normal_views' association, u_j = (R0j u_v0 + R1j u_v1) + R2j u_v2
 *       (u = R^T u_v).  The row is d d / d params = -u^T jac[3 owner .. 3 owner + 2, :], fp64 products of the fp32 Jacobian.
 *       A point with d = 0, exactly on the surface, still gives a row: unlike on a triangle its direction is defined.
 *       -> moments[B,J,12] fp64 (or NULL), for the rows owned by sphere j: S = sum u u^T as (xx, xy, xz, yy, yz, zz),
 *       h = sum d u (3), sum d^2, the number of rows (as a double), and one spare 0.
 *       -> A[B,26,26] fp64 = sum row^T row, formed as sum_j Jc_j^T S_j Jc_j with Jc_j = jac[3j .. 3j + 2, :], all 26
 *       columns of every sphere (no assumption about which parameters move a sphere); the lower triangle is computed and
 *       written to both triangles: bit-symmetric.  g[B,26] fp64 = sum d row = -sum_j Jc_j^T h_j, the gradient of
 *       1/2 sum d^2.  cost[B] fp64 = sum over ALL pixels of all views of (double)dist^2 of the fp32 distance above (a
 *       saturated point counts max_dist^2: a truncated quadratic).  count[B] int32: the rows.  A sample without a row gets
 *       A = 0, g = 0, count = 0.
 *       Summation order (the contract): fixed-order fp64 chains, no atomics.  The pixels of a view in row-major order form
 *       tiles of 1024; every moment of every sphere is one chain from 0 over its rows of the tile in ascending pixel order;
 *       the tiles' values are added from 0, tiles ascending inside a view, views ascending.  The cost runs in the same
 *       order over the pixels with dist != 0, then over the tiles, as a COMPENSATED chain: a pair (hi, lo) from (0, 0),
 *       each term x added by t = hi + x, b = t - hi, lo += (hi - (t - b)) + (x - b), hi = t (a tile's lo is added to lo);
 *       cost = hi + lo, within an ulp or two of the exact sum of the squares.
 *       A entry (a, c), a >= c, is a chain from 0 over the spheres in ascending order
 *       -- a sphere without a row is skipped -- of (Jc[0,a] t0 + Jc[1,a] t1) + Jc[2,a] t2, t_k = (S_k0 Jc[0,c] + S_k1 Jc[1,c])
 *       + S_k2 Jc[2,c]; g_a is minus the chain of (Jc[0,a] h0 + Jc[1,a] h1) + Jc[2,a] h2.  Bitwise reproducible; a sample's
 *       result does not depend on the batch it is in or on the launch shape; no host synchronisation.
 *       workspace: 16-byte aligned, shr_sphere_icp_normal_workspace_bytes(B, V, J, W, H) bytes (-1 on a negative size):
 *       8 (12 J + 4) bytes per (sample, view, tile), written by the call before it is read.
 *   Argument rules, checked before the B == 0 no-op: 1 <= H, W; 1 <= V; 1 <= J; B >= 0; max_dist >= 0, +inf allowed
 *   (SHR_EINVAL otherwise); H, W above 2048, J above 64, B or B V above 65535: SHR_ETOOLARGE.  B == 0 is a no-op.  NULLs
 *   other than moments, dist and owner, and misaligned pointers (4 bytes; A, g, cost, moments 8; view_centres, workspace 16):
 *   SHR_EINVAL. */
long long shr_sphere_icp_normal_workspace_bytes(int B, int V, int J, int W, int H);
int shr_sphere_icp_normal(const float *observed      /* [B,V,H,W] */,
                          const float *view_centres  /* [B,V,J,4]: shr_view_vertices_fwd of the keypoints */,
                          const float *radii         /* [J] */,
                          const float *view          /* [B,V,4,4] */,
                          const float *jac           /* [B,3J,26]: shr_pose_keypoints_jacobian's */,
                          int B, int V, int J, int W, int H, float ax, float bx, float ay, float by,
                          float fg_max, float max_dist,
                          double *A, double *g, double *cost, int32_t *count,
                          double *moments /* [B,J,12] or NULL */, float *dist /* [B,V,H,W] or NULL */,
                          int32_t *owner /* [B,V,H,W] or NULL */, void *workspace, void *stream);

/* The model-to-data term of the sphere fit: Gauss-Newton rows of the RENDERED spheres against observed depth ---------------
 * The reference fits the sphere model with MSELoss(render, observed) + 500 DataToModelLoss (mesh/multiview_utility.py:96-129);
 * shr_sphere_icp_normal above is the second term, this entry is the first: the spheres are rendered as BallRender.forward
 * and the min over the sphere axis render them (mesh/render.py:26-53, :87-89), the render is compared with the
 * observation, and every model pixel gives a row.  A sphere that lies over observed background, or in front of the
 * observed surface, gives no row to shr_sphere_icp_normal and many to this entry.  The reference has no counterpart of
 * the normal equations.  One evaluation of the combined fit is
 *   shr_pose_keypoints_jacobian(trial) -> shr_view_vertices_fwd (NV := J) -> shr_sphere_icp_normal
 *     -> shr_sphere_render_normal(accumulate = 1) -> shr_pose_lm_step
 * on one stream, without a host synchronisation: capturable in a hipGraph.
 *   shr_sphere_render_normal   the normal equations of weight / 2 sum e^2, e = D - O', over the model pixels of all views
 *       with respect to the 26 pose parameters.  observed, view_centres, radii, view, jac, ax, bx, ay, by, fg_max:
 *       shr_sphere_icp_normal's.
 *       Render.  All fp32, one correctly rounded operation per written operator, nothing contracted.  Pixel (row i, column
 *       j) has xg = ax (float)j + bx, yg = ay (float)i + by.  D = background, owner = -1, behind = true; for k ascending
 *       with (x, y, z) = view_centres[b,v,k,0..2], r = radii[k]: dx = xg - x, dy = yg - y, q = (r r - dx dx) - dy dy
 *       (shr_sphere_raster_fwd's sequence); the sphere HITS iff q > 0.01f, and then d = z - sqrt(q), the root correctly
 *       rounded (no root is taken otherwise).  A hit with d < D is taken: D = d, owner = k (a NaN is never taken, equal
 *       depths keep the smallest index).  A hit with d == D while owner == -1 and behind, that is exactly AT the
 *       background with every lower sphere hitting strictly behind it, is taken too: torch.min's first index over maps
 *       that hold the background where a sphere misses.  After a hit behind = behind && d > background; after a miss
 *       behind = false.  For a power-of-two W == H == S, (ax, bx, ay, by) = (300 / S, -150, 300 / S, -150) and
 *       background = 100 the grid is shr_sphere_raster_fwd's bit for bit: depth equals its depth in every bit and owner
 *       its argmin with 255 as -1.
 *       -> depth[B,V,H,W] fp32 (or NULL) = D; owner[B,V,H,W] int32 (or NULL).  Every element of a map that is given is
 *       written, whatever the observation holds.
 *       Residual.  A pixel whose observed depth is a NaN gives no term and no row.  Otherwise O' = observed < fg_max ?
 *       observed : background and e = (double)D - (double)O'.  The pixel's cost term is min(|e|, (double)max_resid)^2: a
 *       truncated quadratic; a pixel without an owner over an observed point has D = background and pays its term, but
 *       has no row.
 *       Row.  A pixel gives a row iff it has an owner, |e| < max_resid and, recomputed in fp64 from the fp32 xg, yg, x, y, r
 *       of the owner, s = sqrt((r r - dx dx) - dy dy) with dx = xg - x, dy = yg - y is finite and > 0.  Then the gradient
 *       of D with respect to the owner's centre in the view's frame is (-dx / s, -dy / s, 1), taken back to the model
 *       frame in fp64 with shr_pose_icp_normal_views' association and negated: u_j = -((R0j v0 + R1j v1) + R2j v2)
 *       (u = -R^T grad).  The row is d e / d params = -u^T jac[3 owner .. 3 owner + 2, :]: shr_sphere_icp_normal's
 *       convention, so that the two entries' A and g add.  A pixel with e = 0 still gives a row.
 *       -> moments[B,J,12] fp64 (or NULL), for the rows owned by sphere j: S = sum u u^T as (xx, xy, xz, yy, yz, zz),
 *       h = sum e u (3), sum e^2 over the rows, the number of rows (as a double), and one spare 0: this term's own,
 *       unweighted.  count[B] int32: the rows, likewise.
 *       weight and accumulate.  With A_r = sum_j Jc_j^T S_j Jc_j, g_r = -sum_j Jc_j^T h_j (Jc_j = jac[3j .. 3j + 2, :], all
 *       26 columns of every sphere) and cost_r = the sum of the cost terms over ALL pixels of all views:
 *         accumulate == 0:  A = w A_r, g = w g_r, cost = w cost_r                  (w = (double)weight)
 *         accumulate == 1:  A += w A_r, g += w g_r, cost += w cost_r: one product and one sum per entry, on top of what
 *                           the buffers hold -- the output of a preceding shr_sphere_icp_normal.  The LOWER triangle of A
 *                           is read and the sum written to both triangles.  With weight == 0 the three are not touched.
 *       Summation order (the contract), shr_sphere_icp_normal's word for word: fixed-order fp64 chains, no atomics.  The
 *       pixels of a view in row-major order form tiles of 1024; every moment of every sphere is one chain from 0 over its
 *       rows of the tile in ascending pixel order; the tiles' values are added from 0, tiles ascending inside a view,
 *       views ascending.  The cost runs in the same order over the pixels with a term != 0, then over the tiles, as a
 *       COMPENSATED chain: a pair (hi, lo) from (0, 0), each term x added by t = hi + x, b = t - hi,
 *       lo += (hi - (t - b)) + (x - b), hi = t (a tile's lo is added to lo); cost_r = hi + lo.  A_r entry (a, c), a >= c, is
 *       a chain from 0 over the spheres in ascending order -- a sphere without a row is skipped -- of
 *       (Jc[0,a] t0 + Jc[1,a] t1) + Jc[2,a] t2, t_k = (S_k0 Jc[0,c] + S_k1 Jc[1,c]) + S_k2 Jc[2,c], written to both
 *       triangles: bit-symmetric; g_r,a is minus the chain of (Jc[0,a] h0 + Jc[1,a] h1) + Jc[2,a] h2.  Bitwise
 *       reproducible; a sample's result does not depend on the batch it is in or on the launch shape; no host
 *       synchronisation.  Every pixel meets every sphere: nothing is pruned.
 *       workspace: 16-byte aligned, shr_sphere_render_normal_workspace_bytes(B, V, J, W, H) bytes (-1 on a negative size):
 *       8 (12 J + 4) bytes per (sample, view, tile), written by the call before it is read.
 *   Argument rules, checked before the B == 0 no-op: 1 <= H, W; 1 <= V; 1 <= J; B >= 0; max_resid >= 0, +inf allowed;
 *   weight finite and >= 0; background finite; accumulate 0 or 1 (SHR_EINVAL otherwise); H, W above 2048, J above 64, B or
 *   B V above 65535: SHR_ETOOLARGE.  B == 0 is a no-op.  NULLs other than moments, depth and owner, and misaligned pointers
 *   (4 bytes; A, g, cost, moments 8; view_centres, workspace 16): SHR_EINVAL.  Centres and radii are taken to be finite
 *   (NOT checked); the rotation is NOT checked to be orthonormal. */
long long shr_sphere_render_normal_workspace_bytes(int B, int V, int J, int W, int H);
int shr_sphere_render_normal(const float *observed      /* [B,V,H,W] */,
                             const float *view_centres  /* [B,V,J,4]: shr_view_vertices_fwd of the keypoints */,
                             const float *radii         /* [J] */,
                             const float *view          /* [B,V,4,4] */,
                             const float *jac           /* [B,3J,26]: shr_pose_keypoints_jacobian's */,
                             int B, int V, int J, int W, int H, float ax, float bx, float ay, float by,
                             float fg_max, float background, float max_resid, float weight, int accumulate,
                             double *A, double *g, double *cost, int32_t *count,
                             double *moments /* [B,J,12] or NULL */, float *depth /* [B,V,H,W] or NULL */,
                             int32_t *owner /* [B,V,H,W] or NULL */, void *workspace, void *stream);

/* The terms beside the image terms of the sphere fit: predicted keypoints as soft anchors, hinges at the joint limits ------
 * shr_sphere_icp_normal and shr_sphere_render_normal above are the two image terms; one depth view does not determine the
 * pose (a finger the view hides is held by shr_pose_lm_step's stiffness alone), and nothing keeps a fitted flex or abduction
 * inside the range a hand can take.  This entry adds the two terms every sphere-model tracker carries beside its image
 * terms: the key-points predicted per view -- they ARE the sphere centres (mesh/render.py:65-88) -- as soft anchors, and
 * hinge penalties at the limits of the pose parameters (the support of dataset/joint_angle.py:7-236's distribution is the
 * table joint_angle.pose_limits() gives).  The reference has no counterpart of the normal equations.  Collision rows couple
 * two spheres, do not fit the per-sphere record and are NOT part of this entry.  One evaluation of the fit is
 *   shr_pose_keypoints_jacobian(trial) -> shr_view_vertices_fwd (NV := J) -> shr_sphere_icp_normal
 *     -> shr_sphere_render_normal(accumulate = 1) -> shr_sphere_prior_normal(accumulate = 1) -> shr_pose_lm_step
 * on one stream, without a host synchronisation: capturable in a hipGraph.
 *   shr_sphere_prior_normal   the normal equations of 1/2 (kp_weight sum w min(|e|, kp_max)^2 + limit_weight sum h^2) with
 *       respect to the 26 pose parameters.  view_centres, view, jac: shr_sphere_icp_normal's; params[B,26]: the pose the
 *       centres belong to (NOT checked).
 *       Keypoint term.  keypoints[B,V,J,3] fp32 in view v's frame (or NULL: no keypoint term), confidence[B,V,J] fp32 >= 0
 *       (or NULL: 1; negative values are NOT checked).  For each pair (v, j): e = k - c in fp64 from the fp32 keypoints
 *       and view_centres, target minus model as shr_sphere_icp_normal's p - c.  The pair has NO term and no row if a
 *       component of k is a NaN or the confidence w is 0 or a NaN.  Otherwise n2 = (e0 e0 + e1 e1) + e2 e2 and
 *       cap2 = (double)kp_max (double)kp_max (exact; +inf for kp_max = +inf); the pair is SATURATED iff not n2 < cap2 (a
 *       distance exactly equal to kp_max is saturated; kp_max = +inf never saturates a finite e), and its cost term is
 *       w t, t = n2 if n2 < cap2, else cap2: w min(|e|, kp_max)^2, a truncated quadratic.  A pair that is not saturated
 *       gives THREE rows, one per axis a of the view's frame: residual e_a, direction u = row a of view's top-left 3 x 3
 *       AS GIVEN (the rotation is NOT checked to be orthonormal), row = d e_a / d params = -u^T jac[3j .. 3j + 2, :]:
 *       shr_sphere_icp_normal's convention, so that the entries' A and g add.  A pair with e = 0 still gives its three
 *       rows: the directions are the axes, there is no singular case.
 *       -> moments[B,J,12] fp64 (or NULL), sphere j over its pairs with rows: S = sum w u u^T as (xx, xy, xz, yy, yz, zz),
 *       h = sum w e_a u (3), sum w e_a^2, the number of PAIRS that gave rows (as a double), and one spare 0: the keypoint
 *       term's own, NOT weighted by kp_weight.  Without keypoints every moment is 0.
 *       Limit term.  lower[26], upper[26] fp32 (both NULL: no limit term).  For parameter i, p = params[b,i]:
 *       h_i = p > upper_i ? (double)p - (double)upper_i : (p < lower_i ? (double)p - (double)lower_i : 0).  A comparison
 *       with a NaN never fires and an unlimited parameter carries -inf / +inf, which never fire; a value exactly ON a
 *       bound gives no row and cost 0.  A parameter with h_i != 0 gives one row: limit_weight on A_ii, limit_weight h_i
 *       on g_i, limit_weight h_i^2 in the cost.
 *       -> count[B,2] int32: the pairs that gave rows (keypoint rows / 3) and the limit rows, whatever the weights.
 *       weights and accumulate.  The keypoint part is USED iff keypoints != NULL and kp_weight > 0, the limit part iff
 *       lower != NULL and limit_weight > 0; a part that is not used is an exact +0 everywhere.  With
 *         A_p[a,c] = kw A_k[a,c] + (a == c and h_a != 0 ? lw : 0),  A_k = sum_j Jc_j^T S_j Jc_j  (Jc_j = jac[3j .. 3j + 2, :])
 *         g_p[a]   = kw (0 - G_a) + (h_a != 0 ? lw h_a : 0),        G = sum_j Jc_j^T h_j
 *         cost_p   = kw K + lw L         (kw = (double)kp_weight, lw = (double)limit_weight)
 *         accumulate == 0:  A = A_p, g = g_p, cost = cost_p
 *         accumulate == 1:  A += A_p, g += g_p, cost += cost_p: one sum per entry on top of what the buffers hold -- the
 *                           output of the image terms.  The LOWER triangle of A is read and the sum written to both
 *                           triangles, so A stays bit-symmetric.  If neither part is used the three are not touched.
 *       Summation order (the contract): fixed-order fp64 chains, no atomics, nothing contracted.  Every moment of sphere j
 *       is a chain from 0 over the views in ascending order of the pair's SUBTOTAL, the subtotal a chain from 0 over the
 *       axes a = 0, 1, 2 of one product x y: (w u_p) u_q for S_pq, (w e_a) u_p for h_p, (w e_a) e_a for sum w e_a^2 -- two
 *       identical views give exactly twice one view's moments.  A_k entry (a, c), a >= c, is a chain from 0 over the
 *       spheres in ascending order -- a sphere without a row is skipped -- of (Jc[0,a] t0 + Jc[1,a] t1) + Jc[2,a] t2,
 *       t_k = (S_k0 Jc[0,c] + S_k1 Jc[1,c]) + S_k2 Jc[2,c], written to both triangles: bit-symmetric; G_a is the chain of
 *       (Jc[0,a] h0 + Jc[1,a] h1) + Jc[2,a] h2.  K is a chain from 0 over the spheres in ascending order of the sphere's
 *       own chain from 0 over the views in ascending order of w t; L is a chain from 0 over i ascending of h_i h_i; the
 *       limits come after the spheres: cost_p = kw K + lw L.  Bitwise reproducible; a sample's result does not depend on
 *       the batch it is in or on the launch shape (one workgroup per sample); no host synchronisation.
 *       workspace: none is needed; shr_sphere_prior_normal_workspace_bytes(B, V, J) is 0 (-1 on a negative size) and
 *       workspace may be NULL (16-byte aligned if given).
 *   Argument rules, checked before the B == 0 no-op: 1 <= V; 1 <= J; B >= 0; kp_max >= 0, +inf allowed; kp_weight and
 *   limit_weight finite and >= 0; accumulate 0 or 1; lower and upper both NULL or both given; confidence without keypoints
 *   (SHR_EINVAL otherwise); J above 64, B or B V above 65535: SHR_ETOOLARGE.  B == 0 is a no-op.  NULLs other than
 *   keypoints, confidence, lower, upper, moments and workspace, and misaligned pointers (4 bytes; A, g, cost, moments 8;
 *   view_centres, workspace 16): SHR_EINVAL. */
long long shr_sphere_prior_normal_workspace_bytes(int B, int V, int J);
int shr_sphere_prior_normal(const float *view_centres  /* [B,V,J,4]: shr_view_vertices_fwd of the keypoints */,
                            const float *view          /* [B,V,4,4] */,
                            const float *jac           /* [B,3J,26]: shr_pose_keypoints_jacobian's */,
                            const float *params        /* [B,26]: the pose the centres belong to */,
                            const float *keypoints     /* [B,V,J,3] in view v's frame, or NULL: no keypoint term */,
                            const float *confidence    /* [B,V,J] >= 0, or NULL = 1 */,
                            float kp_weight, float kp_max,
                            const float *lower /* [26] */, const float *upper /* [26]; both NULL: no limit term */,
                            float limit_weight, int B, int V, int J, int accumulate,
                            double *A, double *g, double *cost, int32_t *count /* [B,2]: keypoint rows / 3, limit rows */,
                            double *moments /* [B,J,12] or NULL */, void *workspace, void *stream);

/* The term against self-penetration of the sphere fit: pairs of spheres held apart ------------------------------------------
 * The three entries above leave nothing in the fit's energy that keeps two fingers, or a finger and the palm, from passing
 * through each other.  The reference carries that energy as CollisionLoss (mesh/render.py:145-176): the sum over a table
 * of 690 pairs of relu(36 - |c_a - c_b|^2), which shr_pair_losses gives as a first-order loss.  That hinge is NOT the square
 * of a residual, so it has no Gauss-Newton rows; the fit uses h = m - |c_a - c_b| instead, whose square has the same
 * support, with the minimum distance m a PER-PAIR table: the shipped radii are a fat proxy (at the rest pose 26 of the 690
 * pairs are closer than r_a + r_b), so "the radius sum" cannot be the threshold, and the reference's constant 6 mm is one
 * choice of the table among others.  The reference has no counterpart of the normal equations.  A row couples TWO
 * spheres; it does not fit the per-sphere moments[B,J,12] of the entries above and is assembled per pair.  The term is
 * view-independent: it reads the MODEL-frame keypoints, not view_centres, and takes no view.  One evaluation of the fit is
 *   shr_pose_keypoints_jacobian(trial) -> shr_view_vertices_fwd (NV := J) -> shr_sphere_icp_normal
 *     -> shr_sphere_render_normal(accumulate = 1) -> shr_sphere_prior_normal(accumulate = 1)
 *     -> shr_sphere_collision_normal(accumulate = 1) -> shr_pose_lm_step
 * on one stream, without a host synchronisation: capturable in a hipGraph.
 *   shr_sphere_collision_normal   the normal equations of 1/2 weight sum_k h_k^2 over the ACTIVE pairs with respect to the
 *       26 pose parameters.  centres[B,J,4]: the keypoints shr_pose_keypoints_jacobian writes beside jac, in the model
 *       frame (component 3 is not read); jac: shr_sphere_icp_normal's.
 *       Pairs.  Pair k is (a, b, m) = (pair_a[k], pair_b[k], pair_min[k]), m in mm.  A pair with an index outside
 *       0 .. J - 1, with a == b, or with m not > 0 (a NaN included) is SKIPPED: no term, no row, penetration 0, and
 *       nothing is read for it -- a bad table cannot make the entry read out of bounds.  Otherwise, in fp64 from the fp32
 *       centres: e = c_a - c_b, n = sqrt((e0 e0 + e1 e1) + e2 e2), the root correctly rounded.  The pair is ACTIVE iff
 *       n < (double)m: a distance exactly equal to m is not active, the reference's hinge at its kink, and a NaN never
 *       fires.  An active pair has h = (double)m - n and the cost term h h.  It gives ONE row iff also n > 0: coincident
 *       centres pay m^2 and have no direction, so no row.  Direction u = e / n (three correctly rounded quotients),
 *       D_ic = (double)jac[3a + i, c] - (double)jac[3b + i, c], and
 *         row_c = 0 - ((u0 D_0c + u1 D_1c) + u2 D_2c) = d h / d params_c:
 *       shr_sphere_icp_normal's convention, so that the entries' A and g add.  Swapping a and b negates e, u and D
 *       exactly and leaves every output bit for bit.
 *       -> count[B] int32: the pairs that gave rows, whatever the weight.  penetration[B,K] fp64 (or NULL): h at an active
 *       pair, 0 elsewhere; the term's own, NOT weighted.
 *       weight and accumulate.  The term is USED iff pair_a != NULL, K > 0 and weight > 0; a term that is not used is an
 *       exact +0 everywhere.  With A_c = sum rows row row^T, G = sum rows h row, C = sum active h h and w = (double)weight:
 *         accumulate == 0:  A = w A_c, g = w G, cost = w C
 *         accumulate == 1:  A += w A_c, g += w G, cost += w C: one product and one sum per entry on top of what the
 *                           buffers hold -- the output of the other terms.  The LOWER triangle of A is read and the sum
 *                           written to both triangles, so A stays bit-symmetric.  If the term is not used the three are
 *                           not touched.
 *       Summation order (the contract): fixed-order fp64 chains, no atomics, nothing contracted.  A_c entry (a, c), a >= c,
 *       is a chain from 0 over the pairs with rows in ascending k of row_a row_c, written to both triangles:
 *       bit-symmetric; G_a is the chain over the same pairs of h row_a; C is the chain from 0 over the ACTIVE pairs in
 *       ascending k of h h.  Bitwise reproducible; a sample's result does not depend on the batch it is in or on the
 *       launch shape (one workgroup per sample); no host synchronisation.  Every pair of the table is met: nothing is
 *       pruned.
 *       workspace: none is needed; shr_sphere_collision_normal_workspace_bytes(B, J, K) is 0 (-1 on a negative size) and
 *       workspace may be NULL (16-byte aligned if given).
 *   Argument rules, checked before the B == 0 no-op: 1 <= J; B >= 0; K >= 0; weight finite and >= 0; accumulate 0 or 1;
 *   pair_a, pair_b and pair_min all NULL or all given; K > 0 without them (SHR_EINVAL otherwise); J above 64, K above 4096,
 *   B above 65535: SHR_ETOOLARGE.  B == 0 is a no-op.  NULLs other than the three pair arrays, penetration and workspace,
 *   and misaligned pointers (4 bytes; A, g, cost, penetration 8; centres, workspace 16): SHR_EINVAL.  The Jacobian and the
 *   centres of the pairs that are met are taken to be finite apart from the NaN rule above (NOT checked). */
long long shr_sphere_collision_normal_workspace_bytes(int B, int J, int K);
int shr_sphere_collision_normal(const float *centres   /* [B,J,4]: shr_pose_keypoints_jacobian's keypoints, MODEL frame */,
                                const float *jac       /* [B,3J,26]: shr_pose_keypoints_jacobian's */,
                                const int32_t *pair_a, const int32_t *pair_b /* [K] */, const float *pair_min /* [K] mm */,
                                float weight, int B, int J, int K, int accumulate,
                                double *A, double *g, double *cost, int32_t *count /* [B] */,
                                double *penetration /* [B,K] or NULL */, void *workspace, void *stream);

/* The pose-VAE prior of the sphere fit: which hand poses are plausible ----------------------------------------------------------
 * None of the terms above knows which poses a hand takes: where the view hides a finger, nothing holds it.  The reference
 * has such a term, the frozen PoseVae behind --prior (network/pose_vae.py:11-99), a 123-256-256-32-256-256-123 MLP with
 * GroupNorm(16, 256) and ReLU trained on the model-frame keypoints / 100 (network/pose_vae.py:169), used first-order as
 * 1e-2 prior_loss(xyz / 100) (network/create_network_and_criterion.py:164, 238-243).  The reference has no counterpart of the
 * normal equations.  Here it is a Gauss-Newton term over the J = 41 sphere centres c (mm, MODEL frame, as the collision
 * term reads them): with x = c / 100 (123 values, one IEEE fp32 division each),
 *   r = 100 (x - recon(x))  [123, mm],   mu = mu(x)  [32],   z = mu: NO reparameterisation draw and NO logvar term,
 *   energy = weight (sum_i r_i^2 + latent_weight sum_k mu_k^2).
 * There is NO truncation of r: a saturating cut is what silences the other terms where this one is needed.  One evaluation
 * of the fit is
 *   shr_pose_keypoints_jacobian(trial) -> ... -> shr_sphere_collision_normal(accumulate = 1)
 *     -> shr_pose_vae_normal(accumulate = 1) -> shr_pose_lm_step
 * on one stream, without a host synchronisation: capturable in a hipGraph.
 *   shr_pose_vae_normal   the normal equations of 1/2 energy with respect to the 26 pose parameters.  kp[B,J,4] and
 *       jac[B,3J,26]: shr_pose_keypoints_jacobian's (component 3 of kp is not read).
 *       Forward mode.  The exact Jacobian is J_r = (I - D) jac with D the network's 123 x 123 input Jacobian, which is NOT
 *       formed: M0 = [x | jac] (123 x 27: the value column and the 26 pose tangents; the layers are linear in a tangent,
 *       so the tangents carry jac itself and the 100 of x and the 100 of r cancel) passes through the network as one
 *       matrix, all fp32:
 *         linear     W M, the bias added to column 0 only.  Every element is ONE fmaf chain over k = 0 .. K - 1 ascending
 *                    (v_mfma_f32_32x32x2_f32: fp32 in, fp32 accumulate) that starts from the bias (column 0) or +0.  The
 *                    exception is mu (256 -> 32): four chains P_v over k = 64 v .. 64 v + 63, P_0 starting from the bias,
 *                    summed ((P_0 + P_1) + P_2) + P_3.
 *         GroupNorm  16 groups of 16 channels, eps 1e-5, biased variance.  Value column: s = the 16 entries summed as
 *                    (chain over channels 0-3, 8-11 of the group) + (chain over 4-7, 12-15), m = s / 16, d = h - m,
 *                    q = sum d d in the same order, rs = 1 / sqrt(q / 16 + eps) (both correctly rounded), h^ = d rs,
 *                    y = h^ gamma + beta.  Tangent column: y' = (gamma rs) ((h' - m1) - h^ m2), m1 = sum h' / 16,
 *                    m2 = sum (h^ h') / 16, the sums in that order.
 *         ReLU       y where y > 0, else +0; a tangent passes where the VALUE column's y > 0.
 *       Rows, fp64 from the fp32 results: r_i = 100 ((double)x_i - (double)recon_i),
 *       J_r[i][c] = (double)jac[i][c] - (double)recon'[i][c]; latent row k is (mu_k, mu'_k), exact conversions.
 *       -> residual[B,123] fp64 (or NULL): r in mm.  latent[B,32] fp64 (or NULL): mu.  relu_mask[B,32] uint32 (or NULL):
 *       the 1024 ReLU decisions of the value column, unit u = 256 l + channel with l = 0 .. 3 the GroupNorm layers in network
 *       order (base 1, base 2, decoder 1, decoder 2): bit u & 31 of word u >> 5 is set iff y > 0.  The three are the term's
 *       own, not weighted, and are written whatever the weight.
 *       weight and accumulate.  With S = sum_i J_r[i] J_r[i]^T, G = sum_i r_i J_r[i], C = sum_i r_i r_i over rows 0 .. 122
 *       and S_l, G_l, C_l the same over the 32 latent rows, lw = (double)latent_weight and w = (double)weight:
 *         A_r = S + lw S_l, g_r = G + lw G_l, cost_r = C + lw C_l  (one product and one sum; lw == 0: A_r = S and so on)
 *         accumulate == 0:  A = w A_r, g = w g_r, cost = w cost_r
 *         accumulate == 1:  A += w A_r, g += w g_r, cost += w cost_r: one product and one sum per entry on top of what the
 *                           buffers hold.  The LOWER triangle of A is read and the sum written to both triangles.
 *         weight == 0:      A, g and cost are NOT touched, in either mode (they may be NULL); with no optional output
 *                           either, nothing is launched.
 *       Summation order (the contract): fixed-order fp64 chains from 0 in ascending row index, no atomics, nothing
 *       contracted; entry (a, c), a >= c, is written to both triangles: bit-symmetric.  Bitwise reproducible; a frame's
 *       result does not depend on the batch it is in or on B (one workgroup per frame); no host synchronisation.
 *       blob: the network packed by the host, blob_floats = shr_pose_vae_blob_floats() = 215 200 fp32.  Per linear layer in
 *       network order (base.0, base.3, mu, decoder.0, decoder.3, decoder.6; K = 124, 256, 256, 32, 256, 256 with the 123
 *       inputs padded to even K by a zero row, OUT = 256, 256, 32, 256, 256, 128 with the 123 outputs padded by zero rows):
 *       the weight, k-major, element ((q OUT + o) 2 + h) 2 + s = W[o][4 q + 2 s + h]; the bias [OUT]; and behind the four
 *       layers followed by a GroupNorm its gamma [256] and beta [256].
 *       workspace: none is needed; shr_pose_vae_normal_workspace_bytes(B, J) is 0 (-1 on a negative size).
 *   Argument rules, checked before the B == 0 no-op: J == 41; B >= 0; weight and latent_weight finite and >= 0; accumulate
 *   0 or 1; blob_floats == shr_pose_vae_blob_floats() (SHR_EINVAL otherwise); B above 65535: SHR_ETOOLARGE.  B == 0 is a
 *   no-op.  NULL kp, jac or blob, NULL A, g or cost with weight > 0, and misaligned pointers (4 bytes; A, g, cost, residual,
 *   latent 8; kp, blob, workspace 16): SHR_EINVAL.  kp and jac are taken to be finite (NOT checked). */
int shr_pose_vae_blob_floats(void);
long long shr_pose_vae_normal_workspace_bytes(int B, int J);
int shr_pose_vae_normal(const float *kp        /* [B,J,4]: shr_pose_keypoints_jacobian's keypoints, MODEL frame */,
                        const float *jac       /* [B,3J,26]: shr_pose_keypoints_jacobian's */,
                        const float *blob      /* [blob_floats]: the packed network */, int blob_floats,
                        float weight, float latent_weight, int B, int J, int accumulate,
                        double *A, double *g, double *cost, double *residual /* [B,123] or NULL */,
                        double *latent /* [B,32] or NULL */, uint32_t *relu_mask /* [B,32] or NULL */,
                        void *workspace, void *stream);

/* A sequence of frames fitted jointly: the temporal term and the block-tridiagonal step ----------------------------------------
 * Every sample of the entries above is an island, and the data is video.  The reference carries the term for that as
 * TemporalSmoothnessLoss (network/util_modules.py:360-381), ClampedL2lLoss(2500) (network/util_modules.py:349-358) between
 * the joints of consecutive samples, weight 1.0 in MultiTaskLoss (create_network_and_criterion.py:242-245).  A row of it
 * couples frame t and frame t + 1, so the normal equations of a sequence are block-TRIDIAGONAL and the accept decision
 * belongs to the sequence, not the frame: shr_pose_lm_step cannot take it.  The reference has no counterpart of the normal
 * equations or of the solve.  Two departures from the reference, both deliberate: it clamps every COMPONENT of the
 * difference at +-2500 before squaring, the term here truncates the squared NORM of a sphere's difference at ts_max^2
 * (section 4.4r's kp_max rule; with ts_max = +inf and at hand scale, where no component reaches 2500 mm, the two energies
 * agree up to the reference's mean over elements); and it DETACHES the previous frame, a one-sided pull of frame t + 1
 * towards frame t, while the Gauss-Newton term is SYMMETRIC: both frames of a pair receive rows.
 * Layout: B = S T frames, S sequences of T consecutive frames, the frames of a sequence adjacent in the batch; frame b is
 * frame t = b mod T of sequence b / T.  One evaluation of the fit is
 *   shr_pose_keypoints_jacobian(trial) -> shr_view_vertices_fwd (NV := J) -> shr_sphere_icp_normal
 *     -> shr_sphere_render_normal(accumulate = 1) -> shr_sphere_prior_normal(accumulate = 1)
 *     -> shr_sphere_collision_normal(accumulate = 1) -> shr_sphere_temporal_normal(accumulate = 1) -> shr_pose_lm_seq_step
 * on one stream, without a host synchronisation: capturable in a hipGraph.
 *   shr_sphere_temporal_normal   the normal equations of 1/2 w sum min(n2, ts_max^2) with respect to the 26 T parameters
 *       of a sequence.  keypoints[B,J,4] and jac[B,3J,26]: shr_pose_keypoints_jacobian's outputs for the trial poses, in
 *       the MODEL frame (component 3 is not read): no view enters.  frame_weight[B] or NULL (1): entry t weighs the pair
 *       (t, t + 1); the last entry of a sequence is not read.  A pair whose weight is not > 0 (0, negative, a NaN) has no
 *       term.  w of a pair = (double)temporal_weight (double)frame_weight.
 *       The term.  Per pair (t, t + 1) with a weight and per sphere j, in fp64 from the fp32 values:
 *       e = c_j(t + 1) - c_j(t), n2 = (e0 e0 + e1 e1) + e2 e2.  A NaN n2 gives NO term: no cost, no row.  Otherwise the
 *       cost term is min(n2, cap2), cap2 = (double)ts_max (double)ts_max, and the sphere gives THREE rows iff n2 < cap2: a
 *       difference of exactly ts_max is saturated, +inf never saturates, and e = 0 still gives rows.  The row of axis a
 *       has +jac[3j + a, :] of frame t + 1 in frame t + 1's columns and -jac[3j + a, :] of frame t in frame t's; its
 *       residual is e_a.
 *       -> A[B,26,26], the DIAGONAL blocks: frame b receives w_prev P + w_next N, P and N the sums of Jc_j(b)^T Jc_j(b) over
 *       the spheres with rows of the pair before it and of the pair after it.  g[B,26], the gradient of 1/2 the cost in
 *       the family's convention, so that the entries' A and g add: w_prev sum Jc_j(b)^T e_j(prev) + w_next (0 - sum
 *       Jc_j(b)^T e_j(next)).  cost[B]: the pair's cost w sum_j min(n2, cap2) belongs to its LATER frame, t + 1.
 *       count[B] int32: the spheres with rows of the pair (t, t + 1), stored at t + 1, 0 at the first frame of a
 *       sequence; whatever temporal_weight.
 *       -> E[B,26,26], the OFF-DIAGONAL blocks, ALWAYS WRITTEN, NEVER accumulated: E_t couples frame t (rows) with frame
 *       t + 1 (columns), E_t = 0 - w sum_j Jc_j(t)^T Jc_j(t + 1).  It is an exact +0 for the last frame of every sequence,
 *       for a pair without a weight, and for every frame when temporal_weight == 0.
 *       accumulate == 0: A, g, cost = the term's (exact +0 where a frame has no weighted pair).  accumulate == 1: the
 *       term is ADDED, one product per pair and one sum per entry on top of what the buffers hold; the LOWER triangle of
 *       A is read and the sum written to both triangles, so A stays bit-symmetric; a frame none of whose pairs has a
 *       weight -- every frame when temporal_weight == 0 or T == 1 -- is not touched.
 *       Summation order (the contract): fixed-order fp64 chains, no atomics, nothing contracted.  Every sum over the
 *       spheres is a chain from 0 over the spheres with rows, ascending; a sphere's term is its three axes in ascending
 *       order, ((x0 y0 + x1 y1) + x2 y2).  P and N are separate chains.  Bitwise reproducible; a sequence does not depend
 *       on the other sequences of the batch; the launch shape is one workgroup per frame; no host synchronisation.
 *       workspace: none is needed; shr_sphere_temporal_normal_workspace_bytes(B, T, J) is 0 (-1 on a negative size).
 *   Argument rules, checked before the B == 0 no-op: 1 <= J, 1 <= T, B >= 0 and B % T == 0, ts_max >= 0 (+inf allowed),
 *   temporal_weight finite and >= 0, accumulate 0 or 1 (SHR_EINVAL otherwise); J above 64, B above 65535: SHR_ETOOLARGE.
 *   NULLs other than frame_weight and workspace, and misaligned pointers (4 bytes; A, g, E, cost 8; keypoints, workspace
 *   16): SHR_EINVAL.
 *   shr_pose_lm_seq_begin, shr_pose_lm_seq_step   shr_pose_lm_begin / shr_pose_lm_step with the unit of decision raised
 *       from the crop to the sequence.  state: shr_pose_lm_seq_state_bytes(B) = 11 520 B bytes (1440 doubles per frame:
 *       the accepted pose's A, E, g, the pose, params0, and in a sequence's first frame its total cost, lambda and
 *       counters); workspace: shr_pose_lm_seq_workspace_bytes(B) = 11 072 B bytes (1384 doubles per frame: L_t, W_t, y_t),
 *       needed with solve != 0; both 8-byte aligned, -1 for B < 0.
 *       Bookkeeping per sequence: one lambda; total_s = the chain over t ascending of (cost_data_t + the stiffness term of
 *       frame t, shr_pose_lm_step's chain); the trial of the WHOLE sequence is accepted iff total_s is finite and below the
 *       state's; lambda x 0.3 on accept, x 10 on reject, clamped to [1e-9, 1e6], the first accepted step leaving it;
 *       cost0[S] is written by the first step after begin; cost[S], params[B,26] as shr_pose_lm_step's.
 *       The solve (solve != 0), on the accepted equations: M_t = A_t + diag(mu); the block-tridiagonal system with
 *       diagonal blocks M_t + lambda diag(M_t), off-diagonal blocks E_t and right-hand side -(g_t + mu (p_t - prior_t)),
 *       by block Cholesky forward over t: D_t = (M_t + lambda diag(M_t)) - W_{t-1} W_{t-1}^T (the previous factor's
 *       outer product subtracted entry by entry, k ascending, then the column recurrence of shr_pose_lm_step), L_t L_t^T
 *       = D_t, W_t = E_t^T L_t^-T by 26 triangular solves, then block forward and back substitution; all fp64, every sum
 *       in index order.  One workgroup per sequence.  A pivot that is not positive and finite ANYWHERE in the sequence
 *       writes trial_out = p for the whole sequence.  trial_out[B,26] fp32 = p + delta (may be trial).
 *       With T == 1 every output and the state's pose are shr_pose_lm_step's BIT FOR BIT (E is then not read and may be
 *       NULL).
 *   Argument rules: state given and 8-byte aligned, B >= 0, 1 <= T, B % T == 0 (SHR_EINVAL otherwise), B above 2^24:
 *   SHR_ETOOLARGE, checked before the B == 0 no-op; lambda0 > 0; NULLs other than prior, stiffness, E with T == 1, and
 *   trial_out and workspace without solve; misaligned pointers (4 bytes; A, g, E, cost_data, workspace 8): SHR_EINVAL. */
long long shr_sphere_temporal_normal_workspace_bytes(int B, int T, int J);
int shr_sphere_temporal_normal(const float *keypoints /* [B,J,4]: shr_pose_keypoints_jacobian's, MODEL frame */,
                               const float *jac       /* [B,3J,26]: shr_pose_keypoints_jacobian's */,
                               const float *frame_weight /* [B] or NULL */, float temporal_weight, float ts_max,
                               int B, int T, int J, int accumulate,
                               double *A, double *g, double *E /* [B,26,26] */, double *cost, int32_t *count /* [B] */,
                               void *workspace, void *stream);
long long shr_pose_lm_seq_state_bytes(int B);
long long shr_pose_lm_seq_workspace_bytes(int B);
int shr_pose_lm_seq_begin(const float *params0, int B, int T, float lambda0, void *state, float *trial, void *stream);
int shr_pose_lm_seq_step(void *state, const double *A, const double *g, const double *E, const double *cost_data,
                         const float *trial, const float *prior, const float *stiffness, int solve, int B, int T,
                         float *trial_out, float *params, float *cost /* [S] */, float *cost0 /* [S] */, void *workspace,
                         void *stream);

/* The constant-velocity term of the sequence fit and the block-pentadiagonal step ----------------------------------------------
 * shr_sphere_temporal_normal penalises the first difference c_j(t + 1) - c_j(t): motion itself, so it lags a hand that
 * really moves.  What a tracker carries instead is a constant-velocity prior, the SECOND difference
 * a = (c_j(k - 1) + c_j(k + 1)) - 2 c_j(k): zero on a hand that moves steadily, and a frame without data is interpolated
 * from both neighbours.  The energy is of the family of network/util_modules.py:349-381 (ClampedL2lLoss,
 * TemporalSmoothnessLoss), one difference further; the reference has no counterpart of this term, of its normal
 * equations or of the solve.  A row couples THREE frames, so the normal equations of a sequence gain a second
 * off-diagonal block F and are block-PENTADIAGONAL: shr_pose_lm_seq_step cannot take them.
 * Layout: shr_sphere_temporal_normal's, B = S T, the frames of a sequence adjacent.  One evaluation of the fit is
 *   ... -> shr_sphere_temporal_normal(accumulate = 1) -> shr_sphere_accel_normal(accumulate = 1, accumulate_E = 1 iff the
 *   first-difference entry was launched) -> shr_pose_lm_seq2_step
 * on one stream, without a host synchronisation: capturable in a hipGraph.
 *   shr_sphere_accel_normal   the normal equations of 1/2 w sum min(n2, acc_max^2) with respect to the 26 T parameters of
 *       a sequence.  keypoints[B,J,4] and jac[B,3J,26]: shr_pose_keypoints_jacobian's outputs for the trial poses, in the
 *       MODEL frame (component 3 is not read).  A triple is centred at frame k of its sequence, 1 <= k <= T - 2;
 *       triple_weight[B] or NULL (1): entry k weighs the triple centred at k; the first and last entry of a sequence are
 *       not read.  A triple whose weight is not > 0 (0, negative, a NaN) has no term.  w_k = (double)accel_weight
 *       (double)triple_weight[k].
 *       The term.  Per triple with a weight and per sphere j, in fp64 from the fp32 values:
 *       a = (c_j(k - 1) + c_j(k + 1)) - 2 c_j(k), n2 = (a0 a0 + a1 a1) + a2 a2.  A NaN n2 gives NO term: no cost, no row.
 *       Otherwise the cost term is min(n2, cap2), cap2 = (double)acc_max (double)acc_max, and the sphere gives THREE rows
 *       iff n2 < cap2: exactly acc_max is saturated, +inf never saturates, and a = 0 still gives rows.  The row of axis x
 *       has +jac(k - 1)[3j + x, :] in frame k - 1's columns, -2 jac(k)[3j + x, :] in frame k's and +jac(k + 1)[3j + x, :]
 *       in frame k + 1's; its residual is a_x.
 *       Outputs.  With G_j(x, y) = Jc_j(x)^T Jc_j(y), S_k the spheres with rows of triple k and w_k = 0 outside
 *       1 ... T - 2, frame b receives
 *         A[b] = (w_{b-1} sum_{S_{b-1}} G_j(b, b) + (4 w_b) sum_{S_b} G_j(b, b)) + w_{b+1} sum_{S_{b+1}} G_j(b, b), three
 *                separate chains;
 *         g[b] = (w_{b-1} sum Jc_j(b)^T a_j(b - 1) - (2 w_b) sum Jc_j(b)^T a_j(b)) + w_{b+1} sum Jc_j(b)^T a_j(b + 1), the
 *                gradient of 1/2 the cost in the family's convention, so that the entries' A and g add;
 *         E[b] = (0 - (2 w_b) sum_{S_b} G_j(b, b + 1)) - (2 w_{b+1}) sum_{S_{b+1}} G_j(b, b + 1): frame b's rows, frame
 *                b + 1's columns;
 *         F[b] = w_{b+1} sum_{S_{b+1}} G_j(b, b + 2): frame b's rows, frame b + 2's columns.
 *       cost[B]: a triple's cost w sum_j min(n2, cap2) belongs to its LAST frame, k + 1.  count[B] int32: the spheres with
 *       rows of the triple centred at b - 1, 0 at the first two frames of a sequence; whatever accel_weight.
 *       accumulate governs A, g and cost as in shr_sphere_temporal_normal: 0 writes the term's (exact +0 where a frame has
 *       no weighted triple); 1 ADDS it, the LOWER triangle of A is read and the sum written to both triangles, so A stays
 *       bit-symmetric, and a frame none of whose triples has a weight -- every frame when accel_weight == 0 or T <= 2 -- is
 *       not touched.  accumulate_E == 0 writes E, an exact +0 where the frame has no term; accumulate_E == 1 adds the
 *       term to what E holds (shr_sphere_temporal_normal's E), a frame without a term left alone.  F is ALWAYS WRITTEN,
 *       NEVER accumulated: an exact +0 for the last two frames of a sequence, for a triple without a weight and when
 *       accel_weight == 0.
 *       Summation order (the contract): fixed-order fp64 chains, no atomics, nothing contracted.  Every sum over the
 *       spheres is a chain from 0 over the spheres with rows, ascending; a sphere's term is its three axes in ascending
 *       order, ((x0 y0 + x1 y1) + x2 y2).  Bitwise reproducible; a sequence does not depend on the other sequences of the
 *       batch; the launch shape is one workgroup per frame; no host synchronisation.
 *       workspace: none is needed; shr_sphere_accel_normal_workspace_bytes(B, T, J) is 0 (-1 on a negative size).
 *   Argument rules, checked before the B == 0 no-op: shr_sphere_temporal_normal's -- 1 <= J, 1 <= T, B >= 0 and
 *   B % T == 0, acc_max >= 0 (+inf allowed), accel_weight finite and >= 0, accumulate and accumulate_E 0 or 1 (SHR_EINVAL
 *   otherwise); J above 64, B above 65535: SHR_ETOOLARGE.  NULLs other than triple_weight and workspace, and misaligned
 *   pointers (4 bytes; A, g, E, F, cost 8; keypoints, workspace 16): SHR_EINVAL.
 *   shr_pose_lm_seq2_begin, shr_pose_lm_seq2_step   shr_pose_lm_seq_begin / shr_pose_lm_seq_step's contract word for word
 *       with one more argument F [B,26,26] after E: the bookkeeping per sequence, the cost chain, the accept rule, lambda,
 *       cost0 and trial_out = p for the whole sequence on a pivot that is not positive and finite ANYWHERE in it are
 *       unchanged.  state: shr_pose_lm_seq2_state_bytes(B) = 16 960 B bytes (2120 doubles per frame: shr_pose_lm_seq_step's
 *       state of the B frames, 1440 doubles each -- the accepted pose's A, E, g, the pose, params0, and in a sequence's
 *       first frame its total cost, lambda and counters -- FOLLOWED by the accepted F of the B frames, 680 doubles each);
 *       workspace: shr_pose_lm_seq2_workspace_bytes(B) = 16 512 B bytes (2064 doubles per frame: shr_pose_lm_seq_step's
 *       workspace of the B frames, 1384 doubles each -- L_t, W_t, y_t -- followed by V_t of the B frames, 680 doubles
 *       each), needed with solve != 0; both 8-byte aligned, every part a multiple of 8 doubles per frame, -1 for B < 0.
 *       A state belongs to the B it began with.  F and V_t stand behind, not inside, the frames' records so that a step
 *       without F can be handed to shr_pose_lm_seq_step as it is.
 *       The solve, on the accepted equations: diagonal blocks M_t + lambda diag(M_t), M_t = A_t + diag(mu), blocks E_t at
 *       (t, t + 1) and F_t at (t, t + 2), right-hand side r_t = -(g_t + mu (p_t - prior_t)), by block Cholesky with
 *       bandwidth two, forward over t:
 *         D_t = (M_t + lambda diag M_t) - W_{t-1} W_{t-1}^T - V_{t-2} V_{t-2}^T, per entry the W product subtracted first
 *               and then the V product, each m ascending, then the column recurrence of shr_pose_lm_step; L_t L_t^T = D_t;
 *         L_t y_t = r_t - W_{t-1} y_{t-1} - V_{t-2} y_{t-2};
 *         W_t = (E_t^T - V_{t-1} W_{t-1}^T) L_t^-T (t <= T - 2), V_t = F_t^T L_t^-T (t <= T - 3), 26 triangular solves each;
 *       backward: L_t^T x_t = y_t - W_t^T x_{t+1} - V_t^T x_{t+2}.  All fp64, every sum in index order, the W term before
 *       the V term.  F of the last two frames and E of the last frame of a sequence are not read.  One workgroup per
 *       sequence.
 *       F == NULL is allowed at any T: the call IS shr_pose_lm_seq_step's, so every output and the state's pose are
 *       shr_pose_lm_seq_step's BIT FOR BIT -- with T == 1 shr_pose_lm_step's (E may then be NULL too).  Give F in every
 *       step of a loop or in none: a step without F solves the accepted equations without their F.
 *   Argument rules: shr_pose_lm_seq_begin / _step's; F 8-byte aligned. */
long long shr_sphere_accel_normal_workspace_bytes(int B, int T, int J);
int shr_sphere_accel_normal(const float *keypoints /* [B,J,4]: shr_pose_keypoints_jacobian's, MODEL frame */,
                            const float *jac       /* [B,3J,26]: shr_pose_keypoints_jacobian's */,
                            const float *triple_weight /* [B] or NULL */, float accel_weight, float acc_max,
                            int B, int T, int J, int accumulate, int accumulate_E,
                            double *A, double *g, double *E, double *F /* [B,26,26] */, double *cost, int32_t *count /* [B] */,
                            void *workspace, void *stream);
long long shr_pose_lm_seq2_state_bytes(int B);
long long shr_pose_lm_seq2_workspace_bytes(int B);
int shr_pose_lm_seq2_begin(const float *params0, int B, int T, float lambda0, void *state, float *trial, void *stream);
int shr_pose_lm_seq2_step(void *state, const double *A, const double *g, const double *E, const double *F /* or NULL */,
                          const double *cost_data, const float *trial, const float *prior, const float *stiffness, int solve,
                          int B, int T, float *trial_out, float *params, float *cost /* [S] */, float *cost0 /* [S] */,
                          void *workspace, void *stream);

/* The uncertainty of the sequence fit: marginal covariances of the banded solve --------------------------------------------------
 * Every fit above returns a pose and a cost and does not say how well the images determined the pose: a finger the view hides
 * (DESIGN.md 4.4t, 4.4u), the direction one depth view leaves free (4.4n), arrive as numbers like any other.  The Gauss-Newton
 * matrix that shr_pose_lm_seq2_step factorises is the inverse covariance of the estimate (the Laplace approximation at the
 * given pose, per unit of residual variance); this entry is the other half of that block Cholesky, the DIAGONAL blocks of the
 * inverse of the block-pentadiagonal matrix (selected inversion), and their projection onto the spheres.  The reference has no
 * counterpart.  Layout: the sequence steps', B = S T, the frames of a sequence adjacent.
 *   shr_pose_lm_seq2_covariance   H is the UNDAMPED matrix of a sequence (lambda = 0): diagonal blocks M_t = A_t + diag(mu)
 *       (the LOWER triangle of A_t read), E_t at (t, t + 1), F_t at (t, t + 2); mu = stiffness[26] or, NULL, 0 -- the prior's
 *       information, so that a pose the images do not determine still has a finite covariance.  F == NULL: no second band.
 *       E == NULL: no coupling (F is then not read either), every frame its own system.  With T == 1 neither is read; E of a
 *       sequence's last frame and F of its last two are never read.
 *       Forward over t, shr_pose_lm_seq2_step's factorisation at lambda = 0, operation for operation:
 *         D_t = M_t - W_{t-1} W_{t-1}^T - V_{t-2} V_{t-2}^T, per entry the W product subtracted first and then the V product,
 *               each m ascending, then the column recurrence of shr_pose_lm_step; L_t L_t^T = D_t;
 *         W_t = (E_t^T - V_{t-1} W_{t-1}^T) L_t^-T (t <= T - 2), V_t = F_t^T L_t^-T (t <= T - 3), the product a chain from 0,
 *               m ascending; N_t = L_t^-1; each by 26 triangular solves, row k of the transposed block
 *               X[k][:] = (((X[k][:] - L[k][0] X[0][:]) - L[k][1] X[1][:]) - ...) / L[k][k], N_t from the identity.
 *       Backward over t, with Z = H^-1, P_t = W_t N_t and Q_t = V_t N_t:
 *         Z_{t+1,t} = (-(Z_{t+1,t+1} P_t)) - Z_{t+2,t+1}^T Q_t
 *         Z_{t+2,t} = (-(Z_{t+2,t+1} P_t)) - Z_{t+2,t+2} Q_t
 *         Z_{t,t}   = (N_t^T N_t - P_t^T Z_{t+1,t}) - Q_t^T Z_{t+2,t}
 *       every matrix product entry by entry a chain from 0 over the inner index, ascending, all 26 terms; a term that reaches
 *       past the end of the sequence (or whose band is absent) is not formed.  For T == 1, Z = N_0^T N_0.
 *       -> cov[B,26,26] = Z_tt, the LOWER triangle computed and mirrored: bit-symmetric.
 *       -> sphere_cov[B,J,6] = xx xy xz yy yz zz of C_j(t) = Jc_j(t) Z_tt Jc_j(t)^T, Jc_j = jac[3j .. 3j + 2, :] promoted to
 *       fp64 (shr_pose_keypoints_jacobian's, MODEL frame): mm^2 per unit of residual variance.  Entry (a, b) =
 *       sum_k (sum_m Jc[a][m] Z[m][k]) Jc[b][k], k and m ascending, chains from 0.  Written iff jac AND sphere_cov are given;
 *       exactly one of the two NULL: SHR_EINVAL.
 *       -> status[S] int32: 0 where the sequence factorised; 1 + t where t is the first frame with a pivot that is not
 *       positive and finite -- every cov and sphere_cov entry of ALL that sequence's frames is then a NaN.
 *       All fp64, every sum in index order, the W (P) term before the V (Q) term, nothing contracted, no atomics: bitwise
 *       reproducible, whatever thread owns an entry.  A sequence does not depend on the other sequences of the batch.  Launch
 *       shape: one workgroup of 256 threads per sequence (the chain over t is inherent), then, with jac, one workgroup per
 *       frame for the projection; no host synchronisation: capturable in a hipGraph.
 *       workspace: shr_pose_lm_seq2_covariance_workspace_bytes(B) = 16 320 B bytes (2040 doubles per frame: N_t, W_t and V_t,
 *       680 each), 16-byte aligned, -1 for B < 0; written before it is read in every call.
 *       What it is NOT: saturated rows are absent from A, so a truncated term is silent here as well; it says nothing about
 *       another basin; the residual variance is the caller's.
 *   Argument rules, checked before the B == 0 no-op: B >= 0, 1 <= T, B % T == 0, 1 <= J (SHR_EINVAL otherwise); J above 64,
 *   B above 65535: SHR_ETOOLARGE.  NULLs other than E, F, stiffness and the pair (jac, sphere_cov); misaligned pointers
 *   (4 bytes; A, E, F, cov, sphere_cov 8; workspace 16): SHR_EINVAL. */
long long shr_pose_lm_seq2_covariance_workspace_bytes(int B);
int shr_pose_lm_seq2_covariance(const double *A, const double *E /* or NULL */, const double *F /* or NULL */,
                                const float *stiffness /* [26] or NULL */, const float *jac /* [B,3J,26] or NULL */,
                                int B, int T, int J, double *cov /* [B,26,26] */,
                                double *sphere_cov /* [B,J,6]: xx xy xz yy yz zz, or NULL */,
                                int32_t *status /* [S] */, void *workspace, void *stream);

/* The sliding window: marginalise the frame that leaves, carry it as a prior -------------------------------------------------------
 * The sequence fits above take their frames at once and forget them.  A fixed-lag smoother keeps a window of constant length
 * over a stream: when the oldest frame leaves, everything the fit knew through it -- its own image terms, its stiffness, the
 * temporal and acceleration rows that reach it and the prior it carried itself -- is folded into a Gaussian prior on the frames
 * that stay.  That prior is the Schur complement of the leaving frame's block; for a block-pentadiagonal system it touches the
 * next two frames only, so the window's equations stay block-pentadiagonal and shr_pose_lm_seq2_step and
 * shr_pose_lm_seq2_covariance take them as they are.  The reference has no counterpart.  Layout: the sequence steps', B = S T.
 *   shr_pose_window_marginalize   Input: the DEPARTING SYSTEM of each sequence, A, E (or NULL), F (or NULL), g, cost_data as
 *       the sequence steps take them, evaluated at the poses trial [B,26] fp32; only frames 0 ... min(T, 3) - 1 of a sequence
 *       are read.  prior [B,26] (or NULL: the trial itself, the difference an exact 0) and stiffness [26] (or NULL: 0) are
 *       applied to FRAME 0 ONLY; the stiffness of the frames that stay remains the step's business.
 *         M_0 = A_0 + diag(mu), the LOWER triangle of A_0 read;  b_0 = g_0 + mu (p_0 - prior_0), the differences in fp64 from
 *         the fp32 values, as in the step's right-hand side;  b_1 = g_1, b_2 = g_2.
 *       Arithmetic, all fp64:
 *         1. L L^T = M_0 by the column recurrence of shr_pose_lm_step (lambda = 0);
 *         2. X = L^-1 [E_0 | F_0 | b_0], 26 + 26 + 1 right-hand sides, by the row recurrence of shr_pose_lm_seq2_covariance:
 *            X[k][:] = (((X[k][:] - L[k][0] X[0][:]) - L[k][1] X[1][:]) - ...) / L[k][k]; its parts are X_E, X_F and y;
 *         3. Lambda_11 = A_1 - X_E^T X_E,  Lambda_12 = E_1 - X_E^T X_F,  Lambda_22 = A_2 - X_F^T X_F,
 *            eta_1 = b_1 - X_E^T y,  eta_2 = b_2 - X_F^T y,
 *            c = ((c_0 + cost_1) + cost_2) - y.y,  c_0 = cost_0 + mu_0 d_0^2 + ... + mu_25 d_25^2 (the step's chain: from
 *            cost_0, ascending, each term mu_i (d_i d_i), d = p_0 - prior_0), the costs of frames that do not exist not added;
 *            every product entry a chain from 0 over the inner index, ascending, all 26 terms, then subtracted ONCE;
 *         4. a band that is absent contributes nothing: without F (F == NULL or T < 3) no X_F product is formed or
 *            subtracted; with T == 2 the blocks and rows of frame 2 are +0; for T == 1 or E == NULL the prior is an exact +0
 *            throughout (Lambda and eta; the LOWER triangles of A_1 and A_2 are read otherwise) and c is as above.
 *       -> Lambda[S,52,52] fp64, frame 1 then frame 2: the LOWER triangle computed and mirrored, bit-symmetric; the
 *       Lambda_12 block has frame 1's rows and frame 2's columns.  -> eta[S,52], offset[S] = c, fp64.
 *       -> point[S,52] fp32: the trial poses of frames 1 and 2, the linearisation point; frames that do not exist: +0.
 *       -> status[S] int32: 0 where every pivot of M_0 is positive and finite, 1 otherwise -- every Lambda, eta and offset
 *       entry of THAT sequence is then an exact +0 and point is still written: the information is dropped, the tracker goes
 *       on, the caller sees the status.
 *       Every sum in index order, nothing contracted, no atomics, no matrix-core instruction: bitwise reproducible, whatever
 *       thread owns an entry.  A sequence does not depend on the other sequences of the batch.  Launch shape: one workgroup of
 *       256 threads per sequence; no host synchronisation: capturable in a hipGraph.  workspace: none is needed;
 *       shr_pose_window_marginalize_workspace_bytes(B, T) is 0 (-1 on a negative size).
 *       What it is NOT: the prior is the system's linearisation at `trial` and is never relinearised; rows that are saturated
 *       there are absent from A and silent in the prior as well; a failed pivot drops the past of that sequence.
 *   Argument rules, checked before the B == 0 no-op: B >= 0, 1 <= T, B % T == 0 (SHR_EINVAL otherwise); B above 65535:
 *   SHR_ETOOLARGE.  NULLs other than E, F, prior, stiffness and workspace; misaligned pointers (4 bytes; A, g, E, F, cost_data,
 *   Lambda, eta, offset 8): SHR_EINVAL.
 *   shr_pose_window_prior_normal   The normal equations of the carried prior at the poses trial [B,26] fp32.  Per sequence,
 *       in fp64 from the fp32 values: d = trial(frames 0, 1) - point, 52 entries (the first 26 when T == 1, and then only the
 *       leading 26 x 26 block of Lambda and the first 26 entries of eta are read).
 *         cost: (d^T (Lambda d) + 2 eta^T d) + offset, added to the sequence's FIRST frame; (Lambda d)_i a chain from 0 over
 *               the columns ascending, d^T (Lambda d) and eta^T d chains from 0, i ascending (d_i (Lambda d)_i; eta_i d_i);
 *         g:    the gradient of 1/2 the cost in the family's convention, (Lambda d)_i + eta_i, split onto frames 0 and 1;
 *         A:    Lambda itself: Lambda_00 onto A_0 and Lambda_11 onto A_1 (the LOWER triangle of either block read),
 *               Lambda_01 (frame 0's rows, frame 1's columns, read as stored) onto E_0.
 *       accumulate as in shr_sphere_temporal_normal: 0 writes the term's A, g and cost of frames 0 and 1 (frame 1's cost an
 *       exact +0); 1 ADDS, the LOWER triangle of A read and the sum written to both triangles.  accumulate_E as in
 *       shr_sphere_accel_normal: 0 writes E_0, 1 adds to it.  Frames 2 ... T - 1, E of every frame but the first, and F are
 *       NEVER touched.  active [S] int32 or NULL: a sequence whose entry is 0 has no term and NONE of its outputs is touched,
 *       so that sequences without a prior yet can share a batch.  One add per entry, no atomics: bitwise reproducible.  Launch
 *       shape: one workgroup per frame; no host synchronisation.  shr_pose_window_prior_normal_workspace_bytes(B, T) is 0
 *       (-1 on a negative size).
 *   Argument rules, checked before the B == 0 no-op: B >= 0, 1 <= T, B % T == 0, accumulate and accumulate_E 0 or 1 (SHR_EINVAL
 *   otherwise); B above 65535: SHR_ETOOLARGE.  NULLs other than active, workspace and, with T == 1, E; misaligned pointers
 *   (4 bytes; Lambda, eta, offset, A, g, E, cost 8): SHR_EINVAL. */
long long shr_pose_window_marginalize_workspace_bytes(int B, int T);
int shr_pose_window_marginalize(const double *A, const double *g, const double *E /* or NULL */, const double *F /* or NULL */,
                                const double *cost_data, const float *trial, const float *prior /* [B,26] or NULL */,
                                const float *stiffness /* [26] or NULL */, int B, int T, double *Lambda /* [S,52,52] */,
                                double *eta /* [S,52] */, double *offset /* [S] */, float *point /* [S,52] */,
                                int32_t *status /* [S] */, void *workspace, void *stream);
long long shr_pose_window_prior_normal_workspace_bytes(int B, int T);
int shr_pose_window_prior_normal(const float *trial, const double *Lambda, const double *eta, const double *offset,
                                 const float *point, const int32_t *active /* [S] or NULL */, int B, int T, int accumulate,
                                 int accumulate_E, double *A, double *g, double *E, double *cost, void *workspace, void *stream);

/* Parameters that the frames of a group SHARE: the arrowhead step --------------------------------------------------------------
 * Every fit above treats the model's constants -- the sphere radii first of all -- as given, and DESIGN.md 4.4p and 4.4s name
 * them as the weakest thing left.  A constant of the hand belongs to the person, not the frame: it is one vector sigma [K]
 * for the N frames of a group while every frame keeps its own pose.  The observation is DataToModelLoss's
 * (mesh/render.py:93-142) with sigma among the unknowns; the reference has no counterpart of the shared solve.  A shared
 * unknown couples every frame of its group, so the normal equations are bordered block-diagonal, an ARROWHEAD: N pose
 * blocks A_b [26 x 26], one shared block R [K x K], a coupling C_b [26 x K] per frame.  shr_pose_lm_step cannot take a shared
 * unknown; the sequence steps are chains over the frames, this one is parallel over them with one reduction in the middle.
 * The step is generic in the shared block, 0 <= K <= 64: what sigma means is decided by the entry that forms C, R and gs.
 * Layout: B = G N frames, the N frames of a group adjacent; frame b belongs to group b / N.
 * The first user is the data-to-model term with the RADII as the shared parameters (K = J).  One evaluation of that fit is
 *   shr_pose_keypoints_jacobian(trial) -> shr_view_vertices_fwd (NV := J) -> shr_sphere_icp_radii_normal(radii := trial_shape)
 *     -> shr_sphere_prior_normal(accumulate = 1) -> shr_sphere_collision_normal(accumulate = 1) -> shr_pose_lm_shared_step
 * on one stream, without a host synchronisation: capturable in a hipGraph.  The keypoint, limit and collision terms do not
 * depend on the radii, so they add to A, g and cost only.  The render term's radius columns are not formed: a term whose
 * radius gradient is missing from gs gives no descent direction for the cost the accept test sees, so the render entry
 * stays out of this loop.
 *   shr_sphere_icp_radii_normal   shr_sphere_icp_normal with one more column per sphere.  radii[G,J] fp32, one table per
 *       group, in place of that entry's radii[J]; N frames per group.  Data points, the fp32 owner search, the fp64 residual
 *       d = n - r, the direction u = R^T u_v, the row rule, the tiles of 1024 pixels and the summation order are
 *       shr_sphere_icp_normal's, the same code (csrc/sphere_icp_scan.h).  Per data row of sphere j the pose part of the row
 *       is that entry's, -u^T Jc_j, and the new column is d d / d r_j = -1, in the column of sphere j only.  Per (frame,
 *       sphere) the scan carries four more chains, sum u (3, model frame) and sum d, in the order and by the
 *       one-owner-per-entry scheme of the twelve: moments[B,J,16] (may be NULL) = the twelve, then sum u, then sum d.
 *       -> A[B,26,26], g[B,26], cost[B], count[B], dist, owner: shr_sphere_icp_normal's.  With G = 1 and the same radii they
 *       and moments[..., :12] are that entry's BITS.
 *       -> C[B,26,J] fp64, the coupling sum row_pose^T row_radius: C[b,a,j] = (Jc[0,a] su_0 + Jc[1,a] su_1) + Jc[2,a] su_2,
 *       Jc = jac[3j .. 3j + 2, :] promoted to fp64, su = sphere j's sum u; an exact +0 for a sphere without a row.
 *       -> R[G,J,J] fp64, written dense: R_jj = the chain over the group's frames, ascending, of the rows of sphere j (an
 *       integer: exact); every off-diagonal entry an exact +0.  gs[G,J] fp64 = 0 - the chain over the frames, ascending, of
 *       sum d: the gradient of 1/2 sum d^2 in r_j.
 *       Radius guard: a group with a radius that is not finite or not > 0 is void -- cost = +inf and A = g = C = 0 for
 *       every frame of it, R = gs = 0 -- so that the step rejects it; moments, count, dist and owner are still the scan's.
 *       (shr_sphere_icp_normal's behaviour for such radii is what it was.)
 *       No atomics, fixed-order fp64 chains, nothing contracted: bitwise reproducible, and a group does not depend on the
 *       batch it is in.  workspace: shr_sphere_icp_radii_normal_workspace_bytes(B, V, J, W, H) bytes (-1 on a negative
 *       size), 16-byte aligned.
 *       Argument rules: shr_sphere_icp_normal's, and 1 <= N, B % N == 0 (SHR_EINVAL), checked before the B == 0 no-op;
 *       C, R and gs given and 8-byte aligned.
 *   shr_pose_lm_shared_begin, shr_pose_lm_shared_step   shr_pose_lm_seq_begin / shr_pose_lm_seq_step's contract with the unit
 *       of decision the GROUP: one lambda, one cost, one cost0 and one accept decision per group.
 *       state: shr_pose_lm_shared_state_bytes(B, G, K) = 8 (760 B + G K (K + 3) + 26 B K) bytes: shr_pose_lm_step's state
 *       of the B frames, 760 doubles each, the group's total cost, lambda and counters in its FIRST frame; BEHIND them per
 *       group the accepted sigma, shape0, gs [K] and R [K x K], and behind those per frame the accepted C [26 x K].
 *       workspace: shr_pose_lm_shared_workspace_bytes(B, G, K) = 8 (B (704 + 26 K) + G (8 + K)) bytes: per frame L_b, z_b,
 *       the factor's verdict and Y_b; per group the decision, the verdict and d sigma.  Both 8-byte aligned, -1 on a negative
 *       size.  The workspace is needed by EVERY step (it carries the decision to the frames), except with K == 0 and N == 1.
 *       begin(params0 [B,26], shape0 [G,K]): trial <- params0, trial_shape <- shape0.
 *       Cost and accept.  total = the chain from 0 over the group's frames, ascending, of shr_pose_lm_step's per-frame total
 *       (cost_data_b + the stiffness term, i ascending), then + nu_k (sigma_k - prior_k)^2, k ascending, sigma the fp32
 *       trial_shape in fp64, prior = shape_prior [G,K] or, NULL, shape0; nu = shape_stiffness [K] >= 0 or, NULL, 0.  The
 *       trial of the WHOLE group -- poses and sigma -- is accepted iff total is finite and below the state's; lambda x 0.3
 *       on accept, x 10 on reject, clamped to [1e-9, 1e6], the first accepted step leaving it.  On accept A, g, C, R, gs,
 *       the poses and sigma become the state's.  cost0 [G] is written by the first step after begin; cost [G];
 *       params [B,26] and shape [G,K] are the state's pose and sigma after the decision.
 *       The solve (solve != 0), on the accepted p, sigma, A, g, C, R, gs; all fp64, every sum in index order:
 *         per frame   M_b = A_b + diag(mu); L_b L_b^T = M_b + lambda diag(M_b) by shr_pose_lm_step's column recurrence;
 *                     z_b = L_b^-1 (-(g_b + mu (p_b - prior_b))) by its forward substitution; Y_b = L_b^-1 C_b, column k
 *                     by Y[m,k] = (((C[m,k] - L[m,0] Y[0,k]) - L[m,1] Y[1,k]) - ...) / L[m,m]: K independent substitutions.
 *         per group   T = R + diag(nu), the LOWER triangle of R read.  S_kl = T_kl, on the diagonal T_kk + lambda T_kk, then
 *                     - Y_b[m,k] Y_b[m,l] subtracted entry by entry, frames ascending, m ascending inside; rhs_k =
 *                     -(gs_k + nu_k (sigma_k - prior_k)), then - Y_b[m,k] z_b[m] in the same order; S = L_s L_s^T by the
 *                     same column recurrence at size K; d sigma by the two substitutions of shr_pose_lm_step at size K.
 *         per frame   L_b^T delta_b = z_b - Y_b d sigma, the product a chain from 0, k ascending.
 *       trial_out [B,26] = (float)(p + delta_b) (may be trial), trial_shape_out [G,K] = (float)(sigma + d sigma) (may be
 *       trial_shape).  A pivot that is not positive and finite, in ANY frame's factor or in S, writes trial_out = p and
 *       trial_shape_out = sigma for the WHOLE group; a group does not depend on the other groups of the batch.
 *       K == 0 (C, R, gs and the shape arrays are not read and may be NULL): no shared block; the frames' steps are
 *       shr_pose_lm_step's own, a bad pivot staying with its frame, and the decision is the group's.  With K == 0 and N == 1
 *       the call IS shr_pose_lm_step's on the state's leading part: every output and the state BIT FOR BIT.
 *       Launch shape: a wave per group (decision), a wave per frame (factor, z, Y), a workgroup of 256 threads per group
 *       (S, d sigma; skipped with K == 0), a wave per frame (back); four launches on one stream, no atomics, no host
 *       synchronisation: capturable in a hipGraph.
 *   Argument rules, checked before the B == 0 no-op: state given and 8-byte aligned, B >= 0, 1 <= N, B % N == 0, K >= 0
 *   (SHR_EINVAL otherwise); K above 64, B above 2^24: SHR_ETOOLARGE.  lambda0 > 0; NULLs other than prior, stiffness,
 *   shape_prior, shape_stiffness, trial_out and trial_shape_out without solve, and with K == 0 every shared array;
 *   misaligned pointers (4 bytes; A, g, C, R, gs, cost_data, workspace 8): SHR_EINVAL. */
long long shr_sphere_icp_radii_normal_workspace_bytes(int B, int V, int J, int W, int H);
int shr_sphere_icp_radii_normal(const float *observed, const float *view_centres /* [B,V,J,4] */,
                                const float *radii /* [G,J] */, const float *view, const float *jac /* [B,3J,26] */,
                                int B, int V, int J, int W, int H, int N, float ax, float bx, float ay, float by, float fg_max,
                                float max_dist, double *A, double *g, double *cost, int32_t *count /* [B] */,
                                double *C /* [B,26,J] */, double *R /* [G,J,J] */, double *gs /* [G,J] */,
                                double *moments /* [B,J,16] or NULL */, float *dist, int32_t *owner /* [B,V,H,W] or NULL */,
                                void *workspace, void *stream);
long long shr_pose_lm_shared_state_bytes(int B, int G, int K);
long long shr_pose_lm_shared_workspace_bytes(int B, int G, int K);
int shr_pose_lm_shared_begin(const float *params0, const float *shape0 /* [G,K] */, int B, int N, int K, float lambda0,
                             void *state, float *trial, float *trial_shape /* [G,K] */, void *stream);
int shr_pose_lm_shared_step(void *state, const double *A, const double *g, const double *C /* [B,26,K] */,
                            const double *R /* [G,K,K] */, const double *gs /* [G,K] */, const double *cost_data,
                            const float *trial, const float *trial_shape /* [G,K] */, const float *prior,
                            const float *stiffness, const float *shape_prior /* [G,K] or NULL */,
                            const float *shape_stiffness /* [K] or NULL */, int solve, int B, int N, int K, float *trial_out,
                            float *trial_shape_out /* [G,K] */, float *params, float *shape /* [G,K] */, float *cost /* [G] */,
                            float *cost0 /* [G] */, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPHEREHAND_HIP_H */
