/*
 * gflow_hip.h -- C ABI of libgflow_hip.so, the MI355X (gfx950) native rasteriser,
 * loss and optimiser kernels behind GFlow's per-frame Gaussian-splatting fit.
 *
 * This is the drop-in boundary: the five operators GFlow calls on the external
 * CUDA extension `msplat` (gflow/utils/render.py:21-105, gflow/trainer.py:955)
 * plus the loss / Adam pieces of the iteration loop (gflow/trainer.py:387-558).
 * msplat's own binding layer is not visible in the reference tree, so each entry
 * point cites the REFERENCE CALL SITE it serves.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named h_*; tensors are dense,
 *     row-major, float32 unless stated; `stream` is a hipStream_t (NULL = default);
 *   - no allocation and no host synchronisation inside: the caller supplies outputs and
 *     workspaces, all work is enqueued on `stream` (graph-capturable).  Process-wide state
 *     is limited to: the thread-local last HIP error (gfl_last_hip_error), the cached
 *     CU count of the device, the optional stage profiler (gfl_profile_*) and THREE
 *     environment switches, read once per process -- every switch the library has:
 *       GFL_EWA_MFMA=1        J Sigma J^T on the matrix cores (same results to rounding; gfl_ewa_on_mfma() reports it);
 *       GFL_RESERVED=0        every iteration bins on the exact three-launch path (no reserved tile regions): the sorted
 *                             lists, render and gradients are bit-identical either way;
 *       GFL_FWD_SPLIT_MIN=<n> list length from which the forward blend walks a queue's first tile on four CUs, sixteen splats
 *                             a step: scheduling only -- that walk forms a pixel's transmittance products in tree order, so T and
 *                             the render differ in the last bits on the tiles that take it (which tiles do depends on the
 *                             schedule as well), lists and contributor counts not at all;
 *     tests/test_gpu_switches.py flips each one in a process of its own and holds the results against the defaults.
 *     A fourth switch belongs to the optical-flow entries alone and is read at every call of theirs:
 *       GFL_OPTFLOW_FUSED=0   every Jacobi sweep of gfl_optflow / gfl_optflow_level is a launch of its own (the comparison
 *                             path of DESIGN.md, "Optical flow"); the flows are bit-identical either way
 *                             (tests/test_gpu_optflow.py flips it in-process).
 *     A fifth, likewise, belongs to gfl_sfm_fill alone:
 *       GFL_SFM_FUSED=0       every Jacobi sweep of gfl_sfm_fill is a launch of its own; the depth is bit-identical either way
 *                             (tests/test_gpu_sfm.py flips it in-process).
 *     (Rounds 3-4 had fourteen; the measured-and-rejected variants behind the others now live in tools/experiments/.)
 *   - return value: GFL_OK or a negative gfl_status; HIP launch errors are
 *     returned as GFL_ERR_HIP and the hipError_t is kept in gfl_last_hip_error();
 *   - *_bwd functions OVERWRITE their gradient outputs (they zero what they
 *     accumulate into).
 */
#ifndef GFLOW_HIP_H
#define GFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gfl_stream_t; /* hipStream_t */

typedef enum gfl_status {
    GFL_OK = 0,
    GFL_ERR_INVALID = -1,   /* null pointer, negative size, unsupported channel count */
    GFL_ERR_WORKSPACE = -2, /* workspace smaller than gfl_*_workspace_bytes() */
    GFL_ERR_HIP = -3        /* a HIP call failed; see gfl_last_hip_error() */
} gfl_status;

/* Rasteriser constants.  They are internal to msplat and NOT observable from the
 * reference: every one is an assumption taken from the published
 * 3DGS/EWA formulation, kept here and mirrored by oracle/msplat_oracle.py.
 * A maintainer who can read the real msplat sources overrides any of them at build time
 * (make -C gflow_amd/csrc CONSTS="-DGFL_NEAREST=0.01f -DGFL_LOWPASS=0.0f") and sets the oracle's
 * copies to match; gfl_constants() reports what a built library uses and
 * tests/test_abi.py::test_library_and_oracle_use_the_same_constants compares the two.
 * GFL_TILE is structural (8x8 pixels per wave, four waves per tile) and stays 16. */
#define GFL_TILE 16
#ifndef GFL_NEAREST
#define GFL_NEAREST 0.2f
#endif
#ifndef GFL_EXTENT
#define GFL_EXTENT 1.3f
#endif
#ifndef GFL_FOV_CLAMP
#define GFL_FOV_CLAMP 1.3f
#endif
#ifndef GFL_LOWPASS
#define GFL_LOWPASS 0.3f
#endif
#ifndef GFL_EIG_FLOOR
#define GFL_EIG_FLOOR 0.1f
#endif
#ifndef GFL_RADIUS_SIGMA
#define GFL_RADIUS_SIGMA 3.0f
#endif
#ifndef GFL_ALPHA_MIN
#define GFL_ALPHA_MIN (1.0f / 255.0f)
#endif
#ifndef GFL_ALPHA_MAX
#define GFL_ALPHA_MAX 0.99f
#endif
#ifndef GFL_T_MIN
#define GFL_T_MIN 1e-4f
#endif
/* where inside pixel (px, py) the composite is SAMPLED: at (px + GFL_PIXEL_CENTER, py + GFL_PIXEL_CENTER) in the coordinates
 * project_point returns.  0 = pixel centres at integer coordinates (3DGS's ndc2Pix convention; what GFlow itself suggests:
 * splats are created AT integer pixels, complex_texture_sampling.py:39, and targets are read at uv.long(), trainer.py:473);
 * 0.5f = the gsplat convention.  If upstream msplat samples at +0.5 every render here is half a pixel off until this is
 * set.  Only the sampling moves: uv, radius and tiles_touched are coordinate quantities and stay. */
#ifndef GFL_PIXEL_CENTER
#define GFL_PIXEL_CENTER 0.0f
#endif
#define GFL_MAX_BLEND_CHANNELS 4 /* per launch; the host splits wider features */

/* 300 (round 5): gfl_fit_state.overflow is int32[4] (was [1] before 200's reserved regions), gfl_tile_sort_ordered reads a
 * trailer of GFL_SORT_ORDER_TRAILER ints behind order[T][4], gfl_fit_iterations' flags are GFL_ITER_RESERVED only
 * (GFL_ITER_PRE_DONE / _PRE_NEXT / _ODD, gfl_fit_next_preprocess_supported and gfl_bwd_rows_on are gone), the fit
 * workspace is smaller.  301: gfl_fit_iteration_snapshot.  302: the tile sorts no longer fill a table of list positions
 * (gfl_tile_sort_with_slots is gone, gfl_tile_sort_ordered / _reserved lost their rec / slot_inv / slot_pool arguments): the
 * per-splat launch finds its pair rows without one.  303: GFL_PIXEL_CENTER, gfl_constants_n.  304: gfl_fit_state.cu_count.
 * 305: gfl_fit_state.flags (was reserved_) and GFL_FIT_DETERMINISTIC, gfl_scan_f64.  306: gfl_track_anchor, gfl_track_frame.
 * 307: gfl_seg_score.  308: gfl_recon_frame.  309: the gradient of the intrinsics -- gfl_reduce_cam_workspace_bytes,
 * gfl_project_point_bwd_cam, gfl_ewa_bwd_cam, gfl_render_bwd_cam; the fit workspace is 12 floats per row of cap larger.
 * 310: gfl_flow_pair, gfl_flow_workspace_bytes.  311: gfl_fit_workspace_layout.  312: gfl_epi_fundamental, gfl_epi_mask,
 * gfl_epi_workspace_bytes; gfl_flow_occlusion was added WITHIN 312 (an additive entry: nothing that existed changed, so the
 * number stays; a binding that needs it looks the symbol up).  gfl_track_history, gfl_track_backward and
 * gfl_track_backward_workspace_bytes were added WITHIN 312 in the same way, and so were gfl_track_vis and gfl_prep_frames with
 * their workspace queries, the four gfl_jpeg_* entries, and gfl_optflow, gfl_optflow_level, gfl_optflow_workspace_bytes,
 * the seven gfl_sfm_* entries, gfl_selftest_block_scan and gfl_label_frame, gfl_label_assign, and the four gfl_png_* entries
 * (gfl_png_strip_rows, gfl_png_workspace_bytes, gfl_png_sizes, gfl_png_emit), and gfl_png_decode with
 * gfl_png_decode_workspace_bytes.  A binding checks
 * gfl_version() >= GFL_VERSION of the header it was written for. */
#define GFL_VERSION 312
int gfl_version(void);
/* out[10] = TILE, NEAREST, EXTENT, FOV_CLAMP, LOWPASS, EIG_FLOOR, RADIUS_SIGMA, ALPHA_MIN, ALPHA_MAX, T_MIN of this build */
int gfl_constants(float* out10);
/* 303: the same list with what came later behind it -- [10] = PIXEL_CENTER.  Writes min(n, GFL_N_CONSTANTS) values, returns
 * GFL_N_CONSTANTS (so a binding written for a shorter list keeps working and one written for a longer list sees the gap). */
#define GFL_N_CONSTANTS 11
int gfl_constants_n(float* out, int n);
/* 1 when this process runs the J Sigma J^T contraction of gfl_fit_forward / gfl_render_fwd on the matrix cores
 * (GFL_EWA_MFMA=1 in the environment when the library first looked), 0 for the VALU form */
int gfl_ewa_on_mfma(void);
const char* gfl_status_string(int status);
int gfl_last_hip_error(void);
/* bytes of scratch any *_bwd that reduces camera gradients needs for N splats */
size_t gfl_reduce_workspace_bytes(int N);
/* 309: the same for the *_bwd_cam entries, which reduce the gradient of the intrinsics beside it (16 floats per 256 splats) */
size_t gfl_reduce_cam_workspace_bytes(int N);

/* ---- A4  msplat.project_point  (render.py:21-24,116-119; trainer.py:955) ------
 * uv[N,2], depth[N,1]; culled splats get uv=(0,0), depth=0 (render.py:29). */
int gfl_project_point_fwd(const float* xyz, const float* intr, const float* extr, int N, int W, int H,
                          float nearest, float extent, float* uv, float* depth, gfl_stream_t stream);
/* d_xyz[N,3], d_extr[12] from d_uv[N,2], d_depth[N,1]; `depth` is the forward output */
int gfl_project_point_bwd(const float* xyz, const float* intr, const float* extr, const float* depth,
                          const float* d_uv, const float* d_depth, int N, float* d_xyz, float* d_extr,
                          void* workspace, size_t workspace_bytes, gfl_stream_t stream);
/* 309: the same plus d_intr[4] = dL/d (fx, fy, cx, cy) -- msplat.project_point is differentiable in its camera, intrinsics
 * included (render.py:21-24 passes both).  u = fx x/z + cx, v = fy y/z + cy over the visible rows; which rows are visible
 * depends on intr too and is not differentiated.  d_xyz and d_extr have the bits gfl_project_point_bwd gives.
 * workspace: gfl_reduce_cam_workspace_bytes(N).  N == 0 zero-fills d_extr and d_intr. */
int gfl_project_point_bwd_cam(const float* xyz, const float* intr, const float* extr, const float* depth,
                              const float* d_uv, const float* d_depth, int N, float* d_xyz, float* d_extr,
                              float* d_intr, void* workspace, size_t workspace_bytes, gfl_stream_t stream);

/* ---- A5  msplat.compute_cov3d  (render.py:37-41) -------------------------------
 * rotate is WXYZ; visible is uint8[N]; cov3d[N,6] = xx,xy,xz,yy,yz,zz */
int gfl_cov3d_fwd(const float* scale, const float* rotate, const uint8_t* visible, int N, float* cov3d,
                  gfl_stream_t stream);
int gfl_cov3d_bwd(const float* scale, const float* rotate, const uint8_t* visible, const float* d_cov3d,
                  int N, float* d_scale, float* d_rotate, gfl_stream_t stream);

/* ---- A6  msplat.ewa_project  (render.py:44-49) ---------------------------------
 * conic[N,3] upper-triangular inverse 2-D covariance, radius[N] int32,
 * tiles_touched[N] int32 */
int gfl_ewa_fwd(const float* xyz, const float* cov3d, const float* intr, const float* extr, const float* uv,
                const uint8_t* visible, int N, int W, int H, float* conic, int32_t* radius,
                int32_t* tiles_touched, gfl_stream_t stream);
/* d_xyz[N,3], d_cov3d[N,6], d_extr[12] from d_conic[N,3]; `radius` is the forward output */
int gfl_ewa_bwd(const float* xyz, const float* cov3d, const float* intr, const float* extr,
                const int32_t* radius, const float* d_conic, int N, int W, int H, float* d_xyz,
                float* d_cov3d, float* d_extr, void* workspace, size_t workspace_bytes, gfl_stream_t stream);
/* 309: the same plus d_intr[4] (render.py:44-49 passes intr): the conic depends on fx, fy through the Jacobian
 * J = [[fx/z, 0, -fx tx/z^2], [0, fy/z, -fy ty/z^2]] and not on cx, cy (d_intr[2] = d_intr[3] = 0).  Where x/z (y/z) is
 * clamped at GFL_FOV_CLAMP W / (2 fx), the third column is -+GFL_FOV_CLAMP W / (2 z) and carries no fx (fy).  radius and
 * tiles_touched are not differentiated.  workspace: gfl_reduce_cam_workspace_bytes(N). */
int gfl_ewa_bwd_cam(const float* xyz, const float* cov3d, const float* intr, const float* extr,
                    const int32_t* radius, const float* d_conic, int N, int W, int H, float* d_xyz,
                    float* d_cov3d, float* d_extr, float* d_intr, void* workspace, size_t workspace_bytes,
                    gfl_stream_t stream);

/* ---- A7  msplat.sort_gaussian  (render.py:52-54) -------------------------------
 * Two phases so the host can size gaussian_ids_sorted exactly when it wants to:
 *   gfl_bin_count: tile_offsets[T+1] = exclusive scan of per-tile splat counts
 *                  (tile_offsets[T] = K, the number of splat-tile pairs);
 *   gfl_bin_sort : fills ids[0..min(K,K_cap)) ordered by (tile, depth, id) and
 *                  tile_range[T,2]; *overflow (device int32) is set to 1 when
 *                  K > K_cap (the lists are then truncated, never overrun).
 * `cutoff` may be NULL; if given (float[N]) a tile is only listed when the splat's
 * exact alpha>=1/255 disc (radius^2 = cutoff) reaches it -- output-preserving
 * tightening used by the fused path. T = ceil(W/16)*ceil(H/16). */
size_t gfl_bin_workspace_bytes(int N, int K_cap, int W, int H);
int gfl_bin_count(const float* uv, const int32_t* radius, const float* cutoff, int N, int W, int H,
                  int32_t* tile_offsets, gfl_stream_t stream);
int gfl_bin_sort(const float* uv, const float* depth, const int32_t* radius, const float* cutoff, int N, int W,
                 int H, const int32_t* tile_offsets, int K_cap, int32_t* ids, int32_t* tile_range,
                 int32_t* overflow, void* workspace, size_t workspace_bytes, gfl_stream_t stream);

/* ---- A8  msplat.alpha_blending  (render.py:58-64,68-74,84-90,99-105,148-154) ---
 * feature[N,C_total]; this launch composites channels [c0, c0+C), 1<=C<=4, into
 * out[C,H,W] (channel-planar, the caller offsets `out` for c0>0).
 * final_T[H,W] and n_contrib[H,W] (int32) are saved for the backward. */
int gfl_blend_fwd(const float* uv, const float* conic, const float* opacity, const float* feature,
                  int C_total, int c0, int C, const int32_t* ids, const int32_t* tile_range, float bg, int W,
                  int H, float* out, float* final_T, int32_t* n_contrib, gfl_stream_t stream);
/* Accumulates d_uv[N,2], d_conic[N,3], d_opacity[N], d_feature[N,C_total] (channels
 * c0..c0+C).  zero_first != 0 zeroes all four first (use 0 for the 2nd.. chunk). */
int gfl_blend_bwd(const float* uv, const float* conic, const float* opacity, const float* feature,
                  int C_total, int c0, int C, const int32_t* ids, const int32_t* tile_range, float bg, int W,
                  int H, const float* final_T, const int32_t* n_contrib, const float* d_out, int N,
                  float* d_uv, float* d_conic, float* d_opacity, float* d_feature, int zero_first,
                  gfl_stream_t stream);

/* ---- A17  compute_sh: real spherical harmonics of degree 0..3 -> colour ------------
 * Optional operator: GFlow never calls msplat.compute_sh (its colour is sigmoid(rgb),
 * trainer.py:68), so there is no reference call site; basis and constants follow the
 * 3D Gaussian Splatting code base.  shs[N][K][3], K = (degree+1)^2 in {1,4,9,16};
 * dirs[N][3] unit view directions; visible[N] or NULL; out[N][3] = sum_k Y_k(dir) shs[k]
 * (no +0.5, no clamp).  Backward: d_shs[N][K][3], d_dirs[N][3] (may be NULL). */
int gfl_sh_fwd(const float* shs, const float* dirs, const uint8_t* visible, int N, int K, float* out,
               gfl_stream_t stream);
int gfl_sh_bwd(const float* shs, const float* dirs, const uint8_t* visible, const float* d_out, int N, int K,
               float* d_shs, float* d_dirs, gfl_stream_t stream);

/* ---- A9  apply_float_colormap(depth,"turbo",non_zero=True)  (color.py:24-44) ----
 * Entirely on the device (the reference round-trips through the host every
 * iteration).  lut[256,3]; out[N,3]; workspace >= 16 bytes. */
int gfl_colormap_nonzero(const float* value, int N, const float* lut, float* out, void* workspace,
                         size_t workspace_bytes, gfl_stream_t stream);

/* ---- A10/A11  photometric + SSIM + depth loss, forward and backward ------------
 * (trainer.py:452-488; utils/pytorch_ssim.py:17-37)
 * render[4,H,W] = rgb + depth_map planes; gt_rgb[H,W,3]; gt_depth[H,W];
 * keep[H,W] uint8 or NULL (0 = pixel of the moving region, zeroed as trainer.py:453-455,484);
 * depth_ab[2] = (depth_a, depth_b) on the device.
 * Outputs: d_render[4,H,W] = d(lambda_rgb*(mse + 1 - ssim) + lambda_depth*depth)/d render;
 *          err_px[H,W] = per-pixel mse (the densification error map, trainer.py:459);
 *          sums[8] (device) = {sum mse_px, sum ssim_map, sum depth_term, d/d depth_a, d/d depth_b, 0,0,0}
 *          (un-normalised sums; the d/d terms already carry lambda_depth / (H*W)).
 * workspace: gfl_loss_workspace_bytes(W,H). */
size_t gfl_loss_workspace_bytes(int W, int H);
/* same kernels, but the scalar sums are left as per-block partial rows inside `workspace`
 * (p_ssim[n_ssim] floats: SSIM-map sums; p_grad[n_grad][4] floats: mse, depth term, d/d depth_a,
 * d/d depth_b) for a consumer that folds them itself (the fused iteration's camera kernel) */
int gfl_loss_fwd_bwd_partials(const float* render, const float* gt_rgb, const float* gt_depth, const uint8_t* keep,
                              const float* depth_ab, float lambda_rgb, float lambda_depth, int W, int H,
                              float* d_render, float* err_px, void* workspace, size_t workspace_bytes,
                              const float** p_ssim, int* n_ssim, const float** p_grad, int* n_grad,
                              gfl_stream_t stream);
/* The ground truth does not change during the iterations of a fit: gfl_loss_prepare_gt computes its
 * two SSIM statistics once (gt_stats[3][2][H][W]: conv(y), conv(y^2), same arithmetic as the full
 * kernel) and the _cached variant then filters three maps instead of five.  keep must be the mask
 * the later calls use. */
int gfl_loss_prepare_gt(const float* gt_rgb, const uint8_t* keep, int W, int H, float* gt_stats, gfl_stream_t stream);
int gfl_loss_fwd_bwd_partials_cached(const float* render, const float* gt_rgb, const float* gt_depth,
                                     const uint8_t* keep, const float* depth_ab, float lambda_rgb, float lambda_depth,
                                     int W, int H, float* d_render, float* err_px, void* workspace,
                                     size_t workspace_bytes, const float* gt_stats, const float** p_ssim, int* n_ssim,
                                     const float** p_grad, int* n_grad, gfl_stream_t stream);
int gfl_loss_fwd_bwd(const float* render, const float* gt_rgb, const float* gt_depth, const uint8_t* keep,
                     const float* depth_ab, float lambda_rgb, float lambda_depth, int W, int H,
                     float* d_render, float* err_px, float* sums, void* workspace, size_t workspace_bytes,
                     gfl_stream_t stream);

/* ---- A13  Adam (torch.optim.Adam defaults, trainer.py:153,554) ------------------
 * One fused step over n floats: p -= lr * m_hat / (sqrt(v_hat) + eps) with bias
 * correction for step `*d_step + 1` read on the device (so a captured graph can
 * replay); `lr_scale` multiplies lr (LinearLR factor computed on the device when
 * total_iters > 0: 1 + (lr_end_factor-1)*min(step,total)/total; trainer.py:384 uses
 * start 1.0, end 0.1).
 * row_zero_grad (uint8 per row of `row_len` floats, or NULL): rows flagged 1 see a
 * zero gradient (moments still decay), which is what trainer.py:543-551 does.
 * gfl_step_increment bumps the device step counter once all groups have stepped. */
int gfl_adam_step(float* param, const float* grad, float* m, float* v, int64_t n, int row_len,
                  const uint8_t* row_zero_grad, float lr, float beta1, float beta2, float eps,
                  const int32_t* d_step, float lr_end_factor, int total_iters, gfl_stream_t stream);
int gfl_step_increment(int32_t* d_step, gfl_stream_t stream);

/* ---- Fused fit iteration  (trainer.py:387-558 in one call) ----------------------
 * Everything the iteration loop does between "build input_group" (trainer.py:390)
 * and "scheduler.step()" (trainer.py:555): activations, render_multiple(["rgb","uv",
 * "depth","depth_map"]), the rgb/SSIM/depth/var/flow/still losses, backward, gradient
 * masking, Adam for the splats, the camera pose and the depth affine pair.
 * Plain structs of device pointers and sizes; the host owns every buffer.
 *   params/adam_m/adam_v [cap][16] f32 rows: x y z | sx sy sz | qw qx qy qz | opacity |
 *                         r g b | pad pad   (raw, pre-activation values, trainer.py:79-86)
 *   rec   [cap][12]: u v A B | C opacity r g | b depth cutoff radius   (outputs: uv =
 *                    rec[:,0:2], depth = rec[:,9], what render.py:21-49 returns)
 *   d_rec [cap][12] or NULL: dL/d(rec[:,0:10]) of the last backward -- nothing in the iteration reads it; written when given
 * Optional per-splat inputs (NULL = term absent): flow_target[cap][2] + flow_w[cap]
 * (weight = mask/(2 count), trainer.py:511-528), still_target[cap][3] + still_w[cap]
 * (weight = mask/count, trainer.py:505-509), row_flags[cap] (bit0: still splat -- xyz gradient
 * frozen, trainer.py:543-546; bit1: the row carries a still/moving label, i.e. it existed when the
 * labels were made: the scale term and nothing else looks at it).
 * workspace: gfl_fit_workspace_bytes(...) bytes, ZERO-INITIALISED ONCE by the host and then left
 * alone between calls: besides scratch it holds the tile scheduler's feedback (the work the
 * backward blend measured per tile, used to balance the next iteration's blend launches over the
 * CUs).  Garbage there cannot change a result, only the balance.  The tile grid is limited to
 * 16384 tiles (GFL_ERR_INVALID beyond). */
typedef struct gfl_fit_state {
    int32_t N, cap, W, H, K_cap;
    int32_t gt_cached;   /* 1: gfl_fit_prepare_targets ran for the current gt_rgb / keep (ignored with foot_flags) */
    float *params, *adam_m, *adam_v;
    float *rec, *d_rec;
    const float *flow_target, *flow_w, *still_target, *still_w;
    const uint8_t* row_flags;
    float *pose, *pose_m, *pose_v;             /* [7] qx qy qz qw tx ty tz (trainer.py:41) */
    float *depth_ab, *depth_ab_m, *depth_ab_v; /* [2] (trainer.py:145-146) */
    const float* intr;                          /* [4] */
    float* extr;                                /* [12] out: world->camera used this iteration */
    float* d_extr;                              /* [12] out: dL/d extr */
    int32_t* step;                              /* device step counter (Adam t-1, LinearLR epoch) */
    const float* gt_rgb;                        /* [H][W][3] */
    const float* gt_depth;                      /* [H][W] or NULL */
    uint8_t* keep;                              /* [H][W] or NULL (0 = masked-out pixel); IN/OUT of
                                                 * gfl_fit_forward when foot_flags is set */
    const uint8_t* move_mask;                   /* [H][W] or NULL: the frame's move mask (informational; the
                                                 * caller initialises keep = !move_mask for the camera-only stage) */
    const uint8_t* foot_flags;                  /* [cap] or NULL.  Non-NULL: every forward clears from keep the
                                                 * footprint of the flagged splats -- the mask GFlow gets from an
                                                 * extra render of the tentative moving splats with "grey > 0",
                                                 * accumulated over the iterations as trainer.py:426-451 does
                                                 * (move_mask = move_gs_mask | move_mask inside the loop) */
    float *render, *final_T;                    /* [4][H][W], [H][W] */
    int32_t* n_contrib;                         /* [H][W] */
    float *d_render, *err_px, *sums;            /* [4][H][W], [H][W], [8] as gfl_loss_fwd_bwd */
    int32_t *tile_offsets, *ids, *tile_range, *overflow; /* [T+1], [K_cap], [T][2], [4].  overflow[0] is sticky: 1 = a
                                                          * forward produced more than K_cap pairs (or wide-splat pair rows) and
                                                          * dropped some, 2 = GFL_ITER_RESERVED without reserved regions.
                                                          * It is only ever raised by the binning launches of a forward --
                                                          * never by a launch that also reads it --, so every update launch of
                                                          * one iteration sees the same value.  While it
                                                          * is set, gfl_fit_backward_step steps NOTHING (rows, moments, pose,
                                                          * depth affine and step counter stay) and adds 1 to overflow[1]: the
                                                          * caller grows the lists, clears the words and runs overflow[1]
                                                          * iterations again (gflow_amd/fused.py: settle_overflow).
                                                          * overflow[2] != 0: THIS iteration is void (a tile outgrew its
                                                          * reserved region: nothing is stepped, overflow[1] counts it, the
                                                          * next iteration is fine again -- with overflow[0] == 0 the caller
                                                          * just runs overflow[1] more iterations); overflow[3]: the same,
                                                          * between the binning launch and the tile sort.
                                                          * tile_offsets[0..T) is written by the exact binning path only;
                                                          * tile_offsets[T] = the number of pairs, always; after an iteration
                                                          * on reserved regions the lists in ids have gaps between them
                                                          * (tile_range says where each one is) */
    void* workspace;
    size_t workspace_bytes;                     /* >= gfl_fit_workspace_bytes() */
    int32_t cu_count;                           /* 304: compute units this state's launches may use -- 0 = the whole device.  The
                                                 * blend launches are persistent grids with one tile queue per CU: a caller that
                                                 * runs a state on a CU-masked stream (hipExtStreamCreateWithCUMask; several clips
                                                 * side by side on one device, each on its share of every XCD: gflow_amd/fit_video.py)
                                                 * says so here, and grids and queues are sized for that share.  Fixed for the life
                                                 * of the state's workspace (the queues in it are built for this many). */
    int32_t flags;                              /* 305: GFL_FIT_* bits below; 0 = the default mode.  Any other bit: GFL_ERR_INVALID */
} gfl_fit_state;

/* Deterministic mode (305).  With GFL_FIT_DETERMINISTIC in gfl_fit_state.flags, every launch of gfl_fit_* and gfl_render_*
 * on the state reduces in an order fixed by its inputs, so the same inputs give BIT-IDENTICAL outputs -- render, final_T,
 * n_contrib, the sorted lists, parameters, Adam moments, pose and depth affine, loss sums, snapshots, d_params / d_extr --
 * run after run, in one process or several, launched eagerly or replayed from a captured graph, on a stream of its own or
 * beside other fits.  What changes against the default mode:
 *   - the backward blend's four waves leave their per-splat sums in one LDS row per 8x8 block with plain stores and the
 *     tile folds the four rows in block order (the default adds them into one row with LDS float atomics, in arrival order);
 *   - the tile schedulers order tiles of equal quantised weight by tile index (the default: by LDS-atomic arrival), so the
 *     choice of the tiles that are walked in segments (backward) or on four CUs (forward) -- which changes the last bits of T,
 *     the render and the gradients -- is a function of the weights alone.
 * The contract holds for the same library build, device model, cu_count and environment switches.  It does NOT promise
 * equality with the default mode, across different cu_count values or CU partitions (the number of queues decides which
 * tiles are split), across GFL_FWD_SPLIT_MIN values, or across ROCm versions.  gfl_render_fwd in this mode also drops the state's
 * scheduler feedback first, so that a render does not depend on what the state rendered before.  Cost: see INTEGRATION.md. */
#define GFL_FIT_DETERMINISTIC 1

typedef struct gfl_fit_hyper {
    float bg, nearest, extent;
    float lambda_rgb, lambda_depth, lambda_var, lambda_flow, lambda_still;
    float lambda_scale;        /* trainer.py:495-502: mean over the rows inside the image (still rows in the
                                * camera-only stage, moving rows in the joint stage, by row_flags) of |scale| / depth */
    float lr, lr_camera, beta1, beta2, eps, lr_end_factor;
    int32_t total_iters;       /* LinearLR total_iters, 0 = constant lr */
    int32_t freeze_rgb;        /* trainer.py:537-540 */
    int32_t freeze_all_splats; /* camera_only, trainer.py:548-551: every splat gradient is zeroed.  The rows and their Adam moments
                                * are then left untouched (not read, not written): what Adam does with zero gradients and
                                * the zero moments a fresh optimiser starts from (trainer.py:383) */
    int32_t step_camera;       /* 1: pose and depth affine are stepped; 0: neither (after densification replaced the
                                * optimiser, trainer.py:951).  While the camera cannot move -- 0, or 1 with lr_camera == 0 (the
                                * first frame and every joint stage) -- an iteration computes no pose gradient and has no camera
                                * launch: d_extr is set to zero, the pose moments stay as they are; loss sums, depth affine
                                * and step counter as always.  2 = as 1, and the gradient (d_extr, pose moments) is wanted
                                * although lr_camera is 0. */
} gfl_fit_hyper;

size_t gfl_fit_workspace_bytes(int cap, int K_cap, int W, int H);
/* the regions of the fit workspace, in address order: returns their number (writes at most `max`), < 0 on invalid sizes.
 * names: static strings; offsets: multiples of 256; bytes: a region's own size, before it is rounded up to 256.  Needs no
 * device: the size query, the library's own carve and this table are one walk over one description. */
int gfl_fit_workspace_layout(int cap, int K_cap, int W, int H,
                             const char** names, size_t* offsets, size_t* bytes, int max);
/* render only: fills rec, ids, tile_range, render, final_T, n_contrib, extr */
int gfl_fit_forward(const gfl_fit_state* st, const gfl_fit_hyper* hp, gfl_stream_t stream);
/* loss + backward + optimiser step on the state gfl_fit_forward left behind */
int gfl_fit_backward_step(const gfl_fit_state* st, const gfl_fit_hyper* hp, gfl_stream_t stream);
int gfl_fit_iteration(const gfl_fit_state* st, const gfl_fit_hyper* hp, gfl_stream_t stream);
/* ``count`` iterations back to back (trainer.py:387-558 ``count`` times; what a caller captures into ONE graph).
 *
 * Reserved tile regions (round 4, the default): the last launch of every full iteration gives each tile a region of the
 * key array sized by what the tile holds now plus a margin (count + count / 4 + 32), and an iteration that FOLLOWS a full
 * iteration bins straight into those regions -- preprocess, column scan and scatter are one launch (one returning atomic
 * per (block of 512 splats, tile) reserves the block's part of the region), six launches per iteration instead of eight.
 * The sorted lists, the render and every gradient are those of the exact path; only the lists' positions in ids differ.
 * Iterations 2 .. count of a call always take it; the first does with
 *   GFL_ITER_RESERVED  the previous launches on this state were a full iteration (gfl_fit_iterations / gfl_fit_iteration /
 *                      gfl_fit_backward_step) and the splats have not been replaced since (checked on the device as far
 *                      as it can be: without reserved regions *overflow becomes 2).  The regions are a PREDICTION: a tile
 *                      that outgrows its region voids that one iteration (overflow[2], counted in overflow[1]; the regions
 *                      reserved at its end are sized by what the tiles wanted): nothing is stepped by it, but what its
 *                      forward left behind -- render, lists, loss sums -- is TRUNCATED; a caller that looks at those
 *                      (snapshot, log entry) checks overflow[2] first and runs the iteration again (gflow_amd/trainer.py).
 * gfl_fit_reserved_supported: 1 if this state's iterations can (tile grids of up to 4096 tiles; GFL_RESERVED=0 in the
 * environment switches it off). */
#define GFL_ITER_RESERVED 8
int gfl_fit_iterations(const gfl_fit_state* st, const gfl_fit_hyper* hp, int count, int flags, gfl_stream_t stream);
int gfl_fit_reserved_supported(const gfl_fit_state* st, const gfl_fit_hyper* hp);
/* ---- the fused rasteriser as a differentiable operator (no loss, no optimiser) ------------------------
 * render(gaussians, camera) -> {rgb, depth_map, uv, depth} = render_multiple(input_group, ["rgb", "uv", "depth",
 * "depth_map"]) of render.py:6-108 in ONE call (last row), and its backward.
 * Same state struct as the fit iteration, read differently:
 *   params [cap][16] hold the ACTIVATED attributes the reference passes to msplat (xyz | scale | unit quaternion
 *   wxyz | opacity | rgb | pad pad), st->extr is an INPUT (world->camera, 12 floats), pose / Adam / target / loss
 *   fields are ignored (may be NULL); hp supplies bg, nearest, extent only.
 * gfl_render_fwd fills rec (uv = rec[:,0:2], depth = rec[:,9]), render[4][H][W] (rgb planes + depth_map),
 * final_T, n_contrib, ids, tile_range.  gfl_render_bwd takes dL/d render [4][H][W] and, optionally (NULL = 0),
 * dL/d uv [N][2] and dL/d depth [N] and returns d_params [N][16] (same column layout as params, the two pad
 * columns zero) and d_extr[12]; it must follow the gfl_render_fwd whose state it differentiates. */
int gfl_render_fwd(const gfl_fit_state* st, const gfl_fit_hyper* hp, gfl_stream_t stream);
int gfl_render_bwd(const gfl_fit_state* st, const gfl_fit_hyper* hp, const float* d_render, const float* d_uv,
                   const float* d_depth, float* d_params, float* d_extr, gfl_stream_t stream);
/* 309: gfl_render_bwd plus d_intr[4], the intrinsics' gradient through projection and EWA of render.py:21-49 (culling,
 * radius and tile rectangles are not differentiated).  d_params and d_extr have the bits gfl_render_bwd gives; in the
 * deterministic mode d_intr is bit-identical run to run as well.  The per-splat launch is gfl_render_bwd's own (it also
 * writes d_rec -- the state's, or rows in the workspace); a second small launch over the splats reduces d_intr from them. */
int gfl_render_bwd_cam(const gfl_fit_state* st, const gfl_fit_hyper* hp, const float* d_render, const float* d_uv,
                       const float* d_depth, float* d_params, float* d_extr, float* d_intr, gfl_stream_t stream);
/* ---- batched inference rasteriser (additive within 312): many (row range, camera) jobs per call -----------------
 * What viewer.py:201-228 does per displayed image and render.py:6-108 per call -- render_multiple(input_group, ["rgb", "uv",
 * "depth", "depth_map"]) followed by render2img -- for J jobs at once, without anything a backward would need.
 *   params   [R][16]  ACTIVATED rows, gfl_render_fwd's column layout
 *   job_rows [J][2]   device: first row, row count (ranges may overlap or repeat)
 *   job_cam  [J][17]  device: intr fx fy cx cy | extr 3x4 row-major | bg
 *   rows_total        room for records: the sum of the counts must not exceed it
 *   out_f32  [J][4][H][W] rgb planes + depth_map, or NULL;  out_u8 [J][H][W][3] = render2img of the very floats of the rgb planes,
 *   or NULL (one of the two is required);  out_rec [sum of counts][12] records in job order (uv = cols 0:2, depth = col 9), or NULL
 *   overflow [J]      device: 1 = the job lost splat-tile pairs, 2 = its row range leaves [0, R) or its records rows_total
 *                     (such rows are not rendered), 0 otherwise
 * Per job the result is gfl_render_fwd's -- same cull set, EWA, radius, tile rectangles, (tile, depth bits, id) order, alpha floor
 * and cap, stop rule and background term, the compile-time constants above -- and a function of the job's own rows and camera
 * only: the same bits alone, first, last or between other jobs, run after run (nothing is added in arrival order).
 * The job tables are read on the device, nothing is read back or allocated, and the call is six launches whatever J, the counts
 * or the data are: it can be captured into a graph on one stream, and a replay renders what the tables hold THEN.
 * The pool of K_cap pairs is shared by the jobs and filled in (job, tile) order; a list that does not fit whole gets no room,
 * nor does any list behind it (a cut list's survivors would depend on arrival order): jobs before the cut have the bytes of a
 * call with enough room, jobs with a non-empty list behind it are flagged.  J == 0 succeeds and writes nothing; a job without
 * rows, or with every row culled, is the background image.  GFL_ERR_INVALID, before anything touches a device: J, R or rows_total
 * < 0, W, H or K_cap <= 0, both images NULL, a required pointer NULL, more than 2^28 (job, tile) pairs, a workspace smaller than
 * gfl_render_batch_workspace_bytes (0 for arguments it rejects). */
size_t gfl_render_batch_workspace_bytes(int J, int rows_total, int K_cap, int W, int H);
int gfl_render_batch(const float* params, int R, const int32_t* job_rows, const float* job_cam, int J, int rows_total, int W,
                     int H, int K_cap, float* out_f32, uint8_t* out_u8, float* out_rec, int32_t* overflow, void* workspace,
                     size_t workspace_bytes, gfl_stream_t stream);
/* ---- row composer (additive within 312): in-between frames, still / moving layers and group edits ---------------
 * The rows of a clip fit keep their index from frame to frame (densification only appends), so two frames of a clip blend row
 * by row.  A job makes the rows of time a + s from the rows of frames a and b, applies an edit per group, and leaves them where
 * gfl_render_batch reads them: params = out_rows, R = rows_total = J rows_max, job_rows = out_job_rows.
 *   params   [R][16]     ACTIVATED rows, gfl_render_fwd's column layout
 *   labels   [R]         a group per row, 0 = still, 1 = moving; NULL = every row in group 0
 *   job_src  [J][4]      device: first_a, count_a, first_b, count_b (ranges may overlap or repeat)
 *   job_s    [J]         device: s in [0, 1]
 *   job_edit [J][G][16]  device, 16-byte aligned, or NULL for no edits; 1 <= G <= 8; an entry is
 *                        gain | size | q wxyz (unit) | pivot xyz | shift xyz | tint rgb | mix
 *   out_rows [J rows_max][16];  out_job_rows [J][2] = (j rows_max, rows kept)
 *   flags    [J]         device: 2 = a source range leaves [0, R) or max(count_a, count_b) > rows_max (the job keeps 0 rows), else 0
 * Source index i in [0, max(count_a, count_b)):  in both ranges, xyz, scale, opacity and rgb are fmaf(s, b - a, a), and the
 * quaternion is the same lerp of a's and b's -- b's negated when its dot with a's is negative --, normalised; s == 0 gives a's
 * row and s == 1 b's, bit for bit.  Only in b (a row appended at frame b): b's row with opacity x s.  Only in a: a's row with
 * opacity x (1 - s).  The row's group is the label of its a row when it has one, else of its b row, and its edit is
 * job_edit[j][group]; a group >= G, or no table, is the identity (nothing is touched).  opacity' = min(opacity gain, 1);
 * rgb' = fmaf(mix, tint - rgb, rgb); and unless size == 1, q == (+-1, 0, 0, 0) and shift == 0 exactly (xyz, scale and rotate
 * then keep their bits): xyz' = fmaf(size, R(q)(xyz - pivot), pivot) + shift, scale' = size scale, rotate' = normalise(q (x) rotate).
 * A row with opacity' <= 0 is dropped; the others are written compacted in ascending i.  A row's place is a function of the
 * keep decisions before it alone (wave ballots, popcounts and a prefix over the chunks of 256 rows; no atomic decides a place):
 * the same bytes alone, first, last or between other jobs, run after run, and nothing is written outside
 * [j rows_max, j rows_max + kept) of out_rows.  The tables are read on the device, nothing is read back or allocated, and the
 * call is three launches whatever J, the counts or the data are: it can be captured into a graph on one stream in front of the
 * gfl_render_batch it feeds.  J == 0 succeeds and writes nothing.  GFL_ERR_INVALID, before anything touches a device: J, R or
 * rows_max < 0, G outside 1 .. 8 with a table, a required pointer NULL, J rows_max beyond 2^31 - 1 or more than 2^30 (job, chunk) pairs, a workspace smaller than
 * gfl_compose_rows_workspace_bytes (0 for arguments it rejects). */
size_t gfl_compose_rows_workspace_bytes(int J, int rows_max);
int gfl_compose_rows(const float* params, const uint8_t* labels, int R, const int32_t* job_src, const float* job_s,
                     const float* job_edit, int G, int J, int rows_max, float* out_rows, int32_t* out_job_rows, int32_t* flags,
                     void* workspace, size_t workspace_bytes, gfl_stream_t stream);
/* The three snapshot images GFlow keeps every 10th iteration (trainer.py:573-582) in one call, entirely on the
 * device: rgb of the last forward, the turbo-coloured depth map and the centre blobs (render.py:76-106; both composites
 * of the same lists, the per-splat values are derived while the records are staged), each clamped, scaled by 255 and
 * truncated like render2img (render.py:158-166).  out_u8 [3 images][H][W][3] uint8; lut [256][3] = the turbo table.
 * For a forward that has already run (an evaluation render, a staged copy): the lists are walked again for
 * depth_map_color. */
size_t gfl_fit_snapshot_workspace_bytes(int N, int W, int H);
int gfl_fit_snapshot(const gfl_fit_state* st, const gfl_fit_hyper* hp, const float* lut, uint8_t* out_u8, void* workspace,
                     size_t workspace_bytes, gfl_stream_t stream);
/* One full iteration (gfl_fit_iteration, exact binning path) whose forward ALSO leaves those three images in out_u8 -- what
 * trainer.py:573-582 does every 10th iteration with three more renders.  rgb and depth_map_color come out of ONE walk of the
 * lists (the second composite has the first one's alphas and transmittances: three more sums per pixel), center from a small
 * kernel over the same lists; nothing is composed twice and nothing waits for the backward.  +~25 us on that iteration
 * (gfl_fit_snapshot after it: ~130 us).  lut [256][3] = the turbo table; out_u8 [3][H][W][3]. */
int gfl_fit_iteration_snapshot(const gfl_fit_state* st, const gfl_fit_hyper* hp, const float* lut, uint8_t* out_u8,
                               gfl_stream_t stream);
/* Copies from one engine to another (same image size, same row count N, capacities at least as large) everything
 * gfl_fit_snapshot reads of a forward: records, sorted ids, tile ranges, the rgb planes of the render and the forward's
 * tile queues -- one launch, ~9 MB at 480p / 60 000 splats.  The snapshot of iteration i can then be taken from the copy,
 * on another stream, BESIDE iteration i + 1 (gflow_amd/companion.py: SnapshotShadow.compose) instead of between the two. */
int gfl_fit_snapshot_stage(const gfl_fit_state* src, const gfl_fit_state* dst, gfl_stream_t stream);
/* once per ground-truth image / keep mask: SSIM statistics of the target into the workspace; set
 * st->gt_cached = 1 afterwards (0 is always valid: everything is then recomputed per iteration) */
int gfl_fit_prepare_targets(const gfl_fit_state* st, gfl_stream_t stream);
/* where the last gfl_fit_forward's tile schedules live in the workspace (device pointers): queue c
 * holds d_counts[c] items d_lists[c * queue_capacity + k] = tile | priority << 28.  Every tile of the
 * frame appears in exactly one queue.  The backward blend's queues (weights: the units it counted per tile in the last
 * iteration) and, _fwd, the forward blend's (its own counts).  For tests and tools; nothing needs them to run. */
int gfl_fit_schedule_info(const gfl_fit_state* st, int* n_queues, int* queue_capacity, const int32_t** d_lists,
                          const int32_t** d_counts);
int gfl_fit_schedule_info_fwd(const gfl_fit_state* st, int* n_queues, int* queue_capacity, const int32_t** d_lists,
                              const int32_t** d_counts);
/* the per-tile sort of gfl_bin_sort alone (keys already scattered into segments) */
int gfl_tile_sort_only(const int32_t* tile_offsets, int T, int K_cap, void* keys, int32_t* ids,
                       int32_t* tile_range, gfl_stream_t stream);
/* same, with the order the workgroups take the tiles in given by the caller: order[T][4] = {tile, start, end, split} per
 * position (16-byte aligned; positions are assigned to the XCDs in contiguous runs, T / 8 each, like the tiles without it),
 * followed by a trailer of GFL_SORT_ORDER_TRAILER ints: trailer[0] = n_split (0 .. GFL_SORT_MAX_SPLIT), trailer[1 + j] =
 * the position of the j-th split list, whose order entry carries split = 1 + j (0 everywhere else).  A split list (64 ..
 * 2048 keys) is cut at a pivot key and sorted by two workgroups, half each; the result is the same sorted list.
 * gfl_fit_iteration's scatter launch writes all of it: every XCD's longest lists first (their workgroups then start with
 * the launch instead of in its second round), the lists of more than 768 keys split.  Any permutation that keeps a tile
 * inside its XCD's run, with or without split entries, is as good for the result. */
#define GFL_SORT_MAX_SPLIT 64
#define GFL_SORT_ORDER_TRAILER (GFL_SORT_MAX_SPLIT + 4)
int gfl_tile_sort_ordered(const int32_t* order, int W, int H, int K_cap, void* keys, int32_t* ids, int32_t* tile_range,
                          gfl_stream_t stream);
/* same for reserved tile regions: order[T][4] = {tile, start, capacity, split}; the list of `tile` is the first
 * min(fill[position], capacity) keys behind `start` (fill[T]: what the binning launch counted, by position in the order);
 * tile_counts[tile] = fill[position];
 * void_words (may be NULL): void_words[0] = void_words[1], void_words[1] = 0 (gfl_fit_state.overflow + 2). */
int gfl_tile_sort_reserved(const int32_t* order, const int32_t* fill, int32_t* tile_counts, int32_t* void_words, int W, int H,
                           int K_cap, void* keys, int32_t* ids, int32_t* tile_range, gfl_stream_t stream);

/* ---- optional per-stage timing of the fused iteration ---------------------------
 * HIP events are recorded on the launch stream around the stages whose bit is set in
 * stage_mask: 0 preprocess, 1 colscan, 2 scatter, 3 tile sort, 4 blend forward, 5 loss,
 * 6 blend backward, 7 preprocess-backward + Adam, 8 camera/affine Adam.
 * gfl_profile_read synchronises on the recorded events, fills total_ms[9] / counts[9]
 * and clears the records. */
/* device self-test of the wave64 reduce-scatter used by the blend backward: in[64][10] ->
 * out_scatter[10] (permlane-swap reduce-scatter) and out_dpp[10] (plain DPP sums) */
int gfl_selftest_reduce10(const float* in, float* out_scatter, float* out_dpp, gfl_stream_t stream);
/* device self-test of the workgroup exclusive scan every kernel uses (block_scan_excl, gfl_common.hpp): ONE workgroup of
 * `block` threads (256, 512 or 1024; anything else: GFL_ERR_INVALID) scans in[0 .. block) and then in[block .. 2 block),
 * back to back on the same LDS scratch -> out_excl[2 block], and the two totals -> out_total[2] */
int gfl_selftest_block_scan(const int32_t* in, int block, int32_t* out_excl, int32_t* out_total, gfl_stream_t stream);
/* device self-test of the EWA contraction Sigma2 = M Sigma M^T (gfl_math.hpp) both ways: m[n][6] = the two rows of
 * M = J W, cov[n][6] = xx xy xz yy yz zz -> out_valu[n][3], out_mfma[n][3] = (a, b, c) before the low-pass.  The
 * MFMA form (v_mfma_f32_4x4x1_16b_f32, sixteen splats per instruction) is what GFL_EWA_MFMA=1 puts into the fused
 * preprocess kernel; the VALU form is the default. */
int gfl_selftest_cov2d(const float* m, const float* cov, int n, float* out_valu, float* out_mfma, gfl_stream_t stream);
/* The blend kernels' culling test on its own: for n records (rows of 12 floats as in gfl_fit_state.rec; columns
 * u v A B | C o . . | . . cutoff .) the 4-bit mask of the four box x box pixel boxes at (x0, y0) the splat can reach
 * with alpha >= 1/255 (box = 8: the blocks of a tile, 4: the quarters of a block), and `truth`: the boxes that hold a
 * visible pixel by brute force with the kernels' own alpha test.  The mask must contain the truth. */
int gfl_selftest_block_mask(const float* rec, int n, int x0, int y0, int box, int32_t* mask, int32_t* truth, gfl_stream_t stream);

/* ---- moving-region hull (HOST function: plain pointers, no device work) ----------------------------------
 * The ring of the concave hull of n 2-D points (concaveman's algorithm, what the `concave_hull` package behind
 * gflow/utils/concave_hull.py:73-92 implements; gflow/trainer.py:604-609 masks the moving region with it).
 * points_xy[n][2]: sorted by x then y, no duplicates (numpy.unique(axis=0)); concavity 2, length_threshold 0 are the
 * package's defaults.  Writes up to cap_vertices ring vertices (not closed) to ring_xy and returns their number, or a
 * negative gfl_status (GFL_ERR_WORKSPACE: cap_vertices too small; 2 n + 8 always suffices). */
int gfl_concave_hull(const double* points_xy, int n, double concavity, double length_threshold, double* ring_xy,
                     int cap_vertices);

/* ---- deterministic inclusive scan of doubles (305) -----------------------------------------------------------------
 * out[i] = in[0] + ... + in[i], summed in an order that depends on n alone (blocks of GFL_SCAN_CHUNK values, a fixed
 * fold inside a block and over the blocks in front of it): the same bits on every call, whatever the device or stream.
 * in and out may not overlap.  workspace: gfl_scan_f64_workspace_bytes(n). */
#define GFL_SCAN_CHUNK 2048
size_t gfl_scan_f64_workspace_bytes(int n);
int gfl_scan_f64(const double* in, int n, double* out, void* workspace, size_t workspace_bytes, gfl_stream_t stream);

/* ---- point tracking (306; gflow_amd/tracking.py, INTEGRATION.md "Point tracking") ---------------------------------
 * gfl_track_anchor: for each of n_new queries query_xy[i] = (x, y) (float64, pixels) the row of uv (N rows of uv_stride
 * floats, (u, v) in the first two: fit records with stride 12, or a dense (N, 2) array) closest to it -- exactly np.argmin
 * over the rows of (u - x)^2 + (v - y)^2 in float64, every product and the sum rounded on its own (no FMA): the lowest
 * index among equal minima, the first NaN distance if there is one.  Writes anchor[i] (int32) and
 * shift_xy[i] = query_xy[i] - (double)uv[anchor[i]].  Deterministic by construction (a lexicographic min over
 * (distance, index); no atomics).  Two launches.  workspace: gfl_track_anchor_workspace_bytes(n_new, N).  N >= 1 when
 * n_new > 0.
 * gfl_track_frame: for each of the first n_anchored queries, with a = anchor[q] and (u, v) = uv[a]:
 *   tracks[q][frame] = (float)((double)u + shift_xy[q].x), (float)((double)v + shift_xy[q].y)   (tracks: [Q][T][2] float32)
 *   occluded[q][frame] = |depth_map[rint(v)][rint(u)] - depth[a * depth_stride]| > occ_threshold  (float32; [Q][T] uint8)
 * rint rounds half to even; a rounded pixel outside [0, W) x [0, H) is occluded (1); an anchor outside [0, N) gives a NaN
 * track, occluded.  depth_map: [H][W] (the fused forward's render plane 3).  Other frames' columns are not touched.
 * Both: no allocation, no host synchronisation; callable on the fit's stream between graph replays. */
size_t gfl_track_anchor_workspace_bytes(int n_new, int N);
int gfl_track_anchor(const float* uv, int uv_stride, int N, const double* query_xy, int n_new, int32_t* anchor,
                     double* shift_xy, void* workspace, size_t workspace_bytes, gfl_stream_t stream);
int gfl_track_frame(const float* uv, int uv_stride, const float* depth, int depth_stride, int N, const float* depth_map,
                    int W, int H, const int32_t* anchor, const double* shift_xy, int n_anchored, int frame, int T,
                    float occ_threshold, float* tracks, uint8_t* occluded, gfl_stream_t stream);

/* ---- backward point tracking (added within 312; gflow_amd/tracking.py, INTEGRATION.md "Point tracking") --------------
 * The frames BEFORE a query's frame.  Rows are only ever appended, N_0 <= N_1 <= ...: a query [t, y, x] is carried back to
 * frame i < t by a splat that frame i already had.  With uv_i the (u, v) of frame i and xy = (x, y):
 *   b = back_anchor[q][i] = argmin over n < N_i of |uv_t[n] - xy|^2   -- positions of the query's OWN frame, candidates cut
 *       to frame i's rows; gfl_track_anchor's key order (float64, products and sum rounded on their own, a NaN distance
 *       first, the lowest index among equal minima).  Hence b == anchor[q] wherever anchor[q] < N_i.
 *   tracks[q][i] = (float)((double)uv_i[b] + (xy - (double)uv_t[b]))
 *   occluded[q][i] = gfl_track_frame's flag of row b in frame i
 * gfl_track_history, once per frame, one lane per row: hist_uv[n] = (u, v) of row n (float32 [N][2]) and hist_occ[n] =
 * |depth_map[rint(v)][rint(u)] - depth[n * depth_stride]| > occ_threshold (uint8 [N]; float32, rint half to even, a rounded
 * pixel outside the image: 1) -- this frame's slice of the clip's history.  Strided inputs as gfl_track_frame's.  N == 0
 * launches nothing.
 * gfl_track_backward, once per clip: hist_uv / hist_occ are the frames' slices concatenated, row_start a DEVICE int64[T + 1]
 * with N_i = row_start[i + 1] - row_start[i] (the caller guarantees N_i >= 1 and N_i <= N_{i+1}: the library cannot check a
 * device array without reading it back; rows past a later frame's count are never read), query_frame a DEVICE int32[Q]
 * (queries sorted by frame are fastest, any order is correct; a frame outside (0, T) leaves the query's row untouched),
 * query_xy float64 [Q][2], hist_uv 8-byte aligned.  Writes ONLY the columns i < t of tracks [Q][T][2], occluded [Q][T] and
 * back_anchor (int32 [Q][T]; may be NULL).  A row that does not exist (N_i == 0) gives a NaN track, occluded, back_anchor
 * -1.  Three launches; deterministic by construction (a lexicographic minimum over (distance, index), no atomics).
 * workspace: gfl_track_backward_workspace_bytes(Q, T) (callable without a device).
 * All: no allocation, no host synchronisation; callable on the fit's stream.  GFL_ERR_INVALID before any launch for null
 * pointers, T <= 0, Q < 0, N < 0, uv_stride < 2, depth_stride < 1; GFL_ERR_WORKSPACE for a workspace that is too small. */
int gfl_track_history(const float* uv, int uv_stride, const float* depth, int depth_stride, int N, const float* depth_map,
                      int W, int H, float occ_threshold, float* hist_uv, uint8_t* hist_occ, gfl_stream_t stream);
size_t gfl_track_backward_workspace_bytes(int Q, int T);
int gfl_track_backward(const float* hist_uv, const uint8_t* hist_occ, const int64_t* row_start, int T,
                       const double* query_xy, const int32_t* query_frame, int Q, float* tracks, uint8_t* occluded,
                       int32_t* back_anchor, void* workspace, size_t workspace_bytes, gfl_stream_t stream);

/* ---- moving-region segmentation score (307; gflow_amd/segmentation.py, INTEGRATION.md "Moving-region segmentation") ----
 * The sums behind the reference's per-frame J and F (gflow/benchmark.py:244-285, utils/measures/jaccard.py:14-34,
 * utils/measures/f_boundary.py:15-132) for a whole clip in one launch.  pred, gt: [T][H][W] uint8, nonzero = foreground.
 * valid: [T] or NULL; a frame with valid[t] == 0 is not read and its row of counts is zero.  counts: [T][6] uint32,
 * WRITTEN (not accumulated) by the call:
 *   0 inter = |pred & gt|        1 uni = |pred | gt|
 *   2 n_fg, 3 n_gt: boundary pixels of pred / of gt -- seg2bmap at equal size: a pixel that differs from its right, lower
 *     or lower-right neighbour; in the last row only the right neighbour counts, in the last column only the lower one,
 *     the bottom-right pixel never
 *   4 fg_match: boundary pixels of pred with a boundary pixel of gt at (dx, dy), dx^2 + dy^2 <= radius^2 (pixels outside
 *     the image contribute nothing: binary_dilation with disk(radius) and a zero border; the disc is symmetric, so this
 *     is the reference's boundary * dilated_other)        5 gt_match: the same with pred and gt exchanged
 * radius in [1, 64], else GFL_ERR_INVALID; T == 0 is GFL_OK.  Integer sums: deterministic in every mode.  No allocation,
 * no workspace, no host synchronisation (a memset of counts and one launch on `stream`). */
int gfl_seg_score(const uint8_t* pred, const uint8_t* gt, const uint8_t* valid, int T, int H, int W, int radius,
                  uint32_t* counts, gfl_stream_t stream);

/* ---- reconstruction score of one frame (308; gflow_amd/quality.py, INTEGRATION.md "Reconstruction score") ----------
 * The two sums behind the reference's per-image PSNR and SSIM (gflow/benchmark.py:191-230: piqa.PSNR() / piqa.SSIM() on the
 * saved PNG).  render: planes r, g, b, [>=3][H][W] float32 (the fused forward's render or any CHW image); gt_rgb: [H][W][3].
 *   prediction: the saved byte k = uint8(clamp(x, 0, 1) * 255), float32 with truncation (render2img), read back as
 *     p = (double)((float)k / 255.0f);  target: g = (double)clamp(gt, 0, 1);  everything after that is float64
 *   sse      = sum of (p - g)^2 over all 3 H W values
 *   ssim_sum = sum of the SSIM map over the 3 channels and the (H - 10)(W - 10) valid window positions (no padding, piqa's
 *     default): window w[i] ~ exp(-(i - 5)^2 / (2 * 1.5^2)), 11 taps, normalised, separable; mu_x, mu_y, E[x^2], E[y^2],
 *     E[xy] under the window, s_xx = E[x^2] - mu_x^2 (s_yy, s_xy likewise);
 *     ss = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2)), C1 = 1e-4, C2 = 9e-4
 * On the host: PSNR = 10 log10(1 / (sse / (3 H W) + 1e-8)), SSIM = ssim_sum / (3 (H - 10)(W - 10)).
 * sums: [T][2] float64; row `frame` is WRITTEN {sse, ssim_sum}, the other rows are not touched.  H < 11, W < 11 or frame
 * outside [0, T): GFL_ERR_INVALID.  workspace: gfl_recon_workspace_bytes(W, H) (per-workgroup partial sums).  Two launches
 * (tiles, then an ordered fold), no atomics: the same bits on every call, in every mode.  No allocation, no host
 * synchronisation; callable on the fit's stream between graph replays. */
size_t gfl_recon_workspace_bytes(int W, int H);
int gfl_recon_frame(const float* render, const float* gt_rgb, int W, int H, int frame, int T, double* sums, void* workspace,
                    size_t workspace_bytes, gfl_stream_t stream);

/* ---- dense optical flow of a frame pair and its end-point error (310; gflow_amd/flow.py, INTEGRATION.md "Flow score") ----
 * The motion field the splats of frame A imply towards frame B, on A's pixel grid, and its distance from a given flow.
 * rec_a: frame A's fit records, [n_a][12] float32, 16-byte aligned (u v A B | C opacity . . | . depth . .: what
 * gfl_fit_forward leaves in gfl_fit_state.rec; only columns 0..5 are read); ids, tile_range: frame A's depth-sorted tile
 * lists, tile_range [T][2] = start / end into ids, T = ceil(W / 16) * ceil(H / 16) (the lists may lie anywhere in ids, with
 * anything between them: reserved regions).  uv_b / depth_b: frame B's rows (n_b rows of uv_b_stride / depth_b_stride
 * floats, (u, v) in the first two / the depth in the first; views of B's records: stride 12).  Rows keep their index
 * from A to B (splats are only ever appended).
 * Every pixel (x, y), sampled at (x + GFL_PIXEL_CENTER, y + GFL_PIXEL_CENTER), walks its tile's list front to back under
 * the rule of gfl_blend_fwd: power > 0 skips; alpha = min(GFL_ALPHA_MAX, o G); alpha < GFL_ALPHA_MIN skips; the walk stops
 * BEFORE adding when T (1 - alpha) < GFL_T_MIN.  With w = alpha T:
 *   row j has a future iff j < n_b and depth_b[j] != 0; then d = (u_b - u_a, v_b - v_a) (one float32 subtraction each),
 *   num += w d, den += w.  A row without a future adds nothing, but occludes like any other: T *= 1 - alpha.
 * The pixel is valid iff den >= min_weight and both components of gt_flow are finite; then F = num / den (float32), else
 * flow_out = (0, 0) and valid_out = 0.  min_weight in (0, 1]: the share of the pixel's colour that must come from splats
 * with a known motion.  gt_flow: [H][W][2], the flow A -> B on A's grid; move_mask: [H][W] uint8 or NULL.
 * Error, float64: ex = (double)F.x - (double)gt.x, ey likewise, epe = sqrt(ex^2 + ey^2).  Three classes -- 0: every pixel,
 * 1: move_mask == 0, 2: move_mask != 0 (NULL mask: classes 1 and 2 stay zero) -- and per class six doubles
 *   {n_pixels, n_valid, epe_sum, n(epe < 1), n(epe < 3), n(epe < 5)}     (the last four over the valid pixels)
 * sums: [n_pairs][3][6] float64; row `pair` is WRITTEN, the other rows are not touched.  flow_out [H][W][2] float32 and
 * valid_out [H][W] uint8: written for every pixel, or NULL.
 * GFL_ERR_INVALID: pair outside [0, n_pairs), min_weight outside (0, 1], W or H < 1, more than 16384 tiles,
 * uv_b_stride < 2, depth_b_stride < 1, negative counts, a null or misaligned pointer that is needed, workspace_bytes <
 * gfl_flow_workspace_bytes(W, H) (0 for sizes that are refused).  n_a == 0 is GFL_OK: every pixel is invalid, only n_pixels
 * is non-zero (rec_a, ids, tile_range are not read).
 * Two launches (one workgroup per tile, then a fold of the tiles' partial sums in a fixed order), no atomics: the same bits
 * on every call, in every mode.  No allocation, no host synchronisation; callable on the fit's stream between graph
 * replays. */
size_t gfl_flow_workspace_bytes(int W, int H);
int gfl_flow_pair(const float* rec_a, int n_a, const int32_t* ids, const int32_t* tile_range, const float* uv_b,
                  int uv_b_stride, const float* depth_b, int depth_b_stride, int n_b, const float* gt_flow,
                  const uint8_t* move_mask, int W, int H, float min_weight, int pair, int n_pairs, double* sums,
                  float* flow_out, uint8_t* valid_out, void* workspace, size_t workspace_bytes, gfl_stream_t stream);

/* ---- object labels through a clip fit (additive within 312; gflow_amd/propagation.py, INTEGRATION.md "Object propagation") ---------------
 * gfl_label_frame: the label map the labelled splats of one frame imply.  rec, n, ids, tile_range: what gfl_flow_pair takes
 * for frame A -- the fit records [n][12] float32, 16-byte aligned (only columns 0..5 are read), and the depth-sorted tile
 * lists, tile_range [T][2] = start / end into ids, T = ceil(W / 16) * ceil(H / 16) (the lists may lie anywhere in ids, with
 * anything between them).  labels: uint8 [n_labels], 0 <= n_labels <= n; row j is LABELLED iff j < n_labels and
 * labels[j] < K; 255 is the canonical "unlabelled", any value >= K counts the same.  K: the number of classes, background
 * class 0 included, 2 <= K <= 16.
 * Every pixel (x, y), sampled at (x + GFL_PIXEL_CENTER, y + GFL_PIXEL_CENTER), walks its tile's list front to back under
 * the rule of gfl_blend_fwd: power > 0 skips; alpha = min(GFL_ALPHA_MAX, o G); alpha < GFL_ALPHA_MIN skips; the walk stops
 * BEFORE adding when T (1 - alpha) < GFL_T_MIN.  With w = alpha T a labelled row adds acc[label] += w (one float32 add);
 * an unlabelled row adds nothing, but occludes like any other: T *= 1 - alpha always.
 *   den = ((acc[0] + acc[1]) + ...) + acc[K - 1].  If den >= min_weight the pixel's label is the smallest k with the largest
 *   acc[k] and conf = acc[k] / den (float32); else the label is `unknown` (0 .. 255) and conf = 0.
 * label_out [H][W] uint8: written for every pixel.  conf_out [H][W] float32: written for every pixel, or NULL.
 * GFL_ERR_INVALID, before anything is launched: K outside [2, 16], min_weight outside (0, 1], W or H < 1, more than 16384
 * tiles, n < 0, n_labels outside [0, n], unknown outside [0, 255], a null or misaligned pointer that is needed (label_out
 * always; rec, ids, tile_range for n > 0; labels for n_labels > 0).  n == 0 is GFL_OK: every pixel is `unknown`, the lists
 * are not read.
 * One launch (a workgroup per tile), no atomics and no sums across lanes: the same bits on every call, in every mode.  No
 * allocation, no host synchronisation; callable on the fit's stream between graph replays.
 *
 * gfl_label_assign: unlabelled rows take the label of the pixel they sit on.  labels_inout: uint8 [n].  For every row
 * j < n with labels_inout[j] == 255: u = rec[j][0], v = rec[j][1], depth = rec[j][9]; if depth != 0 and 0 < u < W - 1 and
 * 0 < v < H - 1 (false for a NaN), m = map[(int)v][(int)u] (truncation), and if m != 255, labels_inout[j] = m.  Everything
 * else is left as it is.  map: [H][W] uint8 -- the first frame's annotation (the mask prompt), or a later frame's
 * label_out (inheritance: appended rows and rows that have just come into view).  rec needs 4-byte alignment only.
 * GFL_ERR_INVALID: W or H < 1, n < 0, a null pointer for n > 0.  n == 0 is GFL_OK.  One launch, a lane per row. */
int gfl_label_frame(const float* rec, int n, const int32_t* ids, const int32_t* tile_range, const uint8_t* labels,
                    int n_labels, int K, int W, int H, float min_weight, int unknown, uint8_t* label_out, float* conf_out,
                    gfl_stream_t stream);
int gfl_label_assign(const float* rec, int n, const uint8_t* map, int W, int H, uint8_t* labels_inout, gfl_stream_t stream);

/* ---- move masks from the flow (312; gflow_amd/move_seg.py, INTEGRATION.md "Move masks from the flow") ------------------
 * What the reference's utility/move_seg.py makes of a forward flow: a fundamental matrix by least median of squares, the
 * per-pixel Sampson error, its threshold and three morphological variants.  The LMedS is this library's own and
 * deterministic -- UNPINNED against cv2.findFundamentalMat(FM_LMEDS), whose sampler and iteration rule cannot be observed
 * here; the morphology is skimage's as recalled, UNPINNED against skimage as well.
 * flow: [H][W][2] float32, the flow i -> i + 1 on frame i's grid, in pixels.  Pixel p = y W + x.
 * Correspondences, in float32 with one rounding per operation (move_seg.py:185-203):
 *   x1 = (2 (x + 0.5) / W - 1, 2 (y + 0.5) / H - 1),   x2 = x1 + (2 flow.x / (W - 1), 2 flow.y / (H - 1))
 * Everything after that is float64.  A pixel is UNKNOWN if a component of x2 is not finite (a flow that is not finite, or
 * so large that 2 flow overflows float32): it enters neither a median nor the maximum, its error is 0 and its mask is 0.
 * Sampson error of F (row-major, move_seg.py:57-71) with h1 = (x1, 1), h2 = (x2, 1), sums from the left, every product and
 * sum rounded on its own (no FMA):
 *   d1 = F h1: d1x = (F0 x1 + F1 y1) + F2, ...;   d2 = F^T h2: d2x = (F0 x2 + F3 y2) + F6, d2y = (F1 x2 + F4 y2) + F7
 *   z = (x2 d1x + y2 d1y) + d1z;   e = z z / (((d1x^2 + d1y^2) + d2x^2) + d2y^2), and e = 0 where that denominator is 0
 *
 * gfl_epi_fundamental: samples [K][8] int32, eight pixel indices per hypothesis, drawn by the caller.  Per hypothesis the
 * Hartley-normalised 8-point fit: each side's centroid to 0 and mean distance to sqrt(2); the null vector of the 8 x 9
 * design matrix (rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1]) by cyclic Jacobi on A^T A; rank 2 by zeroing the
 * smallest singular value; F = T2^T Fn T1, scaled to ||F||_F = 1 with its entry of largest magnitude positive.  A
 * hypothesis is DEGENERATE if an index is outside [0, H W) or repeated, a sampled pixel is unknown, or F is not finite: its
 * row of F_all is zero and its median +inf.  The score of a hypothesis is the EXACT LOWER MEDIAN of e over the known pixels:
 * the element (n - 1) / 2 of the sorted errors (radix selection on the bit patterns, which order like the values for
 * e >= +0; the errors are recomputed per pass, not stored).
 *   F_all [K][9], medians [K] float64: written, or NULL.   best [1] int32: the smallest median, the lowest index among
 *   equals, -1 if every hypothesis is degenerate.   F_best [9] float64: row `best` of F_all, zeros for best = -1.
 * gfl_epi_mask: F [9] float64 ON THE DEVICE (F_best).  err = e ((H + W) / 2)^2 (an error that is not finite counts as 0);
 * r = err / max(err) over the known pixels; err_norm = (float)r; mask = r > threshold.  If the maximum is 0 or no pixel is
 * known, every output is zero (the reference divides by zero there).  Morphology with the footprint
 * disk(R) = {dx^2 + dy^2 <= R^2}: erosion counts pixels outside the image as set, dilation as unset;
 *   open = dilation(erosion(mask, 2), 2),  erode = erosion(mask, 5),  dilate = dilation(mask, 3).
 *   err_norm [H][W] float32; mask, open, erode, dilate [H][W] uint8, 0 or 255: each written for every pixel, or NULL.
 * Both: GFL_ERR_INVALID for W or H < 2, H W < 8 or > 2^30, K < 1 or > 65535, a threshold that is not finite, a null pointer
 * that is needed; GFL_ERR_WORKSPACE for workspace_bytes < gfl_epi_workspace_bytes(W, H, K) (0 for sizes that are refused;
 * gfl_epi_mask uses the part that does not depend on K: any K >= 1 will do).  Integer atomics only (counts, and the maximum
 * on its bit pattern), whose results do not depend on their order: the same inputs give the same bits on every call, in
 * every mode.  No allocation, no host synchronisation, everything on `stream`. */
size_t gfl_epi_workspace_bytes(int W, int H, int K);
int gfl_epi_fundamental(const float* flow, int W, int H, const int32_t* samples, int K, double* F_all, double* medians,
                        double* F_best, int32_t* best, void* workspace, size_t workspace_bytes, gfl_stream_t stream);
int gfl_epi_mask(const float* flow, int W, int H, const double* F, double threshold, float* err_norm, uint8_t* mask,
                 uint8_t* open, uint8_t* erode, uint8_t* dilate, void* workspace, size_t workspace_bytes, gfl_stream_t stream);

/* ---- occlusion masks from the flows (added within 312; gflow_amd/occlusion.py, INTEGRATION.md "Occlusion masks from the
 * flows") ----------------------------------------------------------------------------------------------------------------
 * The forward-backward consistency check that UniMatch runs under --pred_bidir_flow --fwd_bwd_check
 * (forward_backward_consistency_check), restated from memory: UNPINNED -- neither that code nor its defaults alpha = 0.01,
 * beta = 0.5 can be observed here.
 * fwd, bwd: [n_pairs][H][W][2] float32 in pixels, 8-byte aligned.  fwd[p] is the flow a -> b on a's grid, bwd[p] the flow
 * b -> a on b's grid.  For pixel (x, y) of pair p, with a = fwd[p][y][x] and b = bwd[p][y][x], in float32:
 *   |v| = sqrt(v.x v.x + v.y v.y);   thr = alpha (|a| + |b|) + beta      (both flows at the SAME pixel index; one threshold
 *                                                                          for both directions)
 *   d_f = |a + S(bwd[p], x + a.x, y + a.y)|,  occ_fwd = d_f > thr
 *   d_b = |b + S(fwd[p], x + b.x, y + b.y)|,  occ_bwd = d_b > thr
 * S is bilinear sampling in pixel coordinates where a corner outside the image contributes zero: torch's grid_sample(mode=
 * "bilinear", padding_mode="zeros", align_corners=True).  The weights come from the flow's own fraction, which is exact in
 * float32 (x + a.x is never formed): i = floor(a.x), t = a.x - i, columns x + i and x + i + 1 with weights 1 - t and t; the
 * same in y; a corner's weight is the product of the two.  A flow component that is not of magnitude < 2^20 (NaN included)
 * puts every corner outside: S = 0.  Every corner INSIDE the image enters the sum, so a NaN (or an infinity) there makes
 * the sample NaN even at weight 0.
 * A pixel whose d or thr is not finite is UNKNOWN in that direction: its difference is written as 0 and its mask as 0.
 * (In float32 |v| overflows from a component of about 1.8e19 on: such a flow is unknown, and so is every pixel that samples
 * it with a weight that keeps the product that large.)
 *   diff_fwd, diff_bwd [n_pairs][H][W] float32; occ_fwd, occ_bwd [n_pairs][H][W] uint8, 0 or 255: each written for every
 *   pixel, or NULL (all four NULL: GFL_OK, nothing is launched).
 * GFL_ERR_INVALID, before anything is launched: W or H < 2, n_pairs < 1, n_pairs H W > 2^30, an alpha or beta that is not
 * finite or is negative, a null or misaligned input.  ONE launch for all pairs and both directions, one lane per pixel; no
 * workspace, no atomics, no allocation, no host synchronisation, everything on `stream`; the same inputs give the same bits. */
int gfl_flow_occlusion(const float* fwd, const float* bwd, int n_pairs, int W, int H, float alpha, float beta,
                       float* diff_fwd, float* diff_bwd, uint8_t* occ_fwd, uint8_t* occ_bwd, gfl_stream_t stream);

/* ---- track overlays (additive within 312; gflow_amd/track_vis.py, INTEGRATION.md "Track overlays") ----------------------
 * The reference's trajectory visualiser (gflow/utils/traj_visualizer.py: TrajVisualizer.visualize with mode "rainbow",
 * linewidth 2, tracks_leave_trace -1, pad_value 0, query_frame 0, no segm_mask, gt_tracks or visibility) for all T frames of
 * a clip in one call: every track's polyline up to the frame, a disc where its point is visible, a cross where it is occluded.
 *   video, out [T][H][W][3] uint8 (they may not overlap);  tracks [T][N][2] float32 (x, y);  occluded [T][N] uint8 (nonzero =
 *   occluded);  lut [256][3] float32 = the gist_rainbow table;  overflow [1] int32 on the device, WRITTEN by every call with T > 0.
 * Coordinates: c = (int)clamp(v, -2^20, 2^20), truncated toward zero (the reference's .long()); a NaN gives -2^20, so every
 *   non-finite coordinate lies outside the image.  A point is USABLE when 0 <= x < W, 0 <= y < H, x != 0 and y != 0 (the
 *   reference's coord[0] != 0 and coord[1] != 0: it hides the zero rows a track has before its query frame).
 * Colours: byte c of track n = trunc(255 * lut[idx][c]) -- the float32 entry times 255 in float64, which is exact --,
 *   idx = min(int(v * 256), 255), v = (y0[n] - ymin) / (ymax - ymin) over the integer y of frame 0 (every track, usable or not),
 *   v = 0 when ymax == ymin.  With 0 < still_length < N the tracks still_length .. N-1 take ymin, ymax over themselves.  (The
 *   reference compares still_length with T there, traj_visualizer.py:222, which makes the colours depend on the clip's length.)
 * Frame t, in this order, later paint over earlier paint:
 *   1. for s = 0 .. t-1 (outer), i = 0 .. N-1 (inner): the segment tracks[s][i] -> tracks[s+1][i], width 2, drawn only if both
 *      ends are inside the image and its first end is usable;
 *   2. for i = 0 .. N-1: the marker at tracks[t][i] if that point is usable -- occluded: a cross, the segments (x-4, y) ->
 *      (x+4, y) and (x, y-4) -> (x, y+4), width 4; visible: the filled disc dx^2 + dy^2 <= 4^2 + 2.
 * Coverage, exact in integers: pixel p is on the segment (a, b, w), with d = b - a, when 0 <= (p-a).d <= d.d and
 *   4 cross(p-a, d)^2 <= w^2 (d.d), the squares in 64 bits; for a == b the segment is the single pixel a.  (Against PIL's
 *   ImageDraw.line / ellipse: each pixel set lies within one pixel of the other; the disc is PIL's exactly.)
 * Paint is opaque, so a pixel has the colour of the covering primitive with the highest paint index -- segment (s, i): s N + i,
 * marker i: (T-1) N + i -- or the video's: that is what is computed, and the result does not depend on the order in which a
 * list was filled: the same bits run after run, in every mode.
 * The clip's segments are binned ONCE into the 16 x 16 tiles their bounding box, grown by the width, touches; frame t takes the
 * entries with s < t of a tile's list.  The pool holds K_cap (segment, tile) pairs: a clip that needs more raises overflow[0] = 1
 * and its `out` is the video with the markers only, no traces at all; otherwise overflow[0] = 0.  The markers are not binned.
 * One memset and six launches whatever the data; nothing is read back or allocated: the call can be captured into a graph.
 * T == 0 succeeds and writes nothing; N == 0 copies the video.  GFL_ERR_INVALID, before anything touches a device: T or N < 0,
 * W, H or K_cap <= 0, W or H > 16384 (the products above then fit), T N >= 2^31, a NULL video, lut, out, overflow or workspace,
 * NULL tracks or occluded with T N > 0, workspace_bytes < gfl_track_vis_workspace_bytes (0 for arguments it rejects). */
size_t gfl_track_vis_workspace_bytes(int T, int N, int W, int H, int K_cap);
int gfl_track_vis(const uint8_t* video, const float* tracks, const uint8_t* occluded, int T, int N, int W, int H,
                  int still_length, const float* lut, int K_cap, uint8_t* out, int32_t* overflow, void* workspace,
                  size_t workspace_bytes, gfl_stream_t stream);

/* ---- frame preparation (additive within 312; gflow_amd/prep.py, INTEGRATION.md "Frame preparation") ----------------------
 * What the reference does to every file of a sequence after decoding it (gflow/utils/conversion.py:6-19, read.py:7-70,
 * fit_video.py:245-248): to float, torchvision's Resize(n, antialias=True), optionally GaussianBlur(7, 5.0), then depth's
 * scale and offset or the mask test -- for T frames of one shape in one call.
 *   src [T][Hs][Ws][C] uint8 (src_is_u8 = 1) or float32 (0; 4-byte aligned), interleaved as PIL, .flo and .npy give it;
 *   dst [T][Hd][Wd][C] float32, or with as_mask [T][Hd][Wd] uint8 holding 0 or 1.  Per frame and channel, in this order:
 * (a) convert: v = (float)src / div, correctly rounded (div = 255 for 8-bit images, 1 otherwise).
 * (b) resize, unless (Hd, Wd) == (Hs, Ws): bilinear with antialiasing, align_corners = False, the horizontal pass, then the
 *   vertical one.  Per axis, with s = n_in / n_out, support = max(s, 1), inv = 1 / support, output i has the centre
 *   c = s (i + 0.5), reads the taps j in [lo, hi), lo = max(0, (int)(c - support + 0.5)), hi = min((int)(c + support + 0.5),
 *   n_in), with the weights w_j = max(0, 1 - |(j - c + 0.5) inv|) divided by their sum over the taps: all of it in float64,
 *   every operation rounded on its own (nothing fused), the normalised weight then rounded to float32.  A pass is the
 *   float32 sum of w_j v_j in ascending j, product and sum rounded separately.
 *   torch's CPU kernel (F.interpolate(mode="bilinear", antialias=True)) is the SAME filter with float32 weights formed from
 *   float32 coordinates.  Measured against it: values differ by up to 2.8e-6 at 240 columns, growing with the coordinate; a
 *   mask (> 0 after the resize) differs in 1-3 % of its pixels at non-dyadic scales (31x47 -> 7x10, 13x29 -> 5x11, 33x59 ->
 *   13x23; random masks, 3 % set) -- the pixels where a source pixel sits exactly on the edge of the support -- and in none
 *   at the scales 2.0, 2.5, 2.25 or at an upscale of 1.5.  What torch computes there is not reproducible bit for bit; this is.
 * (c) blur, when blur_k > 0 (odd, 3 .. 31, blur_k / 2 < min(Hd, Wd); blur_sigma finite and > 0): the taps
 *   exp(-0.5 (x / sigma)^2) at x = -(k - 1) / 2 .. (k - 1) / 2, normalised in float64 and rounded to float32; reflect padding
 *   (index -i reads i, the edge is not repeated); the horizontal pass, then the vertical one, float32 sums in ascending tap
 *   order.
 * (d) output: r mul + add, a multiply and an add rounded separately (read_depth's * depth_scale + depth_offset; skipped for
 *   mul = 1, add = 0).  With as_mask: 1 where the channels' sum in ascending c is > 0, else 0 (a NaN gives 0); blur_k, mul and
 *   add must then be 0, 1 and 0.
 * GFL_ERR_INVALID, before anything is launched: T < 1, C outside 1 .. 4, an extent < 1 or > 16384, n_in > 64 n_out on an
 * axis, more than 2^31 - 1 elements in src, in the horizontal intermediate [T][Hs][Wd][C] or in dst, a div that is not
 * finite and > 0, a mul or add that is not finite, a bad blur_k or blur_sigma, src_is_u8 or as_mask that is not 0 or 1, a NULL
 * src, dst or workspace, a float32 src or dst that is not 4-byte aligned, a workspace that is not 16-byte aligned or is
 * smaller than gfl_prep_workspace_bytes (0 for arguments it rejects).
 * The launches are fixed by the arguments alone: the tables (one launch: the 256 conversions of a uint8 source and the two
 * axes' taps), the two resize passes -- or one conversion launch where the resize is skipped --, and the two blur passes
 * when on.  No atomics, no allocation, no host synchronisation, everything on `stream`; the same inputs give the same bits. */
size_t gfl_prep_workspace_bytes(int T, int C, int Hs, int Ws, int Hd, int Wd, int blur_k);
int gfl_prep_frames(const void* src, int src_is_u8, int T, int C, int Hs, int Ws, int Hd, int Wd, float div, float mul,
                    float add, int blur_k, float blur_sigma, int as_mask, void* dst, void* workspace, size_t workspace_bytes,
                    gfl_stream_t stream);

/* ---- video files (additive within 312; gflow_amd/video.py, INTEGRATION.md "Video files") ---------------------------------
 * Baseline sequential JPEG (ITU-T T.81, 8 bits per sample) of T images of one shape in two calls: the entropy-coded SCAN of
 * every image.  The host puts the header in front (gflow_amd.video.jpeg_header) and EOI behind.
 *   images [T][H][W][C] uint8, C = 3 (R, G, B -> YCbCr 4:4:4, an MCU is the blocks Y, Cb, Cr) or C = 1 (one grey component);
 *   qtables [2][64] uint16 on the device, natural (row-major) order: [0] luminance / grey, [1] chrominance; 0 counts as 1.
 * Arithmetic, float32, nothing rounded to integers on the way: Y = 0.299 R + 0.587 G + 0.114 B - 128,
 *   Cb = -0.168736 R - 0.331264 G + 0.5 B, Cr = 0.5 R - 0.418688 G - 0.081312 B (JFIF, level shift included; grey: v - 128);
 *   the separable 8x8 DCT-II of A.3.3, rows then columns; coefficient = F / q rounded half away from zero; zigzag.  A block
 *   that hangs over the right or bottom edge repeats the last column / row.
 * Entropy coding: Annex K's four Huffman tables (K.3 - K.6), fixed.  The scan is cut into restart intervals of
 *   GFL_JPEG_RI MCUs in scan order (not per MCU row; a frame's last interval is shorter): each is a byte-aligned bit stream,
 *   padded with 1-bits, whose DC prediction starts from 0, FF stuffed as FF 00, followed -- except the frame's last -- by
 *   RSTm, m = (interval index) mod 8.  One workgroup codes one (frame, interval); the bytes depend on the inputs alone.
 * gfl_jpeg_sizes codes every interval, keeps its length, and scans the lengths: the interval offsets stay in the workspace,
 *   frame_offsets [T + 1] int64 on the device = where frame t's scan starts in `out`, [T] = the total.  gfl_jpeg_emit (same
 *   images, shape, qtables and workspace, after gfl_jpeg_sizes on the same stream) codes again through the same routine and
 *   writes every interval at its offset: exactly frame_offsets[T] bytes.  An interval that would end behind out_bytes is not
 *   written at all -- nothing is ever stored outside [out, out + out_bytes).
 * GFL_ERR_INVALID, before any launch: a NULL pointer, C not 1 or 3, T, W or H < 1, W or H > 65535, more than 2^30
 *   (frame, interval) pairs, out_bytes < 1, a workspace or frame_offsets that is not 8-byte aligned.  GFL_ERR_WORKSPACE:
 *   workspace_bytes < gfl_jpeg_workspace_bytes (0 for arguments it rejects).  No allocation, no host synchronisation;
 *   gfl_jpeg_restart_interval and gfl_jpeg_workspace_bytes need no device. */
#ifndef GFL_JPEG_RI
#define GFL_JPEG_RI 32
#endif
int gfl_jpeg_restart_interval(void);
size_t gfl_jpeg_workspace_bytes(int T, int C, int W, int H);
int gfl_jpeg_sizes(const uint8_t* images, int T, int C, int W, int H, const uint16_t* qtables, int64_t* frame_offsets,
                   void* workspace, size_t workspace_bytes, gfl_stream_t stream);
int gfl_jpeg_emit(const uint8_t* images, int T, int C, int W, int H, const uint16_t* qtables, uint8_t* out, int64_t out_bytes,
                  void* workspace, size_t workspace_bytes, gfl_stream_t stream);

/* Decoding (additive within 312; gflow_amd.video.decode_jpeg, INTEGRATION.md "Decoding video files"; the arithmetic lives
 * in csrc/gfl_jpeg_dec.hpp, which a host compiler takes too: tools/jpeg_dec_host.cpp).  T baseline sequential JPEG images
 * (SOF0, 8 bits, one interleaved scan) of ONE shape, component count and sampling -> images [T][H][W][C] uint8, with the
 * bits libjpeg's default path gives (slow-integer IDCT, fancy upsampling, 16-bit fixed-point YCbCr -> RGB).
 *   C = 1: one grey component, hs = vs = 1.  C = 3: Y sampled hs x vs = 1x1, 2x1 or 2x2 (4:4:4, 4:2:2, 4:2:0), Cb and Cr
 *   1x1; an MCU is the hs * vs blocks of Y row by row, then Cb, then Cr, and covers 8 hs x 8 vs pixels; MCUs run row by row.
 * The host parses the files.  It passes every frame's entropy-coded data (markers removed, FF 00 stuffing left in) in
 * `bytes`, and cuts it into UNITS: a unit is one restart interval of one frame (a file without DRI is one unit), a
 * byte-aligned bit stream whose DC predictors start at 0.
 *   gfl_jpeg_unit, 24 bytes: frame; first_mcu, n_mcu: the MCUs it codes, in scan order of its frame; n_bytes, offset: its
 *     data is bytes[offset, offset + n_bytes).
 *   gfl_jpeg_frame_tables, 1364 bytes, one per frame: q[i]: quantiser table i, 64 entries in NATURAL (row-major) order;
 *     qsel / dcsel / acsel[c]: the table ids of component c (< 4, < 2, < 2); first_unit, n_units: the frame's units are
 *     units[first_unit, first_unit + n_units); huff[0], [1]: the DC tables 0 and 1, huff[2], [3]: the AC tables, each as
 *     the BITS and HUFFVAL lists of a DHT segment (unused entries 0).
 * Two stages.  Entropy: a lane per unit, the frame's Huffman tables (T.81 F.2.2.3: maxcode / valptr) in LDS, quantised
 * coefficients as int16 into the workspace (zeroed first).  Pixels: coef * q, the two-pass 13-bit LL&M inverse DCT (DESCALE
 * by 11, then by 18), + 128, clamp; then triangle upsampling of the cropped chroma planes and the colour transform.
 * Malformed data never becomes a bad address: a reader never looks past its unit's bytes (behind them it supplies 1-bits),
 * every coefficient index is checked, and a unit that goes wrong stops and says so in unit_status [n_units] int32:
 *   0 fine; 1 the unit record is out of range (nothing decoded); 2 a code that matches no Huffman code; 3 a coefficient
 *   index past 63; 4 the data ended early; 5 data left behind the last MCU; 6 a symbol out of range; -1 never run (no frame
 *   lists the unit).  A block is stored only once it is decoded whole: the blocks behind stay zero.
 * GFL_ERR_INVALID, before any launch: a NULL pointer, T or n_units < 1, n_bytes < 0, C / hs / vs not as above, W or H
 *   outside 1 .. 65535, more than 2^30 blocks, a workspace that is not 16-byte aligned.  GFL_ERR_WORKSPACE: workspace_bytes <
 *   gfl_jpeg_decode_workspace_bytes (0 for arguments it rejects; needs no device).  No allocation, no host synchronisation.
 * gfl_jpeg_decode_struct_bytes: sizeof of the two structs, for a binding to check its mirror against. */
typedef struct gfl_jpeg_unit {
    int32_t frame, first_mcu, n_mcu, n_bytes;
    int64_t offset;
} gfl_jpeg_unit;
typedef struct gfl_jpeg_huff_spec {
    uint8_t bits[16];
    uint8_t vals[256];
} gfl_jpeg_huff_spec;
typedef struct gfl_jpeg_frame_tables {
    uint8_t q[4][64];
    uint8_t qsel[4], dcsel[4], acsel[4];
    int32_t first_unit, n_units;
    gfl_jpeg_huff_spec huff[4];
} gfl_jpeg_frame_tables;
size_t gfl_jpeg_decode_workspace_bytes(int T, int C, int W, int H, int hs, int vs, int64_t n_units);
int gfl_jpeg_decode(const uint8_t* bytes, int64_t n_bytes, const gfl_jpeg_unit* units, int64_t n_units,
                    const gfl_jpeg_frame_tables* tables, int T, int C, int W, int H, int hs, int vs, uint8_t* images,
                    int32_t* unit_status, void* workspace, size_t workspace_bytes, gfl_stream_t stream);
int gfl_jpeg_decode_struct_bytes(int* sizeof_unit, int* sizeof_frame_tables);

/* ---- PNG files (additive within 312; gflow_amd/png.py, INTEGRATION.md "PNG files") -----------------------------------------
 * The zlib stream (RFC 1950 / 1951) of T PNG images of one shape in two calls: what an IDAT chunk holds.  The host puts the
 * chunks around it (gflow_amd.png.png_chunks).
 *   images [T][H][W][C] uint8, contiguous, C = 1 (grey, or indices of a palette) or C = 3 (R, G, B).
 * Filtered bytes: every row is the filter-type byte 2 (Up) and its W C bytes minus the RAW row above, mod 256; the row above
 *   row 0 is zeros.  An image is cut into strips of gfl_png_strip_rows(C, W) = clamp(32768 / (1 + W C), 1, 64) rows (its last
 *   strip is shorter), so that a strip's filtered bytes fit in 32 KiB of LDS; 0: one filtered row does not fit, the shape is
 *   refused.  The row above a strip's first row is the previous strip's last row.  One workgroup codes one (image, strip).
 * Tokens: a literal, or a match of length 3 .. 258 at distance 1.  Matches are runs of one byte value inside the strip's filtered
 *   bytes: the run's first byte is a literal, then matches of 258 while 258 bytes are left, then one match of 3 .. 257, or the
 *   1 or 2 bytes left as literals.
 * A strip is one non-final block of dynamic Huffman codes (BTYPE = 10) followed by an empty stored block (000, zero bits to
 *   the byte, 00 00 FF FF), so that every strip ends on a byte -- or, where that would be longer, one stored block (5 + n bytes
 *   for n filtered bytes): a strip never takes more than n + 5 bytes.  The literal / length code is built from the strip's own
 *   histogram (EOB always present, lengths <= 15), the distance alphabet is always one symbol (distance 1) of length 1, the
 *   code-length sequence uses the symbols 16 / 17 / 18 and its own code has lengths <= 7; both codes are complete (Kraft sum 1).
 * An image's stream: 78 01, its strips, 03 00 (a final block that holds EOB alone), the big-endian Adler-32 of all its filtered
 *   bytes -- taken per strip and combined in order: A = A1 + A2 - 1, B = B1 + B2 + n2 (A1 - 1), both mod 65521.
 * gfl_png_sizes codes every strip, keeps its length and Adler-32, scans the lengths and combines the sums: the strip offsets
 *   stay in the workspace, frame_offsets [T + 1] int64 on the device = where image t's stream starts in `out`, [T] = the total.
 *   gfl_png_emit (same images, shape and workspace, after gfl_png_sizes on the same stream) codes again through the same
 *   routine and writes every strip at its offset: exactly frame_offsets[T] bytes.  A strip that would end behind out_bytes is
 *   not written at all -- nothing is ever stored outside [out, out + out_bytes).  The bytes depend on the inputs alone.
 * GFL_ERR_INVALID, before any launch: a NULL pointer, C not 1 or 3, T, W or H < 1, gfl_png_strip_rows(C, W) = 0, more than 2^30
 *   (image, strip) pairs, out_bytes < 1, a workspace or frame_offsets that is not 8-byte aligned.  GFL_ERR_WORKSPACE:
 *   workspace_bytes < gfl_png_workspace_bytes (0 for arguments it rejects).  No allocation, no host synchronisation;
 *   gfl_png_strip_rows and gfl_png_workspace_bytes need no device. */
int gfl_png_strip_rows(int C, int W);
size_t gfl_png_workspace_bytes(int T, int C, int W, int H);
int gfl_png_sizes(const uint8_t* images, int T, int C, int W, int H, int64_t* frame_offsets, void* workspace,
                  size_t workspace_bytes, gfl_stream_t stream);
int gfl_png_emit(const uint8_t* images, int T, int C, int W, int H, uint8_t* out, int64_t out_bytes, void* workspace,
                 size_t workspace_bytes, gfl_stream_t stream);

/* Decoding (additive within 312; gflow_amd.png.decode_png, INTEGRATION.md "Decoding PNG files"; the decoder proper -- bit reader,
 * block headers, table construction, symbol decode -- lives in csrc/gfl_inflate.hpp, which a host compiler takes too:
 * tools/png_dec_host.cpp; the device's input staging and output window are csrc/gfl_png_dec.hip's alone).  The zlib streams of T
 * non-interlaced 8-bit PNG images of one shape -> their pixels, the bits of np.asarray(PIL.Image.open(file)).
 *   data [n_bytes] uint8; offsets [T + 1] int64 on the device (8-byte aligned): image t's stream -- its IDAT payloads put
 *     together -- is data[offsets[t], offsets[t + 1]), clipped to [0, n_bytes] whatever the offsets say.
 *   bpp = bytes per pixel, 1 .. 4 (grey or palette indices, grey + alpha, RGB, RGBA); images [T][H][W][bpp] uint8.
 * Two launches.  inflate: one 64-lane workgroup per image (a stream is serial) turns the stream into its H (1 + W bpp)
 *   filtered bytes in the workspace -- stored, fixed and dynamic blocks, distances up to 32768, overlapping copies; window and
 *   code tables in LDS.  unfilter: filter types 0 .. 4 per row, the row above row 0 zeros, a lane per row.
 * status [T] int32 (4-byte aligned): 0, or the FIRST error of the image's stream in stream order -- decoding of that image
 *   stops there, the image is left entirely zero, other images of the call are unaffected.  The filter-type bytes are looked
 *   at once the stream has passed all other checks.  Bytes behind the checksum are ignored.  Every read of `data` and every
 *   write is bounds-checked against the image's own extent: malformed input gives a status, never an out-of-range access.
 * GFL_ERR_INVALID, before any launch: a NULL pointer, T, W or H < 1, bpp outside 1 .. 4, n_bytes < 0, an image of 2^31 or more
 *   filtered bytes, a workspace that is not 16-byte aligned.  GFL_ERR_WORKSPACE: workspace_bytes <
 *   gfl_png_decode_workspace_bytes (0 for arguments it rejects; needs no device).  No allocation, no host synchronisation. */
#define GFL_PNG_OK 0
#define GFL_PNG_INPUT_END 1        /* the input ends early */
#define GFL_PNG_BAD_HEADER 2       /* zlib header: CM != 8, window > 32 KiB, FCHECK, FDICT set */
#define GFL_PNG_BLOCK_TYPE 3       /* reserved block type */
#define GFL_PNG_STORED_LEN 4       /* a stored block's LEN / NLEN disagree */
#define GFL_PNG_TOO_MANY_CODES 5   /* HLIT > 286 or HDIST > 30 */
#define GFL_PNG_BAD_REPEAT 6       /* a repeat code with nothing to repeat, or one running past the end */
#define GFL_PNG_BAD_CODE 7         /* an over-subscribed code, or an incomplete one (but a single code of length 1) */
#define GFL_PNG_NO_END_OF_BLOCK 8  /* no end-of-block code */
#define GFL_PNG_BAD_SYMBOL 9       /* an undefined symbol, or a length or distance symbol out of range */
#define GFL_PNG_FAR_DISTANCE 10    /* a distance reaching before the start of the output */
#define GFL_PNG_OUTPUT_SIZE 11     /* more or fewer output bytes than H (1 + W bpp) */
#define GFL_PNG_BAD_ADLER 12       /* Adler-32 mismatch */
#define GFL_PNG_BAD_FILTER 13      /* a filter-type byte above 4 */
size_t gfl_png_decode_workspace_bytes(int T, int bpp, int W, int H);
int gfl_png_decode(const uint8_t* data, int64_t n_bytes, const int64_t* offsets, int T, int bpp, int W, int H, uint8_t* images,
                   int32_t* status, void* workspace, size_t workspace_bytes, gfl_stream_t stream);

/* ---- optical flow (additive within 312; gflow_amd/optflow.py, INTEGRATION.md "Flows from the images") --------------------
 * The flow a -> b on a's grid, in pixels, of P pairs of images: a classical coarse-to-fine variational estimate (robust data
 * term on the grey value, robust isotropic smoothness), NOT a learned one.  All arithmetic is float32 in the order written,
 * products and sums rounded separately (nothing fused); tests/optflow_ref.py restates it in float64.
 *   a, b [P][H][W][3] uint8 (src_is_u8 = 1: v / 255) or float32 in [0, 1];  flow_out [P][H][W][2] float32 (8-byte aligned).
 * (1) grey: I = 255 ((0.299 R + 0.587 G) + 0.114 B).
 * (2) pyramid: level 0 is the image; level l + 1 is (ceil(H_l / 2), ceil(W_l / 2)), pixel (x, y) = level l filtered by
 *   ((((f(-2) + 4 f(-1)) + 6 f(0)) + 4 f(1)) + f(2)) / 16 along the rows, then along the columns, border replicated, sampled
 *   at (2x, 2y).  Levels are added while min(H_l, W_l) / 2 (integer) >= min_side.
 * (3) the flow is zero at the coarsest level; flow_l(x, y) = 2 B(flow_{l+1}, x / 2, y / 2), coordinates clamped to the coarse
 *   grid.  B(f, x, y), bilinear: x0 = floor(x), x1 = min(x0 + 1, W - 1), t = x - x0 (y likewise),
 *   (1 - ty) ((1 - tx) f00 + tx f01) + ty ((1 - tx) f10 + tx f11).
 * (4) per level, `warps` times with the current (u, v): Iw(x, y) = B(Ib, x + u, y + v) with the coordinates clamped to the
 *   image, inside = 1 where the unclamped ones lie in [0, W - 1] x [0, H - 1], else 0; D = the central difference
 *   1/2 (f(+1) - f(-1)), border replicated; Ix = 1/2 (Dx Iw + Dx Ia), Iy likewise, It = Iw - Ia; du = dv = 0.  `outer` times:
 *     pd = inside / sqrt(((It + Ix du) + Iy dv)^2 + 1e-6),
 *     ps = alpha / sqrt(((Dx U)^2 + (Dy U)^2) + ((Dx V)^2 + (Dy V)^2) + 1e-6), U = u + du, V = v + dv,
 *     wl = 1/2 (ps + ps_left) and wr, wt, wb likewise, 0 where the neighbour lies outside the image, ws = ((wl + wr) + wt) + wb,
 *     a11 = (pd Ix) Ix + ws, a22 = (pd Iy) Iy + ws, a12 = (pd Ix) Iy, c1 = (pd Ix) It, c2 = (pd Iy) It;
 *   then `sweeps` Jacobi sweeps, each reading only the previous sweep's (du, dv):
 *     su = (((wl U_l + wr U_r) + wt U_t) + wb U_b) - ws u (sv likewise), b1 = su - c1, b2 = sv - c2, det = a11 a22 - a12 a12,
 *     du = (a22 b1 - a12 b2) / det, dv = (a11 b2 - a12 b1) / det.
 *   Then u += du, v += dv.
 * gfl_optflow runs all of it; gfl_optflow_level runs step (4) alone on grey images Ia, Ib [P][H][W] from the starting flow in
 * flow_inout [P][H][W][2], which it replaces (any workspace of gfl_optflow_workspace_bytes(P, H, W, min_side) bytes is large
 * enough for it, whatever min_side).  The sweeps run fused, several per launch on a tile with a ring of as many pixels (the
 * interior then has exactly the bits of that many plain sweeps), and a level that fits one workgroup runs a re-weighting's
 * sweeps in one launch; GFL_OPTFLOW_FUSED=0 in the environment (read at every call) launches every sweep on its own
 * instead, with the same bits.
 * GFL_ERR_INVALID, before any launch: P < 1, H or W < 8, P H W > 2^30, an alpha that is not finite and > 0, warps, outer or
 * sweeps < 1, min_side < 2, src_is_u8 not 0 or 1, a NULL pointer, float images that are not 4-byte aligned, a flow that is not
 * 8-byte aligned, a workspace that is not 16-byte aligned.  GFL_ERR_WORKSPACE: workspace_bytes too small
 * (gfl_optflow_workspace_bytes: 0 for arguments it rejects; needs no device).  No atomics, no allocation, no host
 * synchronisation, everything on `stream`; the same inputs give the same bits, and a problem's result does not depend on
 * the others in its call. */
size_t gfl_optflow_workspace_bytes(int P, int H, int W, int min_side);
int gfl_optflow(const void* a, const void* b, int src_is_u8, int P, int H, int W, float alpha, int warps, int outer, int sweeps,
                int min_side, float* flow_out, void* workspace, size_t workspace_bytes, gfl_stream_t stream);
int gfl_optflow_level(const float* Ia, const float* Ib, float* flow_inout, int P, int H, int W, float alpha, int warps,
                      int outer, int sweeps, void* workspace, size_t workspace_bytes, gfl_stream_t stream);

/* ---- depth and camera from the flows (additive within 312; gflow_amd/sfm.py, INTEGRATION.md "Depth and camera from the
 * flows") -----------------------------------------------------------------------------------------------------------------
 * Classical two-view geometry for P pair problems of one shape at once: what a clip fit otherwise reads from MASt3R's
 * depth and camera files, from the flows alone.  It is NOT MASt3R and is unpinned against it: depth is recovered only where
 * the camera translates (parallax), moving and occluded regions are filled from their surroundings, and it has not been run
 * on real video.  tests/sfm_ref.py restates every stage in float64.
 *   flow [P][H][W][2] float32, in pixels: pixel (x, y) of view 1 -- centres at integer coordinates -- is seen at
 *   (x, y) + flow in view 2.  A pixel is KNOWN when both components are finite.  The camera is fx, fy, cx, cy for both views.
 * gfl_sfm_refit: F_init, F_out [P][9] float64 row-major with x2^T F x1 = 0 in pixel coordinates (they may be the same
 *   array); exclude [P][H][W] uint8 or NULL, nonzero = leave the pixel out.  `rounds` times: e = the Sampson error
 *   z^2 / (d1x^2 + d1y^2 + d2x^2 + d2y^2), z = x2^T F x1, d1 = F x1, d2 = F^T x2 (0 for a zero denominator) of every USABLE
 *   pixel (known, not excluded, e finite); med = its exact lower median (rank (n - 1) / 2, by radix selection on the bit
 *   pattern); inliers are e <= max(2.5^2 1.4826^2 med, e_floor); over them the Hartley-normalised 8-point fit (per view:
 *   centroid to 0, mean distance to sqrt 2; the 45 unique sums of A^T A over the rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1,
 *   y1, 1], its null vector by cyclic Jacobi, rank 2 by dropping F^T F's smallest eigenvector, de-normalised, ||F||_F = 1
 *   with the entry of largest magnitude positive).  A pair with fewer than 8 inliers, or whose fit is not finite, keeps its
 *   F.  Then, with the final F: median [P], counts [P][2] int32 = (usable pixels, inliers), inlier [P][H][W] uint8 0 / 1.
 *   An F that is not finite leaves a pair without usable pixels (median NaN).  0 <= rounds <= 16.
 * gfl_sfm_pose: E = K^T F K, K = [fx 0 cx; 0 fy cy; 0 0 1]; its singular vectors from Jacobi on E^T E, the singular values
 *   taken as (1, 1, 0); the rotations U W V^T and U W^T V^T (det +1), the one with the LARGER TRACE first; t0 = u3 with its
 *   entry of largest magnitude positive.  Candidate c = (rotation c / 2, +t0 for even c, -t0 for odd c).  An inlier votes for
 *   c when both depths of its triangulation (below) are > 0; the winner has the most votes, the lowest c among equals.
 *   parallax = the exact lower median over the inliers of |x2 - K (R x1) / (R x1)_z| in pixels (0 without inliers).
 *   degenerate = usable < 8, or inliers < min_share usable, or F, R or t not finite, or not parallax >= min_parallax; then
 *   t = 0, and R is kept if finite, else the identity.  R [P][9], t [P][3] (unit), parallax [P] float64; votes [P][4],
 *   degenerate [P] int32.  counts, inlier: as gfl_sfm_refit wrote them.
 * gfl_sfm_triangulate: a = R K^-1 (x, y, 1), b = K^-1 (x2, y2, 1), c = a x b: the least-squares solution of z1 a + t = z2 b is
 *   z1 = c . (b x t) / |c|^2, z2 = c . (a x t) / |c|^2; rho = 1 / z1 and weight = |c|^2 / (|a|^2 |b|^2) = sin^2 of the angle,
 *   evaluated in float64 and stored as float32 [P][H][W]; both 0 where z1 <= 0, z2 <= 0, the pixel is not an inlier or the
 *   pair is degenerate.
 * gfl_sfm_median: per row m of M, the exact lower median of the float32 quotient a / b (b NULL: of a) over the pixels with
 *   wa > w_min and wb > w_min (a NULL weight passes) and a finite quotient; median [M] float64 (NaN for none), count [M]
 *   int32.  All arrays [M][H][W] float32.  The baseline ratio of a frame is this with a = rho of its forward pair and b = rho
 *   of its backward pair.
 * gfl_sfm_fuse: rho = (wf (rf sf[t]) + wb (rb sb[t])) / (wf + wb), weight = wf + wb, rho = 0 where the weight is 0; float32,
 *   every operation rounded on its own; scale_f, scale_b [T] float64 on the device (1 / baseline), rounded to float32.
 * gfl_sfm_fill: pull -- level l + 1 is (ceil(H_l / 2), ceil(W_l / 2)) down to 1 x 1, a pixel the weighted mean of the fine
 *   pixels (min(2X + dx, W_l - 1), min(2Y + dy, H_l - 1)), dx, dy in {0, 1}, its weight a quarter of their weights' sum (value 0
 *   without weight); push -- from the coarsest level upward a pixel WITHOUT weight takes the bilinear sample of the filled
 *   coarser level at (x / 2 - 1/4, y / 2 - 1/4) clamped to that grid; then `sweeps` Jacobi sweeps of
 *   min sum w (rho - rho0)^2 + lambda sum_pq (rho_p - rho_q)^2 over the 4-neighbours inside the image: with S, k their sum
 *   (left, right, top, bottom) and number, rho <- rho0 + lambda (S - k rho0) / (w + lambda k) where w > 0, else S / k (kept for
 *   lambda = 0); lambda [T] float64 on the device; depth [T][H][W] = 1 / max(rho, rho_min).  The sweeps run four per launch on
 *   a 32 x 32 LDS tile with a ring of four pixels (the interior then has exactly the bits of four plain sweeps);
 *   GFL_SFM_FUSED=0 in the environment (read at every call) launches every sweep on its own, with the same bits.
 * GFL_ERR_INVALID, before any launch: P (M, T) < 1 or > 65535, H or W < 8 or > 16384, P H W > 2^30, a camera value that is not
 *   finite or a focal <= 0, rounds, sweeps, e_floor, w_min, rho_min, min_parallax or min_share out of range or not finite, a
 *   NULL pointer other than exclude / b / wa / wb, a workspace that is not 16-byte aligned.  GFL_ERR_WORKSPACE:
 *   workspace_bytes < gfl_sfm_workspace_bytes(P, H, W) (0 for arguments it rejects; needs no device).  ONE layout
 *   serves every entry, so the query is the refit's need -- about 19 bytes per pixel and problem -- and gfl_sfm_median and
 *   gfl_sfm_fill ask for more than they touch (fill leaves the 8-byte values and the histograms alone).  No allocation, no
 *   host synchronisation, everything on `stream`.  No float atomics: the sums are per-workgroup float64 partials folded in
 *   a fixed order, the counts integer atomics -- the same inputs give the same bits, and a problem's result does not depend
 *   on the others in its call. */
size_t gfl_sfm_workspace_bytes(int P, int H, int W);
int gfl_sfm_refit(const float* flow, const double* F_init, const uint8_t* exclude, int P, int H, int W, int rounds,
                  double e_floor, double* F_out, int32_t* counts, double* median, uint8_t* inlier, void* workspace,
                  size_t workspace_bytes, gfl_stream_t stream);
int gfl_sfm_pose(const float* flow, const double* F, const uint8_t* inlier, const int32_t* counts, int P, int H, int W, double fx,
                 double fy, double cx, double cy, double min_parallax, double min_share, double* R, double* t, int32_t* votes,
                 double* parallax, int32_t* degenerate, void* workspace, size_t workspace_bytes, gfl_stream_t stream);
int gfl_sfm_triangulate(const float* flow, const uint8_t* inlier, const double* R, const double* t, const int32_t* degenerate,
                        int P, int H, int W, double fx, double fy, double cx, double cy, float* rho, float* weight,
                        gfl_stream_t stream);
int gfl_sfm_median(const float* a, const float* b, const float* wa, const float* wb, float w_min, int M, int H, int W,
                   double* median, int32_t* count, void* workspace, size_t workspace_bytes, gfl_stream_t stream);
int gfl_sfm_fuse(const float* rho_f, const float* w_f, const float* rho_b, const float* w_b, const double* scale_f,
                 const double* scale_b, int T, int H, int W, float* rho, float* weight, gfl_stream_t stream);
int gfl_sfm_fill(const float* rho0, const float* weight, const double* lambda, int T, int H, int W, int sweeps, float rho_min,
                 float* depth, void* workspace, size_t workspace_bytes, gfl_stream_t stream);

/* sizeof(gfl_fit_state), sizeof(gfl_fit_hyper): lets an FFI binding verify its struct mirrors */
int gfl_abi_sizes(int* sizeof_fit_state, int* sizeof_fit_hyper);

#define GFL_PROFILE_STAGES 9
int gfl_profile_enable(unsigned stage_mask);
int gfl_profile_read(double* total_ms, int* counts, int n_stages);

#ifdef __cplusplus
}
#endif
#endif /* GFLOW_HIP_H */
