/* lrf.h -- C ABI of the MI355X-native localrf render path (liblrf_hip.so).
 *
 * The reference (facebookresearch/localrf) has no FFI layer: its hot path is a chain of
 * ATen ops behind two Python call signatures.  This header is the boundary a maintainer
 * binds instead (ctypes stub in INTEGRATION.md).  Each entry point names the reference
 * lines (relative to /root/reference/localTensoRF) whose work it replaces.
 *
 * Conventions: every pointer is a DEVICE pointer to contiguous fp32 (unless typed
 * otherwise) on the current HIP device; `stream` is a hipStream_t passed as void*;
 * no allocation, no host synchronisation and no ownership transfer inside the library;
 * all calls are asynchronous on `stream` and re-entrant per stream (the test hooks of
 * include/lrf_debug.h are process-wide switches and are NOT part of this contract).
 * Return 0 on success, non-zero on error with a message available from lrf_last_error().
 * lrf_render_fwd, lrf_render_fwd_train, lrf_render_bwd and lrf_scene_fwd check all their
 * arguments first: a refused call enqueues nothing on any stream.  A HIP error after the
 * arguments are accepted (a failed launch, say) can still leave a partial sequence enqueued.
 */
#ifndef LRF_H_
#define LRF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRF_ABI_VERSION 7      /* 7: lrf_density_l1_bwd_acc, LrfGrads.zero_base / zero_floats; 6: lrf_batch_gather, lrf_loss_combine_*, lrf_adam_step_pack; 5: lrf_scene_fwd takes a scene workspace (fused multi-field launches), LRF_FLAG_PLANE_EVENTS, lrf_render_bwd_wait buckets 3 / 4, lrf_adam_step_dev, lrf_photo_loss_*, lrf_rows_gather*; 4: lrf_z_schedule, training rows = feat + gradient row only (ACT_LD 32), network configuration in LrfParams / LrfField, lrf_workspace_bytes_bwd_cfg; 3: lrf_render_bwd_wait, unknown flag bits rejected */
#define LRF_MAX_S 4096         /* samples per ray accepted by lrf_render_fwd */
#define LRF_MAX_S_TRAIN 2048   /* ... by lrf_render_fwd_train / lrf_render_bwd (16 B of LDS per sample and ray) */

/* Fixed shape of the VM field this build is specialised for (opt.py:117-119,155-157:
 * n_lamb_sigma=[8,8,8], n_lamb_sh=[24,24,24], data_dim_color=27, featureC=128). */
#define LRF_CD 8      /* density components per plane  */
#define LRF_CA 24     /* appearance components per plane */
#define LRF_APP_DIM 27
#define LRF_FEATC 128

/* flags for lrf_render_fwd / lrf_render_bwd */
#define LRF_FLAG_WHITE_BG   1u   /* tensorBase.py:633-634 */
#define LRF_FLAG_RELU_DENS  2u   /* fea2denseAct == "relu" (tensorBase.py:498-499) */
#define LRF_FLAG_MLP_VALU   4u   /* debug engine: colour MLP on the vector ALU, natural-layout weights */
#define LRF_FLAG_MLP_F32    8u   /* colour MLP on exact-fp32 MFMA (16x16x4 f32) instead of the default
                                    split-bf16 (hi+lo, 3-term) chain on v_mfma_f32_32x32x16_bf16 (k_shade3) */
#define LRF_FLAG_ROWS_SAVED 16u  /* lrf_render_bwd only: the workspace was filled by lrf_render_fwd_train */
#define LRF_FLAG_SORT_RAYS  32u  /* render the batch in direction-sorted order (cube face + Morton key of d / |d|, one small launch):
                                    rays that march through the same texels run on the same XCD at the same time.  Results are
                                    per-ray and do not depend on the order (bit-identical); ignored for R > 32768.  The same value
                                    must be passed to lrf_render_fwd_train and the lrf_render_bwd that follows it. */
#define LRF_FLAG_PE_OFF     64u  /* fea_pe > 0 only: zeros in place of the feature encodings (MLPRender_Fea_late_view.forward with
                                  * refine == False, tensorBase.py:118-126) */
#define LRF_FLAG_PLANE_EVENTS 128u /* lrf_render_bwd only (data parallel): the appearance scatter runs as one pass per plane and records an
                                  * event behind planes 0 and 1 (lrf_render_bwd_wait buckets 3 / 4), so that the all-reduce of a plane's
                                  * gradient overlaps the scatter of the next one.  Same gradients. */
#define LRF_FLAG_DETERMINISTIC 256u /* lrf_render_bwd only (the forward entry points accept and ignore it): bit-reproducible gradients.
                                  * With the same inputs every gradient (the 19 parameter tensors and d/d rays) has the same bits from
                                  * run to run, whatever the partition of the scatter, the order the binning leaves its entries in, the
                                  * stream layout (two streams or one, captured) and LRF_FLAG_PLANE_EVENTS.  The plane / line gradients
                                  * are summed in 64-bit fixed point (one scale per tensor group and plane from the batch's largest
                                  * contribution: a quantum of about 2^-39 of it at 300^3, far below fp32's own rounding of each product)
                                  * into an int64 image in the workspace (lrf_workspace_bytes_bwd_cfg grows by 8 bytes per gradient
                                  * element of the planes and lines when this bit is set: 69 MB at 300^3), converted once into the
                                  * caller's gradients; the results lie within ~1e-6 of each tensor's maximum of the default mode's.
                                  * Cost: the clear and the conversion of the image and integer run sums in the scatter.
                                  * Refused (non-zero return): the generic engine (a non-default network, LRF_FLAG_MLP_VALU) and appearance
                                  * lines longer than 640 cells. */
#define LRF_FLAG_ALL        511u /* any other bit is an error (a caller built against another ABI version) */

/* Parameters of one TensorVMSplit field as the reference stores them (state-dict layout,
 * models/tensoRF.py:18-50, models/tensorBase.py:97-113).  Plane p is [1,C,H_p,W_p] with
 * W_p = gridSize[matMode[p][0]], H_p = gridSize[matMode[p][1]]; line p is [1,C,L_p,1]
 * with L_p = gridSize[vecMode[p]]. */
typedef struct LrfParams {
  const float* density_plane[3];
  const float* density_line[3];
  const float* app_plane[3];
  const float* app_line[3];
  const float* basis;      /* basis_mat.weight          [27,72]   */
  const float* w1;         /* renderModule.mlp.0.weight [128,27]  */
  const float* b1;         /* renderModule.mlp.0.bias   [128]     */
  const float* w2;         /* renderModule.mlp.2.weight [128,128] */
  const float* b2;         /* renderModule.mlp.2.bias   [128]     */
  const float* w3;         /* renderModule.mlp_view.0.weight [3,131] */
  const float* b3;         /* renderModule.mlp_view.0.bias   [3]     */
  int32_t grid[3];         /* gridSize (x,y,z) */
  /* MLPRender_Fea_late_view configuration (tensorBase.py:97-113).  0 / 0 / 128 (opt.py:148-157, what train.py runs) takes the
   * fast kernels and the shapes above; anything else the generic fp32 engine (csrc/lrf_generic.inl), with
   * w1 [feature_c, 27 (1 + 2 fea_pe)], w2 [feature_c, feature_c], w3 [3, feature_c + 3 (1 + 2 view_pe)].
   * fea_pe, view_pe <= 6, feature_c <= 256; feature_c == 0 is read as 128. */
  int32_t fea_pe, view_pe, feature_c;
} LrfParams;

/* Derived, kernel-friendly image of a field ("layout cache").  Built by lrf_pack_field
 * into caller-owned memory of lrf_cache_bytes() bytes; must be rebuilt whenever a
 * parameter changes (optimizer step, upsample_volume_grid models/tensoRF.py:224-233). */
typedef struct LrfField {
  const void*  cache;      /* device buffer written by lrf_pack_field */
  const float* alpha_vol;  /* AlphaGridMask.alpha_volume [Z,Y,X] or NULL (tensorBase.py:36-58) */
  int32_t alpha_dim[3];    /* X,Y,Z of alpha_vol */
  float   alpha_aabb[6];   /* AlphaGridMask.aabb */
  float   aabb[6];         /* field aabb (min xyz, max xyz) */
  int32_t grid[3];
  float   density_shift;   /* tensorBase.py:497 */
  float   distance_scale;  /* tensorBase.py:610 */
  float   weight_thres;    /* rayMarch_weight_thres, tensorBase.py:622 */
  float   term_T;          /* early termination of the march: once the transmittance entering a 64-sample
                            * chunk is below term_T the remaining density lookups are skipped and those
                            * samples count as empty (the forced last sample takes the rest).  No sample
                            * behind that point can pass weight_thres; sum(w z) moves by <= term_T * z_max.
                            * 0 = off (the reference evaluates every sample, tensorBase.py:600-610). */
  /* natural-layout MLP weights (the parameter tensors themselves): read by the generic engine -- any configuration other
   * than fea_pe = view_pe = 0, feature_c = 128, and the LRF_FLAG_MLP_VALU debug engine of that one */
  const float* basis; const float* w1; const float* b1;
  const float* w2; const float* b2; const float* w3; const float* b3;
  int32_t fea_pe, view_pe, feature_c;   /* as in LrfParams */
} LrfField;

/* Gradients wrt the reference's parameters, in the reference's (state-dict) layout.
 * Accumulated into (+=); the caller zeroes them -- or (ABI 7) names ONE range that holds all of them (the flat gradient
 * buffer of localrf_amd: parameters' gradients and d/d rays) and lrf_render_bwd clears it with the launch that clears its own
 * bins: zero_base (16-byte aligned) / zero_floats (a multiple of 4), NULL / 0 = the caller cleared. */
typedef struct LrfGrads {
  float* density_plane[3];
  float* density_line[3];
  float* app_plane[3];
  float* app_line[3];
  float* basis; float* w1; float* b1; float* w2; float* b2; float* w3; float* b3;
  float* zero_base; int64_t zero_floats;
} LrfGrads;

int         lrf_abi_version(void);
const char* lrf_last_error(void);
char*       lrf_error_slot(void);                   /* internal: the calling thread's 512-byte error text */

/* Bytes of the layout cache for a grid (x,y,z). */
size_t lrf_cache_bytes(const int32_t grid[3]);

/* NCHW params -> channel-last planes/lines + MFMA-fragment-ordered MLP image. */
int lrf_pack_field(const LrfParams* p, void* cache, void* stream);

/* Bytes of scratch lrf_render_fwd / lrf_render_bwd need for R rays x S samples. */
size_t lrf_workspace_bytes(int32_t R, int32_t S);

/* TensorBase.forward (tensorBase.py:567-636) for one field, z schedule supplied
 * (tensorBase.py:419-437 is ray-independent, so the host draws the jitter and keeps RNG
 * parity).  rays [R,6] = (origin, un-normalised direction); z [S].
 * Outputs rgb [R,3], depth [R].  Optional debug outputs (may be NULL): weight_out [R,S]
 * (post floater filter, tensorBase.py:612/620), acc_out [R]. */
int lrf_render_fwd(const LrfField* f, const float* rays, const float* z,
                   int32_t R, int32_t S, uint32_t flags, float floater_thresh,
                   float* rgb, float* depth, float* weight_out, float* acc_out,
                   void* workspace, void* stream);

/* Measurement variant of lrf_render_fwd (bench.py only): brackets each kernel with HIP
 * events on `stream`, SYNCHRONISES, and returns ms_out[6] (host) = {march, shade, finalize,
 * total, 0, 0} plus the number of shaded samples (sum over rays of weight > thres).  The default engine has
 * no separate finalize launch (0). */
int lrf_render_fwd_profile(const LrfField* f, const float* rays, const float* z,
                           int32_t R, int32_t S, uint32_t flags, float floater_thresh,
                           float* rgb, float* depth, void* workspace, void* stream,
                           float* ms_out, int32_t* n_shaded_out);

/* Bytes of scratch lrf_render_bwd needs (worst case: every sample shaded).  _cfg: for a network configuration other than
 * the default one (the generic engine keeps the weight-gradient operands as rows: ~ (4 feature_c + in1 + in_view) floats
 * per shaded sample more -- also for the default configuration when `flags` carries LRF_FLAG_MLP_VALU: the backward then runs the
 * generic fp32 engine too, an exact-fp32 training path); lrf_workspace_bytes_bwd = _cfg(..., 0, 0, 128, 0). */
size_t lrf_workspace_bytes_bwd(int32_t R, int32_t S, const int32_t grid[3]);
size_t lrf_workspace_bytes_bwd_cfg(int32_t R, int32_t S, const int32_t grid[3], int32_t fea_pe, int32_t view_pe, int32_t feature_c, uint32_t flags);

/* Training forward: same outputs as lrf_render_fwd (split-bf16 engine, floater_thresh 0), but the
 * per-sample state the backward needs (density features, shaded-sample lists, per-sample colours,
 * activation rows) is left in `workspace` (lrf_workspace_bytes_bwd bytes) instead of being
 * recomputed by lrf_render_bwd: pass the SAME workspace, field, rays and z to lrf_render_bwd with
 * LRF_FLAG_ROWS_SAVED set.  Memory: a 1.5 GB worst-case reservation at 4096 x 512 (0.6 GB touched when 35 % of the samples are shaded) against 288 GB of HBM. */
int lrf_render_fwd_train(const LrfField* f, const float* rays, const float* z, int32_t R, int32_t S,
                         uint32_t flags, float* rgb, float* depth, void* workspace, void* stream);

/* Backward of lrf_render_fwd (replaces autograd through tensorBase.py:567-636,
 * tensoRF.py:112-196): recomputes the forward (unless LRF_FLAG_ROWS_SAVED), scatters parameter gradients into `g`
 * (reference layout, +=) and writes d(loss)/d(rays) [R,6]. The floater filter is eval-only
 * (train.py:107,139) and not differentiated. `workspace`: lrf_workspace_bytes_bwd bytes. */
int lrf_render_bwd(const LrfField* f, const LrfParams* p, const float* rays, const float* z,
                   int32_t R, int32_t S, uint32_t flags,
                   const float* g_rgb, const float* g_depth,
                   const LrfGrads* g, float* g_rays,
                   void* workspace, void* stream);

/* Data-parallel hand-off (no reference counterpart): makes `stream` wait until one bucket of the gradients
 * of the most recent lrf_render_bwd enqueued on the current device is final, so that a collective over that bucket can
 * start while the rest of the backward still runs.  bucket 0: density planes + lines (the per-ray branch finishes
 * early), 1: colour network (basis, mlp, mlp_view), 2: appearance planes + lines (= everything), 3 / 4: appearance plane 0 / 1
 * alone (behind their own scatter pass when the backward ran with LRF_FLAG_PLANE_EVENTS; otherwise the same point as 2).
 * Error if no lrf_render_bwd ran on this device. */
int lrf_render_bwd_wait(int32_t bucket, void* stream);

/* Debug / parity diagnostics: byte offsets inside the training workspace of {activation rows, gradient rows,
 * rowinfo (row -> ray*S+k or ~0), toff}, the row strides {ACT_LD, GRD_LD} in floats, the byte offset of the ReLU mask
 * bits the training forward saved ([tile][layer 1, 2][lane s + 16 g] dwords: bit 4 t + r = unit 16 t + 4 g + r of the
 * tile's sample s), the byte offset of the slot -> ray permutation of LRF_FLAG_SORT_RAYS (int32 [R]; rowinfo and the feature
 * buffer are indexed by SLOT when the batch was sorted), then the byte offset of the density-feature buffer [R,S] (-inf = sample not evaluated: masked,
 * last, or behind an early termination; overwritten with d(loss)/d(feature) by lrf_render_bwd).  Rows are
 * indexed tile*16 + lane; rowinfo is valid after lrf_render_bwd of the same workspace. */
void lrf_workspace_layout_bwd(int32_t R, int32_t S, const int32_t grid[3], uint64_t out[9]);

/* Pieces of the path exposed on their own (unit parity tests; also used by
 * TensorVMSplit.compute_densityfeature / compute_appfeature / compute_alpha):
 * u [P,3] are normalised coordinates in [-1,1] (tensorBase.py:342-345). */
int lrf_density_feature(const LrfField* f, const float* u, int32_t P, float* sigma_feature, void* stream); /* tensoRF.py:112-151 */
int lrf_app_feature(const LrfField* f, const float* u, int32_t P, float* app_features /*[P,27]*/, void* stream); /* tensoRF.py:153-196 */

/* TensorBase.sample_ray (tensorBase.py:396-417): AABB march named by BASELINE.json's
 * north_star (not on train.py's path).  jitter [R] or NULL.  Outputs pts [R,N,3],
 * t [R,N], inside [R,N] (uint8). */
int lrf_sample_ray_aabb(const float* rays, const float aabb[6], float step_size, float near_, float far_,
                        const float* jitter, int32_t R, int32_t N,
                        float* pts, float* t, uint8_t* inside, void* stream);

/* The sample distances of TensorBase.sample_ray_contracted (tensorBase.py:419-437) for N_samples = 6 h: z [2 h] on the
 * device, the first half linear in [0, 1), the second inverse-depth out to 1e3, + 0.1.  u1, u2 [h]: the two jitter draws
 * of train mode (torch.rand_like, in the reference's order), both NULL in eval mode. */
int lrf_z_schedule(int32_t h, const float* u1, const float* u2, float* z, void* stream);

/* TensorBase.sample_ray_contracted (tensorBase.py:419-443): pts [R,S,3] = contract(o + d z) for a caller-supplied
 * schedule z [S] (the second return value of the reference's method; its third is all-true).  rays_o, rays_d [R,3]. */
int lrf_sample_ray_contracted(const float* rays_o, const float* rays_d, const float* z, int32_t R, int32_t S,
                              float* pts, void* stream);

/* Scene-level ends of the path: LocalTensorfs.forward (local_tensorfs.py:382-499).
 * View of ray r is r / per_view (repeat_interleave at local_tensorfs.py:437); R % per_view == 0.
 *
 * lrf_scene_rays: ids2pixel (local_tensorfs.py:23-29) + get_ray_directions_lean / _360
 * (utils/ray_utils.py:14-37) + cam2rf = cam2world (+) world2rf (local_tensorfs.py:427-431) +
 * get_rays_lean (utils/ray_utils.py:39-54), for n_rf fields in one launch.
 *   ray_ids [R] int64; cam2world [V,3,4]; world2rf [n_rf,3]; focal [1], center [2] device
 *   scalars (NULL when fov360); outputs rays [n_rf,R,6], directions [R,3], ij [R,2] int64. */
int lrf_scene_rays(const int64_t* ray_ids, int32_t R, int32_t per_view, const float* cam2world,
                   const float* world2rf, int32_t n_rf, const float* focal, const float* center,
                   int32_t W, int32_t H, int32_t fov360, float* rays, float* directions, int64_t* ij,
                   void* stream);
/* Gradients autograd derives for the above: g_cam2world [V,3,4]; g_intr [V,3] per-view partial
 * sums of (d focal, d center_x, d center_y); g_world2rf [V,n_rf,3] per-view partial sums.
 * g_directions [R,3] may be NULL. */
int lrf_scene_rays_bwd(const int64_t* ray_ids, int32_t R, int32_t per_view, const float* cam2world,
                       int32_t n_rf, const float* focal, const float* center, int32_t W, int32_t H,
                       int32_t fov360, const float* g_rays, const float* g_directions,
                       float* g_cam2world, float* g_intr, float* g_world2rf, void* stream);
/* lrf_scene_blend: rgbs = clamp(E_v (sum_k w[v,k] rgb_k), 0, 1), depth = sum_k w[v,k] depth_k
 * (local_tensorfs.py:468-474,481-499).  rgb_f [n_rf,R,3], depth_f [n_rf,R], blend_w [V,n_rf],
 * exposure [V,3,3] or NULL; pre [R,3] (blended colour before exposure, kept for the backward
 * pass) may be NULL. */
int lrf_scene_blend(const float* rgb_f, const float* depth_f, const float* blend_w, const float* exposure,
                    int32_t R, int32_t per_view, int32_t n_rf, float* rgbs, float* depth, float* pre,
                    void* stream);
/* g_depth and g_exposure [V,3,3] may be NULL. */
int lrf_scene_blend_bwd(const float* g_rgbs, const float* g_depth, const float* pre, const float* blend_w,
                        const float* exposure, int32_t R, int32_t per_view, int32_t n_rf,
                        float* g_rgb_f, float* g_depth_f, float* g_exposure, void* stream);

/* LocalTensorfs.forward without a tape (local_tensorfs.py:397-499) in one call: lrf_scene_rays, then for every chunk of
 * `chunk` rays (<= 0: all at once) lrf_render_fwd of every active field in the reference's order (:440-474), then
 * lrf_scene_blend.  `fields` is a HOST array of n_rf entries; each field brings its own z schedule (S depends on the
 * field's grid, tensorBase.py:252-262), engine flags and workspace (lrf_workspace_bytes(min(chunk, R), S) bytes; fields
 * may share one, the launches are serialised on `stream`).  Scratch supplied by the caller: rays [n_rf,R,6],
 * rgb_f [n_rf,R,3], depth_f [n_rf,R].  Outputs as lrf_scene_rays / lrf_scene_blend.
 * scene_workspace (may be NULL; lrf_workspace_bytes(min(n_rf, 4) * min(chunk, R), S) bytes): with it, groups of up to four fields
 * of one shape (same grid, S, flags, thresholds; default colour engine) render each chunk in ONE march and ONE colour launch over
 * their field-major rays when chunk % 16 == 0 and floater_thresh == 0 (a ragged last chunk goes field by field) -- the same
 * per-ray arithmetic (depths bit-identical, colours to an ulp); otherwise field by field. */
#define LRF_SCENE_MAX_FIELDS 64
typedef struct LrfSceneField {
  const LrfField* field;
  const float*    z;          /* [S] device */
  int32_t         S;
  uint32_t        flags;      /* LRF_FLAG_* of lrf_render_fwd */
  void*           workspace;
} LrfSceneField;
int lrf_scene_fwd(const int64_t* ray_ids, int32_t R, int32_t per_view, const float* cam2world, const float* world2rf,
                  int32_t n_rf, const float* focal, const float* center, int32_t W, int32_t H, int32_t fov360,
                  const LrfSceneField* fields, float floater_thresh, int32_t chunk,
                  const float* blend_w, const float* exposure,
                  float* rays, float* rgb_f, float* depth_f, float* directions, int64_t* ij,
                  float* rgbs, float* depth, void* scene_workspace, size_t scene_workspace_bytes, void* stream);

/* Optimiser step after the path: torch.optim.Adam with the reference's settings
 * (local_tensorfs.py:88-97,146,245; no weight decay, no amsgrad) over up to LRF_ADAM_MAX tensors in
 * one launch.  p, m (exp_avg), v (exp_avg_sq) are updated in place; step_size = lr / (1 - beta1^t)
 * and bc2_sqrt = sqrt(1 - beta2^t) are evaluated by the caller in double, as torch does. */
#define LRF_ADAM_MAX 64
typedef struct LrfAdamTensor {
  float* p; const float* g; float* m; float* v;
  int64_t n;
  float step_size, bc2_sqrt;
} LrfAdamTensor;
int lrf_adam_step(const LrfAdamTensor* tensors /* host array */, int32_t count, float beta1, float beta2,
                  float eps, void* stream);
/* The same launch with step_size / bc2_sqrt read from DEVICE memory when the kernel runs (dev_scalars [count][2]; the two
 * fields of the host structs are ignored): the launch can be captured in a hipGraph and replayed with the learning rates and
 * bias corrections the host wrote before each replay.  bc2_sqrt <= 0 skips a tensor (torch.optim.Adam skips a parameter
 * whose .grad is None: local_tensorfs.py:229-243 steps the poses of sampled views only). */
int lrf_adam_step_dev(const LrfAdamTensor* tensors /* host array */, int32_t count, const float* dev_scalars, float beta1, float beta2,
                      float eps, void* stream);

/* The optimiser step FUSED with the layout refresh (local_tensorfs.py:146,245 step the field's optimiser, and
 * the next forward re-reads every parameter to rebuild the channel-last cache): the same update as lrf_adam_step /
 * lrf_adam_step_dev (dev_scalars NULL: the host fields of the structs) for the tensors of the table, and behind it `cache` --
 * the layout cache of the field whose parameters `p` names (lrf_cache_bytes, as lrf_pack_field fills it) -- holds the NEW
 * values: the field's twelve plane / line tensors are stepped and written channel-last by one kernel (tensors of `p` that
 * are not in the table are only repacked), the other tensors of the table by the table kernel, then the colour network's
 * images are rebuilt.  Equivalent to lrf_adam_step[_dev] followed by lrf_pack_field. */
int lrf_adam_step_pack(const LrfAdamTensor* tensors /* host array */, int32_t count, const float* dev_scalars /* or NULL */,
                       float beta1, float beta2, float eps, const LrfParams* p, void* cache, void* stream);

/* density_L1 regulariser (tensoRF.py:83-92), on by default while
 * rf_iter < n_iters_reg (opt.py:111, local_tensorfs.py:361-375):
 *   out = mean_i sqrt(max(feature2density(sum_p sum_c plane_p[c, i / L_p] line_p[c, i % L_p]), 1e-5))
 * over the g0*g1*g2 lattice, with the reference's per-plane flattening orders.  plane[p]: the
 * density plane [8, hw[p]] (the [1,8,H,W] parameter), line[p]: [8, ll[p]]; hw[p]*ll[p] is the
 * same for all p.  The forward leaves d out_i / d feat_i in the workspace for the backward. */
size_t lrf_density_l1_workspace(const int32_t hw[3], const int32_t ll[3]);
int lrf_density_l1_fwd(const float* const plane[3], const float* const line[3], const int32_t hw[3],
                       const int32_t ll[3], float density_shift, int32_t relu, void* workspace,
                       float* out /* device [1] */, void* stream);
int lrf_density_l1_bwd(const float* const plane[3], const float* const line[3], const int32_t hw[3],
                       const int32_t ll[3], const void* workspace, const float* g_out /* device [1] */,
                       float* const g_plane[3], float* const g_line[3], void* stream);
/* The same, ADDED to what g_plane / g_line hold (every element has one writer; stream order behind whoever filled them): the
 * regulariser's gradient lands in the buffers lrf_render_bwd scattered into -- one autograd node for render + regulariser,
 * no gradient-accumulation passes over the six density tensors between them (TensorVMSplit.fuse_density_L1). */
int lrf_density_l1_bwd_acc(const float* const plane[3], const float* const line[3], const int32_t hw[3],
                           const int32_t ll[3], const void* workspace, const float* g_out /* device [1] */,
                           float* const g_plane[3], float* const g_line[3], void* stream);

/* Pose assembly: LocalTensorfs.get_cam2world (local_tensorfs.py:292-299) with sixD_to_mtx
 * (utils/utils.py:381-388): per frame a 6D rotation [3,2] (Gram-Schmidt -> columns b1, b2, b1 x b2)
 * and a translation [3] -> cam2world [V,3,4].  r6d / trans are HOST arrays of V device pointers (the
 * per-frame parameters are separate tensors), 1 <= V <= LRF_POSE_MAX per call. */
#define LRF_POSE_MAX 64
/* cross_views != 0 (V == 3 only): b3 is the cross product over the VIEW axis, which is what the
 * reference's dim-less torch.cross (utils/utils.py:386) computes for a stack of exactly 3 views. */
int lrf_pose_assemble(const float* const* r6d, const float* const* trans, int32_t V, int32_t cross_views,
                      float* cam2world, void* stream);
/* g_cam2world [V,3,4] -> g_r6d [V,3,2], g_trans [V,3] */
int lrf_pose_assemble_bwd(const float* const* r6d, int32_t V, int32_t cross_views, const float* g_cam2world,
                          float* g_r6d, float* g_trans, void* stream);

/* Alpha-mask rebuild on the device: TensorBase.getDenseAlpha + updateAlphaMask
 * (tensorBase.py:501-536) as two launches, no host synchronisation.
 * lrf_dense_alpha: alpha = 1 - exp(-sigma * length) at every point of the gx x gy x gz lattice spanning the
 * field aabb (lin_* = device arrays torch.linspace(0, 1, g), as :504-508), through the field's CURRENT mask
 * when it has one (compute_alpha, :538-558); output [gz][gy][gx], the order :523 transposes to.
 * lrf_alpha_pool_threshold: clamp(0,1), 3x3x3 max-pool (stride 1, padding 1), out = pooled >= thres ? 1 : 0. */
int lrf_dense_alpha(const LrfField* f, const float* lin_x, const float* lin_y, const float* lin_z,
                    int32_t gx, int32_t gy, int32_t gz, float length, uint32_t flags, float* alpha, void* stream);
int lrf_alpha_pool_threshold(const float* alpha, int32_t gx, int32_t gy, int32_t gz, float thres, float* out,
                             void* stream);

/* TV regulariser (utils/utils.py:293-309 as applied by tensoRF.py:94-110; weights 0 by default,
 * opt.py:112-113): loss = sum_t scale_t * 2 w (sum_h (dx)^2 / (C (H-1) W) + sum_w (dx)^2 / (C H (W-1)))
 * over up to LRF_TV_MAX tensors x_t [C,H,W] (a line is [C,L,1]); scale 1e-2 for planes, 1e-3 for
 * lines.  `segs` is a host array; g (gradient, same shape, written not accumulated) is used by _bwd. */
#define LRF_TV_MAX 16
typedef struct LrfTvSeg { const float* x; float* g; int32_t C, H, W; float scale; } LrfTvSeg;
size_t lrf_tv_workspace(const LrfTvSeg* segs, int32_t count);
int lrf_tv_loss_fwd(const LrfTvSeg* segs, int32_t count, float weight, void* workspace, float* out /* device [1] */,
                    void* stream);
int lrf_tv_loss_bwd(const LrfTvSeg* segs, int32_t count, float weight, const float* g_out /* device [1] */,
                    void* stream);

/* ---- grid upsample and the geometric losses around the path ------------------------------
 * lrf_upsample_bilinear: TensorVMSplit.up_sampling_VM (models/tensoRF.py:198-221) = F.interpolate(mode="bilinear",
 * align_corners=True) of one plane [C,H,W] -> [C,H2,W2] (a line is [C,L,1] -> [C,L2,1]). */
int lrf_upsample_bilinear(const float* src, int32_t C, int32_t H, int32_t W, float* dst, int32_t H2, int32_t W2, void* stream);

/* Optical-flow loss of train.py:385-412 with utils/utils.py:15-48 (pts2px, inverse_pose, get_cam2cams,
 * get_pred_flow).  V views of n rays each (rays of a view contiguous, as LocalTensorfs.forward returns them):
 * arr[v][j] = sum|pred_bwd - bwd_flow| * bwd_mask + sum|pred_fwd - fwd_flow| * fwd_mask (fwd_mask counts as 0 for the
 * views flagged in fwd_off: train.py:396 flags `view_ids == len(cam2world) - 1`, absolute id against slice length),
 * entries above the view's `quantile` (0.9) zeroed (train.py:408).
 * fwd: arr_out [V*n] (after zeroing), view_sum [V] (sum of a view's kept entries; flow_loss_arr.mean() =
 * sum(view_sum) / (V n)).  bwd: gradients of scale * g_loss[0] * sum(arr) with respect to depth [V*n], dirs [V*n,3],
 * cam2world [F,3,4] and (focal, cx, cy) per view [V,3]; workspace = V * 36 floats. */
#define LRF_LOSS_MAX_PER_VIEW 4096
typedef struct LrfFlowLoss {
  const float* cam2world;   /* [F,3,4]: LocalTensorfs.get_cam2world(starting_id) */
  const int32_t* frame;     /* [V]: view id - starting frame id */
  const int32_t* fwd_off;   /* [V]: != 0 -> this view's forward mask is zeroed (train.py:396) */
  const float* dirs;        /* [V*n,3] */
  const float* depth;       /* [V*n] */
  const int64_t* ij;        /* [V*n,2] (col, row) */
  const float* fwd_flow; const float* fwd_mask; const float* bwd_flow; const float* bwd_mask;   /* [V*n,2], [V*n] */
  const float* focal;       /* device [1] */
  const float* center;      /* device [2] */
  int32_t F, V, n;
  float quantile;
} LrfFlowLoss;
int lrf_flow_loss_fwd(const LrfFlowLoss* a, float* arr_out, float* view_sum, void* stream);
int lrf_flow_loss_bwd(const LrfFlowLoss* a, const float* arr_out, const float* g_loss /* device [1] */, float scale,
                      float* g_depth, float* g_dirs, float* g_cam2world, float* g_intr /* [V,3] */, float* workspace,
                      void* stream);
/* Monocular-depth loss of train.py:414-423 with compute_depth_loss (utils/utils.py:50-59) on x = 1 / clamp(depth, 1e-6)
 * and the target inverse depths gt: per view median / mean-abs-deviation normalisation of both, squared difference,
 * entries above the view's `quantile` (0.8) zeroed.  stats [V,6] carries the per-view statistics to the backward. */
int lrf_depth_loss_fwd(const float* depth, const float* gt, int32_t V, int32_t n, float quantile, float* arr_out,
                       float* stats, float* view_sum, void* stream);
int lrf_depth_loss_bwd(const float* depth, const float* gt, int32_t V, int32_t n, const float* arr_out, const float* stats,
                       const float* g_loss /* device [1] */, float scale, float* g_depth, void* stream);

/* Photometric loss of train.py:369-371: loss = mean over [R,3] of 0.25 |rgb - target| w_i / mean(w), one launch each way.
 * w [R] or NULL (unit weights); w_mean: device [1] or NULL (= the mean of w over this batch; under ray sharding the batch-global
 * mean).  loss, aux: device [1] each; aux carries 0.25 / (mean(w) 3 R) to the backward.  g_rgb [R,3] = g_loss[0] d loss / d rgb. */
int lrf_photo_loss_fwd(const float* rgb, const float* target, const float* w, const float* w_mean, int32_t R, float* loss, float* aux, void* stream);
int lrf_photo_loss_bwd(const float* rgb, const float* target, const float* w, const float* aux, const float* g_loss /* device [1] */,
                       int32_t R, float* g_rgb, void* stream);

/* Batch assembly (train.py:352-358, 385-420 index the dataset tensors with the batch's (view, pixel) ids, one ATen gather
 * and one mask expression per tensor): target colours, both optical flows with their masks (forward: the view is not the
 * last image; backward: not the first) and inverse depths of V x n pixels in one launch.  Dataset tensors [n_images, HW, 3 | 2 |
 * 2 | 1] float32, a NULL tensor (or output) is skipped; view_ids int64 [V] (negative ids count from the end); pix int64 [V, n]:
 * pixel ids inside the view. */
typedef struct {
  const float* images; const float* fwd_flow; const float* bwd_flow; const float* invdepths;
  const int64_t* view_ids; const int64_t* pix;
  int32_t V, n, HW, n_images;
} LrfBatchGather;
int lrf_batch_gather(const LrfBatchGather* a, float* target /* [V n, 3] */, float* fwd_flow /* [V n, 2] */, float* fwd_mask /* [V n] */,
                     float* bwd_flow, float* bwd_mask, float* invdepth /* [V n] */, void* stream);

/* Loss assembly (train.py:425-437: loss + flow * w_flow * reg / ((W + H) / 2) + depth * w_depth * reg + L1 ...):
 * total = sum_k w_k sum_j x_k[j] with w_k = a_k + b_k s[0] -- s a device scalar (the schedule weight of the iteration), x_k a
 * device scalar or a vector of n_k partial sums (the per-view sums of lrf_flow_loss_fwd / lrf_depth_loss_fwd, added in index
 * order).  One launch each way instead of a dozen scalar kernels; w_out [count] carries the weights to the backward,
 * g[k] = g_total[0] w_k = d total / d x_k[j]. */
#define LRF_LOSS_TERMS_MAX 8
typedef struct {
  const float* x[LRF_LOSS_TERMS_MAX]; int32_t n[LRF_LOSS_TERMS_MAX];
  float a[LRF_LOSS_TERMS_MAX], b[LRF_LOSS_TERMS_MAX];
  int32_t count; const float* s;
} LrfLossTerms;
int lrf_loss_combine_fwd(const LrfLossTerms* t, float* total /* device [1] */, float* w_out /* device [count] */, void* stream);
int lrf_loss_combine_bwd(const float* w, const float* g_total /* device [1] */, int32_t count, float* g /* device [count] */, void* stream);

/* Row gather out[v,:] = src[idx[v],:] (src [F,K], idx int64 [V], negative ids count from the end) and its backward
 * g_src[f,:] = sum_{v: idx[v]=f} g_out[v,:] in v order (no atomics): the per-view poses / exposures a batch picks out of the per-frame
 * tables (local_tensorfs.py:292-299 stacks the sampled frames' parameters; :496 indexes the stacked exposures). */
int lrf_rows_gather(const float* src, const int64_t* idx, int32_t V, int32_t K, int32_t F, float* out, void* stream);
int lrf_rows_gather_bwd(const float* g_out, const int64_t* idx, int32_t V, int32_t K, int32_t F, float* g_src, void* stream);

/* lrf_image_metrics: test-view image quality of B frame pairs img0 / img1 [B,H,W,3] (contiguous fp32, HWC, the layout of
 * rgb_map.reshape(H, W, 3)) -- the two metrics renderer.render(test=True) computes on the host per frame (renderer.py:162-163):
 *   mse[b]       = mean over all H*W*3 values of (img0 - img1)^2, summed in fp64 (the reference: fp32 torch);
 *   ssim_mean[b] = mean of the SSIM map of utils/utils.py:232-287 (rgb_ssim, the mip-NeRF SSIM);
 *   ssim_map     = that map [B, H-fs+1, W-fs+1, 3] (NULL: not written).
 * SSIM as the reference computes it, in fp64: the separable Gaussian (filter_size taps, filter_sigma, the even-size shift)
 * applied as scipy.signal.convolve2d(mode="valid"), rows' axis first, to x, y, x^2, y^2, xy (squares and product
 * rounded in fp32, as numpy forms them from fp32 arrays); variances clamped at 0, the covariance at sqrt(s00 s11);
 * c1 = (k1 max_val)^2, c2 = (k2 max_val)^2.  NaN inputs give NaN.  Outputs are fp64 device arrays of B entries.
 * No atomics: bit-identical from run to run and independent of B.  Refused before any launch: 1 <= filter_size <= 31 is
 * required, and H, W >= filter_size (the reference would return the NaN of an empty mean).
 * workspace: lrf_image_metrics_workspace_bytes(B, H, W, filter_size) bytes (0 for arguments lrf_image_metrics refuses). */
typedef struct LrfImageMetrics {
  const float* img0;
  const float* img1;
  int32_t B, H, W;
  int32_t filter_size;   /* 1..31 (utils.py default 11) */
  double max_val;        /* 1 for images in [0, 1] (renderer.py:163) */
  double filter_sigma;   /* 1.5 */
  double k1, k2;         /* 0.01, 0.03 */
} LrfImageMetrics;
size_t lrf_image_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t filter_size);
int lrf_image_metrics(const LrfImageMetrics* m, double* ssim_map /* nullable */, double* ssim_mean /* [B] */, double* mse /* [B] */,
                      void* workspace, void* stream);

/* Device frame store: the train split of LocalRFDataset (dataLoader/localrf_dataset.py) as a window of `capacity` frame slots
 * on the device, each frame in separate fp32 planes as the reference stores them (slot s of a plane starts at s * n_px rows):
 *   rgb [capacity, n_px, 3], loss_weight [capacity, n_px], invdepth [capacity, n_px] (NULL: no depth),
 *   fwd_flow / bwd_flow [capacity, n_px, 2] with fwd_mask / bwd_mask [capacity, n_px] (NULL pairs: no flow).
 * slot_of: device int32 [num_images], the slot holding frame v or -1.  status: device uint32 [1], sticky error bits.  The caller
 * rewrites slot_of and status in place with stream-ordered copies: a captured lrf_frames_gather stays valid when the window moves.
 * Every entry point checks the window (positive sizes, the required planes, flow planes paired with their masks) before any launch. */
#define LRF_FRAMES_ERR_NOT_RESIDENT 1u   /* a gathered view lay outside [0, num_images) or had no slot: its rows are NaN */
typedef struct LrfFrameWindow {
  float* rgb; float* loss_weight; float* invdepth;
  float* fwd_flow; float* fwd_mask; float* bwd_flow; float* bwd_mask;
  const int32_t* slot_of;
  uint32_t* status;
  int32_t capacity, n_px, num_images;
} LrfFrameWindow;
/* lrf_frames_gather: the rows sample() returns (localrf_dataset.py:303-313) for V views x n rays in one launch.  view_ids int64 [V],
 * ray_ids int64 [V n]: row r is view view_ids[r / n], pixel ray_ids[r] mod n_px (the reference's global ids view * n_px + pix and
 * per-view pixel ids both work).  Outputs rgbs [V n, 3], loss_weights [V n], invdepths [V n], fwd_flow / bwd_flow [V n, 2],
 * fwd_mask / bwd_mask [V n]; a NULL output is not written.  A view that is not resident gives NaN rows and sets
 * LRF_FRAMES_ERR_NOT_RESIDENT in *status; no trap, no host synchronisation.  Refused: V <= 0, n <= 0, V n >= 2^29, null ids,
 * an output whose plane the window does not hold. */
int lrf_frames_gather(const LrfFrameWindow* w, const int64_t* view_ids, const int64_t* ray_ids, int32_t V, int32_t n,
                      float* rgbs, float* loss_weights, float* invdepths, float* fwd_flow, float* fwd_mask,
                      float* bwd_flow, float* bwd_mask, void* stream);
/* lrf_decode_flow: decode_flow (utils/utils.py:67-71) of an encoded flow image uint16 [H,W,3] (already at the frame's size:
 * the resize stays the caller's) times flow_scale (localrf_dataset.py:193-194) into slot `slot`'s forward (backward = 0) or
 * backward flow plane and mask: flow = (float(e) - 32768) / 256 * float(flow_scale) in fp32 (numpy rounds the Python float to
 * fp32 before the multiply), mask = e[...,2] > 32768.  Refused: H W != n_px, a slot outside the window, no flow planes. */
int lrf_decode_flow(const LrfFrameWindow* w, int32_t slot, int32_t backward, const uint16_t* encoded, int32_t H, int32_t W,
                    double flow_scale, void* stream);
/* lrf_frame_sharpness: the loss weight of localrf_dataset.py:229-235 from slot `slot`'s rgb plane [H,W,3] (already uploaded):
 * grey = OpenCV's 8-bit RGB2GRAY of uint8(trunc(img * 255)) ((4899 R + 9617 G + 1868 B + 8192) >> 14, its documented constants;
 * img * 255 rounded in fp32, values outside [0, 1] clamped), the 3x3 Laplacian of cv2.Laplacian(ksize=1, CV_32F) with
 * BORDER_REFLECT_101, its variance over all pixels (integer sums, exact; one rounding to fp32), times motion_mask (uint8 [n_px],
 * nonzero = 1; NULL = all ones) into the slot's loss_weight plane.  Deterministic (fixed partition, integer partials, no atomics).
 * workspace: lrf_frame_sharpness_workspace_bytes() bytes.  Refused: H W != n_px, n_px > 2^21, a slot outside the window. */
size_t lrf_frame_sharpness_workspace_bytes(void);
int lrf_frame_sharpness(const LrfFrameWindow* w, int32_t slot, int32_t H, int32_t W, const uint8_t* motion_mask,
                        void* workspace, void* stream);

/* lrf_select: exact order statistics of B fp32 rows; row b is x[b * row_stride .. b * row_stride + n_b) (device memory).
 *   LRF_SELECT_QUANTILE: out[b] = np.quantile(row, q) with numpy's default method="linear", bit for bit: q rounded to fp32,
 *     v = fp32(fp32(n - 1) * q), gamma and the two-sided lerp in fp32 as numpy 2.2 forms them (csrc/lrf_select.inl);
 *   LRF_SELECT_MEDIAN: out[b] = torch.median(row), the element of rank floor((n - 1) / 2).
 * A row holding a NaN gives NaN (0x7FC00000); +-inf are ordinary values; -0.0 and +0.0 compare equal and a zero result is
 * +0.0.  Radix select over order-preserving uint32 keys, four 8-bit digit passes plus one min pass: integer atomics only, a
 * fixed launch sequence, no host synchronisation (capturable, bit-reproducible).  n: host array of B row lengths
 * (n_count = B <= LRF_SELECT_MAX_ROWS) or of one length shared by every row (n_count = 1, B <= 65535).  Refused before any
 * launch: a length outside 1 <= n < 2^31, q outside [0, 1], a negative row_stride, null pointers.
 * workspace: lrf_select_workspace_bytes(B, max_n) bytes (0 for shapes lrf_select refuses). */
#define LRF_SELECT_QUANTILE 0
#define LRF_SELECT_MEDIAN 1
#define LRF_SELECT_MAX_ROWS 256
size_t lrf_select_workspace_bytes(int32_t B, int64_t max_n);
int lrf_select(const float* x, int64_t row_stride, const int64_t* n, int32_t n_count, int32_t B, int32_t mode, float q, float* out,
               void* workspace, void* stream);

/* Test-view geometry diagnostics of renderer.render(test=True) (renderer.py:79-124) for V views of H x W pixels.
 * lrf_flow_comparison: per view v (absolute frame index idx[v] in [0, F)) the predicted forward / backward flow of every pixel
 * (utils.py:15-48: neighbours clamp(idx +- 1, 0, F - 1), pts = dirs * depth, pts2px with z clipped at 1e-6, minus float(ij)),
 * written as renderer.py stacks it into fwd_cmp / bwd_cmp [V, 3H, 2W]: column half c = component c; rows 0..H prediction,
 * H..2H dataset flow, 2H..3H |pred - flow| * mask / W.  Rows 0..2H of each half are divided by their np.quantile(., 0.9)
 * (lrf_select; quantiles [V, 4] = fwd c0, fwd c1, bwd c0, bwd c1), then everything is clamped to [0, 1] (NaN stays NaN).
 * fwd_raw / bwd_raw (both or neither): the images before the division and the clamp.
 * Inputs: cam2world [F,3,4], depth [V,HW], dirs [V,HW,3], ij int64 [V,HW,2] (col, row), flows [V,HW,2], masks [V,HW] (0 / 1),
 * focal device [1], center device [2].  Refused before any launch: V outside 1..LRF_EVAL_MAX_VIEWS, an idx outside [0, F),
 * H or W <= 0, 6 H W >= 2^31, null pointers.  workspace: lrf_flow_comparison_workspace_bytes(V, H, W) bytes. */
#define LRF_EVAL_MAX_VIEWS 64
typedef struct LrfFlowComparison {
  const float* cam2world;
  const float* depth; const float* dirs; const int64_t* ij;
  const float* fwd_flow; const float* fwd_mask; const float* bwd_flow; const float* bwd_mask;
  const float* focal; const float* center;
  int32_t F, V, H, W;
  int32_t idx[LRF_EVAL_MAX_VIEWS];
} LrfFlowComparison;
size_t lrf_flow_comparison_workspace_bytes(int32_t V, int32_t H, int32_t W);
int lrf_flow_comparison(const LrfFlowComparison* c, float* fwd_cmp, float* bwd_cmp, float* fwd_raw /* nullable */,
                        float* bwd_raw /* nullable */, float* quantiles, void* workspace, void* stream);
/* lrf_depth_comparison: compute_depth_loss (utils.py:50-59) of x = 1 / clamp(depth, 1e-6) against y = invdepth (both [V, HW])
 * into out [V, 3H, W] = vstack(0.5 x^, 0.5 y^, (x^ - y^)^2) clamped to [0, 1], with ^ = (. - median) / mean|. - median|.
 * stats [V, 4] = (median x, median y, mad x, mad y); medians exact (torch.median), each MAD summed in fp64 in a fixed order
 * and rounded once to fp32 (the reference's fp32 mean differs in the last bits).  Refused: V outside 1..32767, H or W <= 0,
 * 6 H W >= 2^31, null pointers.  workspace: lrf_depth_comparison_workspace_bytes(V, H, W) bytes. */
size_t lrf_depth_comparison_workspace_bytes(int32_t V, int32_t H, int32_t W);
int lrf_depth_comparison(const float* depth, const float* invdepth, int32_t V, int32_t H, int32_t W, float* out, float* stats,
                         void* workspace, void* stream);

/* lrf_encode_frames: the bytes renderer.render(test=False) writes per frame (renderer.py:130-148,172-174), for V frames of
 * H x W pixels: rgb [V,H,W,3] and depth [V,H,W] fp32 (device, 16-byte aligned) ->
 *   rgb8 [V,H,W,3] uint8 = clamp(rint(fp32(255 * x)), 0, 255), ties to even, NaN -> 0 (cv2.imwrite's saturate_cast);
 *     rgb and rgb8 are both null for the depth images alone;
 *   depth_idx [V,H,W] uint8 (nullable) = the index image visualize_depth (utils/utils.py:179-197) passes to
 *     cv2.applyColorMap, in numpy 2.2's fp32 arithmetic: x = nan_to_num(d); uint8(fp32(255 * clip(fp32(x - mi) / D, 0, 1)));
 *   depth8 [V,H,W,3] uint8 = lut[depth_idx], lut a device [256,3] uint8 table whose channel order is kept.
 * fixed_range: host {mi, ma, D} (mi and D already rounded to fp32 as numpy rounds the caller's numbers), or null for the
 * automatic range of visualize_depth(minmax=None), per frame: mi = min(x[x > 0]) (NaN when the frame has no positive value),
 * ma = max(x) (-0.0 read as +0.0), D = fp32(fp32(ma - mi) + 1e-8f).  range_out [V,2] (nullable) receives (mi, ma) per frame.
 * One launch with a fixed range, two with the automatic one (per-workgroup integer extrema of order-preserving keys, reduced
 * in a fixed order: no float atomics, no host synchronisation, bit-reproducible).  Refused before any launch: V < 1,
 * H or W <= 0, 3 V H W >= 2^31, null or misaligned pointers (outputs 4-byte aligned), the automatic range without a
 * workspace of lrf_encode_frames_workspace_bytes(V) bytes (0 for V outside 1..2^24). */
size_t lrf_encode_frames_workspace_bytes(int32_t V);
int lrf_encode_frames(const float* rgb /* nullable */, const float* depth, int32_t V, int32_t H, int32_t W, const uint8_t* lut,
                      const float* fixed_range /* nullable */, uint8_t* rgb8 /* nullable */, uint8_t* depth8, uint8_t* depth_idx /* nullable */,
                      float* range_out /* nullable */, void* workspace, void* stream);

/* lrf_points_fuse: V rendered depth images fused into one filtered, ordered, coloured world-space point list.
 * depth [V,H,W] fp32, rgb8 [V,H,W,3] uint8 (nullable, with rgb8_out), cam2world [V,3,4] fp32, focal device [1] / center
 * device [2] (pinhole; as lrf_scene_rays takes them) or fov360.  Candidates are the pixels (i, j) with i % stride == 0 and
 * j % stride == 0.  A candidate is kept when its depth d is finite, positive and inside [d_min, d_max] and, with n_neigh > 0
 * (pinhole only), when its world point pw = R_v (pixel_dir * d) + t_v, reprojected into the frames v + neigh[k] that exist,
 * agrees with the depth found there (|z - dn| <= rel_tol * dn at the nearest pixel, ties to even) in at least
 * min(min_consistent, offsets in range) of them; csrc/lrf_points.inl states the arithmetic, fp32 without contraction.
 * Kept candidates are written in (frame, row, column) order, the same list on every run: xyz [M,3], rgb8_out [M,3]
 * (nullable), src [M,2] = (frame, pixel id j * W + i).  count (device int64 [1]) receives the true total M; rows at or beyond
 * capacity are not written.  Three launches, no atomics, no host synchronisation.  Refused before any launch: null pointers,
 * V, H, W or stride < 1, V H W >= 2^31, capacity < 0, d_min > d_max (or NaN), n_neigh outside [0, LRF_POINTS_MAX_NEIGH], a zero
 * or repeated offset, rel_tol < 0 (or NaN), min_consistent < 0, a consistency test with fov360, misaligned pointers.
 * workspace: lrf_points_workspace_bytes(V, H, W, stride) bytes (0 for shapes lrf_points_fuse refuses), 8-byte aligned. */
#define LRF_POINTS_MAX_NEIGH 8
typedef struct LrfPointsFuse {
  const float* depth; const uint8_t* rgb8 /* nullable */; const float* cam2world;
  const float* focal; const float* center;
  int32_t V, H, W, fov360, stride;
  float d_min, d_max;
  int32_t n_neigh, neigh[LRF_POINTS_MAX_NEIGH];
  float rel_tol;
  int32_t min_consistent;
} LrfPointsFuse;
size_t lrf_points_workspace_bytes(int32_t V, int32_t H, int32_t W, int32_t stride);
int lrf_points_fuse(const LrfPointsFuse* a, int64_t capacity, float* xyz, uint8_t* rgb8_out /* nullable */, int32_t* src,
                    int64_t* count /* device [1] */, void* workspace, void* stream);

/* Surface normals from the gradient of the density feature (csrc/lrf_normals.inl states the arithmetic, all fp32).
 * lrf_density_gradient: u [P,3] normalised coordinates -> grad_u [P,3] = d density_feature / du, analytic from the taps
 * the value reads (piecewise constant per cell along an axis, 0 along an axis the border clamps), and feat [P] (nullable):
 * the bits lrf_density_feature returns.  P = 0 launches nothing.
 * lrf_render_normals: per ray N = sum over the samples the colour pass shades (w_i > weight_thres) of w_i n_i, with
 * n_i = -grad_x g / max(|grad_x g|, 1e-8) of g(x) = density_feature(u(contract(x))) and w the weights lrf_render_fwd leaves
 * in weight_out (alpha mask, forced last sample and floater filter applied).  N is not normalised, |N| <= acc; a ray
 * without a shaded sample gives exactly (0, 0, 0).  One forward render into the workspace, then one launch without atomics:
 * the same bits on every run.  flags, floater_thresh: as lrf_render_fwd takes them.  blend_w (nullable; [ceil(R / per_view)])
 * scales ray r's N and acc by blend_w[r / per_view]; accumulate = 1 adds to normals / acc instead of overwriting them (a
 * scene sums its fields in field order).  normals [R,3], acc [R] (nullable).  Refused before any launch: null pointers,
 * R <= 0, S outside [2, 4096], unknown flag bits, per_view < 1 with blend_w, accumulate outside {0, 1}, misaligned pointers
 * (workspace: 256 bytes).  workspace: lrf_normals_workspace_bytes(R, S) bytes = the forward's workspace, the [R,S] weights
 * and 5 R floats of per-ray outputs (0 for a refused shape). */
int lrf_density_gradient(const LrfField* f, const float* u /* [P,3] normalised */, int64_t P, float* grad_u /* [P,3] */,
                         float* feat /* [P] or NULL */, void* stream);
size_t lrf_normals_workspace_bytes(int32_t R, int32_t S);
int lrf_render_normals(const LrfField* f, const float* rays, const float* z, int32_t R, int32_t S, uint32_t flags,
                       float floater_thresh, const float* blend_w /* nullable */, int32_t per_view, int32_t accumulate,
                       float* normals /* [R,3] */, float* acc /* [R] or NULL */, void* workspace, void* stream);

/* A TSDF volume and a triangle mesh from it (csrc/lrf_mesh.inl states the arithmetic, fp32 without contraction).
 * A volume is a lattice of Nx x Ny x Nz points at origin + (ix, iy, iz) * voxel, x fastest: tsdf [Nz,Ny,Nx] (starts at 1),
 * weight [Nz,Ny,Nx] (starts at 0), rgb [Nz,Ny,Nx,3] in [0, 1] (nullable, starts at 0).
 * lrf_tsdf_integrate: V pinhole frames (depth [V,H,W], rgb8 [V,H,W,3] uint8 -- nullable, with the volume's rgb --, cam2world
 * [V,3,4], focal device [1], center device [2]) are folded into the volume in frame order, one lane per lattice point, the
 * volume read and written once per call: a point is projected into frame v as lrf_points_fuse's consistency test projects;
 * with dn the depth at the nearest pixel (finite, positive, in [d_min, d_max]), sdf = dn - z; a frame with sdf < -trunc is
 * skipped, else s = min(1, sdf / trunc), tsdf = (tsdf weight + s) / (weight + 1), rgb likewise from rgb8 / 255, weight += 1.
 * No atomics; frames k..V integrated on the state of frames 0..k give the bits of one call.  Refused before the launch: null or
 * misaligned pointers, Nx, Ny or Nz < 1, Nx Ny Nz >= 2^31, voxel <= 0, trunc <= 0 (or NaN), d_min > d_max (or NaN), V, H or
 * W < 1, V H W >= 2^31, rgb without rgb8 or the reverse.
 * lrf_mesh_extract: marching tetrahedra (the Kuhn split, six per cell) of any scalar volume at `level`; a lattice point is
 * inside when value < level; a cell counts when its eight corners have weight >= min_weight (> 0; every cell when weight is
 * null).  An indexed, watertight-by-construction mesh: vertices [Nv,3] on lattice edges in (z, y, x, edge) order, rgb8_out
 * [Nv,3] (nullable, with rgb) the interpolated colour encoded as lrf_encode_frames encodes, faces [Nf,3] int32 in (cell,
 * tetrahedron, triangle) order, wound so that the normal points towards value > level.  counts (device int64 [2]) receives
 * the true (Nv, Nf); rows at or beyond max_vertices / max_faces are not written, and with both 0 nothing is written (a
 * counting call).  Three launches, no atomics, no host synchronisation, the same bytes on every run.  The indices are right
 * while Nv and Nf stay below 2^31.  Refused before any launch: null or misaligned pointers, dims < 1, Nx Ny Nz >= 2^31,
 * voxel <= 0, a NaN level, min_weight <= 0 with weight, capacities outside [0, 2^31), rgb without rgb8_out or the reverse.
 * workspace: lrf_mesh_workspace_bytes(Nx, Ny, Nz) bytes (0 for a refused shape), 4-byte aligned. */
typedef struct LrfTsdfVolume {
  float* tsdf; float* weight; float* rgb /* nullable */;
  int32_t Nx, Ny, Nz;
  float origin[3], voxel, trunc;
} LrfTsdfVolume;
int lrf_tsdf_integrate(const LrfTsdfVolume* vol, const float* depth, const uint8_t* rgb8 /* nullable */, const float* cam2world,
                       const float* focal, const float* center, int32_t V, int32_t H, int32_t W, float d_min, float d_max,
                       void* stream);
typedef struct LrfMeshExtract {
  const float* value; const float* weight /* nullable */; const float* rgb /* nullable */;
  int32_t Nx, Ny, Nz;
  float origin[3], voxel, level, min_weight;
} LrfMeshExtract;
size_t lrf_mesh_workspace_bytes(int32_t Nx, int32_t Ny, int32_t Nz);
int lrf_mesh_extract(const LrfMeshExtract* m, int64_t max_vertices, int64_t max_faces, float* vertices,
                     uint8_t* rgb8_out /* nullable */, int32_t* faces, int64_t* counts /* device [2] */, void* workspace,
                     void* stream);

/* A block-sparse TSDF volume: the dense volume above, of which only the 8 x 8 x 8 blocks that some depth pixel's truncation
 * band reaches are stored (csrc/lrf_tsdf_blocks.inl states the arithmetic, fp32 without contraction).  The virtual lattice
 * has 8Bx x 8By x 8Bz points at origin + (ix, iy, iz) * voxel.  marks uint8 [Bz,By,Bx] (starts at 0), table int32 [Bz,By,Bx]
 * (-1, or the block's pool index; starts at -1), coords int32 [capacity,3] ((bx, by, bz) in pool order), pools tsdf
 * [n_blocks,8,8,8] (a new block starts at 1), weight [n_blocks,8,8,8] (0) and rgb [n_blocks,8,8,8,3] (nullable; 0), x fastest;
 * n_blocks: the blocks the table and the pools hold.  No hash, no atomics, no workgroup waits on another: a block's pool
 * index is a fixed function of the frames and the call sequence, and every run leaves the same bytes.
 * lrf_tsdf_blocks_touch: one lane per depth pixel (finite, positive, in [d_min, d_max]); with a, b the pixel's world points at
 * depths max(d - trunc, 0) and d + trunc and m = voxel + (d + trunc) / focal, marks every block of the grid that meets the box
 * [min(a, b) - m, max(a, b) + m], per axis floor((box - origin) / (8 voxel)) clipped to the grid.  Needs marks; pools unused.
 * lrf_tsdf_blocks_assign: every marked block without a pool index gets the next indices, in block-linear (z, y, x) order, after
 * the n_blocks that exist; count (device int64 [1]) receives the number of such blocks.  When n_blocks + count exceeds
 * max_blocks the table is left as it was.  coords rows below coords_capacity are (re)written for every block of the table.
 * With max_blocks = n_blocks nothing could fit: a counting call of two launches that writes count alone.  The caller counts,
 * reads count back, grows coords and the pools, calls again (three launches) and adds count to n_blocks.  Needs marks;
 * pools unused.  workspace: lrf_tsdf_blocks_assign_workspace_bytes(Bx, By, Bz) bytes (0 for a refused grid).
 * lrf_tsdf_blocks_integrate: lrf_tsdf_integrate over the stored blocks, one workgroup per block, the pools read and written
 * once per call: a stored point ends with the bits lrf_tsdf_integrate gives the same lattice point over the same frames.
 * n_blocks = 0 launches nothing.
 * lrf_mesh_extract_blocks: lrf_mesh_extract of the tsdf pool with the weight pool (min_weight > 0: always gated); a lattice
 * point in no block reads as (tsdf 1, weight 0), so a missing block can leave a hole but never creates or moves a face.
 * Vertices come in pool order, then (z, y, x, edge) inside the block; faces in the pool order of the cell's lowest corner,
 * then (tetrahedron, triangle).  counts, capacities and the counting call as lrf_mesh_extract has them.  workspace:
 * lrf_mesh_extract_blocks_workspace_bytes(n_blocks) bytes (0 for a refused count).
 * Refused before any launch: null or misaligned pointers, Bx, By or Bz < 1, 8 B >= 2^31 on an axis, Bx By Bz >= 2^31, n_blocks
 * < 0 or 512 n_blocks >= 2^31, voxel <= 0, trunc <= 0 (or NaN), d_min > d_max (or NaN), V, H or W < 1, V H W >= 2^31, rgb
 * without rgb8 / rgb8_out or the reverse, a NaN level, min_weight <= 0, capacities outside [0, 2^31). */
typedef struct LrfTsdfBlocks {
  uint8_t* marks; int32_t* table; int32_t* coords;
  float* tsdf; float* weight; float* rgb /* nullable */;
  int32_t Bx, By, Bz, n_blocks;
  float origin[3], voxel, trunc;
} LrfTsdfBlocks;
int lrf_tsdf_blocks_touch(const LrfTsdfBlocks* g, const float* depth, const float* cam2world, const float* focal,
                          const float* center, int32_t V, int32_t H, int32_t W, float d_min, float d_max, void* stream);
size_t lrf_tsdf_blocks_assign_workspace_bytes(int32_t Bx, int32_t By, int32_t Bz);
int lrf_tsdf_blocks_assign(const LrfTsdfBlocks* g, int64_t max_blocks, int64_t coords_capacity, int64_t* count /* device [1] */,
                           void* workspace, void* stream);
int lrf_tsdf_blocks_integrate(const LrfTsdfBlocks* g, const float* depth, const uint8_t* rgb8 /* nullable */,
                              const float* cam2world, const float* focal, const float* center, int32_t V, int32_t H, int32_t W,
                              float d_min, float d_max, void* stream);
size_t lrf_mesh_extract_blocks_workspace_bytes(int32_t n_blocks);
int lrf_mesh_extract_blocks(const LrfTsdfBlocks* g, float level, float min_weight, int64_t max_vertices, int64_t max_faces,
                            float* vertices, uint8_t* rgb8_out /* nullable */, int32_t* faces, int64_t* counts /* device [2] */,
                            void* workspace, void* stream);

/* The connected components of an indexed triangle mesh, and the mesh without its small components (csrc/lrf_mesh_clean.inl
 * states the algorithm).  Integers only: positions and colours are copied bit for bit, and every call leaves the same bytes on
 * every run.  A mesh is vertices [Nv,3] fp32, rgb8 [Nv,3] uint8 (nullable), faces [Nf,3] int32 (null allowed when Nf = 0).  Two
 * vertices are connected when a face holds both; the label of a vertex is the smallest vertex index of its component; a vertex
 * that no face holds is a component of its own with 0 faces.
 * lrf_mesh_components_init: parent[v] = v.  One launch.
 * lrf_mesh_components_round: one round of min-label hooking on parent (int32 [Nv], from _init or an earlier round): changed
 * (device int32 [1]) = 0; per face with roots ra, rb, rc = parent[a], parent[b], parent[c] and m their minimum, an int32
 * atomicMin(&parent[r], m) for each r > m, and bit 0 of changed when one lowered its target; then every vertex walks its
 * strictly decreasing parents (at most Nv steps) and stores the root it reaches.  A face with an index outside [0, Nv) -- or,
 * from a foreign parent array, a parent outside it -- is never dereferenced: it is skipped and sets bit 1 of changed.  The
 * caller reads changed back; the first round that leaves bit 0 clear found every face inside one tree: parent then holds the
 * labels.  No compare-and-swap loop, no waiting on another lane, wave or workgroup.  Three launches (two with Nf = 0: no face
 * kernel).
 * lrf_mesh_components_count: faces_of[l] = the faces whose first vertex has label l (faces with an index out of range are
 * skipped), vertices_of[l] = the vertices with label l, both int32 [Nv] and 0 where l is no label; summary (device int64 [3]) =
 * the number of components, the number of components with at least one face, the face count of the largest component.  Integer
 * atomics.  Four launches (three with Nf = 0).
 * lrf_mesh_filter: keeps the components with faces_of[label] >= threshold.  vertices_out [Nv,3], rgb8_out [Nv,3] (nullable, with
 * rgb8) and faces_out [Nf,3] (null allowed when Nf = 0) must hold the input's rows; the kept vertices and faces are written in
 * the input's order from row 0, a kept vertex's new index is the number of kept vertices before it, and kept faces are
 * rewritten through that map.  counts (device int64 [3]) receives the kept vertices, kept faces and kept components.  labels
 * and faces_of must come from the calls above (a label outside [0, Nv) drops its vertex; a face with an index outside [0, Nv) is
 * dropped without being dereferenced).  Three launches, no atomics, no host synchronisation.  workspace:
 * lrf_mesh_filter_workspace_bytes(Nv, Nf) bytes (0 for a refused shape), 8-byte aligned.
 * Refused before any launch: null or misaligned pointers (int32 and float arrays 4 bytes; summary, counts and workspace 8),
 * Nv < 1, Nf < 0, Nv or Nf >= 2^31, a negative threshold, rgb8 without rgb8_out or the reverse. */
typedef struct LrfMeshFilter {
  const float* vertices; const uint8_t* rgb8 /* nullable */; const int32_t* faces;
  const int32_t* labels; const int32_t* faces_of;
  int64_t Nv, Nf;
} LrfMeshFilter;
int lrf_mesh_components_init(int32_t* parent, int64_t Nv, void* stream);
int lrf_mesh_components_round(int32_t* parent, const int32_t* faces, int64_t Nv, int64_t Nf, int32_t* changed /* device [1] */,
                              void* stream);
int lrf_mesh_components_count(const int32_t* labels, const int32_t* faces, int64_t Nv, int64_t Nf, int32_t* faces_of,
                              int32_t* vertices_of, int64_t* summary /* device [3] */, void* stream);
size_t lrf_mesh_filter_workspace_bytes(int64_t Nv, int64_t Nf);
int lrf_mesh_filter(const LrfMeshFilter* m, int32_t threshold, float* vertices_out, uint8_t* rgb8_out /* nullable */,
                    int32_t* faces_out, int64_t* counts /* device [3] */, void* workspace, void* stream);

/* An indexed triangle mesh simplified by uniform vertex clustering (csrc/lrf_mesh_simplify.inl states the semantics and the
 * kernels): the vertices of one cell of a uniform grid of edge `cell`, anchored at `origin`, become one vertex at their mean,
 * faces follow their vertices, faces that collapse are dropped and, with dedupe, so are all but the first of the faces that
 * have become equal.  Integer sums, fp64 operations each rounded on its own and an order-independent choice among duplicates:
 * every call leaves the same bytes on every run.  No sort, no floating-point atomics, no loop that waits on another lane.
 * lrf_mesh_simplify_bounds: out (device int32 [7]) = lo[3], hi[3], the per-axis minimum and maximum of the vertices' cell
 * indices floor((v - origin) / cell), and a flag word whose bit 0 says that some vertex is bad -- a coordinate that is not finite
 * or a cell index outside (-2^30, 2^30) --; bad vertices enter neither bound.  origin: HOST array of 3 doubles.  Two launches.
 * lrf_mesh_simplify: the box lo, dims = hi - lo + 1 of the call above (cells = dims[0] dims[1] dims[2] < 2^31).  vertices_out
 * [Nv,3], rgb8_out [Nv,3] (nullable, with rgb8) and faces_out [Nf,3] (null allowed when Nf = 0) must hold the input's rows.
 * counts (device int64 [5]) = vertices out, faces out, occupied cells, degenerate faces, duplicate faces; counts[1] = -1 when a
 * face held an index outside [0, Nv) (such a face is never dereferenced), counts[0] = -1 when a vertex was bad or outside the
 * box (never used as an index): the outputs then mean nothing.  Twelve launches (eleven without dedupe, five -- and an empty
 * mesh -- with Nf = 0: no face kernel), no host synchronisation.  workspace: lrf_mesh_simplify_workspace_bytes(Nv, Nf, cells)
 * bytes (0 for refused arguments), 8-byte aligned.
 * Refused before any launch: null or misaligned pointers (float and int32 arrays 4 bytes; counts and workspace 8), Nv < 1,
 * Nf < 0, Nv or Nf >= 2^31, rgb8 without rgb8_out or the reverse, a dims entry < 1, cells >= 2^31, a box outside (-2^30, 2^30),
 * a non-finite origin, a cell that is not finite and positive. */
typedef struct LrfMeshSimplify {
  const float* vertices; const uint8_t* rgb8 /* nullable */; const int32_t* faces;
  int64_t Nv, Nf;
  double origin[3], cell;
  int32_t lo[3], dims[3];
  int32_t dedupe, reserved;
} LrfMeshSimplify;
int lrf_mesh_simplify_bounds(const float* vertices, int64_t Nv, const double* origin /* host [3] */, double cell,
                             int32_t* out /* device [7] */, void* stream);
size_t lrf_mesh_simplify_workspace_bytes(int64_t Nv, int64_t Nf, int64_t cells);
int lrf_mesh_simplify(const LrfMeshSimplify* m, float* vertices_out, uint8_t* rgb8_out /* nullable */, int32_t* faces_out,
                      int64_t* counts /* device [5] */, void* workspace, void* stream);

/* The same simplification with every emitted cluster's vertex placed where the summed plane quadric of the faces that touch
 * the cluster is smallest, inside the cluster's closed cell (Lindstrom's out-of-core simplification; rules a-d in
 * csrc/lrf_mesh_simplify.inl).  Cells, clusters, faces, colours, dedupe and the output order are lrf_mesh_simplify's; only
 * the positions differ.  int64 sums of coefficients scaled by one power of two per cluster (integer atomicAdd, int32
 * atomicMax), then fp64 operations each rounded on its own: the same bytes on every run, whatever the order of the input.
 * regularize in (0, 1] pulls towards the mean of the cluster's vertices with weight regularize * trace: it decides the
 * position inside a plane and along a crease.  A cluster keeps the mean when it has no contribution, 2^21 or more of them,
 * or a system that does not solve (trace <= 0, determinant <= 0, a non-finite solution).
 * counts (device int64 [7]) = the five of lrf_mesh_simplify, then the emitted clusters left at the mean and the emitted
 * clusters whose solution was clamped to the cell.  Sixteen launches (fifteen without dedupe, six with Nf = 0), no host
 * synchronisation.  workspace: lrf_mesh_simplify_quadric_workspace_bytes(Nv, Nf, cells) bytes (0 for refused arguments),
 * 8-byte aligned.  Refused before any launch: everything lrf_mesh_simplify refuses, and a regularize that is not finite or
 * lies outside (0, 1]. */
typedef struct LrfMeshSimplifyQuadric {
  LrfMeshSimplify mesh;
  double regularize;
} LrfMeshSimplifyQuadric;
size_t lrf_mesh_simplify_quadric_workspace_bytes(int64_t Nv, int64_t Nf, int64_t cells);
int lrf_mesh_simplify_quadric(const LrfMeshSimplifyQuadric* q, float* vertices_out, uint8_t* rgb8_out /* nullable */,
                              int32_t* faces_out, int64_t* counts /* device [7] */, void* workspace, void* stream);

/* The faces around each vertex of an indexed triangle mesh, and what is built on them: boundary and non-manifold edge counts,
 * area-weighted vertex normals and Taubin lambda|mu smoothing (csrc/lrf_mesh_smooth.inl states the semantics and the kernels).
 * Integer counts, int64 sums of fixed-point values and fp64 operations each rounded on its own: every call leaves the same
 * bytes on every run.  No sort, no floating-point atomics, no loop that waits on another lane.  A face with an index outside
 * [0, Nv) is never dereferenced; a face with two equal indices is degenerate; both take part in nothing.
 * info (device int64 [8], written by every call) = flag bits, degenerate faces, boundary edges, non-manifold edges, zero
 * normals, pinned vertices, incidence entries, 0.  Flag bits: 1 a face index outside [0, Nv); 2 a vertex held by 2^20 faces
 * or more; 4 a vertex coordinate that is not finite (normals); 8 a smoothing step left the fixed-point range (diverged).  With
 * a flag set the other outputs mean nothing.
 * lrf_mesh_incidence: the lists alone, in the workspace (E 8 bytes, row_start int32 [Nv + 1], a cursor int32 [Nv], int32
 * [ceil(Nv / 256)], row_faces int32 [3 Nf], a byte mask [Nv]).  Six launches, four with Nf = 0.
 * lrf_mesh_topology: the lists, then per directed edge (a, b) of a valid face the counts opp (edges (b, a)) and same (edges
 * (a, b) of other faces): info[2] = edges with opp == 0, info[3] = edges with same > 0 or opp > 1, boundary (device uint8
 * [Nv]) = 1 at both ends of every edge with opp == 0, else 0.  Seven launches.
 * lrf_mesh_vertex_normals: normals (device fp32 [Nv,3]) = the unit sum of the face normals around each vertex, (0, 0, 0) --
 * counted in info[4] -- where that sum is 0.  Eight launches.
 * The three above take a workspace of lrf_mesh_incidence_workspace_bytes(Nv, Nf) bytes (0 for refused arguments).
 * lrf_mesh_smooth_bounds: out (device int32 [7]) = the per-axis minimum [3] and maximum [3] of the vertices as order-preserving
 * integers (bits ^ ((bits >> 31) & 0x7fffffff), -0 read as +0) and a flag word, 1 when a coordinate is not finite.  Two launches.
 * lrf_mesh_smooth: the lists, the topology, then `iterations` times a step with factor lam and (mu != 0) a step with factor mu,
 * each reading one position buffer and writing the other; the last writes vertices_out [Nv,3], which must not be the input.
 * lo (the minima above, as doubles) and s (36 - the binary exponent of the largest extent; 0 for a box of zero extent) fix
 * the fixed point of the whole call.  pin_boundary != 0 keeps the vertices of the boundary mask where they are; info[5]
 * counts them.  All launches are queued by this one call, with no host synchronisation.  workspace:
 * lrf_mesh_smooth_workspace_bytes(Nv, Nf) bytes.
 * Refused before any launch: null or misaligned pointers (float and int32 arrays 4 bytes; info and workspace 8), Nv < 1,
 * Nf < 0, Nv >= 2^31, 3 Nf >= 2^31, iterations outside [0, 1000], lam outside (0, 1], mu outside [-1, 0], a non-finite lo,
 * |s| > 256. */
typedef struct LrfMeshSmooth {
  const float* vertices; const int32_t* faces;
  int64_t Nv, Nf;
  double lo[3], lam, mu;
  int32_t s, iterations, pin_boundary, reserved;
} LrfMeshSmooth;
size_t lrf_mesh_incidence_workspace_bytes(int64_t Nv, int64_t Nf);
int lrf_mesh_incidence(const int32_t* faces, int64_t Nv, int64_t Nf, int64_t* info /* device [8] */, void* workspace, void* stream);
int lrf_mesh_topology(const int32_t* faces, int64_t Nv, int64_t Nf, uint8_t* boundary /* device [Nv] */,
                      int64_t* info /* device [8] */, void* workspace, void* stream);
int lrf_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t Nv, int64_t Nf, float* normals,
                            int64_t* info /* device [8] */, void* workspace, void* stream);
int lrf_mesh_smooth_bounds(const float* vertices, int64_t Nv, int32_t* out /* device [7] */, void* stream);
size_t lrf_mesh_smooth_workspace_bytes(int64_t Nv, int64_t Nf);
int lrf_mesh_smooth(const LrfMeshSmooth* m, float* vertices_out, int64_t* info /* device [8] */, void* workspace, void* stream);

/* The small holes of an indexed triangle mesh found and closed (csrc/lrf_mesh_fill.inl states the semantics and the kernels).
 * A boundary edge is a directed edge (a, b) of a valid face whose reverse no valid face holds (lrf_mesh_topology's opp == 0); a
 * vertex is simple when exactly one boundary edge leaves it and exactly one enters it; next(a, b) is the boundary edge leaving b
 * when b is simple.  A fillable loop is a cycle of next of 3 .. max_edges edges.  Loop r, ranked by its first edge in face
 * order, adds vertex Nv + r at the mean of the loop's vertices -- positions in the fixed point of lrf_mesh_smooth (lo and s from
 * lrf_mesh_smooth_bounds, the caller's to compute: lo the minima as doubles, s = 36 - the binary exponent of the largest
 * extent), summed in int64; colours as the rounded integer mean per channel -- and every edge (a, b) of the loop, in face order,
 * appends the face (b, a, Nv + r).  The input's vertices, colours and faces are the output's prefix, bit for bit.  Holes that
 * touch in a vertex, rims through a non-manifold edge and loops of more than max_edges edges are left alone.  Integer counts,
 * integer minima, exact sums: every call leaves the same bytes on every run.
 * info (device int64 [8], written by both calls) = flag bits, degenerate faces, boundary edges, non-manifold edges, fillable
 * loops, edges in fillable loops, the longest fillable loop, boundary edges in no fillable loop.  Flag bits: 1 a face index
 * outside [0, Nv); 2 a vertex held by 2^20 faces or more; 8 a coordinate outside the fixed-point range of lo and s; 16 (fill) a
 * capacity below Nv + loops or Nf + edges in loops -- nothing is written past cap_v or cap_f rows.  With a flag set the other
 * outputs mean nothing.
 * lrf_mesh_holes: the analysis alone.  lrf_mesh_fill: the same analysis, then vertices_out [cap_v,3], rgb8_out [cap_v,3]
 * (nullable, with rgb8) and faces_out [cap_f,3], of which Nv + info[4] and Nf + info[5] rows are written.  All launches are
 * queued by the one call, with no host synchronisation.  workspace: lrf_mesh_holes_workspace_bytes(Nv, Nf) bytes (0 for refused
 * arguments) for either.
 * Refused before any launch: null or misaligned pointers (float and int32 arrays 4 bytes; info and workspace 8), Nv < 1,
 * Nf < 0, Nv >= 2^31, 3 Nf >= 2^31, max_edges outside [3, 4096] (the bound of the serial walk along a loop), a non-finite lo,
 * |s| > 256, cap_v < Nv, cap_f < Nf, a capacity of 2^31 or more, rgb8 without rgb8_out or the reverse, an output that is its input. */
typedef struct LrfMeshHoles {
  const float* vertices; const uint8_t* rgb8 /* nullable */; const int32_t* faces;
  int64_t Nv, Nf;
  double lo[3];
  int32_t max_edges, s;
} LrfMeshHoles;
size_t lrf_mesh_holes_workspace_bytes(int64_t Nv, int64_t Nf);
int lrf_mesh_holes(const LrfMeshHoles* m, int64_t* info /* device [8] */, void* workspace, void* stream);
int lrf_mesh_fill(const LrfMeshHoles* m, float* vertices_out, uint8_t* rgb8_out /* nullable */, int32_t* faces_out, int64_t cap_v,
                  int64_t cap_f, int64_t* info /* device [8] */, void* workspace, void* stream);

/* An indexed triangle mesh rasterised into V pinhole cameras, and two depth maps compared (csrc/lrf_mesh_raster.inl states the
 * coverage rule, the arithmetic and the kernels).  The inverse of lrf_tsdf_integrate: depth [V,H,W] comes out in the convention
 * that call takes (a multiple of the un-normalised pixel direction whose z is -1), 0.0 where no face was hit.  One ray per pixel
 * tested against every face with edge functions of exact sign, the nearest kept hit chosen by a 64-bit unsigned atomicMin over
 * (depth bits, face index): every call leaves the same bytes on every run, for every launch geometry and stream.
 * lrf_mesh_rasterize: vertices [Nv,3], faces [Nf,3] (both may be null when Nf = 0), rgb8 [Nv,3] (nullable, with rgb8_out),
 * cam2world [V,3,4], focal [1] and center [2] on the device.  cull: 0 keeps both orientations, 1 drops the faces seen from
 * behind their winding's normal, 2 those seen from its side.  A hit is kept when its depth is finite, positive and inside
 * [d_min, d_max].  Outputs: depth [V,H,W], face int32 [V,H,W] (-1: none), rgb8_out uint8 [V,H,W,3] (the vertex colours under the
 * hit's barycentric weights in fp64, rounded to nearest, ties to even), weights fp32 [V,H,W,3] (nullable: those weights),
 * crossings int32 [V,H,W] (nullable: the kept hits of both orientations, whatever cull is), info (device int64 [4]) = faces
 * skipped for an index outside [0, Nv) (never dereferenced), for two equal indices, for a coordinate that is not finite, 0.
 * Four launches (two with Nf = 0), no host synchronisation.  workspace: lrf_mesh_rasterize_workspace_bytes(V, H, W, Nf) bytes (0
 * for refused arguments) = 8 V H W of keys, 8 V Nf of (frame, face) list and its cursor; 8-byte aligned.
 * Refused before any launch: null or misaligned pointers (float and int32 arrays 4 bytes; info and workspace 8), V, H or W < 1,
 * V H W >= 2^31, Nv < 0 or >= 2^31, Nf < 0, V Nf >= 2^31, faces without vertices, rgb8 without rgb8_out or the reverse, cull
 * outside {0, 1, 2}, d_min > d_max (or NaN).
 * lrf_depth_agreement: mesh_depth and depth [V,H,W] -> counts (device int64 [V,16]) per frame = pixels valid (finite, positive,
 * inside [d_min, d_max]) in both maps, in mesh_depth only, in depth only, in neither; the sum over the both-valid pixels of
 * llrint(min(|mesh_depth - depth| / depth, 16) 2^24); three zeros; and at 8 + k the both-valid pixels with |mesh_depth - depth|
 * <= rel_tols[k] depth.  rel_tols: HOST array of n_tols values >= 0, n_tols <= LRF_AGREEMENT_MAX_TOLS.  error_map [V,H,W]
 * (nullable): the relative error unclamped, NaN where not both are valid.  Two launches.  Refused before any launch: null or
 * misaligned pointers, V outside [1, 65535], H or W < 1, V H W >= 2^31, n_tols outside [0, 8], a tolerance that is negative or
 * NaN, d_min > d_max. */
#define LRF_AGREEMENT_MAX_TOLS 8
typedef struct LrfMeshRaster {
  const float* vertices; const uint8_t* rgb8 /* nullable */; const int32_t* faces;
  const float* cam2world; const float* focal; const float* center;
  int64_t Nv, Nf;
  int32_t V, H, W, cull;
  float d_min, d_max;
} LrfMeshRaster;
size_t lrf_mesh_rasterize_workspace_bytes(int32_t V, int32_t H, int32_t W, int64_t Nf);
int lrf_mesh_rasterize(const LrfMeshRaster* m, float* depth, int32_t* face, uint8_t* rgb8_out /* nullable */,
                       float* weights /* nullable */, int32_t* crossings /* nullable */, int64_t* info /* device [4] */,
                       void* workspace, void* stream);
int lrf_depth_agreement(const float* mesh_depth, const float* depth, int32_t V, int32_t H, int32_t W,
                        const float* rel_tols /* host [n_tols] */, int32_t n_tols, float d_min, float d_max,
                        int64_t* counts /* device [V,16] */, float* error_map /* nullable */, void* stream);

/* A texture atlas baked for an indexed triangle mesh from encoded frames (csrc/lrf_mesh_texture.inl states the layout, the
 * arithmetic and the kernels).  Layout: a patch of patch x patch texels (4 <= patch <= 64) per pair of faces, cols cells per
 * row, rows = ceil(ceil(Nf / 2) / cols); the atlas is rows patch by cols patch texels.  state: device float4 per texel
 * [rows patch, cols patch, 4] = (c_r, c_g, c_b, w), zero before the first bake.
 * bake: per texel the frames [V,H,W,3] uint8 in frame order -- projected into the frame (cam2world [V,3,4], focal [1],
 * center [2] on the device), tested against mesh_depth [V,H,W] (the mesh's own depth at those poses: |nz - dm| <= vis_tol dm)
 * and for facing (cos >= min_cos; two_sided = 0 also drops the frames behind the face's winding normal), weighted by
 * cos^2 / distance^2, sampled bilinearly, and folded into the state: blend 0 adds w c and w, blend 1 keeps the sample of the
 * largest weight (the earliest frame of equal ones).  One launch (none with Nf = 0), state read and written once, no atomics:
 * calls add up, frames k..V on top of 0..k leave the bytes of one call over 0..V.  rgb8 is not read.
 * resolve: atlas uint8 [rows patch, cols patch, 3] = c / w (blend 0) or c (blend 1) rounded to nearest, ties to even; mask
 * uint8 [rows patch, cols patch] = w > 0.  A texel no frame saw takes its face's vertex colours (rgb8 [Nv,3], nullable) under
 * its barycentric weights, else fill (HOST uint8 [3]); a texel without a face takes fill.  info (device int64 [8]) = faces with
 * an index outside [0, Nv) (never dereferenced), with two equal indices, with a coordinate not finite, with a zero normal (none
 * of them is baked); texels that belong to a face, observed, coloured from the vertices, without a face.  Two launches (one
 * with Nf = 0); only the mesh, layout and blend members are read.
 * lrf_mesh_texture_state_bytes: 16 bytes per texel; cols <= 0 takes the default ceil(sqrt(ceil(Nf / 2))) (1 for Nf = 0); 0
 * for refused arguments and for Nf = 0.
 * Refused before any launch: null or misaligned pointers (float and int32 arrays 4 bytes, info 8, state 16), patch outside
 * [4, 64], cols < 1, Nf < 0, Nv < 0 or >= 2^31, faces without vertices, 2^31 texels or more, blend outside {0, 1}; bake also
 * V, H or W < 1, V H W >= 2^31, two_sided outside {0, 1}, vis_tol < 0 or NaN, min_cos outside [0, 1]. */
typedef struct LrfMeshTexture {
  const float* vertices; const uint8_t* rgb8 /* nullable */; const int32_t* faces;
  const uint8_t* frames; const float* mesh_depth; const float* cam2world; const float* focal; const float* center;
  int64_t Nv, Nf;
  int32_t patch, cols, blend, two_sided;
  int32_t V, H, W;
  float vis_tol, min_cos;
  int32_t reserved;
} LrfMeshTexture;
size_t lrf_mesh_texture_state_bytes(int64_t Nf, int32_t patch, int32_t cols);
int lrf_mesh_texture_bake(const LrfMeshTexture* m, float* state, void* stream);
int lrf_mesh_texture_resolve(const LrfMeshTexture* m, const float* state, const uint8_t* fill /* host [3] */, uint8_t* atlas,
                             uint8_t* mask, int64_t* info /* device [8] */, void* stream);

/* The closest point of an indexed triangle mesh for a batch of points, surface samples of a mesh, and a distance tensor
 * summarised (csrc/lrf_mesh_distance.inl states the pair arithmetic, the grid, the search and its stopping rule, the sampling
 * hash and the summary words).  Unsigned distance.  Faces with an index outside [0, Nv) (never dereferenced) or a corner that is
 * not finite are skipped and counted; zero-area faces are kept as the segments or points they are.  Every call leaves the same
 * bytes on every run.
 * lrf_mesh_index_bounds: out (device int64 [8]) = bad_index_faces, nonfinite_faces, used_faces, 0, then six int32 -- the
 * order-preserving keys (lrf_mesh_smooth_bounds') of the used faces' per-axis minima and maxima --, 0.  Two launches.
 * The index: grid, lrf_mesh_index_workspace_bytes(cells) bytes (a start and an end per cell; 0 when cells is outside
 * [1, 2^31)), and list, int32 [entries].  lo, cell, dims: the grid; a point's cell on axis k is floor((x - lo_k) / cell) in
 * fp64, clamped to [0, dims_k - 1].  lrf_mesh_index_build with list null is the count pass (three launches): it leaves the
 * cells' starts in grid and the number of entries in total (device int64 [1]); the caller reads it back, allocates list, and
 * calls again with list and entries: the fill pass (two launches).
 * lrf_mesh_closest: points [N,3] -> distance [N] ((float)sqrt of the fp64 squared distance; +inf without a face within
 * max_distance; NaN for a point that is not finite), face int32 [N] (the smallest index among equal distances; -1), closest
 * [N,3] (nullable; NaN without a face).  One launch, no atomics.  The result does not depend on cell.
 * lrf_mesh_sample_count: offsets (device uint32 [Nf]) = the samples before each face, info (device int64 [4]) = the total,
 * bad_index_faces, nonfinite_faces, faces that would take more than 2^21 samples (the caller refuses).  Three launches.
 * lrf_mesh_sample_emit: points [M,3] and face int32 [M] in face order; rows at M and beyond are not written.  One launch.
 * lrf_distance_summary: distance [N] -> words (device int64 [16]) = finite, infinite, NaN entries, sum1, sum2, the largest
 * finite bits, 0, 0, and at 8 + k the finite entries <= thresholds[k].  thresholds: HOST array.  Two launches (one with N = 0).
 * Refused before any launch: null or misaligned pointers (float and int32 arrays 4 bytes; out, info, total, words and grid 8),
 * Nv outside [1, 2^31), Nf outside [0, 2^31) (index build, closest and sampling: Nf < 1), dims < 1 or 2^31 cells or more, cell
 * or lo not finite, cell <= 0, entries outside [0, 2^31), N outside [1, 2^31) (summary: [0, 2^31)), max_distance < 0 or NaN,
 * spacing, unit or a threshold not finite or <= 0, M outside [1, 2^31), n_thresholds outside [0, 8]. */
#define LRF_DISTANCE_MAX_THRESHOLDS 8
typedef struct LrfMeshIndex {
  const float* vertices; const int32_t* faces; void* grid; int32_t* list /* null: the count pass */;
  int64_t Nv, Nf, entries;
  double lo[3]; double cell;
  int32_t dims[3]; int32_t reserved;
} LrfMeshIndex;
int lrf_mesh_index_bounds(const float* vertices, const int32_t* faces, int64_t Nv, int64_t Nf, int64_t* out /* device [8] */,
                          void* stream);
size_t lrf_mesh_index_workspace_bytes(int64_t cells);
int lrf_mesh_index_build(const LrfMeshIndex* m, int64_t* total /* device [1]; nullable in the fill pass */, void* stream);
int lrf_mesh_closest(const LrfMeshIndex* m, const float* points, int64_t N, double max_distance, float* distance, int32_t* face,
                     float* closest /* nullable */, void* stream);
int lrf_mesh_sample_count(const float* vertices, const int32_t* faces, int64_t Nv, int64_t Nf, double spacing,
                          uint32_t* offsets /* device [Nf] */, int64_t* info /* device [4] */, void* stream);
int lrf_mesh_sample_emit(const float* vertices, const int32_t* faces, int64_t Nv, int64_t Nf, double spacing,
                         const uint32_t* offsets, int64_t M, float* points, int32_t* face, void* stream);
int lrf_distance_summary(const float* distance, int64_t N, const float* thresholds /* host [n_thresholds] */,
                         int32_t n_thresholds, float unit, int64_t* words /* device [16] */, void* stream);

/* Registration around lrf_mesh_closest: a similarity applied to points, the exact moments of corresponding pairs, and the
 * normal equations of one linearised point-to-plane similarity step (csrc/lrf_align.inl states every rule and the overflow
 * bounds; the fit itself is the host's: localrf_amd/alignment.py).  Integer sums: the same words on every run and for every
 * order of the points.
 * lrf_align_transform: T, HOST, 12 doubles, row-major 3 x 4; out_k = (float)(((T[4k] x + T[4k+1] y) + T[4k+2] z) + T[4k+3]) in
 * fp64 without contraction.  out may be points.  One launch (none with N = 0).
 * lrf_align_pairs: a, b [N,3]; keep uint8 [N] (nullable: every pair is kept).  Per coordinate the integer rint((x - c_k) / h).
 * words (device int64 [24]) = pairs summed, out_of_range (an integer coordinate of magnitude >= 2^20), masked (keep == 0),
 * nonfinite, sum a [3], sum b [3], sum a_i b_j [9] row-major, sum |a|^2, sum |b|^2, 0, 0, 0.  Two launches (one with N = 0).
 * lrf_align_plane: points, closest [N,3], face int32 [N] and distance [N] as lrf_mesh_closest wrote them for points against the
 * mesh; gate: fp32, +inf allowed.  words (device int64 [48]) = points summed, unmatched (no face, a distance not finite),
 * gated (distance > gate), degenerate (a face without area), out_of_range (a coordinate of (p - c) / u or (q - c) / u beyond
 * [-1, 1]), 0, sum llrint(r r 2^36), sum llrint(J_k r 2^36) [7], sum llrint(J_k J_l 2^36) for k <= l [28], 0 .. 0, with r the
 * point-to-plane residual and J = (pt x n, n, pt . n) in units of u.  Two launches (one with N = 0).
 * lrf_align_plane_cloud: the same step against a cloud: closest, index int32 [N] and distance as lrf_cloud_closest wrote them
 * for points against the cloud, normals [M,3] fp32 one per cloud point (lrf_cloud_normals'; any length > 0 -- the kernel
 * normalises in fp64).  The plane of a point is the one through its closest point with the normal stored for index.  The same
 * 48 words in the same layout; unmatched: an index outside [0, M) or a distance not finite; degenerate: a normal with a word
 * that is not finite, or of length 0.  Two launches (one with N = 0).
 * Refused before any launch: null or misaligned pointers (float, int32 arrays 4 bytes; T and words 8), N outside [0, 2^20]
 * (transform: [0, 2^31)), h or u not a positive power of two, c or T not finite, gate < 0 or NaN, Nv outside [1, 2^31), Nf
 * outside [1, 2^31), M outside [1, 2^31). */
typedef struct LrfAlignFrame { double c[3]; double h; } LrfAlignFrame;
typedef struct LrfAlignPlane {
  const float* vertices; const int32_t* faces; const float* points; const float* closest; const int32_t* face;
  const float* distance;
  int64_t Nv, Nf, N;
  double c[3]; double u;
  float gate; int32_t reserved;
} LrfAlignPlane;
int lrf_align_transform(const double* T /* host [12] */, const float* points, int64_t N, float* out, void* stream);
int lrf_align_pairs(const LrfAlignFrame* fr, const float* a, const float* b, const uint8_t* keep /* nullable */, int64_t N,
                    int64_t* words /* device [24] */, void* stream);
int lrf_align_plane(const LrfAlignPlane* p, int64_t* words /* device [48] */, void* stream);
typedef struct LrfAlignPlaneCloud {
  const float* points; const float* closest; const int32_t* index; const float* distance; const float* normals;
  int64_t N, M;
  double c[3]; double u;
  float gate; int32_t reserved;
} LrfAlignPlaneCloud;
int lrf_align_plane_cloud(const LrfAlignPlaneCloud* p, int64_t* words /* device [48] */, void* stream);

/* A point cloud indexed for neighbour queries -- the point-cloud counterpart of the mesh index above -- and a cloud reduced to
 * one point per cell of a voxel grid (csrc/lrf_cloud.inl states the pair arithmetic, the grid, the walk and its stopping rule,
 * the k-best slots and the voxel rule).  A cloud point with a coordinate that is not finite is skipped and counted and is never
 * returned.  Every call leaves the same bytes on every run.
 * lrf_cloud_index_bounds: out (device int64 [8]) = nonfinite_points, used points, 0, 0, then six int32 -- the order-preserving
 * keys (lrf_mesh_smooth_bounds') of the used points' per-axis minima and maxima --, 0.  Two launches.
 * The index: grid, lrf_cloud_index_workspace_bytes(cells) bytes (8 bytes, then a start and an end per cell; 0 when cells is
 * outside [1, 2^31)), and records, entries x 16 bytes: x, y, z and the point's index as bits, in cell order; entries = the used
 * points of the bounds pass.  lo, cell, dims: the grid, as in LrfMeshIndex.  lrf_cloud_index_build: five launches (zero, count,
 * scan, copy, fill); a used point beyond `entries` records is not written.
 * lrf_cloud_closest: points [N,3] -> distance [N] ((float)sqrt of the fp64 squared distance; +inf without a point within
 * max_distance; NaN for a query that is not finite), index int32 [N] (the smallest index among equal distances; -1), closest
 * [N,3] (nullable; the winner's own words; NaN without one).  One launch, no atomics.  The result does not depend on cell.
 * lrf_cloud_knn: distance, index [N,k], ascending in (squared distance, index); a slot without a neighbour within max_distance
 * holds +inf, -1; a query that is not finite NaN, -1.  self_first = -1, or query i skips the cloud point self_first + i.  One launch.
 * lrf_cloud_radius_count: count int32 [N] = the used points with squared distance <= radius radius in fp64 (-1 for a query that
 * is not finite); self_first as above.  One launch.
 * lrf_cloud_normals: per query point the normal of the cloud around it: the eigenvector to the smallest eigenvalue of the
 * covariance of the used points within radius (squared distance <= radius radius, the boundary and the query's own twin
 * included), from integer sums on a lattice of step h -- the host passes the smallest power of two with radius / h <= 2^15 --
 * and a fixed number of cyclic Jacobi sweeps in fp64 (csrc/lrf_cloud.inl item 9 writes out every operation).  normal [N,3],
 * eigenvalues [N,3] (ascending, in squared world units) and count int32 [N] (the neighbours).  viewpoints (nullable): one
 * viewpoint (stride 0) or one per query (stride 3); the normal is turned towards it; without one, or where it lies in the
 * normal's plane, the component of largest magnitude is made positive.  Fewer than min_neighbours neighbours, or coincident
 * ones: normal (0, 0, 0), the true count.  A query that is not finite: NaN, NaN, -1.  points == NULL: the queries are the
 * cloud's own points, N == M, walked in the order of the index's records and written to the rows of the points (two launches:
 * the rows of points that are not finite, then the records); the same bytes as points = the cloud's.  Otherwise one launch;
 * none with N = 0.  Refused: N outside [0, 2^31), radius not finite or <= 0, h not that power of two, min_neighbours < 3, a
 * stride other than 0 or 3, points == NULL with N != M.
 * lrf_cloud_voxel_bounds: a point's integer cell is floor((x - origin) / cell) per axis (lrf_mesh_simplify's); out (device int64
 * [8]) = bad points (not finite, or a cell index of magnitude >= 2^30), used points, 0, 0, then six int32: the per-axis minimum
 * and maximum cell index of the used points, 0.  Two launches.
 * lrf_cloud_voxel: lo, dims = that box.  points_out [M,3], rgb8_out [M,3] (null iff rgb8 is), count_out int32 [M]: the first
 * counts[2] rows are written, one per occupied cell in cell order (x fastest): the mean position and rounded mean colour by
 * lrf_mesh_simplify's integer arithmetic, and the number of points.  cluster_of int32 [M]: each point's row, -1 for a bad point
 * or one outside the box.  counts (device int64 [8]): word 2 = occupied cells, the others 0.  workspace:
 * lrf_cloud_voxel_workspace_bytes(M, cells) bytes (0 for a refused shape).  Six launches.
 * Refused before any launch: null or misaligned pointers (float and int32 arrays 4 bytes; out, counts, workspace and grid 8;
 * records 16), M outside [1, 2^31), entries outside [0, M], N outside [1, 2^31), k outside [1, 8], radius negative, NaN or
 * infinite, max_distance negative or NaN, self_first < -1 or self_first + N > M, cell, lo or origin not finite, cell <= 0,
 * dims < 1 or 2^31 cells or more, a voxel box outside (-2^30, 2^30), rgb8 without rgb8_out or the reverse. */
#define LRF_CLOUD_MAX_K 8
typedef struct LrfCloudIndex {
  const float* points; void* grid; void* records;
  int64_t M, entries;
  double lo[3]; double cell;
  int32_t dims[3]; int32_t reserved;
} LrfCloudIndex;
typedef struct LrfCloudVoxel {
  const float* points; const uint8_t* rgb8 /* nullable */;
  int64_t M;
  double origin[3]; double cell;
  int32_t lo[3]; int32_t dims[3];
} LrfCloudVoxel;
int lrf_cloud_index_bounds(const float* points, int64_t M, int64_t* out /* device [8] */, void* stream);
size_t lrf_cloud_index_workspace_bytes(int64_t cells);
int lrf_cloud_index_build(const LrfCloudIndex* a, void* stream);
int lrf_cloud_closest(const LrfCloudIndex* a, const float* points, int64_t N, double max_distance, float* distance, int32_t* index,
                      float* closest /* nullable */, void* stream);
int lrf_cloud_knn(const LrfCloudIndex* a, const float* points, int64_t N, int32_t k, double max_distance, int64_t self_first,
                  float* distance /* [N,k] */, int32_t* index /* [N,k] */, void* stream);
int lrf_cloud_radius_count(const LrfCloudIndex* a, const float* points, int64_t N, double radius, int64_t self_first,
                           int32_t* count, void* stream);
int lrf_cloud_normals(const LrfCloudIndex* a, const float* points /* null: the cloud's own, record order */, int64_t N, double radius,
                      double h, int32_t min_neighbours, const float* viewpoints /* nullable */,
                      int64_t viewpoint_stride /* 0: one for all, 3: per query */, float* normal, float* eigenvalues, int32_t* count,
                      void* stream);
int lrf_cloud_voxel_bounds(const float* points, int64_t M, const double* origin /* host [3] */, double cell,
                           int64_t* out /* device [8] */, void* stream);
size_t lrf_cloud_voxel_workspace_bytes(int64_t M, int64_t cells);
int lrf_cloud_voxel(const LrfCloudVoxel* a, float* points_out, uint8_t* rgb8_out /* nullable */, int32_t* count_out,
                    int32_t* cluster_of, int64_t* counts /* device [8] */, void* workspace, void* stream);

/* Depth quantiles of a ray: the distance at which its accumulated weight first reaches q; q = 0.5 is the median depth, which
 * always lies on a surface the ray met (csrc/lrf_quantile.inl states the arithmetic: fp32 without contraction, one fixed
 * summation order per ray).  With C_i the inclusive prefix sum of the weights lrf_render_fwd leaves in weight_out and i* the
 * smallest i with C_i >= q: t = clamp((q - C_{i*-1}) / w_{i*}, 0, 1), depth = (z_{i*} + t (z_{i*+1} - z_{i*})) / |d|.  A ray
 * whose opacity never reaches q (or that meets a NaN weight first) gives depth exactly 0 and index -1.
 * lrf_render_depth_quantiles: one forward render into the workspace, then one launch without atomics: the same bits on every
 * run.  q: HOST array of K quantiles, 1 <= K <= 4, each in (0, 1], any order.  flags, floater_thresh: as lrf_render_fwd takes
 * them.  depth [K,R]; wsum [K,R] (nullable): 1 where found, else 0; index int32 [K,R] (nullable): i* or -1; acc [R]
 * (nullable): the forward's acc.  blend_w (nullable; [ceil(R / per_view)]) scales ray r's depth, wsum and acc by
 * blend_w[r / per_view]; accumulate = 1 adds to depth / wsum / acc instead of overwriting them: a scene sums its fields in
 * field order and divides depth by wsum at the end.  Refused before any launch: null pointers, R <= 0, S outside [2, 4096],
 * K outside [1, 4], a q outside (0, 1] or NaN, unknown flag bits, per_view < 1 with blend_w, accumulate outside {0, 1},
 * accumulate = 1 with index, blend_w without wsum, misaligned pointers (workspace: 256 bytes).  workspace:
 * lrf_quantile_workspace_bytes(R, S) bytes = the forward's workspace, the [R,S] weights and 5 R floats of per-ray outputs (0 for
 * a refused shape). */
size_t lrf_quantile_workspace_bytes(int32_t R, int32_t S);
int lrf_render_depth_quantiles(const LrfField* f, const float* rays, const float* z, int32_t R, int32_t S, uint32_t flags,
                               float floater_thresh, const float* q /* host [K] */, int32_t K, const float* blend_w /* nullable */,
                               int32_t per_view, int32_t accumulate, float* depth /* [K,R] */, float* wsum /* [K,R] or NULL */,
                               int32_t* index /* [K,R] or NULL */, float* acc /* [R] or NULL */, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRF_H_ */
