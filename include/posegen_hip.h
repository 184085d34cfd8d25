/*
 * posegen_hip.h -- C ABI of the MI355X-native A-NeRF renderer (libposegen_hip.so).
 *
 * The reference (mgholamikn/PoseGen) has no FFI: its renderer is the Python object
 * stored under render_kwargs['ray_caster'] (core/raycasters.py:156-178), called at
 * exactly one site, core/trainer.py:74.  This header is the boundary that object's
 * MI355X replacement (posegen_amd.HipRayCaster) binds through ctypes; every entry
 * point names the reference code it replaces.  SURVEY.md section 8(b).
 *
 * Conventions
 *   - every function returns 0 on success or a negative PG_E* code and never throws;
 *     pg_last_error() returns a human-readable message for the last failure
 *   - pointers are borrowed for the duration of the call
 *   - `stream` is a hipStream_t (torch's current HIP stream); pg_render_rays and the
 *     pg_stage_* entry points are asynchronous with respect to the host
 *   - "device pointer" = memory of the handle's HIP device
 *   - calls on one handle must be serialised by the caller (not re-entrant)
 */
#ifndef POSEGEN_HIP_H
#define POSEGEN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_ABI_VERSION 11

/* error codes */
#define PG_OK 0
#define PG_EINVAL (-1)      /* bad argument / unsupported configuration */
#define PG_ENOMEM (-2)      /* device allocation failed */
#define PG_EHIP (-3)        /* a HIP runtime call failed */
#define PG_ESTATE (-4)      /* weights / embedder not loaded yet */

/* precision of the fused embed+MLP kernel (arithmetic of the MFMA operands;
 * accumulation, biases, embedding and compositing are always fp32) */
#define PG_PREC_FP32 0      /* v_mfma_f32_32x32x2_f32, exact fp32 chain (parity mode) */
#define PG_PREC_BF16 1      /* bf16 x bf16 (BASELINE config 2) */
#define PG_PREC_BF16X3 2    /* split bf16: hi*hi + hi*lo + lo*hi */
#define PG_PREC_FP16 3      /* fp16 x fp16 */
#define PG_PREC_FP16X3 4    /* split fp16: hi*hi + hi*lo + lo*hi */
#define PG_PREC_FP16C 5     /* compensated fp16: two fp16 products per MAC into one fp32 accumulator,
                             * 128 f16(W/129) * f16(x) + f16(W1 + 129 (W/129 - W1)) * f16(x1 + 129 (x - x1)):
                             * the cross terms W_lo x and W x_lo are recovered to 2^-7 of their size, so the
                             * operand rounding of plain fp16 drops ~30x (<= 1e-5 on rgb/acc) */
#define PG_PREC_COUNT 6     /* kernel arithmetics above; the modes below are plans over them */
#define PG_PREC_FP16M 6     /* mixed: PG_PREC_FP16C for every pass whose maps are returned (the fine pass;
                             * the coarse pass when N_importance == 0; density queries), plain PG_PREC_FP16
                             * for the coarse pass of a hierarchical render, which only places the
                             * importance samples.  STATUS: cannot meet 1e-4 on acc_map (1.1e-4 measured on
                             * the benchmark frame, rgb_map 9e-5): the fp16 error of the coarse weights
                             * moves the importance samples, and the fine quadrature follows them.  Kept as
                             * a speed / accuracy point between fp16 (2.5e-4 / 2.9e-4) and fp16c (5e-6 /
                             * 8e-6) at 1.3x fp16c's rate, not as an in-tolerance mode; bound asserted in the
                             * tests: 2e-4.
                             * rgb0/disp0/acc0/alpha0 are plain fp16's.  With single_net the coarse raw enters
                             * the returned maps, so no pass is a guide pass: fp16c throughout. */
#define PG_PREC_MODES 7

/* density activation of raw2outputs (get_density_fn, core/raycasters.py:230-238) */
#define PG_ACT_RELU 0       /* F.relu                                                  */
#define PG_ACT_SOFTPLUS 1   /* F.softplus(x - softplus_shift, beta=1) (threshold 20)   */

/* flags of pg_render_rays */
#define PG_FLAG_LINDISP 1   /* sample linearly in inverse depth (ray_utils.py:224-227) */

/* Network / embedding description: the subset of the reference's flags that shapes
 * the renderer (run_nerf.py:186-490; create_raycaster, core/raycasters.py:17-184).
 * The kernels are specialised for the architecture every shipped reference config
 * uses: 24 joints, multires 7/{4,0}/0, 8x256 trunk with the skip after layer 4,
 * 128-wide view layer; pg_create rejects anything else with PG_EINVAL.
 * multires_views = 0 (configs/surreal/surreal_single.txt) is the row 0 (v * w) of the
 * multires_views = 4 embedding: its [128, 256+72(+16)] view weight is widened once where
 * weights enter the handle (sin/cos columns zero), and every kernel runs the 4-band layout. */
typedef struct pg_config {
    int32_t n_joints;        /* 24                       SMPLSkeleton                 */
    int32_t multires;        /* 7                        --multires                   */
    int32_t multires_views;  /* 4 or 0                   --multires_views             */
    int32_t multires_bones;  /* 0                        --multires_bones             */
    int32_t net_depth;       /* 8                        --netdepth                   */
    int32_t net_width;       /* 256                      --netwidth                   */
    int32_t skip_layer;      /* 4                        raycasters.py:82             */
    int32_t view_width;      /* 128 = net_width/2        nerf.py:78                   */
    int32_t framecode_ch;    /* 0, or 16 with --opt_framecode (nerf.py:86-87)         */
    int32_t n_framecodes;    /* rows of framecodes.codes.weight                       */
    int32_t chunk;           /* rays per nanmean group = --chunk (trainer.py:64-81)   */
    int32_t precision;       /* PG_PREC_*                                             */
    float cutoff_dist;       /* cutoff_mm * ext_scale   (raycasters.py:33)            */
    float density_scale;     /* --density_scale (B of raw2outputs)                    */
    float rgb_eps;           /* 1e-3                     nerf.py:151                  */
    float softplus_shift;    /* --softplus_shift (used when density_act == PG_ACT_SOFTPLUS)       */
    int32_t density_act;     /* --density_type: PG_ACT_RELU | PG_ACT_SOFTPLUS (get_density_fn,
                              * core/raycasters.py:230-238: the act_fn of raw2outputs, nerf.py:164) */
    int32_t single_net;      /* 0 | 1                    --single_net: network_fine is network
                              * (core/raycasters.py:99-104, 446-469): one set of weights (net 0);
                              * the importance pass evaluates only the N_importance new points,
                              * drawn from the is_only pdf (ray_utils.py:255-289), and the fine
                              * maps composite the coarse and new raw merged in depth order.
                              * PG_PREC_FP16M runs fp16c throughout (the coarse raw enters the
                              * fine maps: no pass is a guide pass). */
} pg_config;

/* Device output pointers of one pg_render_rays call; any may be NULL (not wanted).
 * Keys of RayCaster._collect_outputs (core/raycasters.py:711-724). */
typedef struct pg_outputs {
    float* rgb_map;   /* [n,3]                      fine (or coarse if N_importance==0) */
    float* disp_map;  /* [n]                                                          */
    float* acc_map;   /* [n]                                                          */
    float* alpha;     /* [n, N_samples+N_importance]                                  */
    float* rgb0;      /* [n,3]   coarse pass (only written when N_importance > 0)     */
    float* disp0;     /* [n]                                                          */
    float* acc0;      /* [n]                                                          */
    float* alpha0;    /* [n, N_samples]                                               */
    /* optional intermediates (tests / debugging; pg_render_scene's lists), reference names in comments.  A z_* / raw_* array on a
     * 256-byte boundary is the pass's own buffer (written in place), any other is filled by a copy at the end of the call. */
    float* near_far;  /* [n,2]  get_near_far_in_cylinder                              */
    float* z_coarse;  /* [n, N_samples]                 sample_from_lineseg           */
    float* z_fine;    /* [n, N_samples+N_importance]    isample_from_lineseg (sorted) */
    float* raw_coarse;/* [n, N_samples, 4]              run_network(network)          */
    float* raw_fine;  /* [n, N_samples+N_importance, 4] run_network(network_fine)
                       * (single_net: the coarse and the new raw merged in depth order) */
    float* weights0;  /* [n, N_samples]                 raw2outputs 'weights'         */
} pg_outputs;

typedef struct pg_handle pg_handle;

int pg_abi_version(void);

/* Replaces create_raycaster (core/raycasters.py:17-184) and its nn.DataParallel wrapper
 * (raycasters.py:157, re-pointed at run_gan.py:162-163): builds the renderer on n_devices HIP
 * devices of THIS process (1..64; device_ids required for more than one; a device may be listed
 * twice).  The weights are replicated once per device at load time.  Ray-level calls
 * (pg_render_rays, pg_render_frame, pg_stage_*, pg_query_density, pg_pose_kinematics) run on
 * device_ids[0]; pg_render_frames spreads frames over all of them.  Limits of the fused kernels:
 * N_samples in [16, 256] (32 for the 16-bit and compensated kernels' fast paths, below that the
 * k-major kernel runs), N_importance in {0, 2..64}, N_samples + N_importance <= 256. */
int pg_create(const pg_config* cfg, int n_devices, const int* device_ids, pg_handle** out);
int pg_device_count(const pg_handle* h);
void pg_destroy(pg_handle* h);
const char* pg_last_error(const pg_handle* h);   /* h may be NULL: last global error */

/* Replaces RayCaster.load_state_dict / load_ckpt_from_path (core/raycasters.py:768-788,
 * core/cutoff_embedder.py:227-238).  which_net: 0 = 'network_fn_state_dict' (coarse),
 * 1 = 'network_fine_state_dict' (not with single_net).  tensors[i] are HOST fp32 arrays in nn.Linear layout
 * [out,in] row-major, in this fixed order (n_tensors = 24):
 *   pts_linears.{0..7}.weight, pts_linears.{0..7}.bias,        (index 2*l, 2*l+1)
 *   alpha_linear.{weight,bias}, feature_linear.{weight,bias},
 *   views_linears.0.{weight,bias}, rgb_linear.{weight,bias}
 * shapes: 2 int64 per tensor (rows, cols; cols = 1 for biases); checked.  With multires_views = 0
 * views_linears.0.weight is [128, 256+72(+16)] (the reference's shape) and is widened here. */
int pg_load_weights(pg_handle* h, int which_net, const float* const* tensors,
                    const int64_t* shapes, int n_tensors);

/* CutoffEmbedder state: which 0 = embed_fn ('embed_state_dict'), 1 = embeddirs_fn
 * ('embeddirs_state_dict'): cutoff_dist Parameter[24] and the tau buffer
 * (core/cutoff_embedder.py:89-94, 181-183). */
int pg_set_embedder(pg_handle* h, int which, const float* cutoff_dist, float tau);

/* framecodes.codes.weight [n_codes, framecode_ch] (core/networks/embedding.py:6-46);
 * a row holding the mean code is appended internally (eval with idx < 0). */
int pg_set_framecodes(pg_handle* h, int which_net, const float* codes, int n_codes);

/* Select the MFMA operand precision (PG_PREC_*) for subsequent renders. */
int pg_set_precision(pg_handle* h, int precision);

/* Rays per nanmean group for subsequent renders: the `chunk` argument of render_path /
 * batchify_rays (run_nerf.py:28, core/trainer.py:64); callers pass different values
 * (run_gan.py:2318 args.chunk, run_nerf.py:157 args.chunk//8). */
int pg_set_chunk(pg_handle* h, int chunk);

/* Replaces RayCaster.forward / render_rays in eval mode (core/raycasters.py:345-474):
 * near/far in cylinder (per `chunk`-ray group nanmean patch), coarse samples, bone
 * relative embedding, coarse MLP, compositing, deterministic importance samples,
 * fine MLP on the merged samples, compositing.
 *   ray_batch [n,11] device: (o, d, near, far, viewdir) as packed by trainer.py:118-137
 *   skts      [*,24,4,4] device, row-major; pose_stride = floats between consecutive
 *             rays' pose (0 = one pose shared by all n rays, 384 = per-ray poses)
 *   cyls      [*,5] device (cx, cz, radius, top, bot); cyl_stride likewise (0 or 5)
 *   cams      [n] device float frame-code indices or NULL (NULL / negative -> mean code)
 * kps and bones of the reference call are numerically dead for the shipped encoders
 *  and are not part of the ABI. */
int pg_render_rays(pg_handle* h, void* stream, int64_t n, const float* ray_batch,
                   const float* skts, int64_t pose_stride,
                   const float* cyls, int64_t cyl_stride, const float* cams,
                   int n_samples, int n_importance, int flags, const pg_outputs* out);

/* The random draws of one training-mode render_rays call (render_kwargs_train,
 * core/raycasters.py:156-165: perturb, raw_noise_std, ray_noise_std), made by the CALLER:
 * torch's generator belongs to the host program, and the reference's own deterministic test mode
 * (pytest=True, ray_utils.py:171-180, 241-244; nerf.py:179-182) overwrites them with fixed numbers
 * in exactly these places.  All device pointers, any may be NULL (= that term off, as with std 0 /
 * perturb 0):
 *   t_rand    [n, N_samples]                  U[0,1): stratified jitter, z = lower + (upper-lower) t
 *                                             (sample_from_lineseg, ray_utils.py:229-246)
 *   u_rand    [n, N_importance]               U[0,1): inverse-cdf positions of sample_pdf with
 *                                             det=False (ray_utils.py:166-170)
 *   noise0    [n, N_samples]                  added to raw_density / B before the activation in the
 *                                             coarse raw2outputs (nerf.py:164, 174-184); the caller
 *                                             scales: randn * raw_noise_std * B
 *   noise1    [n, N_samples+N_importance]     same for the fine pass (in sorted sample order)
 *   ray_noise [n, N_samples+N_importance, 3]  position noise randn * ray_noise_std: rows [:N_samples]
 *                                             of a ray are added to its coarse points
 *                                             (raycasters.py:660-661), rows [N_samples:] to its
 *                                             importance points (raycasters.py:673-674); the fine
 *                                             pass sees every point with the noise it was drawn
 *                                             with, permuted by the depth sort like the reference's
 *                                             merged encodings (raycasters.py:458-460)
 * With ray_noise the per-ray (a + z b) table of the factorised kernels does not apply: both passes
 * run the direct kernels (q = R (o + z d + noise) + t per point). */
typedef struct pg_train_draws {
    const float* t_rand;
    const float* u_rand;
    const float* noise0;
    const float* noise1;
    const float* ray_noise;
} pg_train_draws;

/* RayCaster.forward / render_rays in training mode: pg_render_rays with the draws above.
 * draws == NULL is an error (eval mode is pg_render_rays). */
int pg_render_rays_train(pg_handle* h, void* stream, int64_t n, const float* ray_batch,
                         const float* skts, int64_t pose_stride,
                         const float* cyls, int64_t cyl_stride, const float* cams,
                         int n_samples, int n_importance, int flags,
                         const pg_train_draws* draws, const pg_outputs* out);

/* ---- the training step (backward through embedding inputs, MLP and compositing) ----
 * Replaces `render(..., **render_kwargs_train)` + `loss.backward()` of Trainer.train_batch (core/trainer.py:232-275,
 * 463) for one ray batch, in exact fp32 arithmetic.  The parameters are the CALLER's device tensors (a torch
 * optimiser owns them), nn.Linear layout, the 24 tensors of pg_load_weights' order; `codes` = framecodes.codes.weight
 * with the MEAN ROW APPENDED ([n_codes + 1, 16], embedding.py:25-26), NULL without frame codes. */
typedef struct pg_net_params {
    const float* w[24];
    const float* codes;
    int32_t n_codes;
} pg_net_params;
/* gradients, device, same shapes as the parameters (codes: [n_codes, 16], the mean row's share spread over all rows);
 * OVERWRITTEN by pg_train_backward */
typedef struct pg_net_grads {
    float* w[24];
    float* codes;
} pg_net_grads;

/* Forward of RayCaster.render_rays in training mode (core/raycasters.py:361-474; draws as in pg_render_rays_train,
 * may be NULL) with every activation kept on a tape inside the handle: arguments as pg_render_rays; `fine` may be
 * NULL when n_importance == 0.  The parameter tensors and the tape stay in use until pg_train_backward.  The handle
 * holds ONE tape: *tape_id (may be NULL) receives the id of this pass, which pg_train_backward must present -- a
 * forward pass in between overwrites the tape and makes the older id stale (PG_ESTATE) instead of silently
 * differentiating the wrong activations.
 * single_net handles: ONE net -- `coarse` holds its parameters, `fine` is not read (may be NULL) -- evaluated at the
 * n_samples coarse and the n_importance new points of every ray; pg_train_backward / pg_train_backward_pose write ONE set of
 * gradients into their `coarse` argument (`fine` not read).  With multires_views = 0 tensor 20 and its gradient are the
 * reference's [128, 256 + 72 (+16)] view weight.  Two nets with multires_views = 0 are refused (PG_EINVAL). */
int pg_train_forward(pg_handle* h, void* stream, int64_t n, const float* ray_batch, const float* skts, int64_t pose_stride,
                     const float* cyls, int64_t cyl_stride, const float* cams, int n_samples, int n_importance, int flags,
                     const pg_train_draws* draws, const pg_net_params* coarse, const pg_net_params* fine, const pg_outputs* out,
                     int64_t* tape_id);

/* Backward of the pg_train_forward that returned `tape_id` (it must still be the last one): given dL/d(rgb_map) [n,3], dL/d(acc_map) [n], dL/d(rgb0) [n,3], dL/d(acc0) [n]
 * (device, any may be NULL = zero; what Trainer.compute_loss reads, core/trainer.py:321-383), the gradient of L with
 * respect to every parameter tensor of both nets.  The importance samples are constants (`z_samples.detach()`,
 * core/utils/ray_utils.py:285). */
int pg_train_backward(pg_handle* h, void* stream, int64_t tape_id, const float* d_rgb_map, const float* d_acc_map,
                      const float* d_rgb0, const float* d_acc0, const pg_net_grads* coarse, const pg_net_grads* fine);

/* pg_train_backward plus the gradient of L with respect to the poses the forward pass read: pose refinement, the
 * reference's opt_pose (PoseOptLayer's kps / bones / skts with autograd history, core/pose_opt.py:240-447,
 * core/trainer.py:286-313; loss.backward() reaching them through the bone-relative transform and the embedding,
 * core/raycasters.py:476-555, core/encoders.py:8-37, 101-122, 172-193, core/cutoff_embedder.py:111-174; the pose
 * optimiser's step, trainer.py:453-485).  Only skts reaches the network inputs of the shipped encoders: kps and bones get
 * no gradient.  d_skts (device) is OVERWRITTEN with dL/dskts: d_pose_stride 384 -> [n,24,4,4], one gradient per ray
 * (whatever pose_stride the forward had: an expanded single pose is summed by the caller); 0 -> [24,4,4], the sum over
 * the rays in a fixed order.  Row 3 of every 4x4 is 0.  Bitwise repeatable.  The skts the forward read must still be
 * alive.  PG_EINVAL: d_pose_stride other than 0 / 384, d_skts null or not 16-byte aligned; PG_ESTATE: a stale tape. */
int pg_train_backward_pose(pg_handle* h, void* stream, int64_t tape_id, const float* d_rgb_map, const float* d_acc_map,
                           const float* d_rgb0, const float* d_acc0, const pg_net_grads* coarse, const pg_net_grads* fine,
                           float* d_skts, int64_t d_pose_stride);

/* ---- the pose layer of pose refinement: PoseOptLayer.calculate_kinematic (core/pose_opt.py:372-445) for the configuration
 * the shipped configs train with -- SMPL skeleton, use_rot6d, no cache.  Per unique pose u < n_poses: 6-D parameters -> rotation
 * (rot6d_to_rotmat, core/utils/skeleton_utils.py:507-523), the kinematic chain over the rest pose's offsets (pose_opt.py:399-414,
 * the levels of unrolled_kinematic_chain, pose_opt.py:482-521), + pelvis on every joint's translation (pose_opt.py:423-432),
 * skts = torch.inverse(l2ws) (pose_opt.py:435), kps = l2ws[..., :3, -1] (pose_opt.py:443); then the gather by inverse_idxs
 * (pose_opt.py:438-441): every output is written PER RAY through the ray -> pose map.
 *   bones     device [n_poses,24,rot_dim] f32, rot_dim = 6: a joint's 6 numbers viewed as [3,2], columns a1, a2
 *   pelvis    device [n_poses,3] f32
 *   rest_pose device f32: [24,3] shared by all poses (rest_stride 0) or [n_poses,24,3] (rest_stride 72)
 *   parents   HOST [24]: the joint tree, parent < child (parents[0] is not read beyond that check: joint 0 is the root)
 *   ray_pose  HOST [n_rays] int32: the pose of every ray (inverse_idxs); NULL: n_rays == n_poses and ray u is pose u
 *   rots [n_rays,24,3,3], l2ws [n_rays,24,4,4], skts [n_rays,24,4,4], kps [n_rays,24,3]: device f32 outputs, any may be NULL
 * float64 arithmetic inside, outputs rounded once.  The index arrays are HOST pointers so that they are checked before anything
 * is launched; they are copied into a buffer of the handle.  PG_EINVAL, nothing launched: rot_dim != 6, rest_stride other than
 * 0 / 72, a joint that does not come after its parent, a ray_pose entry outside [0, n_poses), NULL ray_pose with n_rays != n_poses.
 * Asynchronous on `stream`. */
int pg_poseopt_forward(pg_handle* h, void* stream, int64_t n_poses, int rot_dim, const float* bones, const float* pelvis,
                       const float* rest_pose, int64_t rest_stride, const int32_t* parents, int64_t n_rays, const int32_t* ray_pose,
                       float* rots, float* l2ws, float* skts, float* kps);

/* The transpose of pg_poseopt_forward: what loss.backward() does between the per-ray kps / skts / l2ws / rots and the parameters
 * (the autograd graph of core/pose_opt.py:387-443; the pose optimiser's step follows, core/trainer.py:453-485).  Stateless: the
 * forward of every pose is formed again from the parameters.  The per-ray cotangents d_rots / d_l2ws / d_skts / d_kps (device f32,
 * shapes of the forward's outputs, any may be NULL = zero) of a pose's rays are summed in ASCENDING RAY ORDER without atomics --
 * the reference's backward of skts[inverse_idxs] is an atomic scatter-add in no fixed order on a GPU -- then carried through the
 * inverse (dL2W = -S^T dS S^T, S = skt), the pelvis shift, the chain (children before parents), the cross product and the two
 * normalisations (below F.normalize's eps 1e-12: its derivative 1 / eps).  Outputs, device f32, OVERWRITTEN: d_bones
 * [n_poses,24,6], d_pelvis [n_poses,3].  Bitwise repeatable.
 *   seg_start HOST [n_poses + 1], seg_rays HOST [n_rays]: the rays of pose u are seg_rays[seg_start[u] .. seg_start[u + 1])
 * PG_EINVAL, nothing launched: the refusals of pg_poseopt_forward; seg_start not monotone from 0 to n_rays; seg_rays not a
 * permutation of 0 .. n_rays - 1, or not ascending inside a segment.  Asynchronous on `stream`. */
int pg_poseopt_backward(pg_handle* h, void* stream, int64_t n_poses, int rot_dim, const float* bones, const float* pelvis,
                        const float* rest_pose, int64_t rest_stride, const int32_t* parents, int64_t n_rays, const int32_t* seg_start,
                        const int32_t* seg_rays, const float* d_rots, const float* d_l2ws, const float* d_skts, const float* d_kps,
                        float* d_bones, float* d_pelvis);

/* One frame with its front and back end on the device.  Replaces, per
 * frame: get_rays + the bounding-box gather of kp_to_valid_rays (core/utils/ray_utils.py:6-28,
 * 83-136), render()'s ray_batch packing (core/trainer.py:118-137), RayCaster.forward on the
 * box's rays, and render_path's scatter into the background frame (run_nerf.py:98-137) --
 * no per-frame meshgrid, no host->device copy of rays, no device->host copy of ray maps.
 *   c2w         HOST [3,4] row-major camera-to-world (12 floats)
 *   intrinsics  HOST (fx, fy, cx, cy)
 *   box         HOST (tl_x, tl_y, br_x, br_y) of cylinder_to_box_2d (skeleton_utils.py:711-787),
 *               br row/column excluded like the reference's torch.arange(tl, br)
 *   skts [24,4,4], cyl [5] device (one pose per frame); cam: frame-code index (< 0: mean code)
 *   bg          device [H*W,3] background or NULL for the constant base_bg (1 = white_bkgd)
 *   rgb [H*W,3], disp [H*W] (NaN of empty rays -> 0), acc [H*W] device outputs (disp, acc may
 *   be NULL); rgb8 [H*W,3] optional uint8 frame = trunc(clamp(rgb*255)) (run_gan.py:2327). */
int pg_render_frame(pg_handle* h, void* stream, int H, int W, const float* c2w, const float* intrinsics,
                    const int* box, float near, float far, const float* skts, const float* cyl, float cam,
                    int n_samples, int n_importance, int flags, const float* bg, float base_bg,
                    float* rgb, float* disp, float* acc, uint8_t* rgb8);

/* The two halves of pg_render_frame, for callers that spread ONE frame over several processes (one process per
 * GPU, posegen_amd.dist: the counterpart of nn.DataParallel's scatter of a ray chunk over the GPUs,
 * core/raycasters.py:157, run_gan.py:162): rays [ray_begin, ray_end) of the box's row-major ray list
 * (kp_to_valid_rays order) -> their maps, device pointers rgb_map [ray_end-ray_begin,3], disp_map, acc_map
 * [ray_end-ray_begin].  ray_begin must be 0 or a multiple of the nanmean group size (pg_set_chunk), so that the
 * groups -- and with them every value -- are those of the whole frame rendered in one call.  Other arguments
 * as pg_render_frame.  Asynchronous on `stream`. */
int pg_render_frame_range(pg_handle* h, void* stream, int H, int W, const float* c2w, const float* intrinsics,
                          const int* box, float near, float far, const float* skts, const float* cyl, float cam,
                          int n_samples, int n_importance, int flags, int64_t ray_begin, int64_t ray_end,
                          float* rgb_map, float* disp_map, float* acc_map);

/* render_path's scatter of a box's maps over the background frame (run_nerf.py:98-137), alone: device maps of the
 * WHOLE box (rgb_map [n_box,3], disp_map, acc_map [n_box], e.g. assembled from pg_render_frame_range pieces) ->
 * rgb [H*W,3], disp, acc [H*W] (may be NULL), rgb8 (may be NULL), background as in pg_render_frame.  A box that reaches
 * outside the frame is clamped to it (tl to >= 0, br to <= W, H), and the maps are read as those of the CLAMPED box, row-major
 * with the clamped width: what pg_render_frame_range produces for the same box.  The maps of a box without pixels may be NULL. */
int pg_compose_frame(pg_handle* h, void* stream, int H, int W, const int* box, const float* rgb_map, const float* disp_map,
                     const float* acc_map, const float* bg, float base_bg, float* rgb, float* disp, float* acc, uint8_t* rgb8);

/* Frames on all devices of the handle, host in / host out: replaces the frame loop of render_path
 * (run_nerf.py:27-147) together with nn.DataParallel's scatter / gather.
 * One host thread and one stream per device.  Work plan (pg_plan_frames): the unit is a nanmean group (`chunk`
 * consecutive rays of a box); frames go to devices whole, largest first, while they fit under the per-device
 * target load; the frames that do not fit -- the tail of a batch whose size is not a multiple of the device
 * count (20 frames on 8 GPUs, run_gan.py:2042-2047), or every frame when there are fewer frames than devices --
 * are cut into runs of whole groups that fill the devices up to the target, rendered there, gathered on the
 * frame's owner by device-to-device copies (peer access is enabled at pg_create) and composed there.  The result
 * is bit-identical to one device either way.  No collective on the data path.
 *   c2ws [F,3,4], intrinsics [F,4], boxes [F,4] (tl_x, tl_y, br_x, br_y), skts [F,24,4,4], cyls [F,5],
 *   cams [F] or NULL: HOST; bg HOST [H*W,3] or NULL (one background for all frames)
 *   rgbs [F,H,W,3] f32, disps [F,H,W], accs [F,H,W], rgb8 [F,H,W,3] u8: HOST outputs, any but one of
 *   rgbs / rgb8 may be NULL.  Synchronous. */
int pg_render_frames(pg_handle* h, int n_frames, int H, int W, const float* c2ws, const float* intrinsics,
                     const int* boxes, float near, float far, const float* skts, const float* cyls,
                     const float* cams, int n_samples, int n_importance, int flags, const float* bg, float base_bg,
                     float* rgbs, float* disps, float* accs, uint8_t* rgb8);

/* ---- the subject bank: S >= 1 complete models ("subjects": independent checkpoints of ONE architecture) behind one
 * handle (frames drawn from >= 2 weight sets; the reference's subject_idxs).  A handle is created with one
 * subject, and with one subject nothing differs from a handle without a bank.  Per subject: both nets (tensors, packed
 * weight images, frame codes -- n_codes may differ between subjects) and the embedder state (cutoff_dist, tau) with a
 * device copy of the cutoffs of its own.  Shared by the bank: pg_config's geometry (single_net, multires_views,
 * framecode_ch, the density activation), precision, chunk, on-chip mode, the skip switches, every workspace.
 * Training acts on the selected subject; the bank is not changed and no other subject selected while a training tape is
 * outstanding (a pg_train_forward whose backward has not run). */
#define PG_MAX_SUBJECTS 64

/* 1 <= n <= PG_MAX_SUBJECTS subjects.  Growing keeps the loaded subjects (new ones are empty: no weights, the config's
 * cutoff_dist, tau 20, embedder not set); shrinking frees the dropped subjects' device memory (waits for the device).
 * PG_EINVAL: n out of range, the active subject would be dropped (select one that stays first), a tape outstanding. */
int pg_set_subject_count(pg_handle* h, int n);
int pg_subject_count(const pg_handle* h);

/* Subject s becomes the active model: every entry point (pg_load_weights, pg_load_weights_device, pg_set_embedder,
 * pg_set_framecodes, pg_render_rays*, pg_render_frame*, pg_query_density, pg_stage_*, the training entry points) then acts
 * on it, on every device of the handle.  A swap of host-side pointers: no device allocation, no packing, no copy, no
 * synchronisation -- safe between two launches enqueued on one stream (a launch has taken its subject's pointers when the
 * call that enqueued it returns).  PG_EINVAL: s outside [0, count), a tape outstanding. */
int pg_select_subject(pg_handle* h, int s);

/* Which nets of subject s are loaded (bit 0: coarse, bit 1: fine), the device bytes its packed weight images hold, and how
 * many images have been built for it so far (packed and uploaded by the first call that needed them, or re-formed on the
 * device by pg_load_weights_device) -- on the handle's first device; any pointer may be NULL.  A render that alternates
 * between subjects builds nothing once every subject has rendered in the precision. */
int pg_subject_info(pg_handle* h, int s, int32_t* loaded_nets, int64_t* image_bytes, int64_t* image_builds);

/* pg_render_frames with one subject per frame: subjects HOST [F] (NULL: every frame with the active subject, which is
 * pg_render_frames).  The work plan is unchanged; every device selects the subject of the task it is about to enqueue, so
 * the runs of a frame that is cut over several devices keep the frame's subject.  Every device holds every subject's
 * weights (pg_load_weights replicates as it does for one model).  The active subject is the same before and after.
 * PG_EINVAL: a subject outside [0, count); subjects given while a tape is outstanding. */
int pg_render_frames_subjects(pg_handle* h, int n_frames, int H, int W, const float* c2ws, const float* intrinsics,
                              const int* boxes, float near, float far, const float* skts, const float* cyls,
                              const float* cams, int n_samples, int n_importance, int flags, const float* bg, float base_bg,
                              float* rgbs, float* disps, float* accs, uint8_t* rgb8, const int32_t* subjects);

/* Host-only: the work plan pg_render_frames uses (and posegen_amd.dist.plan_tasks restates for the one-process-
 * per-GPU path): tasks (frame, ray_begin, ray_end, worker, owner) for frames of n_rays[f] rays on n_workers
 * devices with nanmean groups of `chunk` rays; every ray of every frame is in exactly one task, every cut is a
 * multiple of `chunk`, the loads differ by about one group.  out_tasks [cap,5] may be NULL to query n_tasks. */
int pg_plan_frames(int n_frames, const int64_t* n_rays, int n_workers, int chunk, int32_t* out_tasks, int cap,
                   int* n_tasks);

/* Batched pose kinematics on the device: replaces get_smpl_l2ws and
 * the kp / skts derivation of load_retarget (core/utils/skeleton_utils.py:379-463,
 * run_gan.py:2211-2257) so that generator outputs can stay on the GPU.
 *   bones     device [n_poses,24,3] float64 axis-angle
 *   bone_offsets HOST [24,3] float64: rest[0] for the root, rest[j] - rest[parent[j]] otherwise,
 *             formed by the caller in the rest pose's own dtype as the reference does (float32
 *             for smpl_rest_pose); parents HOST [24] (joint tree, parent < child)
 *   kps [n,24,3] f32, skts [n,24,4,4] f32 (= l2w^-1), l2ws [n,24,4,4] f64: device, any may be NULL
 * float64 arithmetic like the reference; float32 outputs are rounded once. */
int pg_pose_kinematics(pg_handle* h, void* stream, int64_t n_poses, const double* bones, const double* bone_offsets,
                       const int32_t* parents, float* kps, float* skts, double* l2ws);

/* Bounding cylinder and its projected integer box per pose, on the device: replaces
 * get_kp_bounding_cylinder + cylinder_to_box_2d (core/utils/skeleton_utils.py:635-685, 700-787) as
 * kp_to_valid_rays calls them (core/utils/ray_utils.py:89-104: head '-y', SMPL root joint 0), so that key
 * points produced on the GPU (pg_pose_kinematics) need not come back to the host before rendering.
 *   kps    device [n,24,3] f32        w2c  DEVICE [n or 1,4,4] f64 row-major (the reference's float32
 *          np.linalg.inv(swap_mat(c2w)) widened; w2c_stride = 16, or 0 for one camera)
 *   ring   DEVICE [50,2] f64: cos, sin of np.linspace(0, 2 pi, 50) as the caller's numpy computes them
 *   extension = extend_mm * ext_scale; top_ / bot_extension = extension * 1.60 / 1.10 (the caller's doubles)
 *   fx, fy focal lengths; off_x, off_y = int(W/2), int(H/2) or the integer principal point
 *   cyls   device [n,5] f32 (cx, cz, radius, top, bot)     boxes device [n,4] i32 (tl_x, tl_y, br_x, br_y)
 * float32 cylinder, float64 projection, like numpy in the reference; the box is an integer and equals the
 * reference's on every pose of the golden fixture. */
int pg_pose_boxes(pg_handle* h, void* stream, int64_t n_poses, const float* kps, const double* w2c, int64_t w2c_stride,
                  const double* ring, double extension, double top_extension, double bot_extension, double fx, double fy,
                  int H, int W, int off_x, int off_y, float* cyls, int32_t* boxes);

/* ---- stage entry points (same kernels, exposed for parity tests and profiling) ---- */

/* get_rays + the bounding-box gather of kp_to_valid_rays + render()'s ray_batch packing (ray_utils.py:6-28, 83-136,
 * trainer.py:118-137): the frame front end of pg_render_frame alone, nothing rendered.  Rays [ray_begin, ray_end) of the
 * box's row-major ray list -> rays [ray_end-ray_begin,11] (origin, direction, near, far, unit direction) and, unless NULL,
 * cams [ray_end-ray_begin] = cam: the caller's device buffers.  H, W, c2w, intrinsics, box (clamped to the frame) as in
 * pg_render_frame.  No nanmean alignment of ray_begin.  PG_EINVAL, nothing launched: a null handle or pointer, a range
 * outside the box, ray_begin > ray_end.  An empty range launches nothing.  Asynchronous on `stream`. */
int pg_stage_frame_rays(pg_handle* h, void* stream, int H, int W, const float* c2w, const float* intrinsics, const int* box,
                        float near, float far, float cam, int64_t ray_begin, int64_t ray_end, float* rays /*[n,11]*/,
                        float* cams /*[n] or NULL*/);

/* get_near_far_in_cylinder + sample_from_lineseg (ray_utils.py:204-251, 292-344). */
int pg_stage_sample_coarse(pg_handle* h, void* stream, int64_t n, const float* ray_batch,
                           const float* cyls, int64_t cyl_stride, int n_samples, int flags,
                           float* near_far /*[n,2]*/, float* z /*[n,S]*/);

/* encode_inputs + run_network (raycasters.py:476-577, nerf.py:90-148) on n*S points
 * p = o + d*z: the fused embedding + MLP kernel.  raw [n,S,4] = (rgb_raw, sigma_raw).
 * dbg (optional, [n*S,256] floats) receives one intermediate activation per point,
 * selected by dbg_stage: 0 = pre-activation of density layer 0; 1..7 = output of density
 * layer 1..7 (post-ReLU); 8 = feature_linear output; 9 = view layer output (128 used);
 * 10 = view cutoff weights wd (24 used); 11 = the first 16 units of view-layer input values as
 * the MFMA sees them; 12..17 = floats 64(s-12).. of the lane half's view table as found in LDS at the
 * end of the pass.  Stages > 0 are only honoured by the fp32-grade kernels (PG_PREC_FP32 / *X3).
 * dbg_stage 97 (measurement aid; the 16-bit and compensated modes on rays with >= 64 samples): dbg is an array of >= 3
 * ZEROED unsigned counters instead, to which the launch adds: [0] workgroup passes, [1] limbs left out of whole passes
 * (of 6 per pass), [2] limbs left out per wave / column tile (of 48 per pass) -- what the cutoff embedding's limb masks
 * (pg_set_far_skip) are worth on this call; [3] empty waves (of 8 per pass in pg_eval16r.hip: every valid point of the wave
 * has sigma <= 0; the other kernels leave it 0), [4] those of them that left the colour branch out (pg_set_empty_skip).  A
 * stage-97 call runs as a render call's launch would: `raw` holds rgb = 0 for the points of the waves counted in [4]. */
int pg_stage_eval(pg_handle* h, void* stream, int which_net, int64_t n, int n_samples,
                  const float* ray_batch, const float* z, const float* skts,
                  int64_t pose_stride, const float* cams, float* raw, float* dbg, int dbg_stage);

/* Density query on explicit points: replaces RayCaster.render_pts_density
 * / the forward function of _get_density_fwd_fn (core/raycasters.py:598-646) for one pose:
 * bone-relative embedding of pts [n_points,3] (device) + the trunk of net `which_net`.
 * raw [n_points,4] device: raw[:,3] = alpha_linear output (the reference's raw density, no
 * activation); raw[:,0:3] = rgb_raw for a zero view direction (ignore).  The frame code, if the
 * model has one, is the mean code.  which_net = 1 on a single_net handle is PG_EINVAL. */
int pg_query_density(pg_handle* h, void* stream, int which_net, int64_t n_points, const float* pts,
                     const float* skts, float* raw);

/* Mesh extraction (the reference's run_render.render_mesh): the density grid and marching cubes on the
 * device.
 *
 * pg_grid_density: raw density (alpha_linear output, no activation) of net `which_net` for one pose on the (res+1)^3 grid
 * root + (t[a], t[b], t[c]), t = linspace(-radius, radius, res+1) formed in double and rounded to float like numpy's, the
 * sums in float like the reference's `grid + kps[0,0]`.  sigma [R,R,R] device, c fastest: the layout of
 * RayCaster.render_mesh_density (core/raycasters.py:579-596) after its transpose.  root HOST [3], skts device [24,4,4].
 * A grid row is a ray of res+1 samples, so the call runs the fused kernel forms of a render call; rows shorter than the
 * form's minimum of samples per ray, or longer than 256, run as explicit points formed on the device (the forms of
 * pg_query_density).  The grid goes in slabs of slab_rays rows (0: chosen so that a slab's raw output stays within
 * 256 MiB), rounded down to a multiple of 256 / gcd(res+1, 256) rows (at least one such multiple) so that every slab starts
 * on a pass boundary of the kernels: the values do not depend on the slab size.  Refusals as pg_query_density; res outside [1, 1023] or a radius that
 * is not positive and finite is PG_EINVAL. */
int pg_grid_density(pg_handle* h, void* stream, int which_net, int res, double radius, const float* root,
                    const float* skts, int64_t slab_rays, float* sigma);

/* Marching cubes on a device float grid [nx,ny,nz] (nz fastest, every dimension >= 2, at most 4e8 points); needs no loaded
 * weights.  With f = max(grid, clamp) (clamp = 0: the reference's np.maximum(raw, 0); -INFINITY: the grid as it is), a point
 * is inside when f > threshold.  One vertex per grid edge whose ends differ: on the edge from point i to i + 1 along axis a,
 * coordinate i + (threshold - fa) / (fb - fa) on that axis (float), the integer indices on the other two -- index
 * coordinates.  Vertices are ordered by the linear index of the edge's lower point, then by axis; triangles by cell, then by
 * the case table's order (posegen_amd/mesh.py, compiled in); they index the vertices, which neighbouring cells share.
 * Normals point away from the inside.  Two calls on the same grid give the same bytes.
 * pg_mesh_count synchronises the stream, returns the two counts (0, 0 when nothing crosses: no error) and keeps its flags
 * and scans in the handle; pg_mesh_emit writes vertices [nv,3] and triangles [nt,3] (device) from them and is PG_ESTATE
 * unless shape, threshold, clamp and both counts are those of the last pg_mesh_count.  The grid must not change in between. */
int pg_mesh_count(pg_handle* h, void* stream, const float* grid, int nx, int ny, int nz, float threshold, float clamp,
                  int64_t* n_vertices, int64_t* n_triangles);
int pg_mesh_emit(pg_handle* h, void* stream, const float* grid, int nx, int ny, int nz, float threshold, float clamp,
                 float* vertices, int32_t* triangles, int64_t n_vertices, int64_t n_triangles);

/* ---- training batches from an image bank on the device: what BaseH5Dataset.__getitem__ + RayImageSampler + ray_collate_fn
 * (core/dataset.py:57-105, 277-364, 756-802; core/load_data.py:71-84) produce per step on the host.  The dataset's pixels
 * stay on the device as the uint8 they are stored as; none of the four entry points needs loaded weights, none uses atomics,
 * and two calls on the same inputs give the same bytes.  All are asynchronous on `stream` and check their host arguments
 * before anything is launched: PG_EINVAL, nothing launched and no output written, on a NULL required pointer, F or P not
 * positive (P above 2^31 - 2), k outside [1, 1024], an image / camera row outside its array, a background index outside the bank.
 *
 * The pixel index (once per bank) replaces the per-item `np.where(sampling_mask > 0)` (dataset.py:285-287).
 *   sampling_masks  device uint8 [F,P], P = H W; a pixel is valid when its byte is > 0
 * pg_pixel_index_count writes counts (device int64 [F]) and keeps the per-tile prefixes in the handle;
 * pg_pixel_index_emit, given start (device int64 [F + 1], the exclusive scan of counts with the total as last entry) and
 * total, writes ids (device int32 [total]): image f's valid flat pixel ids, ascending, at ids[start[f] .. start[f + 1]).
 * It is PG_ESTATE unless masks, F and P are those of the last pg_pixel_index_count on this handle; the masks must not change
 * in between (a store never leaves image f's range if they do). */
int pg_pixel_index_count(pg_handle* h, void* stream, const uint8_t* sampling_masks, int64_t F, int64_t P, int64_t* counts);
int pg_pixel_index_emit(pg_handle* h, void* stream, const uint8_t* sampling_masks, int64_t F, int64_t P, const int64_t* start,
                        int64_t total, int32_t* ids);

/* np.sort(np.random.choice(valid_idxs, k, replace=False)) of dataset.py:287-290, 321 for every image of a batch: a uniformly
 * random k-subset of the image's valid pixels, ascending.  The random numbers are the caller's, as everywhere in this ABI:
 * draws, device float64 [n_img,k] in [0, 1).  Per image with m valid pixels, Floyd's algorithm in the order of the draws:
 * for j = m - k .. m - 1 with u = draws[a, j - (m - k)], t = min((int64) floor(u (j + 1)), j); the rank inserted is j if t is
 * already chosen, else t.  The chosen ranks are sorted and pixel_idxs[a, :] (device int32 [n_img,k]) = ids[start[img] + rank].
 *   ids, start  device: the pixel index;  counts HOST int64 [F]: its counts;  img_rows HOST int32 [n_img]: the batch's
 *   images in the given order (the same image twice is two independent rows of draws), copied into a buffer of the handle.
 * PG_EINVAL also when k > counts[img] for an image of the batch. */
int pg_batch_sample_pixels(pg_handle* h, void* stream, const int32_t* ids, const int64_t* start, const int64_t* counts, int64_t F,
                           const int32_t* img_rows, int64_t n_img, int k, const double* draws, int32_t* pixel_idxs);

/* The bank a batch is gathered from.  Pixel arrays are device uint8, camera arrays device float32; bkgd_idxs is a HOST array. */
typedef struct pg_image_bank {
    const uint8_t* imgs;        /* [F,P,3] */
    const uint8_t* masks;       /* [F,P] (the reference's [F,P,1]) */
    const uint8_t* bkgds;       /* [n_bkgd,P,3] or NULL: no backgrounds */
    const int32_t* bkgd_idxs;   /* HOST [F]: the background of every image (required with bkgds) */
    const float* c2ws;          /* [n_cam,3,4] row-major: c2w[:3,:4] */
    const float* focals;        /* [n_cam,2]: (fx, fy) */
    const float* centers;       /* [n_cam,2]: (cx, cy), or NULL: the frame's centre (W 0.5, H 0.5) */
    int64_t F, P, n_bkgd, n_cam;
    int32_t H, W;               /* H W = P */
    int32_t mask_img;           /* target = target fg + (1 - fg) bg (dataset.py:272-273); ignored without backgrounds */
} pg_image_bank;

/* get_img_data + get_rays (dataset.py:259-275, 142-162, 346-364) and render()'s ray packing (core/trainer.py:118-137) for the
 * n = n_img k rays of a batch: ray r = a k + b is pixel p = pixel_idxs[r] (row = p / W, col = p % W) of image img_rows[a] seen
 * by camera cam_rows[a] (NULL: the image rows).  Device float32 outputs:
 *   target_s [n,3] = imgs[img, p] / 255 (IEEE division; with mask_img: target fg + (1 - fg) bg, each operation rounded)
 *   fgs [n,1] = masks[img, p];  bgs [n,3] = bkgds[bkgd_idxs[img], p] / 255 (NULL without backgrounds)
 *   rays_o [n,3] = c2w[:3,3];  rays_d [n,3]: with x = (col - W 0.5) / fx, y = (-(row - H 0.5)) / fy (centers: x = (col - cx) / fx,
 *   y = (-row + cy) / fy) and z = -1, rays_d[c] = (x R[c,0] + y R[c,1]) + z R[c,2], R = c2w[:3,:3] -- float32, in this order,
 *   nothing contracted (an identity R gives the reference's shortcut bit for bit)
 *   ray_batch [n,11] = (o, d, near 0, far 1, d / |d|)
 * img_rows / cam_rows are HOST int32 [n_img], copied into a buffer of the handle together with the images' background rows.
 * A pixel id outside [0, P) (the ids are device data) reads nothing: that ray's pixel values and direction are NaN. */
int pg_batch_gather(pg_handle* h, void* stream, const pg_image_bank* bank, const int32_t* img_rows, const int32_t* cam_rows, int64_t n_img,
                    int k, const int32_t* pixel_idxs, float* target_s, float* fgs, float* bgs, float* rays_o, float* rays_d, float* ray_batch);

/* ---- the regressor's input batch from uint8 pictures on the device: what pose_dataset, mpii_dataset and mpii_nerf_dataset
 * (run_gan.py:1636-1735) and the inner loop of train_gan (:2057-2081) do per image on the host -- slice the crop, process_sample
 * (divide by 255, normalise), skimage.transform.resize(image, (3, R, R), anti_aliasing=True) -- for a batch of (image, crop box)
 * items in one launch.  Relative to the crop (the image outside the box does not exist, as after the reference's slice):
 *   v[c,y,x] = (u8 / 255 - mean[c]) / std[c]
 *   per axis n -> R (rows n = y1 - y0, columns n = x1 - x0): sigma = max(0, (n / R - 1) / 2), r = int(4 sigma + 0.5);
 *     g = v when r = 0, else g[i] = sum_{t = -r..r} k_t v[m(i + t)], k_t = exp(-t^2 / (2 sigma^2)) / (their sum);
 *     m mirrors about the centres of the first and the last pixel (period 2 (n - 1); m = 0 for n = 1);
 *     output o samples x = (o + 0.5) n / R - 0.5 (double): i0 = floor(x), t = x - i0, (1 - t) g[m(i0)] + t g[m(i0 + 1)]
 * which is scipy.ndimage.gaussian_filter(v, (0, sigma_y, sigma_x), mode='mirror') followed by scipy.ndimage.zoom(..., order=1,
 * mode='mirror', grid_mode=True): the two calls skimage >= 0.19 makes.  Per axis the two steps run as one filter of 2 r + 2 taps
 * whose weights are formed in double and rounded to float32 once; sums are float32 fmas, columns first, then rows.
 *   pixels   device uint8, n_bytes of it: RGB-interleaved images [H,W,3] at the items' byte offsets
 *   items    HOST [n]: offset (bytes into pixels), the image's H and W, the box 0 <= x0 < x1 <= W, 0 <= y0 < y1 <= H; copied into
 *            a buffer of the handle, so every check runs on the host
 *   out_res  R;  mean, std  HOST float [3];  out  device float32 [n,3,R,R]
 * Asynchronous on `stream`; needs no loaded weights; no atomics, two calls give the same bytes, and an item's bytes do not depend
 * on the other items of the launch.  PG_EINVAL, nothing launched and nothing written, on a NULL pointer, n < 0, R outside [1, 512],
 * a mean or std that is not finite or a std of 0, an image that leaves the n_bytes of pixels, a box that is empty or leaves its
 * image, a crop side above 16 R (so sigma <= 7.5 and r <= 30).  n = 0 is PG_OK and does nothing. */
typedef struct pg_crop_item { int64_t offset; int32_t H, W, x0, y0, x1, y1; } pg_crop_item;
int pg_regressor_input(pg_handle* h, void* stream, const uint8_t* pixels, int64_t n_bytes, const pg_crop_item* items, int32_t n,
                       int32_t out_res, const float mean[3], const float std[3], float* out);

/* ---- scoring a rendered frame against its ground truth: the sums behind the PSNR, the SSIM and their foreground-masked variants of
 * the reference's two evaluate_metric functions (run_render.py:888-974 -- in the frame's 2-D box, :910-961;
 * core/utils/evaluation_helpers.py:257-385 -- whole frames, box = the frame), with the SSIM map of the vendored
 * pytorch_msssim.ssim (pytorch-msssim/pytorch_msssim/__init__.py:7-59).  The frame and the bank's bytes stay on the device, no map
 * is written, and a frame's scores are eight doubles.  Asynchronous on `stream`; needs no loaded weights; no atomics: two calls on
 * the same inputs give the same bytes.
 *   bank     imgs, masks (NULL: no foreground, the masked sums are 0), F, P, H, W; with PG_METRICS_BG also bkgds, bkgd_idxs, n_bkgd
 *   img_row  the ground-truth image, in [0, F)
 *   box      HOST int32 (x0, y0, x1, y1): top-left inclusive, bottom-right exclusive, as render_path's bboxes; h = y1 - y0, w = x1 - x0
 *   rgb      device float32 [H,W,3]: the rendered frame, H W = the bank's
 *   flags    PG_METRICS_BG: gt = mask ? img : bkgds[bkgd_idxs[img_row]] (run_render.py:935-937; masks are binary, so a selection)
 *   sums     device float64 [8] = (n, se, n_fg, se_fg, n_map, ssim, n_fg_map, ssim_fg):
 *     gt = byte / 255 rounded to float32; m = 1 where the mask byte is > 0, else 0
 *     n = 3 h w;  se = sum (gt - rgb)^2 over box and channels;  n_fg = 3 sum m;  se_fg = sum m (gt - rgb)^2
 *     map = ssim_map of pytorch_msssim.ssim(rgb, gt): 11 x 11 Gaussian (sigma 1.5, the float32 taps of gaussian(), the window their
 *     outer product), valid convolution -- (h - 10) x (w - 10) per channel -- of x, y, x^2, y^2, xy; L = 1, C1 = 1e-4, C2 = 9e-4
 *     n_map = 3 (h - 10)(w - 10);  ssim = sum map
 *     masked SSIM -- THIS PROJECT'S definition (the reference multiplies a per-image mean by a full-size mask and cannot run): a map
 *     value is weighted by the mask at its window's centre pixel, m_c(i, j) = m(y0 + 5 + i, x0 + 5 + j);
 *     n_fg_map = 3 sum m_c;  ssim_fg = sum m_c map
 *   Every sum and the map's arithmetic is float64 on the float32 frame and the bytes.  A box with h < 11 or w < 11 has no map (the
 *   reference's SSIM raises): n_map = ssim = n_fg_map = ssim_fg = 0, the first four sums are filled.
 * The host arguments are checked before anything is launched.  PG_EINVAL, nothing launched and nothing written: a NULL pointer, a
 * box that is empty or reaches outside the frame, img_row outside [0, F), H W != P, unknown flags, PG_METRICS_BG without bkgds /
 * bkgd_idxs / masks or with a background index outside the bank.  The tiles' partial sums live in a buffer of the handle: calls
 * enqueued on different streams must be ordered by the caller. */
#define PG_METRICS_BG 1
int pg_frame_metrics(pg_handle* h, void* stream, const pg_image_bank* bank, int32_t img_row, const int32_t box[4], const float* rgb,
                     int flags, double* sums);

/* The trainer's validation scoring (run_nerf.py:586-589 -> evaluation_helpers.py:257-385 with eval_both and render_factor): the
 * frame is given at the size it was rendered at, rgb_h x rgb_w <= H x W, and scored as its bilinear upsampling U to H x W; beside
 * the eight sums over `box` (pg_frame_metrics with the frame = U) come four over a second rectangle `valid` of the frame -- the
 * frame's 2-D box at the bank's resolution, whose pixels the reference's valid_masks mark.
 *   rgb      device float32 [rgb_h,rgb_w,3], 1 <= rgb_h <= H, 1 <= rgb_w <= W
 *   U        F.interpolate(mode='bilinear', align_corners=False) with the index arithmetic in double.  Per axis, n_in -> n_out, pixel d:
 *              src = max((n_in / n_out) (d + 0.5) - 0.5, 0);  i0 = min((int)src, n_in - 1);  i1 = i0 + (i0 < n_in - 1);
 *              l1 = src - i0;  l0 = 1 - l1
 *            U[y,x,c] = float32( ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d) ) with the texels a (y0,x0), b (y0,x1), c (y1,x0),
 *            d (y1,x1) widened to double, every product and sum rounded on its own.  rgb_h = H and rgb_w = W: U = rgb bit for bit.
 *   valid    HOST int32 (vx0, vy0, vx1, vy1) or NULL; x0 <= x1, y0 <= y1 (it may be empty), inside the frame; it may reach outside
 *            `box` or miss it
 *   sums     device float64 [12]: [0..7] as pg_frame_metrics, then (n_valid, se_valid, n_valid_map, ssim_valid), all 0 for NULL:
 *     n_valid = 3 |box n valid|;  se_valid = sum (gt - U)^2 over those pixels
 *     n_valid_map = 3 x the map pixels of `box` whose window-centre pixel lies in `valid`;  ssim_valid = sum map over those
 * Asynchronous on `stream`, no loaded weights, no atomics, the slot buffer and the ordering rule of pg_frame_metrics.  PG_EINVAL,
 * nothing launched and nothing written: everything pg_frame_metrics refuses, rgb_h / rgb_w outside [1, H] / [1, W], a malformed
 * valid. */
int pg_frame_metrics_val(pg_handle* h, void* stream, const pg_image_bank* bank, int32_t img_row, const int32_t box[4],
                         const float* rgb, int32_t rgb_h, int32_t rgb_w, const int32_t valid[4] /* or NULL */,
                         int flags, double* sums /* device float64 [12] */);

/* raw2outputs (nerf.py:150-205) and, if n_importance > 0, isample_from_lineseg
 * (ray_utils.py:157-201, 255-289): wave-per-ray prefix-product compositing.  The pdf follows the
 * handle: is_only weights 0.5 (max(w_l, w_k) + max(w_k, w_u)) + 0.01 with single_net. */
int pg_stage_composite(pg_handle* h, void* stream, int64_t n, int n_samples,
                       const float* ray_batch, const float* z, const float* raw,
                       float* rgb, float* disp, float* acc, float* alpha, float* weights,
                       int n_importance, float* z_fine /*[n,S+N] or NULL*/);

/* The sampling, compositing and composite-backward kernels on the caller's own buffers, with everything the render and training
 * calls can hand them (tests/test_gpu_composite_stages.py).  All check their host arguments before any launch and return
 * PG_EINVAL on: a null required pointer, n < 0, N_samples outside [2,256] (the sampler, which has no upper limit: below 2), N_importance outside {0, 2..64}, N_samples +
 * N_importance > 256, importance samples with N_samples < 3, ld_new < N_importance.  None needs loaded weights.
 *
 * pg_stage_sample_coarse_draws: pg_stage_sample_coarse with the stratified draws t_rand [n,S] (or NULL: the same call).  Chunks of
 * more than 256 rays run as two launches, partial nanmean sums then depths; PG_FLAG_STAGE_ONE_LAUNCH in `flags` (this entry point
 * only) runs the one-launch form at any chunk, so that the two can be compared on the same groups.
 *
 * pg_stage_composite_form: one composite launch in the form the caller names (not the handle's single_net).
 *   PG_COMP_PLAIN / PG_COMP_IS_ONLY: z [n,S], raw [n,S,4]; noise [n,S] and u_rand [n,N] or NULL; rgb / disp / acc / alpha /
 *     weights as pg_stage_composite; with N_importance > 0: z_fine [n,S+N] (required) and order [n,S+N] int32 (or NULL), the
 *     stable sort permutation of cat(z, new depths).  IS_ONLY draws from the is_only pdf and also stores the new depths in
 *     sample order in z_new [n,ld_new] (or NULL), columns N.. repeating the last one.  raw_new / raw_out are not read.
 *   PG_COMP_MERGED: the fine pass of the single-net pair.  z [n,S+N] the merged depths, raw [n,S,4] the coarse points' raw,
 *     raw_new [n,ld_new,4] the new points', order [n,S+N] (required, an INPUT: out-of-range entries are clamped), noise
 *     [n,S+N] or NULL; raw_out [n,S+N,4] (or NULL) receives the raw gathered by order.  u_rand, weights, z_fine, z_new are
 *     not read.
 *
 * pg_stage_composite_bwd: d_raw [n,S,4] of one composite from d_rgb [n,3] and d_acc [n] (either may be NULL: zero), the
 * backward of raw2outputs as pg_train_backward runs it per net.
 *
 * pg_stage_merged_composite_bwd: the backward of the single-net pair.  raw / d_raw [n S + n N, 4]: the coarse points' rows
 * ray-major, then the N new points of every ray; z_coarse [n,S], z_fine / order / noise1 [n,S+N], noise0 [n,S]; d_rgb / d_acc
 * of the fine maps, d_rgb0 / d_acc0 of the coarse maps, any NULL.  With N_importance = 0 the one composite is the coarse one
 * (z_fine, order, d_rgb, d_acc are not read).  d_raw is zeroed by the call, then every ray's thread adds the fine and the
 * coarse share in that order: two calls give the same bytes.  raw and d_raw must be 16-byte aligned.  The transmittances
 * [S+N][n] are kept in the handle's workspace. */
#define PG_FLAG_STAGE_ONE_LAUNCH 256
#define PG_COMP_PLAIN 0
#define PG_COMP_IS_ONLY 1
#define PG_COMP_MERGED 2
int pg_stage_sample_coarse_draws(pg_handle* h, void* stream, int64_t n, const float* ray_batch, const float* cyls,
                                 int64_t cyl_stride, int n_samples, int flags, const float* t_rand,
                                 float* near_far /*[n,2]*/, float* z /*[n,S]*/);
int pg_stage_composite_form(pg_handle* h, void* stream, int form, int64_t n, int n_samples, int n_importance,
                            const float* ray_batch, const float* z, const float* raw, const float* noise, const float* u_rand,
                            float* rgb, float* disp, float* acc, float* alpha, float* weights, float* z_fine, int32_t* order,
                            float* z_new, int ld_new, const float* raw_new, float* raw_out);
int pg_stage_composite_bwd(pg_handle* h, void* stream, int64_t n, int n_samples, const float* ray_batch, const float* z,
                           const float* raw, const float* noise, const float* d_rgb, const float* d_acc, float* d_raw);
int pg_stage_merged_composite_bwd(pg_handle* h, void* stream, int64_t n, int n_samples, int n_importance, const float* ray_batch,
                                  const float* z_coarse, const float* z_fine, const float* raw, const float* noise0,
                                  const float* noise1, const int32_t* order, const float* d_rgb, const float* d_acc,
                                  const float* d_rgb0, const float* d_acc0, float* d_raw);

/* ---- several posed people in one frame, in front of and behind each other (the reference has no counterpart: its
 * frames hold one character).  A scene is one camera and 1 <= P <= PG_SCENE_MAX_PEOPLE people; person p is a subject of the bank,
 * a pose (skts, cyl: device), a 2-D box and a frame-code index (HOST data; cam < 0: the mean code).
 *   1. Person p is rendered over ITS OWN box exactly as pg_render_frame renders it -- the same rays, `chunk`-ray nanmean groups,
 *      kernel forms and precision -- with its subject selected before the launches; the selection is the same before and after
 *      the call.  Kept per ray: the depths z_p [S_f] and the raw_p [S_f,4] the person's final maps are composited from,
 *      S_f = N_samples + N_importance (single_net: the merged raw).
 *   2. Per sample, on the person's own list: delta_i = (z_{i+1} - z_i) |d|, the last 1e10 |d|; sigma = act(raw.w / density_scale);
 *      alpha_i = 1 - exp(-sigma delta_i); c_i = sigmoid(raw.xyz) (1 + 2 rgb_eps) - rgb_eps (raw2outputs, nerf.py:150-205).
 *   3. Per pixel the lists of the people whose clipped box holds it are merged by depth: (q,k) precedes (p,i) if z_qk < z_pi, or
 *      z_qk == z_pi and (q,k) < (p,i).  In merged order T = prod_earlier (1 - alpha + 1e-10), w = alpha T, rgb_map = sum w c,
 *      depth = sum w z, Wt = sum w, acc_map = min(Wt, 1), disp_map = 1 / max(1e-10, depth / (Wt + 1e-10)) (0 where |Wt| <= 1e-8),
 *      person_acc[p] = min(sum_{i in p} w, 1): how much of person p is visible there.
 *   4. A pixel inside no box has all-zero maps; the frame is composed as pg_render_frame composes it (rgb = rgb_map + (1 - acc) bg,
 *      NaN disparity -> 0, optional uint8 frame).
 * One person gives the one-person frame; people with disjoint boxes give each box its one-person frame.
 *   person_acc device [P,H W] or NULL (0 outside a person's box); lists HOST array of 2 P device pointers or NULL (tests):
 *   lists[2 p] receives z_p [n_p,S_f], lists[2 p + 1] raw_p [n_p,S_f,4], n_p = the pixels of the clipped box, row-major; either may
 *   be NULL.  The other arguments are pg_render_frame's.
 * Asynchronous on `stream`; no atomics: two calls give the same bytes.  The lists live in a grow-only buffer of the handle
 * (20 B per sample).  PG_EINVAL with nothing launched: P outside [1, PG_SCENE_MAX_PEOPLE], a subject outside the bank,
 * N_samples + N_importance > 256, a training tape outstanding, a handle on several devices. */
#define PG_SCENE_MAX_PEOPLE 8
typedef struct pg_scene_person {
    int32_t subject;        /* in [0, pg_subject_count) */
    int32_t box[4];         /* (tl_x, tl_y, br_x, br_y), clipped to the frame */
    const float* skts;      /* device [24,4,4] */
    const float* cyl;       /* device [5] */
    float cam;              /* frame-code index (negative: the mean code) */
} pg_scene_person;
int pg_render_scene(pg_handle* h, void* stream, int H, int W, const float* c2w, const float* intrinsics, float near, float far,
                    int n_people, const pg_scene_person* people, int n_samples, int n_importance, int flags, const float* bg,
                    float base_bg, float* rgb, float* disp, float* acc, uint8_t* rgb8, float* person_acc, float* const* lists);

/* Step 3 above on the caller's own buffers (tests/test_gpu_scene_stages.py): z / raw HOST arrays of P device pointers, list p of
 * n_rows[p] (HOST) rows [.,S] / [.,S,4] (raw 16-byte aligned); rows device int32 [P,n_pix]: the row of pixel i in list p, anything
 * outside [0, n_rows[p]) = person p does not cover it; dirs device [n_pix,3]: the pixels' ray directions.  rgb [n_pix,3], disp,
 * acc [n_pix], person_acc [P,n_pix] or NULL.  The density line follows the handle's config; no loaded weights needed.  PG_EINVAL,
 * nothing launched: a null pointer, P outside [1, PG_SCENE_MAX_PEOPLE], S outside [1, 256]. */
int pg_stage_scene_composite(pg_handle* h, void* stream, int64_t n_pix, int n_people, int n_samples, const float* const* z,
                             const float* const* raw, const int64_t* n_rows, const int32_t* rows, const float* dirs, float* rgb,
                             float* disp, float* acc, float* person_acc);

/* ---- 3-D poses scored against their ground truth on the device (posegen_amd/pose_eval.py) -----------------------
 * What the reference computes per pose on the host: Criterion_MPJPE, Criterion3DPose_leastQuaresScaled and
 * Criterion3DPose_ProcrustesCorrected over `procrustes` (core/utils/evaluation_helpers.py:387-522), compute_similarity_transform and
 * reconstruction_error (run_gan.py:1380-1456), and the PCK / AUC shares of evaluate_pampjpe_from_smpl_params (:595-601).
 *
 * p, g: rows `joints` of pred, gt after row `root` of each was subtracted from it (root = -1: nothing subtracted).  All arithmetic
 * is float64 on the float32 inputs.  Per pose:
 *   raw     = mean_j |p_j - g_j|
 *   Z       = p aligned to g by `align`:  NONE      Z = p
 *                                          SCALE     Z = s p, s = <p,g> / <p,p> (no mean removed)
 *                                          BEST      Z = normX (sum s) Y0 T + muX with X = g, Y = p, X0 Y0 the centred sets scaled to
 *                                                    unit Frobenius norm, A = X0^T Y0 = U diag(s) V^T, T = V U^T (reflections allowed)
 *                                          ROTATION  as BEST, but where det T < 0 the smallest singular direction and its singular
 *                                                    value change sign: det T = +1
 *   aligned = mean_j |Z_j - g_j|,  d = sum |Z_j - g_j|^2 / sum |g_j - mean g|^2,  scale = the factor applied to p (1 for NONE)
 * per_pose [B,4] = raw, aligned, d, scale; aligned [B,J,3] = Z; joint_err [B,J] = |Z_j - g_j| (each may be NULL).
 * summary [4 + 2 T] = B, mean raw, mean aligned, mean d, then for each of the T thresholds (HOST doubles, in the inputs' unit) the
 * share of the B J joint distances STRICTLY below it: T shares of |p_j - g_j|, then T shares of |Z_j - g_j|.
 * A pose whose p or g has no spread (J = 1, all joints equal) has NaN aligned, d and scale under BEST and ROTATION (0 / 0) and a
 * valid raw; a pose with a non-finite coordinate among its selected joints or its root is NaN in every output, that pose only;
 * the means propagate NaN; a NaN distance is below no threshold.
 * Asynchronous on `stream`; no atomics, every sum in a fixed order: two calls give the same bytes, and a pose's own numbers do not
 * depend on B or on its place in the batch.  The singular value decomposition runs a fixed number of Jacobi sweeps.
 * PG_EINVAL, nothing launched and nothing written: pred, gt or summary NULL; B < 1; J outside [1, 64] (joints = NULL: J = J_in);
 * a joint or root index outside J_in; an unknown mode; T outside [0, 64]. */
#define PG_POSE_ALIGN_NONE     0  /* plain MPJPE */
#define PG_POSE_ALIGN_SCALE    1  /* Criterion3DPose_leastQuaresScaled */
#define PG_POSE_ALIGN_BEST     2  /* evaluation_helpers.procrustes, scaling=True, reflection='best' */
#define PG_POSE_ALIGN_ROTATION 3  /* run_gan.compute_similarity_transform: det(R) = +1 */
int pg_pose_scores(pg_handle* h, void* stream, int64_t B, int J_in, const float* pred, const float* gt, const int32_t* joints, int J,
                   int root, int align, const double* thresholds, int T, double* per_pose, float* aligned, float* joint_err,
                   double* summary);

/* ---- the SMPL body on the device (posegen_amd/smpl.py) -------------------------------------------------------------
 * The model as the library reads it: device arrays built once per model by the caller (posegen_amd.smpl.BodyModel).  blend and skin
 * hold the model's float32 values unchanged; rest_joints is J_regressor applied to each of the first 1 + NB blend rows in float64
 * (the rest joints are linear in beta: J = rest_joints[0] + sum_l beta_l rest_joints[1 + l], exactly). */
typedef struct pg_body_model {
    int32_t V, NB;              /* vertices >= 1; shape coefficients, 1..16 */
    const float*  blend;        /* [1+NB+207, 3V]: row 0 v_template, rows 1..NB shapedirs[:,:,l] flattened (v,xyz), then the 207 rows of posedirs as stored */
    const float*  skin;         /* [V,24] lbs_weights, treated as DENSE */
    const double* rest_joints;  /* [1+NB,24,3] */
    int32_t parents[24];        /* parents[0] = -1, parent < child */
} pg_body_model;

/* smplx.lbs.lbs(betas, pose, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, pose2rot = !pose_is_rotmat)
 * (smplx/smplx/lbs.py:152-248) followed by vertices2joints(regress, verts) (:251-268): what SMPL.forward and
 * `J_regressor @ vertices` compute in evaluate.test (run_gan.py:1584-1634) and SMPLEvalHelper + vertices2joints in
 * evaluate_pampjpe_from_smpl_params (core/utils/evaluation_helpers.py:542-612).
 *   betas     device [B,NB] (betas_stride = NB), or one row for every pose (betas_stride = 0)
 *   pose      device [B,24,3] axis-angle, or [B,24,3,3] rotation matrices with pose_is_rotmat
 *   regress   device [K,V], K in 0..64 (NULL with K = 0)
 *   verts [B,V,3], joints [B,24,3] (J_transformed), regressed [B,K,3]: device float32, each may be NULL, not all three
 * Axis-angle follows batch_rodrigues as written (:295-329): angle = |r + 1e-8|, rot_dir = r / angle, R = I + sin K + (1 - cos) K K.
 * Rodrigues, the rest joints, the chain and the relative transforms A_j (batch_rigid_transform, :345-401) are float64 on the float32
 * inputs and rounded once; blend (v_template + shapedirs beta + posedirs (R - I), one GEMM on v_mfma_f32_16x16x4_f32), skinning
 * (T = sum_j skin[v,j] A_j, T [v_posed; 1]) and regression are float32 products; the regression adds 4 vertices in float32 and
 * everything above that in float64.  Vertices and per-vertex transforms reach memory only where `verts` is given.
 * Asynchronous on `stream`; no atomics, every sum in a fixed order: two calls give the same bytes, and a pose's outputs are the same
 * bytes whatever B is and wherever the pose sits in the batch (the vertex range is cut by V alone).  A pose with a non-finite input
 * is non-finite in its own outputs only.
 * Workspace: the handle's grow-only buffer, at most 48 MiB plus the carving's alignment: a long batch is walked in slices of at most
 * 4096 poses inside the call (fewer where K times the vertex chunks, at most 256, makes a pose's partial sums large).
 * PG_EINVAL, nothing launched and nothing written: m, betas or pose NULL; all three outputs NULL; B < 1; NB outside [1, 16]; V < 1 or
 * (1 + NB + 207) 3 V >= 2^31; a NULL model array; K outside [0, 64]; K > 0 with regress NULL; regressed with K = 0; betas_stride
 * neither NB nor 0; parents not ordered parent before child from parents[0] = -1. */
int pg_smpl_forward(pg_handle* h, void* stream, const pg_body_model* m, int64_t B, const float* betas, int64_t betas_stride,
                    const float* pose, int pose_is_rotmat, const float* regress, int K, float* verts, float* joints, float* regressed);

/* The transpose of pg_smpl_forward for the same inputs: the gradients that the reference gets by autograd through
 * smplx.lbs.lbs and vertices2joints.  The forward is computed again from (betas, pose), nothing is kept between calls.
 *   betas, betas_stride, pose, pose_is_rotmat, regress, K   as for pg_smpl_forward
 *   blend_t      device [3V, 1+NB+207] float32: m->blend transposed, built once per model by the caller; NULL: the kernel reads
 *                m->blend strided (slow, the same sums)
 *   d_verts      device [B,V,3], d_joints device [B,24,3], d_regressed device [B,K,3] float32: the cotangents of the forward's three
 *                outputs; any may be NULL (zero), not all three; d_regressed requires K > 0 and regress
 *   d_betas      device [B,NB] float32, ALWAYS one row per pose (with betas_stride = 0 the caller adds the rows); may be NULL
 *   d_pose       device [B,24,3] (axis-angle: the derivative of batch_rodrigues exactly as written, angle = |r + 1e-8|, in float64,
 *                finite at r = 0) or [B,24,3,3] (pose_is_rotmat: the nine entries of every matrix are free variables, as in
 *                pg_pose_kinematics_rot_bwd; joint 0's matrix gets no pose-feature term); may be NULL, not both outputs
 * Per 64-vertex tile v_posed again (the forward's GEMM), dv = d_verts + regress^T d_regressed, d v_posed = T_R^T dv,
 * dA += skin (dv (x) [v_posed; 1]) and d feat += blend d v_posed, all on v_mfma_f32_16x16x4_f32: one tile is added in float32, tiles
 * in float64 in tile order per vertex chunk (min(tiles, 64) chunks, a function of V alone).  A closing kernel, float64, one wave per
 * pose: the chunks in chunk order, d_joints, A = [G_R | G_t - G_R J] undone, the chain walked back, dJ into d_betas through
 * rest_joints, the d feat rows, Rodrigues; rounded to float32 once.  With d_joints alone no vertex-tile kernel is launched.
 * Asynchronous on `stream`; no atomics, every sum in a fixed order: two calls give the same bytes, and a pose's rows are the same
 * bytes whatever B is and wherever the pose sits.  A non-finite value in one pose's input or cotangent stays in that pose's rows.
 * Workspace: the handle's grow-only buffer, at most 96 MiB plus the carving's alignment (a pose and chunk leave 512 doubles; a long
 * batch is walked in slices inside the call, each a whole number of rounds of one workgroup per CU where the batch is that long).
 * PG_EINVAL, nothing launched and nothing written: the cases of pg_smpl_forward (its outputs' cases apart); all three cotangents
 * NULL; d_regressed with K = 0; both outputs NULL. */
int pg_smpl_backward(pg_handle* h, void* stream, const pg_body_model* m, int64_t B, const float* betas, int64_t betas_stride,
                     const float* pose, int pose_is_rotmat, const float* regress, int K, const float* blend_t, const float* d_verts,
                     const float* d_joints, const float* d_regressed, float* d_betas, float* d_pose);

/* Mesh errors per pose: per_pose[b] = mean_v |a[b,v] - b[b,v]|, the `ume` / `pme` lines of evaluate.test (run_gan.py:1630-1631).
 *   a, b device [B,V,3] float32; per_pose device [B] float64; summary device [2] float64 = B, the mean of per_pose (may be NULL)
 * float64 arithmetic, ordered sums, no atomics; a non-finite coordinate makes its own pose NaN and the mean with it.
 * PG_EINVAL: a, b or per_pose NULL; B < 1; V < 1. */
int pg_vertex_errors(pg_handle* h, void* stream, int64_t B, int V, const float* a, const float* b, double* per_pose, double* summary);

/* pg_pose_kinematics with the rotations given: get_smpl_l2ws_torch(pose, axis_to_matrix=False) (core/utils/skeleton_utils.py:379-463),
 * which the GAN loop applies to the regressor's rotation matrices (run_gan.py:2080-2091).
 *   rotmats   device [n_poses,24,3,3] float32
 *   bone_offsets, parents, kps, skts, l2ws: as pg_pose_kinematics (HOST offsets and joint tree; device outputs, any may be NULL)
 * float64 arithmetic on the float32 matrices; float32 outputs are rounded once. */
int pg_pose_kinematics_rot(pg_handle* h, void* stream, int64_t n_poses, const float* rotmats, const double* bone_offsets,
                           const int32_t* parents, float* kps, float* skts, double* l2ws);

/* ---- training on pose error (posegen_amd/pose_losses.py) -----------------------------------------------------------
 * The transpose of pg_pose_kinematics for its `kps` output: d_bones = (d kps / d bones)^T d_kps.
 *   bones     device [n_poses,24,3] float64 axis-angle, bone_offsets / parents HOST, as in the forward
 *   d_kps     device [n_poses,24,3] float32: the cotangent of kps
 *   d_bones   device [n_poses,24,3] float64
 * The rotation map is the forward's own (rotation vector -> unit quaternion -> matrix, k = sin(theta/2) / theta); below theta = 1e-3
 * the gradient is the derivative of the series the forward uses there, written in theta^2: k = 1/2 - theta^2/48 + theta^4/3840,
 * q_w = 1 - theta^2/8 + theta^4/384 (cos(theta/2) to below 1e-22), so the gradient at a zero rotation vector is finite: the rotation
 * generators'.  No cotangents for skts / l2ws (pg_poseopt_backward has those for the training path).
 * float64 arithmetic; the forward is computed again from `bones`, nothing is kept between calls.  Asynchronous on `stream`; no
 * atomics, every sum in a fixed order: two calls give the same bytes, and a pose's rows are the same bytes whatever n_poses is and
 * wherever the pose sits.  A non-finite value in one pose stays in that pose's rows.
 * PG_EINVAL, nothing launched and nothing written: a NULL pointer, n_poses < 0, a joint that does not come after its parent. */
int pg_pose_kinematics_bwd(pg_handle* h, void* stream, int64_t n_poses, const double* bones, const double* bone_offsets,
                           const int32_t* parents, const float* d_kps, double* d_bones);

/* The transpose of pg_pose_kinematics_rot for `kps`: the nine entries of every matrix are free variables, as in the reference's
 * autograd through get_smpl_l2ws_torch(axis_to_matrix=False); the matrices are used as given, not re-orthogonalised.
 *   rotmats, d_rotmats   device [n_poses,24,3,3] float32;   d_kps device [n_poses,24,3] float32
 * float64 arithmetic on the float32 inputs, rounded once; otherwise as pg_pose_kinematics_bwd. */
int pg_pose_kinematics_rot_bwd(pg_handle* h, void* stream, int64_t n_poses, const float* rotmats, const double* bone_offsets,
                               const int32_t* parents, const float* d_kps, float* d_rotmats);

/* The pose losses of the GAN loop with their gradients.  p, g: rows `joints` of pred, gt after row `root` of each was subtracted
 * (root = -1: nothing subtracted; joints = NULL: all J_in rows), float64 on the float32 inputs, as in pg_pose_scores.  Per pose
 *   MPJPE         e_b = (1/J) sum_j |p_j - g_j|                                        (mpjpe, run_gan.py:1458-1464, :2091)
 *   NORM_MATCHED  s_b = |g|_F / |p|_F,  e_b = (1/J) sum_j |s_b p_j - g_j|              (train_spin, run_gan.py:1902-1906)
 * per_pose[b] = weight e_b.  cap = +inf keeps every pose and NaN propagates; a finite cap keeps the poses with per_pose[b] < cap
 * (strict; a NaN pose is not kept; :1907-1908).  loss = sum of the kept per_pose / n_kept: NaN when nothing is kept, as torch.mean of
 * an empty tensor is.
 *   summary   device [3] float64: loss, n_kept, B
 *   per_pose  device [B] float64, may be NULL
 *   d_pred, d_gt   device [B,J_in,3] float32, each may be NULL: the gradients of `loss` (upstream 1).  Rows that are not selected and
 *             poses that are not kept are exactly zero; the root row receives minus the sum of the selected rows' gradients; a zero
 *             distance contributes a zero gradient (as torch's norm backward); with nothing kept everything is zero.  The gradient
 *             rows of a pose that is itself non-finite are unspecified.
 * A pose with |p|_F = 0 is NaN under NORM_MATCHED, that pose only.  Asynchronous on `stream`; no atomics, every sum in a fixed
 * order: two calls give the same bytes.  Workspace: B doubles of the handle's grow-only buffer where per_pose is NULL.
 * PG_EINVAL, nothing launched and nothing written: pred, gt or summary NULL; B < 1; J outside [1, 64]; a joint or root index outside
 * J_in; a joint selected twice; an unknown kind; weight or cap NaN; cap <= 0. */
#define PG_POSE_LOSS_MPJPE        0
#define PG_POSE_LOSS_NORM_MATCHED 1
int pg_pose_loss(pg_handle* h, void* stream, int64_t B, int J_in, const float* pred, const float* gt, const int32_t* joints, int J,
                 int root, int kind, double weight, double cap, double* per_pose, double* summary, float* d_pred, float* d_gt);

/* ---- what a training step optimises (posegen_amd/train_losses.py, posegen_amd/trainer.py) ---------------------------
 * The reference Trainer's losses, pose regulariser and gradient norms (core/trainer.py:193-205, 321-443).  All three entry points:
 * asynchronous on `stream`, no host synchronisation; no atomics, every sum in a fixed order that depends on the sizes alone (not on
 * the device, not on where an array lies), so two calls give the same bytes on every machine; float64 arithmetic on the float32
 * inputs, outputs rounded once; at most three launches; nothing is kept between calls except grow-only scratch in the handle.
 * PG_EINVAL means nothing was launched and nothing written.
 *
 * pg_train_loss: Trainer._compute_nerf_loss for the fine pass and, with rgb0 / acc0, the coarse pass, summed as compute_loss sums
 * them (trainer.py:321-383).
 *   rgb_map [n,3], acc_map [n], target [n,3]   device float32;  rgb0 [n,3], acc0 [n]: both NULL = no coarse pass
 *   bgs [n,3] or NULL (then the scalar base_bg);  fgs [n] (batch['fgs'][..., 0]), may be NULL with PG_TRAIN_REG_NONE
 *   pred = rgb + (1 - acc) bg with use_background, else rgb; the loss is the mean over the 3n elements of (pred - target)^2 (MSE),
 *   |pred - target| (L1) or F.smooth_l1_loss(beta) (HUBER: quadratic strictly below beta; beta = 0 is L1); the coarse pass's loss is
 *   multiplied by coarse_weight.  PG_TRAIN_REG_BCE: acc2bce(acc, fgs, reduction='off') reg_coef per pass, i.e. the mean of
 *   -(y log(x + 1e-8) + (1 - y) log(1 - x + 1e-8)) over the rays with y < 1.0 only; with no such ray that term (and the total) is NaN
 *   and its gradient zero, the convention of pg_pose_loss.  PG_TRAIN_REG_L1 / PG_TRAIN_REG_MSE are refused: the reference calls them
 *   with reduction='off', which they answer with the unreduced tensor, and its backward() raises.
 *   summary   device [10] float64: total, rgb_loss, rgb_loss0, reg_loss, reg_loss0, psnr, psnr0, mean(acc_map), and the two passes'
 *             BCE ray counts; psnr = -10 log10(mean((pred - target)^2)) of the composited prediction whatever the loss kind; the
 *             entries of a pass or a term that is absent are 0
 *   d_rgb_map [n,3], d_acc_map [n], d_rgb0, d_acc0   device float32, each may be NULL: the gradient of `total` at upstream 1, in the
 *             shapes pg_train_backward takes, overwritten.  The L1 derivative at a zero difference is 0, as in torch.
 * A NaN in an input reaches the sums, as in the reference.  PG_EINVAL: a required pointer NULL; rgb0 without acc0 or the reverse;
 * n outside [1, 2^31 - 1]; an unknown kind; HUBER with beta < 0 or NaN; BCE without fgs; REG_L1 / REG_MSE. */
#define PG_TRAIN_LOSS_MSE   0
#define PG_TRAIN_LOSS_L1    1
#define PG_TRAIN_LOSS_HUBER 2
#define PG_TRAIN_REG_NONE 0
#define PG_TRAIN_REG_BCE  1
#define PG_TRAIN_REG_L1   2
#define PG_TRAIN_REG_MSE  3
int pg_train_loss(pg_handle* h, void* stream, int64_t n, const float* rgb_map, const float* acc_map, const float* rgb0, const float* acc0,
                  const float* target, const float* bgs, double base_bg, const float* fgs, int loss_kind, double beta, int use_background,
                  double coarse_weight, int reg_kind, double reg_coef, double* summary, float* d_rgb_map, float* d_acc_map, float* d_rgb0,
                  float* d_acc0);

/* Trainer._compute_kp_loss for opt_rot6d (trainer.py:384-443).
 *   rots [n,24,3,3], kps [n,24,3]   device float32, per ray (the pose layer's outputs)
 *   anchor_rots [N,24,3,3], anchor_kps [N,24,3]   device float32;  kp_idx HOST int32 [n], every entry in [0, N): checked before
 *             anything is launched and copied into the handle (as pg_poseopt_forward's ray_pose)
 *   The 6-D bone of a joint is the first two columns of its matrix ([..., :3, :2].flatten(-2)).  x = (anchor - bone)^2 over joints
 *   1..23; an element contributes x - tol where x > tol (strict; tol is rounded to float32 first, the value the reference compares
 *   with) and 0 elsewhere (a NaN stays a NaN); kp_loss = coef times the mean over n 23 of the per-joint sums.
 *   prev_rots, prev_kps, next_rots, next_kps (per ray, constants; all four or none) with temp_val [n] and temp_coef add
 *   temp_loss = temp_coef mean over n 24 of (sum_6 ((b - b_prev) - (b_next - b))^2 + sum_3 likewise on kps) temp_val, all 24 joints.
 *   summary   device [4] float64: kp_loss, temp_loss (0 without the term), MPJPC = mean |anchor_kps - kps| / ext_scale (no
 *             gradient), kp_loss + temp_loss
 *   d_rots [n,24,3,3], d_kps [n,24,3]   device float32, each may be NULL, overwritten: the gradient of the total.  The third column
 *             of every d_rots matrix is zero; the root joint gets only the temporal term.
 * PG_EINVAL: a required pointer NULL; n or N < 1; a kp_idx entry outside [0, N); some but not all of prev / next; the temporal term
 * without temp_val; a NaN scalar; ext_scale <= 0. */
int pg_pose_reg_loss(pg_handle* h, void* stream, int64_t n, const float* rots, const float* kps, int64_t N, const float* anchor_rots,
                     const float* anchor_kps, const int32_t* kp_idx, double tol, double coef, double ext_scale, const float* prev_rots,
                     const float* prev_kps, const float* next_rots, const float* next_kps, const float* temp_val, double temp_coef,
                     double* summary, float* d_rots, float* d_kps);

/* get_gradnorm (trainer.py:193-205) without its launch and host synchronisation per tensor.
 *   grads     HOST table of n_tensors device pointers to float32 gradients, counts HOST [n_tensors] their element counts.  A pointer
 *             need only be 4-byte aligned (a parameter may be a view): the 16-byte loads peel heads and tails, and an element's place
 *             in the sum does not depend on the alignment.
 *   out       device [2 + n_tensors] float64: total_norm = sqrt(sum_t |g_t|^2), avg_norm = sqrt(total_norm^2 / n_tensors), then every
 *             tensor's own norm
 * One difference from the reference, stated: it rounds every tensor's norm to float32 before squaring; here nothing is rounded.
 * PG_EINVAL: n_tensors outside [1, PG_GRAD_NORMS_MAX] (the reference divides by zero at 0); a NULL pointer with a positive count. */
#define PG_GRAD_NORMS_MAX 256
int pg_grad_norms(pg_handle* h, void* stream, int n_tensors, const float* const* grads, const int64_t* counts, double* out);

/* Test / measurement aid: on = 0 makes the fused 16-bit and compensated kernels compute every limb of the density input
 * for every point instead of leaving out the limbs a wave / a pass is out of cutoff range of (a joint farther than
 * cutoff_dist + 24 / (tau log2 e) has a cutoff weight 1 - sigmoid(tau (v - c)) below 2^-24, cutoff_embedder.py:139-146:
 * DESIGN.md 2.1; an embedder with tau <= 0 has no such radius: nothing is left out).  Default on.  The two settings agree to
 * ~1e-7 per skipped product. */
int pg_set_far_skip(pg_handle* h, int on);

/* The fused 16x16x32 kernel (pg_eval16r.hip; bf16 / fp16 renders of rays with >= 64 samples) leaves the colour branch --
 * view layer, rgb head -- out for a wave whose 32 points all have sigma <= 0 and writes rgb_raw = 0 for them: under the
 * ReLU density such a point composites with weight exactly +0, so the maps are bitwise the same.  Only launches of
 * pg_render_rays / pg_render_rays_train (and the frame entry points on top of them) whose raw nobody else sees do so: ReLU
 * density, no density noise (noise0 / noise1) in the call, no raw_coarse / raw_fine output.  on = 0 switches it off (tests,
 * A/B); default on.  One difference, deliberate: a non-finite colour pre-activation at an empty point gave NaN maps
 * (0 x NaN) before and gives finite ones now. */
int pg_set_empty_skip(pg_handle* h, int on);

/* Measurement aid: counts = >= 16 ZEROED 32-bit device words (or NULL: off).  While set, every pg_eval16r.hip launch of a
 * render call on this handle that takes the on-chip form with one pose and no frame codes adds the counters of
 * pg_stage_eval's dbg_stage 97 to them -- what the call's own launches skipped.  The caller owns the memory. */
int pg_debug_wave_counts(pg_handle* h, uint32_t* counts);

/* New values of a loaded net's 24 tensors (pg_load_weights order, fp32, DEVICE pointers; and of the frame codes [n_codes,16]
 * when the handle has them) between optimiser steps and a render -- the reference renders with the module it trains
 * (core/trainer.py:463); here the fused kernels' packed weight images follow the parameters.  The images of the fast paths
 * are re-formed on the device, bitwise as pg_load_weights would pack them; every other image is re-packed from refreshed host
 * copies by the first call that needs it.  Needs a prior pg_load_weights (and pg_set_framecodes) of the net; single-device
 * handles only.  Enqueued on `stream`. */
int pg_load_weights_device(pg_handle* h, void* stream, int which_net, const float* const* d_tensors, int n_tensors,
                           const float* d_codes, int n_codes);

/* Which form of the fused 16-bit kernel (pg_eval16r.hip) calls with >= 64 samples per ray take -- both compute
 * encode_inputs + NeRF.forward (core/raycasters.py:476-577, core/networks/nerf.py:90-148), they differ in where the
 * per-ray part (bone-local rays, the view layer's direction part, the frame code's part) is formed:
 *   PG_ONCHIP_RECORDS (0): per-ray records in HBM (8.75 KiB per ray) written by a record kernel in front of every launch;
 *   PG_ONCHIP_AUTO    (1): by sample count -- on chip up to 112 samples per ray, records above (the faster form of the
 *                          two on MI355X: profiles/r5_ab_onchip_by_samples.txt); the default;
 *   PG_ONCHIP_ALWAYS  (2): on chip whatever the sample count (no record workspace, a quarter of the HBM traffic at
 *                          128 + 16 samples, 2 % slower there).
 * The environment variable POSEGEN_ONCHIP = 0 / 1 / 2 sets the initial mode of handles created by the process.  The
 * compensated mode (PG_PREC_FP16C) has no per-ray records: the setting does not reach it. */
#define PG_ONCHIP_RECORDS 0
#define PG_ONCHIP_AUTO 1
#define PG_ONCHIP_ALWAYS 2
int pg_set_onchip(pg_handle* h, int mode);

/* Arithmetic of the TRAINING step (pg_train_forward / pg_train_backward), independent of the rendering precision
 * (pg_set_precision): PG_PREC_FP32 (default; the reference trains in fp32, core/trainer.py:232-275: gradients within 1e-4
 * of its autograd) or PG_PREC_BF16 (the tape and the large GEMMs' operands in bf16, fp32 accumulate: opt-in).  The mode is
 * read by pg_train_forward and recorded on the tape: a tape's backward runs in the mode its forward ran in. */
int pg_set_train_precision(pg_handle* h, int precision);

/* Optional in-library timing of the fused embed+MLP kernel (the dominant kernel): while
 * enabled, every launch is bracketed by hipEvents on the caller's stream.  pg_profile_read
 * synchronises, returns the number of launches, their summed device time [ms] and the
 * number of points they evaluated since the last read, and resets the counters. */
int pg_profile_enable(pg_handle* h, int on);
int pg_profile_read(pg_handle* h, int64_t* n_launches, double* total_ms, int64_t* n_points);
/* The same for the small per-ray record kernel that runs in front of every factorised 16-bit launch (what depends
 * on the ray only -- bone-local ray, the view layer's direction part -- computed once per ray, encoders.py:25-37,
 * cutoff_embedder.py:111-174): launches and summed device time [ms] since the last read. */
int pg_profile_read_aux(pg_handle* h, int64_t* n_launches, double* total_ms);

/* Host-only (no GPU touched): pack one net's tensors (same 24-tensor order as
 * pg_load_weights) into the weight stream and bias table the kernels consume, for tests
 * of the packing / stream-program logic.  stream_out may be NULL to query the size.
 * view_fact != 0 selects the stream of the factorised view layer the 16-bit kernels use
 * when a ray has >= 64 samples; view_fact == 3: the on-chip variant of the 16x16x32 kernel (no per-ray records);
 * view_fact == 4 with PG_PREC_FP16C: the weight image of pg_evalc2.hip (pg_program.h T; bias_out: the 16-row table).
 * PG_PREC_FP16C packs 0 (the k-major stream of pg_eval32.hip) and 4 only: 1, 2 and 3 return PG_EINVAL. */
int pg_debug_pack(const float* const* tensors, const int64_t* shapes, int n_tensors,
                  int framecode_ch, int precision, int view_fact, uint8_t* stream_out, int64_t stream_cap,
                  int64_t* stream_bytes, float* bias_out /* 82*32 floats or NULL */,
                  int32_t* chunk_bytes /* out: ring chunk size the library was built with */);

/* Host-only: the source map of a packed image -- per 16-bit (form 0, 1) or fp32 (form 2) output element (flat source offset << 2)
 * | kind (0 plain, 1 / 2 = plane 0 / 1 of the compensated pair), or -1 for a zero -- and the flat source vector it indexes (the
 * 24 tensors in pg_load_weights order, then the folded view layer's weights and bias): what pg_load_weights_device gathers from.
 * form 0: the on-chip stream of the 16x16x32 kernel, 1: pg_evalc2.hip's image, 2: the 16-row bias table. */
int pg_debug_pack_map(const float* const* tensors, const int64_t* shapes, int n_tensors, int framecode_ch, int form,
                      int32_t* map_out, int64_t map_cap, int64_t* map_n, float* src_out, int64_t src_cap, int64_t* src_n);

/* Host-only: the widening of a multires_views = 0 view weight that pg_load_weights and pg_load_weights_device apply:
 * view_w [128, 256+72+framecode_ch] -> out [128, 256+648+framecode_ch]: columns 256..327 copied (row 0 of the 4-band
 * embedding is v * w, the whole 0-band embedding), every sin/cos column zero, the frame-code columns moved behind.
 * out may be NULL to query the size (floats). */
int pg_debug_widen_views(const float* view_w, int64_t rows, int64_t cols, int framecode_ch, float* out, int64_t cap,
                         int64_t* out_n);

/* Host-only: the Y-stage weights of the factorised view layer (16-bit precisions), laid out
 * [wave 8][unit][64 lanes x 16 B] as the kernel reads them.  out may be NULL to query the size. */
int pg_debug_pack_vy(const float* const* tensors, const int64_t* shapes, int n_tensors, int framecode_ch,
                     int precision, uint8_t* out, int64_t cap, int64_t* out_bytes);

/* Compute units and maximum engine clock [kHz] of the handle's device (hipDeviceProp), for
 * re-deriving the MFMA peak on the box: n_cu x 4 SIMDs x 1024 bf16 FLOP/clk x clock. */
int pg_device_info(const pg_handle* h, int32_t* n_cu, int32_t* clock_khz);

/* Measurement aid (bench.py): the rate the handle's device SUSTAINS on bare
 * v_mfma_f32_32x32x16_{bf16 (f16 = 0), f16 (f16 = 1)}: register operands with full mantissas, 2 waves
 * per SIMD on every CU, nothing else in the loop, one launch of at least min_ms.  Synchronous.  The
 * fused kernels are priced against the nominal 2.5 PFLOP/s; this is what the chip's clock management
 * leaves of it under MFMA load on this box.  lds_fed = 1: the A operand of every MFMA is read from LDS
 * (one conflict-free ds_read_b128 per MFMA and wave, like the weight ring): the ceiling of the fused
 * 16-bit kernels' structure (32 points per wave, weights from LDS). */
int pg_calibrate_mfma(pg_handle* h, int f16, int lds_fed, double min_ms, double* tflops, double* ms);

/* Static facts for the host: bytes of the packed weight stream of one net, and the
 * MFMA instructions one 32-point group issues, for the given precision (16-bit precisions:
 * of the factorised-view program used when a ray has >= 64 samples). */
int pg_query(const pg_handle* h, int precision, int64_t* stream_bytes, int64_t* mfma_per_group);

#ifdef __cplusplus
}
#endif
#endif /* POSEGEN_HIP_H */
