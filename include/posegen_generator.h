/*
 * posegen_generator.h -- the pose generator of the PoseGen loop behind the C ABI of libposegen_hip.so: the noise MLPs of
 * BAGenerator and RTGenerator (run_gan.py:767-980; five layers of Linear -> BatchNorm1d -> LeakyReLU each, the BatchNorm in
 * training or in eval mode) forward and backward, the bone-angle head with its backward, and the rotation / translation head.
 * DESIGN.md 2.17.
 *
 * A third public header beside posegen_hip.h and posegen_gan.h, with their conventions: every function returns 0 or a negative
 * PG_E* code and never throws (pg_last_error has the message); `pg_handle*` first and `void* stream` (a hipStream_t) second;
 * pointers are borrowed for the call; "device pointer" = memory of the handle's HIP device; calls on one handle are serialised by
 * the caller.  The ABI version does not move: nothing that posegen_hip.h declares changes.
 *
 * The five compute entry points are asynchronous on `stream`: nothing is enqueued on any other stream and nothing waits for the
 * device, except that a workspace that has to grow is reallocated behind a device synchronise (grow-only: the first call of a
 * size).  No atomics, no grid-wide barrier: BatchNorm couples the rows of a batch only within a column, and the workgroup that owns
 * a tile of 16 columns walks all B rows.  Every sum has a fixed order that depends on B alone, so two calls give the same bytes.
 * The arguments are checked before the handle is: a refusal is a refusal with any handle.
 */
#ifndef POSEGEN_GENERATOR_H
#define POSEGEN_GENERATOR_H

#include "posegen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_GEN_MAX_TRUNKS 4
#define PG_GEN_MAX_STAGES 4
#define PG_GEN_MAX_LAYERS 9                /* 1 + 2 PG_GEN_MAX_STAGES */
#define PG_GEN_MAX_DIM 512                 /* nz and width: a [16, K] weight slab sits in the workgroup's LDS */
#define PG_GEN_MAX_ROWS 1048576            /* B: one workgroup walks every row of its 16 columns */
#define PG_GEN_MAX_JOINTS 64

/* One trunk: nz -> width, then n_stages blocks of two width -> width layers (run_gan.py's `Linear`), every layer a
 * Linear -> BatchNorm1d -> LeakyReLU: 1 + 2 n_stages BatchNorm layers. */
typedef struct pg_gen_trunk {
    int32_t nz;                            /* 1 .. PG_GEN_MAX_DIM: columns of the trunk's noise */
    int32_t width;                         /* 1 .. PG_GEN_MAX_DIM */
    int32_t n_stages;                      /* 0 .. PG_GEN_MAX_STAGES */
} pg_gen_trunk;

typedef struct pg_gen_spec {
    int32_t n_trunks;                      /* 1 .. PG_GEN_MAX_TRUNKS */
    pg_gen_trunk trunk[PG_GEN_MAX_TRUNKS];
    float slope;                           /* LeakyReLU's negative slope (nn.LeakyReLU(): 0.01); finite and >= 0: a negative slope would
                                              turn the sign that posegen_gan.h's masks are read from, and is refused here as there */
    float eps;                             /* BatchNorm1d's eps (1e-5); finite and > 0 */
    float momentum;                        /* BatchNorm1d's momentum (0.1); in [0, 1] */
} pg_gen_spec;

/* Per trunk and layer the device pointers into the nn.Linear / nn.BatchNorm1d tensors where torch keeps them (there is no packed
 * copy: the optimiser rewrites them every step): w [out,in] row-major, b [out], gamma [out], beta [out] float32, and the running
 * statistics [out] float32, which a training-mode forward updates in place.  Layer order: w1 / batch_norm1 (the stem), then per
 * stage w1 / batch_norm1, w2 / batch_norm2. */
typedef struct pg_gen_params {
    const float* w[PG_GEN_MAX_TRUNKS][PG_GEN_MAX_LAYERS];
    const float* b[PG_GEN_MAX_TRUNKS][PG_GEN_MAX_LAYERS];
    const float* gamma[PG_GEN_MAX_TRUNKS][PG_GEN_MAX_LAYERS];
    const float* beta[PG_GEN_MAX_TRUNKS][PG_GEN_MAX_LAYERS];
    float* running_mean[PG_GEN_MAX_TRUNKS][PG_GEN_MAX_LAYERS];
    float* running_var[PG_GEN_MAX_TRUNKS][PG_GEN_MAX_LAYERS];
} pg_gen_params;

/* The gradients of w, b, gamma and beta, written (not added to).  A NULL pointer = that gradient is not wanted. */
typedef struct pg_gen_grads {
    float* w[PG_GEN_MAX_TRUNKS][PG_GEN_MAX_LAYERS];
    float* b[PG_GEN_MAX_TRUNKS][PG_GEN_MAX_LAYERS];
    float* gamma[PG_GEN_MAX_TRUNKS][PG_GEN_MAX_LAYERS];
    float* beta[PG_GEN_MAX_TRUNKS][PG_GEN_MAX_LAYERS];
} pg_gen_grads;

/* The tape of a trunk forward over B rows.
 *   floats   per trunk, in trunk order, per layer, in layer order:  Z [B,width] (the Linear's output, before the BatchNorm),
 *            scale [width], shift [width].  The layer's activation is lrelu(fmaf(Z, scale, shift)) and is never stored.
 *            *n_floats = sum_t layers_t (B + 2) width_t.
 *   doubles  per trunk, per layer:  mean [width], var [width] (the biased variance; in eval mode the running statistics).
 *            *n_doubles = sum_t layers_t 2 width_t.
 * Host only.  PG_EINVAL: a spec outside the limits above, B < 1 or B > PG_GEN_MAX_ROWS, a NULL result pointer. */
int pg_gen_tape_size(const pg_gen_spec* spec, int64_t B, int64_t* n_floats, int64_t* n_doubles);

/* Every trunk t with noise[t] != NULL on its noise [B,nz_t] (device float32); `noise` is a host array of n_trunks device pointers,
 * a NULL entry leaves that trunk and its part of the tape untouched.  One launch per layer for all trunks.  A workgroup of 16 waves
 * owns 16 output columns: Z[:, tile] = H_prev W[tile, :]^T + b in float32 on v_mfma_f32_16x16x4_f32, K in chunks of 16 round four
 * accumulators that are added as a tree, so a row's Z bytes depend on that row of H_prev and the parameters alone.  H_prev is formed
 * from the previous layer's Z, scale and shift while the operand is loaded.
 *   training != 0   the column mean and the biased variance of the workgroup's own Z in double, two passes (the mean, then the
 *                   centred squares); scale = gamma / sqrt(var + eps) and shift = beta - mean scale formed in double and rounded
 *                   once; running_mean and running_var updated in place by torch's rule (momentum, the unbiased variance).
 *                   A non-finite row makes the whole trunk non-finite, as in torch, and leaves the other trunks alone.
 *   training == 0   scale and shift from the running statistics; nothing is reduced, nothing but the tape is written, and a row's
 *                   bytes do not depend on B, on the row's position or on the other rows.
 * tape device [n_floats] float32, stats device [n_doubles] float64 (pg_gen_tape_size).  Asynchronous on `stream`.
 * PG_EINVAL, nothing launched and nothing written: a NULL spec, params, noise, tape or stats; no trunk with noise; a spec outside
 * its limits (a negative or non-finite slope among them); B < 1 or B > PG_GEN_MAX_ROWS = 1048576; training with B < 2 (torch
 * raises); a NULL parameter pointer of a trunk in use; a misaligned array; a NULL handle. */
int pg_gen_trunk_forward(pg_handle* h, void* stream, const pg_gen_spec* spec, const pg_gen_params* params, const float* const* noise,
                         int64_t B, int32_t training, float* tape, double* stats);

/* The backward of a training-mode pg_gen_trunk_forward.  training: the mode of the forward call that wrote `tape` and `stats`, as the
 * caller passed it there; 0 is refused (the backward of eval mode is not built).  The library keeps no record of tapes: a flag that
 * does not match the tape gives a meaningless gradient.  d_out: a host array of n_trunks device pointers, the cotangent of trunk
 * t's output [B,width_t] or NULL: such a trunk is skipped entirely.  noise: as in the forward (read for the stem's dW; required for
 * every trunk with a cotangent).  One launch per layer: the workgroup that owns 16 columns of layer l forms dH_l[:, tile] =
 * dZ_{l+1} W_{l+1}[:, tile] (the last layer: the cotangent), recomputes the LeakyReLU mask with the forward's own expression
 * (fmaf(Z, scale, shift) > 0 ? 1 : slope) and x^ = (Z - mean) / sqrt(var + eps) from the tape, sums d_beta = sum dY and d_gamma =
 * sum dY x^ over the rows in double, and writes dZ_l = gamma / sqrt(var + eps) / B (B dY - d_beta - x^ d_gamma), formed in double from
 * the tape's doubles (not from the rounded float32 scale) and rounded once.  One grouped launch at the end forms
 * every wanted dW_l = dZ_l^T H_{l-1} (H recomputed on load; rows in chunks of 64, each from a zero accumulator, the partials added
 * in chunk order) and db_l = colsum(dZ_l) in double, rounded once.  A NULL gradient pointer suppresses that product and leaves the
 * other results' bytes unchanged; grads NULL = none.  Workspace: dZ of every layer in a grow-only buffer of the handle.
 * Asynchronous on `stream`.
 * PG_EINVAL as pg_gen_trunk_forward, and: no trunk with a cotangent; training == 0. */
int pg_gen_trunk_backward(pg_handle* h, void* stream, const pg_gen_spec* spec, const pg_gen_params* params, const float* const* noise,
                          int64_t B, int32_t training, const float* tape, const double* stats, const float* const* d_out,
                          const pg_gen_grads* grads);

/* BAGenerator's head on trunk `trunk` of `tape`:  y = H w2^T + b2  [B,4J] on the same tile code (no BatchNorm), then per joint
 * a = y[b,j,0:3], theta = y[b,j,3]:  pose[b,j,:] = a / |a| theta, joint 0 times 6.28f (the reference's literal 3.14*2), in float32
 * in the reference's order of operations.  |a| = 0 gives NaN, as the reference does.  w2 device [4J,width], b2 [4J]; y device
 * [B,4J] (the head's tape: its backward reads it), pose device [B,J,3].  J in 1 .. PG_GEN_MAX_JOINTS.  Asynchronous on `stream`.
 * PG_EINVAL: a NULL or misaligned array, a spec outside its limits, trunk outside [0, n_trunks), J or B outside their limits. */
int pg_gen_ba_head_forward(pg_handle* h, void* stream, const pg_gen_spec* spec, int32_t trunk, const float* tape, int64_t B, int32_t J,
                           const float* w2, const float* b2, float* y, float* pose);

/* The backward of pg_gen_ba_head_forward at the cotangent d_pose [B,J,3]: with s = 6.28f for joint 0 and 1 otherwise, a^ = a / |a|
 * and g = d_pose[b,j]:  d a = s theta (g - a^ (a^ . g)) / |a|,  d theta = s a^ . g;  then d_w2 = dy^T H [4J,width], d_b2 =
 * colsum(dy) [4J] (in double, rounded once) and d_h = dy w2 [B,width], the cotangent of the trunk's output.  d_w2, d_b2 and d_h may
 * each be NULL: that product does not run and the others' bytes do not change.  Workspace: dy [B,4J] in a grow-only buffer of the
 * handle.  Asynchronous on `stream`.  PG_EINVAL as the forward. */
int pg_gen_ba_head_backward(pg_handle* h, void* stream, const pg_gen_spec* spec, int32_t trunk, const float* tape, int64_t B, int32_t J,
                            const float* w2, const float* y, const float* d_pose, float* d_w2, float* d_b2, float* d_h);

/* RTGenerator's head, one wave per pose, forward only (the loop never differentiates R and T).  With r = the output of trunk
 * `trunk_r` itself (w2_R is never applied in the reference; width >= 7) and eps [B,3] the caller's standard-normal draws:
 *   axis = r[0:3] + r[3:6]^2 eps;  rotation vector = axis / |axis| r[6];  R = its matrix through the unit quaternion (pg_kin.h's
 *   route, which is pytorch3d.axis_angle_to_matrix's), in double, rounded once;
 *   t = h_T w2_t^T + b2_t with h_T the output of trunk `trunk_t`, t[2] <- t[2]^2;
 *   pose_rt[b,j] = R (x[b,j] - x[b,0]) + t.
 * w2_t device [3,width], b2_t [3], x device [B,J,3]; R device [B,3,3], T device [B,3], pose_rt device [B,J,3].  Asynchronous on
 * `stream`.  PG_EINVAL: a NULL or misaligned array, a spec outside its limits, a trunk index outside [0, n_trunks), the R trunk
 * narrower than 7, J or B outside their limits. */
int pg_gen_rt_head(pg_handle* h, void* stream, const pg_gen_spec* spec, int32_t trunk_r, int32_t trunk_t, const float* tape, int64_t B,
                   int32_t J, const float* w2_t, const float* b2_t, const float* eps, const float* x, float* R, float* T, float* pose_rt);

#ifdef __cplusplus
}
#endif
#endif /* POSEGEN_GENERATOR_H */
