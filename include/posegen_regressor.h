/*
 * posegen_regressor.h -- the regression head of the SPIN / HMR regressor behind the C ABI of libposegen_hip.so: what HMR.forward
 * (run_gan.py:1343-1356) does after the ResNet trunk has produced xf [B,n_feat] -- n_iter rounds of cat([xf, state]) -> fc1 -> Dropout
 * -> fc2 -> Dropout -> decpose / decshape / deccam -> residual add -- and rot6d_to_rotmat (:1188-1202), forward and backward.
 * DESIGN.md 2.18.
 *
 * A fourth public header beside posegen_hip.h, posegen_gan.h and posegen_generator.h, with their conventions: every function returns
 * 0 or a negative PG_E* code and never throws (pg_last_error has the message); `pg_handle*` first and `void* stream` (a hipStream_t)
 * second; pointers are borrowed for the call; "device pointer" = memory of the handle's HIP device; calls on one handle are
 * serialised by the caller.  The ABI version does not move: nothing that posegen_hip.h declares changes.
 *
 * The two compute entry points are asynchronous on `stream`: nothing is enqueued on any other stream and nothing waits for the
 * device, except that the backward's workspace, when it has to grow, is reallocated behind a device synchronise (grow-only: the first
 * call of a size).  No atomics, no grid-wide barrier.  Nothing couples the rows of a batch in the forward: a row's bytes depend on
 * that row, its masks and the parameters alone.  Every sum has a fixed order that depends on the sizes alone, so two calls give the
 * same bytes.  The arguments are checked before the handle is: a refusal is a refusal with any handle.
 *
 * The state of a row is s = [pose (6 n_joints), shape (n_shape), cam (n_cam)], S = 6 n_joints + n_shape + n_cam columns, in the
 * order of the reference's torch.cat.
 */
#ifndef POSEGEN_REGRESSOR_H
#define POSEGEN_REGRESSOR_H

#include "posegen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_HMR_MAX_FEAT 4096
#define PG_HMR_MAX_HIDDEN 2048
#define PG_HMR_MAX_JOINTS 64
#define PG_HMR_MAX_SHAPE 64
#define PG_HMR_MAX_CAM 16
#define PG_HMR_MAX_ITER 8
#define PG_HMR_MAX_ROWS 1048576

typedef struct pg_hmr_spec {
    int32_t n_feat;                        /* F, 1 .. PG_HMR_MAX_FEAT: columns of xf (HMR: 2048) */
    int32_t n_hidden;                      /* H, 1 .. PG_HMR_MAX_HIDDEN: width of fc1 and fc2 (1024) */
    int32_t n_joints;                      /* J, 1 .. PG_HMR_MAX_JOINTS: the pose state has 6 J columns (24) */
    int32_t n_shape;                       /* 0 .. PG_HMR_MAX_SHAPE (10) */
    int32_t n_cam;                         /* 0 .. PG_HMR_MAX_CAM (3) */
    int32_t n_iter;                        /* 1 .. PG_HMR_MAX_ITER rounds (3) */
    float p_drop;                          /* nn.Dropout's p, in [0, 1) (0.5); applied only where masks are given */
} pg_hmr_spec;

/* Device pointers into the five nn.Linears where torch keeps them (no packed copy: the optimiser rewrites them every step), all
 * float32 row-major: fc1_w [H, F + S] (its first F columns meet xf, the last S the state), fc1_b [H], fc2_w [H,H], fc2_b [H],
 * decpose_w [6J,H], decpose_b [6J], decshape_w [n_shape,H], decshape_b [n_shape], deccam_w [n_cam,H], deccam_b [n_cam].  The
 * pointers of a decoder with no columns (n_shape = 0, n_cam = 0) are not read and may be NULL. */
typedef struct pg_hmr_params {
    const float* fc1_w;
    const float* fc1_b;
    const float* fc2_w;
    const float* fc2_b;
    const float* decpose_w;
    const float* decpose_b;
    const float* decshape_w;
    const float* decshape_b;
    const float* deccam_w;
    const float* deccam_b;
} pg_hmr_params;

/* The gradients of the same ten, written (not added to).  A NULL pointer = that gradient is not wanted. */
typedef struct pg_hmr_grads {
    float* fc1_w;
    float* fc1_b;
    float* fc2_w;
    float* fc2_b;
    float* decpose_w;
    float* decpose_b;
    float* decshape_w;
    float* decshape_b;
    float* deccam_w;
    float* deccam_b;
} pg_hmr_grads;

/* The tape of a forward over B rows, float32, in this order:
 *   P [B,H]                          xf W1[:, :F]^T + b1, formed once
 *   s_i [B,S], i = 0 .. n_iter       the state before round i; s_{n_iter} is the final one
 *   h1_i [B,H], h2_i [B,H] per round, i = 0 .. n_iter - 1, after dropout
 * *n_floats = B H + (n_iter + 1) B S + 2 n_iter B H.
 * Host only.  PG_EINVAL: a spec outside its limits, B < 1 or B > PG_HMR_MAX_ROWS, a NULL result pointer. */
int pg_hmr_tape_size(const pg_hmr_spec* spec, int64_t B, int64_t* n_floats);

/* The head on xf [B,F] (device float32).  init: the state before round 0 (the reference's init_pose / init_shape / init_cam side by
 * side), device float32 [S] shared by all rows (init_per_row == 0) or [B,S] (init_per_row != 0).
 *   P = xf W1[:, :F]^T + b1 once; per round i:  h1_i = drop(P + s_i W1[:, F:]^T),  h2_i = drop(h1_i W2^T + b2),
 *   s_{i+1} = s_i + (h2_i Wd^T + bd), Wd the three decoders read through their own pointers.  There is no non-linearity between fc1
 *   and fc2: the reference has none.
 * Every product runs in float32 on v_mfma_f32_16x16x4_f32: a wave owns a 16 x 16 tile of the result, K in chunks of 16 round four
 * accumulators that are added as a tree, the bias (or the residual operand) added after the tree: the order depends on K alone.
 * masks: device uint8 [n_iter, 2, B, H] (round, then drop1 / drop2), non-zero = kept: a kept element is fl32(x fl32(1 / (1 - p_drop))),
 * a dropped one is +0.  masks == NULL is eval mode: no dropout, and a row's bytes do not depend on B or on the row's position.
 * rotmat [B,J,3,3]: rot6d_to_rotmat of the final pose state in the reference's layout -- of a joint's six numbers a1 = elements
 * 0, 2, 4 and a2 = elements 1, 3, 5; b1 = a1 / max(|a1|, 1e-12), b2 the same normalisation of a2 - (b1 . a2) b1, b3 = b1 x b2, the
 * columns of R are b1, b2, b3 -- in double from the float32 state, rounded once; a1 = 0 gives the reference's zeros, not NaN.
 * shape [B,n_shape] and cam [B,n_cam]: those columns of the final state.  rotmat, shape and cam may each be NULL: not written.
 * tape: device [n_floats] (pg_hmr_tape_size).  A NaN row of xf stays in its row.  Asynchronous on `stream`.
 * PG_EINVAL, nothing launched and nothing written: a NULL spec, params, xf, init or tape; a NULL parameter pointer of a tensor in
 * use; a misaligned array; a spec outside its limits (a p_drop that is not finite or outside [0, 1) among them); B < 1 or B >
 * PG_HMR_MAX_ROWS = 1048576; a NULL handle. */
int pg_hmr_head_forward(pg_handle* h, void* stream, const pg_hmr_spec* spec, const pg_hmr_params* params, const float* xf,
                        const float* init, int32_t init_per_row, const uint8_t* masks, int64_t B, float* tape, float* rotmat,
                        float* shape, float* cam);

/* The backward of pg_hmr_head_forward from its tape, with the forward's xf and masks (NULL = it ran in eval mode).  Cotangents:
 * d_rotmat [B,J,3,3], d_shape [B,n_shape], d_cam [B,n_cam], each may be NULL (= zero), not all three.  The cotangent of the final
 * pose state is the autograd of the rot6d expression above, clamp included (a norm below 1e-12 passes g / 1e-12), in double, rounded
 * once.  Then round by round from the last:  d_h2 = d_s Wd,  dz2 = drop'(d_h2),  dz1 = drop'(dz2 W2),  d_s <- d_s + dz1 W1[:, F:]
 * on the forward's tile code, the masks and the scale re-applied from `masks`.  One grouped launch at the end forms every wanted
 * weight gradient as one product over the n_iter B stacked rows (round-major; rows in chunks of 64, each from a zero accumulator,
 * the partials added in chunk order), d_fc1_w[:, :F] = D^T xf and d_xf = D W1[:, :F] with D = sum_i dz1_i added in round order as the
 * operand is loaded (H in chunks of 64 for d_xf), and the bias gradients as column sums over the stacked rows in double, rounded
 * once.  d_xf [B,F] and d_init [B,S] (the cotangent of the state before round 0, per row also where the forward shared one init)
 * and every entry of grads (grads NULL = none) may be NULL: that product does not run and the others' bytes do not change.
 * Workspace: d_s, dz2 and dz1 of every round in a grow-only buffer of the handle.  Asynchronous on `stream`.
 * PG_EINVAL as pg_hmr_head_forward, and: no cotangent at all. */
int pg_hmr_head_backward(pg_handle* h, void* stream, const pg_hmr_spec* spec, const pg_hmr_params* params, const float* xf,
                         const uint8_t* masks, int64_t B, const float* tape, const float* d_rotmat, const float* d_shape,
                         const float* d_cam, const pg_hmr_grads* grads, float* d_xf, float* d_init);

#ifdef __cplusplus
}
#endif
#endif /* POSEGEN_REGRESSOR_H */
