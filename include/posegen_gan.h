/*
 * posegen_gan.h -- the adversarial game of the PoseGen loop behind the C ABI of libposegen_hip.so: the part-path pose
 * discriminators (Pos3dDiscriminator / Pos2dDiscriminator / Disc_Joint_Path, run_gan.py:982-1046) forward and backward, the
 * least-squares GAN loss with the discriminator accuracy (get_adv_loss, train_dis, get_discriminator_accuracy, :1101-1177) and the
 * pool of generated poses (Sample_from_Pool, :578-599).  DESIGN.md 2.16.
 *
 * A second public header beside posegen_hip.h, with that header's conventions: every function returns 0 or a negative PG_E* code
 * and never throws (pg_last_error has the message); `pg_handle*` first and `void* stream` (a hipStream_t) second; pointers are
 * borrowed for the call; "device pointer" = memory of the handle's HIP device; calls on one handle are serialised by the caller.
 * PG_ABI_VERSION does not move: nothing that posegen_hip.h declares changes.
 *
 * All four compute entry points are asynchronous on `stream`: nothing is enqueued on any other stream and nothing waits for the
 * device, except that a workspace that has to grow is reallocated behind a device synchronise (grow-only: the first call of a
 * size).  No atomics anywhere; every sum has a fixed order, so two calls give the same bytes.
 */
#ifndef POSEGEN_GAN_H
#define POSEGEN_GAN_H

#include "posegen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_DISC_MAX_PATHS 8
#define PG_DISC_MAX_POINTS 24
#define PG_DISC_LAYERS 5

/* One path: a five-layer LeakyReLU MLP  n_sel point_dim -> width -> width -> width -> mid -> 1  over the rows sel[0 .. n_sel) of a
 * pose, in that order (Disc_Joint_Path(num_joints, channel, channel_mid)). */
typedef struct pg_disc_path {
    int32_t n_sel;                         /* 1 .. n_points */
    int32_t sel[PG_DISC_MAX_POINTS];       /* each in [0, n_points); a row may repeat */
    int32_t width;                         /* 1 .. 2^20 */
    int32_t mid;                           /* 1 .. 2^20 */
} pg_disc_path;

typedef struct pg_disc_spec {
    int32_t n_paths;                       /* 1 .. PG_DISC_MAX_PATHS */
    int32_t n_points;                      /* 1 .. PG_DISC_MAX_POINTS: rows of a pose */
    int32_t point_dim;                     /* 3 or 2 */
    pg_disc_path path[PG_DISC_MAX_PATHS];
    float slope;                           /* LeakyReLU's negative slope (nn.LeakyReLU(): 0.01); finite and >= 0, see pg_disc_backward */
} pg_disc_spec;

/* Per path the five weights [out,in] row-major float32 and the five biases [out], nn.Linear's own layout, read where torch keeps
 * them (device pointers; there is no packed copy: the optimiser rewrites them every step).  Layer order: layer_1, layer_2,
 * layer_3, layer_last, layer_pred. */
typedef struct pg_disc_params {
    const float* w[PG_DISC_MAX_PATHS][PG_DISC_LAYERS];
    const float* b[PG_DISC_MAX_PATHS][PG_DISC_LAYERS];
} pg_disc_params;

/* The same shapes, written (not added to).  A NULL pointer = that gradient is not wanted. */
typedef struct pg_disc_grads {
    float* w[PG_DISC_MAX_PATHS][PG_DISC_LAYERS];
    float* b[PG_DISC_MAX_PATHS][PG_DISC_LAYERS];
} pg_disc_grads;

/* The tape of a forward call over B rows: per path p, in path order, the four post-activation layers h1 [B,width], h2 [B,width],
 * h3 [B,width], h4 [B,mid] one after the other, float32.  *n_floats = B * sum_p (3 width_p + mid_p).  Host only.
 * PG_EINVAL: a spec outside the limits above, B < 1, n_floats NULL. */
int pg_disc_tape_floats(const pg_disc_spec* spec, int64_t B, int64_t* n_floats);

/* pred[b,p] = path p on x[b].  x device [B,n_points,point_dim] float32, pred device [B,n_paths] float32, tape device
 * [pg_disc_tape_floats] float32 or NULL (then the activations stay in the handle's workspace).  One launch per layer for all paths:
 * float32 products with float32 accumulation on v_mfma_f32_16x16x4_f32 (K in chunks of 16 round four accumulators that are added
 * at the end), bias and LeakyReLU in the epilogue, the head a per-row reduction.  A row's pred and tape bytes depend on that row of x and the parameters alone, not on B or the row's position; a
 * non-finite row stays in its row.  Asynchronous on `stream`.
 * PG_EINVAL, nothing launched: a NULL handle, spec, params, x or pred; a spec outside its limits (a width or mid above 2^20 and a
 * negative, infinite or NaN slope among them); B < 1 or B > 64 * 65535 = 4194240 (a launch has at most 65535 row tiles of 64); a
 * NULL parameter pointer of a path in use; a misaligned array. */
int pg_disc_forward(pg_handle* h, void* stream, const pg_disc_spec* spec, const pg_disc_params* params, const float* x, int64_t B,
                    float* pred, float* tape);

/* The backward of pg_disc_forward at the cotangent d_pred [B,n_paths]: dZ = dH (tape > 0 ? 1 : slope) (at exactly 0 the slope, as
 * torch), layer by layer.  The mask is read off the TAPE's sign, not the pre-activation's: with slope >= 0 the two agree (a negative
 * z leaves z slope <= 0), with a negative slope a negative z would leave a positive tape value and the mask would say 1 where the
 * derivative is `slope`.  Hence a negative slope is refused, here and in pg_disc_forward.
 *   d_x     device [B,n_points,point_dim] or NULL.  Every element is written exactly once: the contributions of the paths that select
 *           a row are added in path order (and within a path in selection order); a row that no path selects is zero.  Bitwise the
 *           same with and without `grads`, and a row's bytes do not depend on B or its position.
 *   grads   NULL, or the gradients wanted: dW = dZ^T H_prev, db = colsum(dZ).  The rows are reduced in chunks of 64 rows (a size
 *           that depends on nothing), each chunk from a zero accumulator, the chunks' partials added in chunk order; dW in float32
 *           on the MFMA, db in double, rounded once.  A non-finite row of x does reach dW and db.
 * With d_x NULL the chain stops above layer 1; with grads NULL no weight-gradient product runs.  Workspace: the layer gradients
 * (two [B, sum_p max(width_p, mid_p)] buffers and [B, sum_p n_sel_p point_dim]) in grow-only buffers of the handle.  Asynchronous
 * on `stream`.  PG_EINVAL as pg_disc_forward, and a NULL tape or d_pred. */
int pg_disc_backward(pg_handle* h, void* stream, const pg_disc_spec* spec, const pg_disc_params* params, const float* x, int64_t B,
                     const float* tape, const float* d_pred, float* d_x, const pg_disc_grads* grads);

/* The least-squares GAN loss over n = B n_paths predictions against one label, with the discriminator accuracy:
 *   out[0] = weight mean((pred - label)^2)
 *   out[1] = the count of values with fabsf(pred - label) <= 0.5f, compared in float32 as numpy compares them in
 *            get_discriminator_accuracy (a NaN counts as wrong; numpy's `where(d > 0.5, 0, 1)` there counts it as right: the one
 *            value on which the two differ)
 *   out[2] = n
 *   d_pred  device [n] float32 or NULL: weight 2 (pred - label) / n, formed in double and rounded once
 * pred device [n] float32, out device [3] float64.  The sum is in double: thread t of one 256-thread workgroup adds elements t,
 * t + 256, ... in that order, then a fixed tree -- an order that depends on n alone.  Asynchronous on `stream`.
 * PG_EINVAL: a NULL handle, pred or out; n < 1; a NaN label or weight. */
int pg_disc_loss(pg_handle* h, void* stream, const float* pred, int64_t n, float label, double weight, double* out, float* d_pred);

/* Sample_from_Pool.__call__ for one batch at the caller's draws, with the reference's sequential meaning.
 *   pool   device [cap,row_floats] float32, of which the first `cur` rows are filled (0 <= cur <= cap); updated in place
 *   items  device [n,row_floats];  out device [n,row_floats]: what the call returns (must not overlap items or pool)
 *   swap   device [n] uint8, slot device [n] int32 in [0, cap): read only for items i with cur + i >= cap
 * While cur + i < cap item i is appended (pool row cur + i) and returned.  After that an item with swap[i] != 0 returns what pool
 * row slot[i] holds at that moment -- the latest earlier swapped item of this call with the same slot, else the pool's row as it
 * was before the call, which includes rows appended by this call -- and takes its place; the last swapped item of a slot is what the
 * pool keeps.  Other items pass through.  The caller advances cur by min(n, cap - cur).  One launch, no atomics: a workgroup per
 * item scans the other items' draws.  A slot outside [0, cap) is treated as no swap.  Asynchronous on `stream`.
 * PG_EINVAL: a NULL handle or array; cap < 1 or cap > INT32_MAX (slots are int32); row_floats < 1; n < 1 or n > 8192 (the items'
 * effective slots sit in the workgroup's LDS, 4 bytes each); cur outside [0, cap]; a misaligned array. */
int pg_pool_exchange(pg_handle* h, void* stream, float* pool, int64_t cap, int32_t row_floats, int64_t cur, const float* items, int64_t n,
                     const uint8_t* swap, const int32_t* slot, float* out);

#ifdef __cplusplus
}
#endif
#endif /* POSEGEN_GAN_H */
