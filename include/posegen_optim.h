/*
 * posegen_optim.h -- the optimiser step behind the C ABI of libposegen_hip.so: clip_grad_norm_ over the tensors of the call followed
 * by torch.optim.Adam's update of every one of them, in one call.  DESIGN.md 2.19.
 *
 * A fifth public header beside posegen_hip.h, posegen_gan.h, posegen_generator.h and posegen_regressor.h, with their conventions:
 * the function returns 0 or a negative PG_E* code and never throws (pg_last_error has the message); `pg_handle*` first and `void*
 * stream` (a hipStream_t) second; pointers are borrowed for the call; "device pointer" = memory of the handle's HIP device; calls on
 * one handle are serialised by the caller.  The ABI version does not move: nothing that posegen_hip.h declares changes.
 *
 * No atomics, no grid-wide barrier.  Every sum has a fixed order that depends on the sizes alone, so two calls give the same bytes.
 * Without clipping an element's new bytes depend on that element and its group alone: not on where the tensor lies, not on its
 * neighbours in the table.  The arguments are checked before the handle is: a refusal is a refusal with any handle.
 */
#ifndef POSEGEN_OPTIM_H
#define POSEGEN_OPTIM_H

#include "posegen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_ADAM_MAX_TENSORS 4096
#define PG_ADAM_MAX_GROUPS 64
#define PG_ADAM_SEGMENT 16384 /* elements one workgroup updates */
#define PG_ADAM_NO_CLIP (-1.0)

/* torch.optim.Adam's hyperparameters of one param_group, under torch's own checks: lr >= 0, eps >= 0, 0 <= beta < 1,
 * weight_decay >= 0 (coupled L2: added to the gradient). */
typedef struct pg_adam_group {
    double lr, beta1, beta2, eps, weight_decay;
} pg_adam_group;

/* One parameter tensor: device float32 arrays of `count` elements each, 4-byte aligned is enough (views into flat buffers at any
 * element offset are legal).  count == 0: the tensor is skipped and its pointers are not read. */
typedef struct pg_adam_tensor {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t count;
    int32_t group; /* index into `groups` */
    int32_t step;  /* the step being taken, >= 1 */
} pg_adam_tensor;

/* clip_grad_norm_(tensors, max_norm, norm_type=2, error_if_nonfinite=False) and Adam (amsgrad=False, maximize=False) on the
 * n_tensors entries of `tensors` (HOST array) with the hyperparameters of `groups` (HOST array), evaluated in double from the
 * float32 inputs:
 *   coef = min(max_norm / (|g|_2 + 1e-6), 1) over all gradients of the call; 1 with max_norm == PG_ADAM_NO_CLIP
 *   g' = coef g (+ weight_decay p);  m <- m + (g' - m)(1 - beta1);  v <- beta2 v + (1 - beta2) g'^2
 *   p <- p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps),  t = the tensor's `step`
 * p, m and v are each rounded to float32 once.  NaN and inf follow the formula: without clipping a NaN gradient element poisons its
 * own element only; a NaN norm makes coef NaN and with it every element of the call.
 * write_grads != 0: grad is overwritten with float32(coef g), what a reader of .grad sees after clip_grad_norm_; else grad is only read.
 * out: device double [2] or NULL: the total norm before clipping, and coef.
 * One launch without clipping and without `out`; otherwise three: partial sums of squares per segment of PG_ADAM_SEGMENT elements
 * in double, one workgroup that adds each tensor's segments in ascending order and folds the tensors in a fixed tree, and the update.
 * Asynchronous on `stream`: nothing is enqueued on any other stream and nothing waits for the device, except that a workspace that
 * has to grow is reallocated behind a device synchronise (grow-only: the first call of a size).
 * PG_EINVAL, nothing launched and nothing written: n_tensors outside [1, PG_ADAM_MAX_TENSORS]; n_groups outside [1,
 * PG_ADAM_MAX_GROUPS]; a NULL table; a group index out of range; step < 1; count < 0; a NULL pointer with count > 0; a pointer not
 * 4-byte aligned; out not 8-byte aligned; max_norm NaN, or negative and not PG_ADAM_NO_CLIP; lr < 0, eps < 0, a beta outside [0, 1),
 * weight_decay < 0 (NaN included); more than 2^31 - 1 segments; a NULL handle. */
int pg_adam_step(pg_handle* h, void* stream, int n_tensors, const pg_adam_tensor* tensors, int n_groups, const pg_adam_group* groups,
                 double max_norm, int write_grads, double* out);

#ifdef __cplusplus
}
#endif
#endif /* POSEGEN_OPTIM_H */
