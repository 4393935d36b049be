/*
 * fedmlp_hip_drift.h -- client-drift correction: the four entry points behind FedProx and SCAFFOLD (conventions: fedmlp_hip.h).
 *
 * Like the RoFL client's two they live in a header of their own, with their own ctypes table (fedmlp_amd/_lib.py:
 * DRIFT_SYMBOLS) and their own Python wrappers (fedmlp_amd/drift.py): fedmlp_hip.h's entry points are a closed list that the
 * test suite enumerates name by name.  tests/test_drift_cpu.py holds header = table = exports for these four.
 *
 * While a correction is installed, every optimizer step of the handle -- the fused fm_step_*, fm_backward_step, fm_adam_step,
 * fm_adamw_step, fm_sgd_step and the three fm_*_step_groups -- is preceded by ONE launch on the engine's stream that writes a
 * corrected copy r of the gradient g the step would have read, and the optimizer kernel reads r.  Per element of the trainable
 * arena, in fp32, every operation rounded on its own (no fused multiply-add), in this order:
 *     r = g
 *     mu != 0 :  d = p - a;  m = mu * d;  r = r + m        p the weights before the step, a the anchor: FedProx
 *     shift   :  r = r + s                                 SCAFFOLD's c - c_i
 *     track   :  S = S + g                                 the raw gradient, before correction
 * g is never written: fm_get_grads, fm_grad_norm and the clips keep seeing the raw gradient, and a clip therefore acts before
 * the correction.  Under a requires_grad mask (fm_set_trainable) the frozen entries get r = 0 and no sum.  A handle that never
 * installs a correction runs the launches it always ran, with the same bits.  A step the optimizer skips (an empty
 * accumulator) is not corrected and not counted.
 * All device tensors are in net.grads() layout (fm_get_grads: state_dict order, fm_state_sizes' float count, the BatchNorm
 * running statistics' slots ignored on input and zero on output).  Everything is enqueued on the engine's stream; nothing
 * synchronises.  The four arenas behind this (anchor, shift, running sum, corrected gradient: the trainable arena's size each)
 * are allocated by the first install that needs them and freed by fm_destroy.
 */
#ifndef FEDMLP_HIP_DRIFT_H
#define FEDMLP_HIP_DRIFT_H

#include "fedmlp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Install a correction.  The anchor a becomes a copy of the student's parameters as they are now (a later fm_set_state does not
 * move it); shift_dev (may be NULL: no shift) is copied, so the caller's tensor is free once the call is enqueued; the running
 * sum and the step count start at zero.  track != 0 keeps the running sum of raw gradients for fm_drift_end.
 * FM_ERR_ARG, with nothing enqueued: a correction is already installed; mu negative or not finite; mu == 0 with no shift and
 * track == 0 (nothing to install).  fm_adam_reset and the other optimizer resets do not touch an install. */
int fm_drift_begin(fm_engine* e, float mu, const float* shift_dev, int32_t track);
/* The corrected gradient r of the most recent optimizer step -> out_dev.  FM_ERR_ARG before the first step since fm_drift_begin. */
int fm_drift_last(fm_engine* e, float* out_dev);
/* Uninstall.  mean_dev (may be NULL) receives S / (float)K, one IEEE division per element, K the optimizer steps since
 * fm_drift_begin -- zeros when K == 0 or the install did not track.  steps_host (may be NULL) receives K.
 * FM_ERR_ARG when no correction is installed. */
int fm_drift_end(fm_engine* e, float* mean_dev, int64_t* steps_host);
/* 1 while a correction is installed, else 0 */
int fm_drift_active(fm_engine* e);

#ifdef __cplusplus
}
#endif

#endif /* FEDMLP_HIP_DRIFT_H */
