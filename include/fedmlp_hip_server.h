/*
 * fedmlp_hip_server.h -- server optimizers: FedAvgM, FedAdagrad, FedAdam and FedYogi (Reddi et al., Adaptive Federated
 * Optimization, ICLR 2021) on the engine's resident model (conventions: fedmlp_hip.h).
 *
 * Like the RoFL client's and the drift correction's entry points they live in a header of their own, with their own ctypes table
 * (fedmlp_amd/_lib.py: SERVER_SYMBOLS) and their own Python wrappers (fedmlp_amd/server_opt.py): fedmlp_hip.h's entry points are
 * a closed list that the test suite enumerates name by name.  tests/test_server_opt_cpu.py holds header = table = exports.
 *
 * The aggregation of a round leaves the weighted mean a of the client models in the engine's state.  fm_server_opt_step treats
 * d = a - x, x the global model the round started from, as a pseudo-gradient and takes one momentum or adaptive step from x, in
 * ONE launch on the engine's stream.  Per element of the parameter arena, in fp32, every operation rounded on its own (no fused
 * multiply-add), IEEE division and square root, in this order:
 *     d  = a - x
 *     m  : AVGM     m = beta1*m + d
 *          others   t = beta1*m ; u = omb1*d ; m = t + u            omb1 = 1.0f - beta1, formed once on the host in fp32
 *     v  : ADAGRAD  q = d*d ; v = v + q
 *          ADAM     q = d*d ; t = beta2*v ; u = omb2*q ; v = t + u   omb2 = 1.0f - beta2, likewise
 *          YOGI     q = d*d ; s = sign(v - q)  (sign(0) = 0) ; u = omb2*q ; u = u*s ; v = v - u
 *     x' : AVGM     t = lr*m ; x' = x + t
 *          others   r = sqrt(v) ; r = r + tau ; t = lr*m ; t = t / r ; x' = x + t
 * No bias correction (the paper has none).  x' replaces a in the engine's state, m and v are updated in place, x is only read.
 * The BatchNorm running statistics and the num_batches_tracked counters are not parameters: they stay the aggregate's plain
 * averages (x' = a there, which in place is no work at all).  Where a and x are both zero -- the padding of the matrices --
 * x' stays an exact zero.  A handle that never installs a server optimizer runs the launches it always ran, with the same bits.
 * The moments are two arenas of the parameter arena's size, allocated by the first install and freed by fm_destroy;
 * fm_set_state, the optimizer resets and fm_drift_* do not touch an install.  Everything is enqueued on the engine's stream;
 * nothing synchronises.
 */
#ifndef FEDMLP_HIP_SERVER_H
#define FEDMLP_HIP_SERVER_H

#include "fedmlp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FM_SERVER_AVGM 0
#define FM_SERVER_ADAGRAD 1
#define FM_SERVER_ADAM 2
#define FM_SERVER_YOGI 3

/* rule: 0 AVGM (beta1 is the momentum; beta2 and tau are ignored), 1 ADAGRAD (beta2 ignored), 2 ADAM, 3 YOGI */
typedef struct { int32_t rule; float lr, beta1, beta2, tau; } fm_server_opt;

/* Install.  m = 0; for the adaptive rules v = tau*tau rounded to fp32 (the paper's v_{-1} >= tau^2); the step count is zero.
 * FM_ERR_ARG, with nothing enqueued: an install is already there; an unknown rule; lr negative or not finite; a beta the rule
 * reads outside [0, 1); tau not finite or <= 0 for an adaptive rule. */
int fm_server_opt_begin(fm_engine* e, const fm_server_opt* hp);
/* One server step: the engine's state a -> x' (see above).  x_old_dev: x in fm_state_device's layout and length, a device buffer
 * that is not the engine's own state.  delta_norm_dev (may be NULL) receives |d|_2 as one double: over the real state_dict
 * elements of the parameters only (layout padding and gaps never enter), fp64 sums in a fixed order, no atomics -- the same
 * operands give the same 8 bytes.  The step changes the student's weights: every derived copy is marked stale exactly as
 * fm_state_scale and fm_fedavg_allreduce mark it.
 * FM_ERR_ARG, with nothing enqueued and nothing moved: nothing installed; x_old_dev null or inside the engine's state buffer. */
int fm_server_opt_step(fm_engine* e, const float* x_old_dev, double* delta_norm_dev);
/* The moments in net.grads() layout (fm_optim_get_state's change of layout: the running statistics' slots zero on output and
 * ignored on input) and the number of steps since fm_server_opt_begin.  Any of the three pointers of get may be NULL; AVGM has
 * no second moment: v comes out as zeros and set ignores v_dev (which may be NULL).
 * FM_ERR_ARG: nothing installed; set: m_dev null, v_dev null under an adaptive rule, steps < 0. */
int fm_server_opt_get_state(fm_engine* e, float* m_dev, float* v_dev, int64_t* steps_host);
int fm_server_opt_set_state(fm_engine* e, const float* m_dev, const float* v_dev, int64_t steps);
/* Uninstall (the arenas stay allocated for the next install).  FM_ERR_ARG when nothing is installed. */
int fm_server_opt_end(fm_engine* e);
/* 1 while a server optimizer is installed, else 0 */
int fm_server_opt_active(fm_engine* e);

#ifdef __cplusplus
}
#endif

#endif /* FEDMLP_HIP_SERVER_H */
