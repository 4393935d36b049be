/*
 * fedmlp_hip_debug.h -- kernel-level test hooks of libfedmlp_hip.so (tests/ and tools/ only).
 *
 * NOT part of the drop-in surface of fedmlp_hip.h: nothing behind build_model() / LocalUpdate / FedAvg* calls these.
 * They expose single kernels (one convolution forward / data gradient / weight gradient, one BatchNorm / stem-pool / plane-writer
 * launcher, one depthwise / squeeze-excite / BN+activation launcher of the EfficientNet-B0 path, one classifier-head or loss launcher
 * on caller-supplied tensors), the activations the last train-mode forward kept, and the gradients of the last step, so that the
 * parity tests can compare each kernel with a CPU yardstick.
 */
#ifndef FEDMLP_HIP_DEBUG_H
#define FEDMLP_HIP_DEBUG_H

#include "fedmlp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* info[0..12] = cin, cout, k, stride, pad, hin, win, hout, wout, cin_p (padded
 * input channels of the NHWC operand), Kw (row length of the engine-layout
 * weight matrix [cout_p][Kw] = [cout_p][k][kw_p][cin_p]), kw_p, cout_p (padded output
 * channels of the NHWC result; = cout for ResNet-18); info[13..15] = 0. */
int fm_debug_conv_info(fm_engine* e, int32_t conv, int32_t* info16);
int fm_debug_num_convs(fm_engine* e);
/* op 0: raw forward  x[imgs,hin,win,cin_p] -> out[imgs,hout,wout,cout]; if stats_dev
 *       != NULL also the per-group per-channel (sum, sumsq) [groups][2][cout]
 * op 1: data gradient dy[imgs,hout,wout,cout] -> out[imgs,hin,win,cin]; on the stem conv (cin = 3: conv 0 of ResNet-18,
 *       the first conv of EfficientNet-B0, dy with cout_p channels) the input-gradient kernel of fm_backward_grads_x with its
 *       NHWC store
 * op 2: weight gradient (x, dy) -> out[cout][Kw] (engine layout)
 * All tensors NHWC fp32 on device; weights are the engine's current state. */
int fm_debug_conv(fm_engine* e, int32_t op, int32_t conv, const float* x_dev, const float* dy_dev,
                  float* out_dev, int32_t imgs, int32_t groups, float* stats_dev);

/* The forward of one convolution with the optional operands the engine's graphs hand to it (a precision-0 handle of either model;
 * weights are the engine's current state): x[imgs,hin,win,cin_p] -> out[imgs,hout,wout,cout_p].  On an EfficientNet-B0 handle out
 * (and the dy of fm_debug_conv) carries cout_p channels, the pad channels included; on a ResNet-18 handle cout_p = cout, and the
 * packed stem is framed as fm_debug_conv frames it.
 *   epilogue: scale, shift [cout_p], res [imgs,hout,wout,cout_p] | NULL, act 0 none / 1 relu / 2 swish:
 *             out = act(conv * scale + shift + res)
 *   prologue: gate [imgs][cin_p], psc, psh [groups][cin_p] | NULL: the operand is x * gate[img], with psc / psh
 *             swish(x * psc[g] + psh[g]) * gate[img]
 *   stats:    per-group per-channel (sum, sumsq) [groups][2][cout_p] of the raw convolution, folded as by fm_debug_conv
 * Exactly the three forms the graphs use are taken:
 *   plain / train  no epilogue, no prologue, stats optional;
 *   eval           scale + shift (+ res, act), no stats, groups = 1; may carry the gate-only prologue; no res on a stem;
 *   prologue       gate alone without stats, or psc + psh + gate with stats and without an epilogue -- on a 1x1 stride-1
 *                  convolution of an EfficientNet-B0 handle that streams through conv1x1.hip (cin_p <= 256) only.
 * Anything else (half a pair, res or act without scale / shift, res on a stem, groups > 1 or stats with an epilogue, a prologue on
 * another conv or on a ResNet-18 handle) returns FM_ERR_ARG before any launch and leaves the handle usable. */
int fm_debug_conv_fwd(fm_engine* e, int32_t conv, const float* x_dev, float* out_dev, int32_t imgs, int32_t groups,
                      const float* scale_dev, const float* shift_dev, const float* res_dev, int32_t act, const float* psc_dev,
                      const float* psh_dev, const float* gate_dev, float* stats_dev);

/* One convolution of forward_eval in planes mode (a planes-mode precision-0 ResNet-18 handle, a non-stem conv; weights are the
 * engine's current state), called as forward_eval calls conv_fwd: the operand is xp = the block-major bf16 planes of
 * x[imgs,hin,win,cin] ([cin/32][3][imgs*hin*win][32] 16-bit words: the header comment of planes_ew.hip), one group, no statistics:
 *   v = relu?(conv * scale + shift + residual), scale / shift [cout] required, relu 0 / 1,
 *   residual = res fp32 [imgs,hout,wout,cout] | resp, the same tensor as planes | neither (never both),
 *   v goes to out fp32 [imgs,hout,wout,cout] and / or to outp as planes (at least one of them).
 * imgs <= max_images.  Anything else returns FM_ERR_ARG before any launch and leaves the handle usable.  The call synchronises the
 * stream and returns a deferred launch error, if there is one. */
int fm_debug_conv_planes(fm_engine* e, int32_t conv, const uint16_t* xp_dev, int32_t imgs, const float* scale_dev,
                         const float* shift_dev, const float* res_dev, const uint16_t* resp_dev, int32_t relu, float* out_dev,
                         uint16_t* outp_dev);

/* Which launcher fm_debug_conv's op (0 forward = conv_fwd, 1 data gradient, 2 weight gradient = conv_wgrad) takes for `imgs` images
 * on this handle (precision 0): a host-side query, nothing is launched.  It returns the launchers' own decision: the arm those
 * functions switch on.  A data gradient of several parity classes reports FM_ARM_PCONV_TAP if any class runs per tap.
 * Returns an FM_ARM_* code (>= 0) or a negative error code. */
enum { FM_ARM_IGEMM = 0, FM_ARM_IGEMM_STEM, FM_ARM_STEM_ROWS, FM_ARM_PCONV_TS, FM_ARM_PCONV_TAP, FM_ARM_PWGRAD, FM_ARM_PWGRAD_RING,
       FM_ARM_WGRAD_GENERIC, FM_ARM_WGRAD_SKINNY, FM_ARM_STEM_DGRAD };
int fm_debug_conv_arm(fm_engine* e, int32_t op, int32_t conv, int32_t imgs);

/* Input gradient of a stride-2 residual block of ResNet-18 (block = index of the basic block: 2, 4, 6), as backward_and_step
 * runs it: dx[imgs,hin,win,cin] = dgrad(conv1; dy1) + dgrad(downsample; dyd), dy1 / dyd [imgs,hout,wout,cout] fp32 NHWC on
 * device.  Planes mode: ONE grouped launch of the per-tap planes kernel (the planes of dy1 / dyd are made inside); every
 * element of dx is written. */
int fm_debug_block_dgrad(fm_engine* e, int32_t block, const float* dy1_dev, const float* dyd_dev, float* dx_dev, int32_t imgs);

/* bf16 pointwise-convolution kernels of a precision-1 engine (conv must be a 1x1 convolution):
 * op 0: x bf16 [imgs,h,w,cin_p] -> out bf16 [imgs,h,w,cout_p] raw; stats_dev (optional) per-group (sum, sumsq)
 *       [groups][2][cout_p] fp32; gate_dev != NULL applies the operand prologue
 *       x <- swish(x*psc[g]+psh[g]) * gate[img]   (psc_dev NULL: x * gate[img]); psc/psh [groups][cin_p], gate [imgs][cin_p]
 * op 1: dy bf16 [imgs,h,w,cout_p] -> out bf16 [imgs,h,w,cin_p]; x_dev (optional) = residual added to the result
 * op 2: (x, dy) -> out fp32 [cout_p][cin_p], with the same optional prologue on x; also the stem (see fm_debug_pw_fwd) */
int fm_debug_pw(fm_engine* e, int32_t op, int32_t conv, const void* x_dev, const void* dy_dev, void* out_dev,
                int32_t imgs, int32_t groups, const float* psc_dev, const float* psh_dev, const float* gate_dev,
                float* stats_dev);

/* The forward of one convolution of a precision-1 EfficientNet-B0 handle through conv_fwd, with the optional operands the engine's
 * graphs hand to it: the bf16 counterpart of fm_debug_conv_fwd (weights are the engine's current state, i.e. its bf16 shadow).
 * A 1x1 convolution: x bf16 [imgs,h,w,cin_p] -> out bf16 [imgs,h,w,cout_p].  The stem: x is the fp32 NCHW batch [imgs][3][H][W]; the
 * hook first forms the stem's operand as the graphs do (k_stem_im2col into the handle's im2col buffer, for `groups` views of
 * imgs / groups images), out bf16 [imgs,hout,wout,cout_p].
 *   epilogue: scale, shift [cout_p] fp32, res bf16 [imgs,hout,wout,cout_p] | NULL, act 0 none / 2 swish:
 *             out = act(conv * scale + shift + res)
 *   prologue: gate [imgs][cin_p], psc, psh [groups][cin_p] | NULL, all fp32: the operand is x * gate[img], with psc / psh
 *             swish(x * psc[g] + psh[g]) * gate[img], re-rounded to bf16
 *   stats:    per-group per-channel (sum, sumsq) [groups][2][cout_p] fp32 of the raw convolution, taken from the fp32 accumulators
 *             (not from the rounded bf16 output) and folded as by fm_debug_conv
 * The forms taken:
 *   plain / train  no epilogue, stats optional;
 *   eval           scale + shift (+ res, act), no stats, groups = 1; may carry the gate-only prologue; no res on the stem;
 *   prologue       what fm_debug_pw op 0 offers (gate, or psc + psh + gate; stats optional), on a 1x1 convolution.
 * Anything else (half a pair, res or act without scale / shift, stats or groups > 1 with an epilogue, psc / psh under an epilogue,
 * a prologue or a residual on the stem, act = 1, another kind of convolution, a precision-0 or ResNet-18 handle) returns FM_ERR_ARG
 * before any launch and leaves the handle usable.
 * The stem's weight gradient is fm_debug_pw op 2 on the stem conv: x = the fp32 NCHW batch (the im2col matrix is formed from it in
 * the same way), dy bf16 [imgs,hout,wout,cout_p], out fp32 [cout_p][Kw]; no prologue. */
int fm_debug_pw_fwd(fm_engine* e, int32_t conv, const void* x_dev, void* out_dev, int32_t imgs, int32_t groups,
                    const float* scale_dev, const float* shift_dev, const void* res_dev, int32_t act, const float* psc_dev,
                    const float* psh_dev, const float* gate_dev, float* stats_dev);

/* Fused backward of a project convolution (pw_proj_bwd_kernel: blocks 0-4 of a precision-1 EfficientNet engine, tensors bf16;
 * pw_proj_bwd_f32_kernel: blocks 0-2 of a precision-0 one, every "bf16" below is then fp32):
 * dyp bf16 [imgs,h,w,cout_p] (= d y_p), yd bf16 [imgs,h,w,cin_p] (the depthwise output y_d), bn [7][groups][cin_p] fp32 =
 * BN1's scale, shift, mean, istd and the BN1-backward coefficients ca, cb, cc; gate / ds fp32 [imgs][cin_p].
 * phase 0: out = fp32 dW [cout_p][cin_p] with a_s = swish(yd*scale+shift)*gate, pool5 = fp32 [imgs][5][cin_p], the five
 *          per-image sums of (d a_s, y_d) that the squeeze-excite and BN1 backward need (d a_s = bf16(dyp W));
 * phase 1: out = bf16 d y_d [imgs,h,w,cin_p] = ca*((d a_s*gate + ds/HW)*swish'(v)) + cb*yd + cc. */
int fm_debug_proj_bwd(fm_engine* e, int32_t conv, int32_t phase, const void* dyp_dev, const void* yd_dev, const float* bn_dev,
                      const float* gate_dev, const float* ds_dev, int32_t imgs, int32_t groups, void* out_dev,
                      float* pool5_dev);

/* Fused backward of an expand convolution with its BatchNorm + Swish (pw_exp_bwd_kernel, precision 1: tensors bf16;
 * pw_exp_bwd_f32_kernel, precision 0: fp32; conv = an expand conv of blocks 1-3):  da = d a_e and ye = y_e [imgs,h,w,cout_p],
 * x = the block input [imgs,h,w,cin_p], res (optional) = the skip connection's gradient [imgs,h,w,cin_p], bn [5][groups][cout_p]
 * fp32 = the BN0-backward coefficients ca, cb, cc and the forward's scale, shift.
 * dx = d y_e W (+ res) [imgs,h,w,cin_p] with d y_e = ca*(da*swish'(ye*scale+shift)) + cb*ye + cc; dw = fp32 [cout_p][cin_p]. */
int fm_debug_exp_bwd(fm_engine* e, int32_t conv, const void* da_dev, const void* ye_dev, const void* x_dev, const void* res_dev,
                     const float* bn_dev, int32_t imgs, int32_t groups, void* dx_dev, float* dw_dev);

/* Post-ReLU activations the last train-mode forward kept (ResNet-18): kind 0 = relu(bn1(conv1)) of
 * basic block `block`, kind 1 = the block's output relu(bn2(conv2) + identity); NHWC fp32 for the first
 * `imgs` images, dims4 = {imgs, H, W, C}.  host_nhwc may be NULL to query the dims only.  Parity tests
 * hand the ReLU masks (value > 0) to the oracle's backward pass, so a pre-activation within rounding
 * distance of zero cannot turn a 1e-6 forward difference into a percent-level gradient difference. */
int fm_debug_activation(fm_engine* e, int32_t kind, int32_t block, int32_t imgs, float* host_nhwc,
                        int32_t* dims4);

/* The discrete decisions of the ResNet-18 stem in the last train-mode forward, for the same purpose: the ReLU mask of
 * relu(bn1(conv1(x))) over the dense [imgs][H/2][W/2][64] map, bit-packed (byte b of a pixel = channels 8b .. 8b+7, bit j =
 * channel 8b + j: relu_bits_host [imgs][H/2][W/2][8]), and the 3x3 / stride-2 max-pool's choice per pooled element
 * (argmax_host [imgs][H/4][W/4][64], code kh * 3 + kw of the chosen window position).  groups = the views of that forward
 * (BatchNorm statistics are per view). */
int fm_debug_stem_masks(fm_engine* e, int32_t imgs, int32_t groups, uint8_t* relu_bits_host, uint8_t* argmax_host);

/* Fault injection for the stream-K fix-up of the planes conv GEMMs (pconv.hip): on = 1 makes the owners of partial tiles keep
 * their arrival announcements to themselves (and shortens the finisher's bounded wait), so that every shared tile times out.
 * Expected behaviour, which tests/test_engine_gpu.py checks: the step's optimizer update is skipped on the device (weights,
 * moments unchanged) and the NEXT call that ends a step or synchronises returns FM_ERR_HIP once.  Process-wide; on = 0 restores. */
int fm_debug_lose_part(int32_t on);

/* Schedule perturbation for the two-lane order (main lane = the caller's stream, side lane = teacher forward and weight
 * gradients): hold one lane back at one of its launch points, so that the other lane runs as far ahead as its event waits allow.
 * With every wait in place the results are the bits of a one-stream handle, wherever the delay sits (tests/test_lane_delay_gpu.py).
 *
 * Delay points, counted per lane (0 main, 1 side) from the arming call on: every launcher of the engine's graphs (the OP(lane, ..)
 * scopes), and -- on the main lane -- one point at the entry of every call that enqueues a step, a forward or a backward, ahead of
 * its first enqueue (input staging and weight-shadow rebuilds included).
 *
 * fm_debug_lane_delay arms the handle: both counters and the wait counts below restart at 0, and when lane `lane` reaches its
 * point number `at` (0-based) the engine first enqueues, once, a delay kernel of `micros` microseconds on that lane's stream: one
 * workgroup of 64 threads that touches no memory and spins on the wall clock, bounded by the time asked for and by an iteration cap
 * that ends it within a small multiple of that time.  micros = 0 only counts.  FM_ERR_ARG, with nothing armed or enqueued: a lane
 * other than 0 / 1, lane 1 on a handle without a side stream, at < 0, micros outside 0 .. FM_LANE_DELAY_MAX_US.
 * fm_debug_lane_points: out16[0], [1] = points passed by the main / side lane since arming, [2] = 1 once the delay kernel was
 * enqueued, [3 + k] = cross-lane waits of kind k reached, [3 + FM_WAIT_KINDS + k] = those of them that were skipped; disarm != 0
 * ends the counting (a disarmed handle pays one predictable branch per launch).
 *
 * fm_debug_drop_wait (on = 1 / 0; per handle, off by default, kept across arming calls) is the mutant that shows the delay sweep
 * sees a lost dependency: the engine skips the hipStreamWaitEvent of ONE kind, the event records stay:
 *   FM_WAIT_SIDE_BEGIN  the side lane's wait for the main lane's producer of a gradient tensor (side_begin)
 *   FM_WAIT_SIDE_GUARD  the main lane's wait for the side lane's weight gradient before it overwrites that tensor (side_guard)
 *   FM_WAIT_SIDE_JOIN   the main lane's wait for every weight gradient before the optimizer (side_join)
 *   FM_WAIT_EV_IN       the side lane's wait before the teacher's forward (ev_in)
 *   FM_WAIT_EV_T        the main lane's wait for the teacher before the loss head (ev_t; both call sites)
 * A dropped wait only reorders reads and writes of buffers the step owns: allocations, sizes and kernel arguments are what they
 * always are, so the outcome is wrong values, never an access outside those buffers.  Neither hook reads the environment. */
enum { FM_WAIT_SIDE_BEGIN = 0, FM_WAIT_SIDE_GUARD, FM_WAIT_SIDE_JOIN, FM_WAIT_EV_IN, FM_WAIT_EV_T };
#define FM_WAIT_KINDS 5
#define FM_LANE_DELAY_MAX_US 20000
int fm_debug_lane_delay(fm_engine* e, int32_t lane, int64_t at, int32_t micros);
int fm_debug_lane_points(fm_engine* e, int64_t* out16, int32_t disarm);
int fm_debug_drop_wait(fm_engine* e, int32_t which, int32_t on);

/* Gradients of the last step in state_dict order (running-stat slots are 0). */
int fm_debug_get_grads(fm_engine* e, float* host_f32);
/* The raw engine-layout arenas behind the optimizers (NP floats each, layout padding included; the trainable part of
 * fm_state_device's layout): which = 0 first moment, 1 second moment, 2 the gradient accumulator (allocated if it was not), 3 the gradients of the last backward (what fm_debug_get_grads
 * reorders; for comparisons on the device). */
int fm_debug_optim_arena(fm_engine* e, int32_t which, float** dev_ptr, int64_t* numel);
/* The entry table of the grouped optimizer steps and the masked accumulate: off_len[2 i] = arena offset, off_len[2 i + 1] =
 * span length in floats of state entry i (reference key order), summed over its chunks; -1 / 0 for running statistics and
 * counters.  Floats of the trainable arena outside every span are layout gaps nobody writes. */
int fm_debug_entry_spans(fm_engine* e, int64_t* off_len, int32_t n_entries);

/* One launcher of csrc/kernels.h -- the BatchNorm, stem max-pool and plane-writer kernels between ResNet-18's conv GEMMs
 * (elementwise.hip, planes_ew.hip, the two plane converters of pconv.hip) -- on caller-supplied device tensors, on the handle's
 * main stream, followed by a stream synchronisation.  A precision-0 ResNet-18 handle; no engine state is read or written:
 * every operand and workspace is a caller buffer.  p[] = FM_EW_NPTR device pointers (NULL = the optional operand is absent,
 * unused slots NULL), d[] = FM_EW_NDIM dimensions, sc[] = FM_EW_NSCAL scalars.  Arguments outside a kernel's contract (a missing
 * required operand, a dimension < 1, C % 4 != 0, C % 32 != 0 for an op that reads or writes planes, odd H or W for the stem
 * pool, C not a power of two for the two reduce passes) return FM_ERR_ARG before any launch.
 *
 * Activations are fp32 NHWC [groups * pix][C]; per-channel vectors are [groups][C] unless noted; `planes` are 16-bit words
 * [C/32][3][P][32] over all P = groups * pix pixels (layout: the header comment of planes_ew.hip), 3 * P * C words.
 * nblk(n) = max(1, min(1024, ceil(n / 64))) is the number of partial-sum blocks per group of a reduce pass over n pixels.
 * A partials workspace of T tiles per group holds groups * T * 2 * C floats, and when T > 64 another groups * 32 * 2 * C floats
 * right behind them (the fold area the finalize pass writes).
 *
 * FM_EW_SPLIT_PLANES        p = {x, planes};  d = {P, C}
 * FM_EW_PLANES_TO_F32       p = {planes, x};  d = {P, C}
 * FM_EW_BN_FINALIZE         p = {stats [groups][tiles][2][C] (+ fold area), gamma [C], beta [C], run_mean [C] | NULL, run_var [C] |
 *                           NULL, mean, istd, scale, shift, skip (one int32) | NULL};  d = {groups, tiles, C, count};
 *                           sc = {eps, momentum}
 * FM_EW_BN_FINALIZE_FROZEN  p = {gamma, beta, run_mean, run_var, mean, istd, scale, shift, skip | NULL};  d = {groups, C};  sc = {eps}
 * FM_EW_BN_EVAL_AFFINE      p = {gamma, beta, run_mean, run_var, scale, shift} all [n];  d = {n};  sc = {eps}
 * FM_EW_BN_APPLY            p = {y, scale, shift, res | NULL, y2 | NULL, scale2 | NULL, shift2 | NULL, out};  d = {groups, pix, C, relu}
 * FM_EW_BN_APPLY_PLANES     the same with out | NULL, and p[8] = out planes, p[9] = res planes | NULL (then res is NULL)
 * FM_EW_STEM_POOL           p = {y [groups * ipg][H][W][C], scale | NULL, shift | NULL, pooled [..][H/2][W/2][C], idx uint8 (pooled's
 *                           shape) | NULL};  d = {groups, ipg, H, W, C}
 * FM_EW_STEM_POOL_PLANES    the same with pooled | NULL, and p[5] = pooled planes
 * FM_EW_STEM_POOL_BWD       p = {dpooled, pooled, idx, dy [imgs][H][W][C]};  d = {imgs, H, W, C}
 * FM_EW_STEM_POOL_BN_REDUCE p = {dpooled, pooled, idx, y, mean, istd, part [groups][nblk(ipg H/2 W/2)][2][C], gamma [C], beta [C]};
 *                           d = {groups, ipg, H, W, C}
 * FM_EW_STEM_POOL_BN_APPLY  p = {dpooled, pooled, idx, y, ca, cb, cc, dy};  d = {groups, ipg, H, W, C}
 * FM_EW_BN_BWD_REDUCE       p = {dz, z | NULL, y, mean, istd, part [groups][nblk(pix)][2][C], mask_scale | NULL, mask_shift | NULL,
 *                           z planes | NULL};  d = {groups, pix, C}
 * FM_EW_BN_BWD_FINALIZE     p = {part (+ fold area), gamma [C], mean, istd, ca, cb, cc, dgamma [C], dbeta [C]};
 *                           d = {groups, nblk, C, count, frozen}
 * FM_EW_BN_BWD_APPLY        p = {dz, z | NULL, y, ca, cb, cc, dy, dyh_out | NULL, mask_scale | NULL, mask_shift | NULL};  d = {groups, pix, C}
 * FM_EW_BN_BWD_APPLY_PLANES the same with dy | NULL, and p[10] = dy planes, p[11] = z planes | NULL */
enum {
    FM_EW_SPLIT_PLANES = 0, FM_EW_PLANES_TO_F32, FM_EW_BN_FINALIZE, FM_EW_BN_FINALIZE_FROZEN, FM_EW_BN_EVAL_AFFINE, FM_EW_BN_APPLY,
    FM_EW_BN_APPLY_PLANES, FM_EW_STEM_POOL, FM_EW_STEM_POOL_PLANES, FM_EW_STEM_POOL_BWD, FM_EW_STEM_POOL_BN_REDUCE,
    FM_EW_STEM_POOL_BN_APPLY, FM_EW_BN_BWD_REDUCE, FM_EW_BN_BWD_FINALIZE, FM_EW_BN_BWD_APPLY, FM_EW_BN_BWD_APPLY_PLANES
};
#define FM_EW_NPTR 12
#define FM_EW_NDIM 5
#define FM_EW_NSCAL 2
int fm_debug_ew(fm_engine* e, int32_t op, void* const* p, const int32_t* d, const float* sc);

/* One launcher of csrc/kernels.h -- the depthwise-convolution, squeeze-excite and BN+activation kernels of the EfficientNet-B0 path
 * (effnet.hip) -- on caller-supplied device tensors, on the handle's main stream, followed by a stream synchronisation.  Any EfficientNet-B0
 * handle, of either precision: the storage type is a dimension (dt: 0 = fp32, 1 = bf16 words), no engine state is read or
 * written.  p[] = FM_EFF_NPTR pointers (NULL = the optional operand is absent, unused slots NULL), d[] = FM_EFF_NDIM dimensions
 * (unused ones 0), sc = reserved (no launcher here takes a scalar; may be NULL).  Arguments outside a kernel's contract return
 * FM_ERR_ARG before any launch: a missing required operand, a dimension < 1, C % 4 != 0 (C % 8 != 0 for the squeeze-excite
 * ops in bf16 storage: 16-byte pieces), K outside {3, 5}, stride outside {1, 2}, Ho / Wo != ceil(Hi / stride) / ceil(Wi / stride),
 * a padding outside 0 .. K-1, act outside 0 .. 2, imgs % ipg != 0, Cs > 48 for SE_WGRAD, a half-given optional group, and what the
 * BN+activation passes list below.
 *
 * p[FM_EFF_NPTR - 1] = `served`, ONE int32 in HOST memory (optional unless a request is made): for the launchers that return bool
 * it receives 1 when the kernel served the statistics / pooling request and 0 when it declined (the caller then reduces by
 * itself; a declined request leaves rec and stats_out / pool_out untouched).  The return value stays an error code.
 *
 * Tensors marked T are dt-typed (fp32, or bf16 words), everything else is fp32.  Activations are NHWC; depthwise weights
 * w [K*K][C] (tap kh * K + kw); TF-"same" padding is (pad_t, pad_l) at the top / left, whatever remains at the bottom / right.
 *
 * depthwise ops: d = {dt, imgs, Hi, Wi, Ho, Wo, C, K, stride, pad_t, pad_l, act, groups}   (groups >= 1 always)
 * FM_EFF_DW_FWD    p = {x T [imgs][Hi][Wi][C], w, y T [imgs][Ho][Wo][C], scale [C] | NULL, shift [C] | NULL, rec | NULL,
 *                  stats_out | NULL, pool_out | NULL};  y = conv(x, w), with scale / shift: y = act(conv * scale + shift), act 0 none /
 *                  1 relu / 2 swish.  rec + stats_out = the statistics request: when served, stats_out [groups][T][2][C], T =
 *                  dw_stats_tiles() = 8, holds partial (sum, sum of squares) of the STORED y (bf16: of the rounded values) per group;
 *                  their sum over T is the statistic.  A group is an equal run of the kernel's row steps: whole images whenever
 *                  groups divides imgs.  rec + pool_out = the pooling request: pool_out [imgs][C] = per-image channel sums of the
 *                  stored y.  Workspaces (fm_debug_eff_ws): floats[0] = rec of a statistics request, [1] = stats_out, [2] = rec of a
 *                  pooling request, [3] = pool_out; a rec size of 0 says that the launch will decline that request.
 * FM_EFF_DW_DGRAD  p = {dy T [imgs][Ho][Wo][C], w, dx T [imgs][Hi][Wi][C], ye T (dx's shape) | NULL, mean, istd, scale, shift (each
 *                  [groups][C]), rec, stats_out};  dx = the data gradient.  ye (with the seven operands after it) requests the
 *                  BN0-backward sums: stats_out [groups][8][2][C] partials of S1 = sum dx' swish'(v), S2 = sum dx' swish'(v) xhat,
 *                  dx' = the stored dx, v = ye scale + shift, xhat = (ye - mean) istd.  Workspaces: [0] = rec, [1] = stats_out.
 * FM_EFF_DW_WGRAD  p = {dy T, x T, part, out [K*K][C]};  out = the weight gradient.  Workspaces: [0] = part, [1] = out.
 *
 * squeeze-excite ops: d = {dt, imgs, HW, C, Cs, ipg, flag};  W1 [Cs][C], b1 [Cs], W2 stored transposed [Cs][C], b2 [C];  scale / shift /
 * mean / istd [imgs / ipg][C], image i in group i / ipg (ipg = 1 and d[4] = 1 where unused)
 * FM_EFF_SE_FWD    p = {a T [imgs][HW][C] | NULL, scale | NULL, shift | NULL, pool_ws, W1, b1, W2, b2, sq [imgs][C], rpre [imgs][Cs],
 *                  gate [imgs][C]};  A = a, or swish(a scale + shift) with scale / shift;  sq = mean_HW A, rpre = W1 sq + b1,
 *                  gate = sigmoid(W2^T swish(rpre) + b2).  flag = pooled: `a` is not read and pool_ws [imgs][C] holds the
 *                  per-image channel SUMS on entry (no scale / shift then).  Workspaces: [0] = pool_ws.
 * FM_EFF_SE_SCALE  p = {a T, scale | NULL, shift | NULL, gate [imgs][C], out T};  out = A * gate
 * FM_EFF_SE_BWD_BN1 p = {dout T | NULL, y T, scale, shift, mean, istd, pool_ws, gate, rpre, W1, W2, dgp [imgs][C], drp [imgs][Cs],
 *                  ds [imgs][C], bn_part};  with v = y scale + shift, A = swish(v), sg = swish'(v), xh = (y - mean) istd the pass
 *                  leaves pool_ws [imgs][nch][5][C] = partial per-image sums of (dout A, dout sg, dout sg xh, sg, sg xh); with R, P1,
 *                  P2, Q1, Q2 their sums over nch:  dgp = R gate (1 - gate), drp = (W2 dgp) swish'(rpre), ds = W1^T drp, and
 *                  bn_part [imgs / ipg][splits][2][C] = partials of S1 = sum_img gate P1 + ds / HW Q1, S2 = sum_img gate P2 + ds / HW Q2.
 *                  flag = nch_ready: > 0 says that pool_ws already holds that many records per image (the fused project-conv
 *                  backward left them); the pooling pass is skipped and dout may be NULL.  Workspaces: [0] = pool_ws, [1] =
 *                  bn_part, [2] = splits (a count, not a size).
 * FM_EFF_SE_WGRAD  d = {imgs, C, Cs};  p = {dgp, drp, rpre, sq, part, dW1};  dW1 = start of the contiguous gradient range
 *                  [dW1 [Cs][C] | db1 [Cs], padded with zeros to a multiple of 4 | dW2 (transposed) [Cs][C] | db2 [C]].
 *                  Workspaces: [0] = part, [1] = the range.
 *
 * BN+activation passes: d = {ty, ta, groups, pix_per_group, HW, C, mode, act}.  ty = storage type of the raw convolution output (y, dy),
 * ta = that of the activations and their gradients (res, out, a, dz); (ty, ta) is one of (fp32, fp32), (fp32, bf16), (bf16, bf16).
 * Tensors are [groups * pix_per_group][C], an image is HW consecutive pixels (pix_per_group % HW == 0), per-channel vectors are
 * [groups][C], per-image ones (rowscale [imgs], gate / dsv [imgs][C]) count images over all groups.  C % 4 == 0, C % 8 == 0 when
 * both types are bf16 (16-byte pieces); gate and dsv come together; mode and act are 0 where unused.
 * FM_EFF_BNACT_APPLY     p = {y TY, scale, shift, res TA | NULL, rowscale | NULL, out TA};  out = act(y scale + shift) * rowscale[img]
 *                  + res, act 0 none / 1 relu / 2 swish
 * FM_EFF_CHAN_REDUCE     p = {a TA | NULL, y TY, mean | NULL, istd | NULL, scale | NULL, shift | NULL, rowscale | NULL, part, gate |
 *                  NULL, dsv | NULL};  part [groups][nblk][2][C], nblk = bn_bwd_blocks(pix_per_group); its sum over nblk is, mode 0:
 *                  (sum y, sum y^2) -- only y and part are read; mode 1: (sum dyh, sum dyh xhat) with d = a (with gate: a gate[img] +
 *                  dsv[img] / HW), dyh = d act'(y scale + shift) rowscale[img], xhat = (y - mean) istd.  Mode 1 needs a, mean, istd;
 *                  act is 0 or 2, and 2 needs scale and shift.  Workspaces: [0] = part.
 * FM_EFF_BNACT_BWD_APPLY p = {dz TA, y TY, ca, cb, cc, scale | NULL, shift | NULL, rowscale | NULL, dy TY, gate | NULL, dsv | NULL};
 *                  dy = ca dyh + cb y + cc with dyh as above from d = dz; act is 0 or 2, and 2 needs scale and shift. */
enum { FM_EFF_DW_FWD = 0, FM_EFF_DW_DGRAD, FM_EFF_DW_WGRAD, FM_EFF_SE_FWD, FM_EFF_SE_SCALE, FM_EFF_SE_BWD_BN1, FM_EFF_SE_WGRAD,
       FM_EFF_BNACT_APPLY, FM_EFF_CHAN_REDUCE, FM_EFF_BNACT_BWD_APPLY };
#define FM_EFF_NPTR 16
#define FM_EFF_NDIM 13
#define FM_EFF_NWS 4
int fm_debug_eff(fm_engine* e, int32_t op, void* const* p, const int32_t* d, const float* sc);
/* floats[FM_EFF_NWS] = the number of floats each workspace / result of `op` needs for the dimensions d (listed per op above),
 * from the host functions that size the kernels' grids.  The same FM_ERR_ARG contract on d. */
int fm_debug_eff_ws(int32_t op, const int32_t* d, int64_t* floats);

/* One launcher of csrc/kernels.h -- the classifier head and the loss heads (heads.hip) -- on caller-supplied tensors, on the
 * handle's main stream, followed by a stream synchronisation.  Any handle; no engine state is read or written.  p[] = FM_HD_NPTR
 * pointers (NULL = the optional operand is absent, unused slots NULL), d[] = FM_HD_NDIM dimensions (unused ones 0), sc[] =
 * FM_HD_NSCAL scalars.  Pointers marked HOST are float[C] arrays in host memory, as fm_step_* take them; everything else is fp32
 * on the device unless marked T (dt-typed: 0 = fp32, 1 = bf16 words).  Arguments outside a kernel's contract return FM_ERR_ARG
 * before any launch: a missing required operand, a dimension < 1, a class count C > FM_MAX_CLASSES (the by-value class vectors; the
 * channel count of AVGPOOL is not a class count), B > 2048 for FIXMATCH (its confident-row table in LDS), a dt outside {0, 1}.
 *
 * FM_HD_AVGPOOL       p = {x T [imgs][HW][C], feat [imgs][C]};  d = {dt, imgs, HW, C};  feat = mean over HW
 * FM_HD_FC_FWD        p = {feat [imgs][D], W [C][D], b [C], logits [imgs][C]};  d = {imgs, D, C};  logits = feat W^T + b
 * FM_HD_FC_BWD        p = {dz [imgs][C], feat [imgs][D], W [C][D], mask [imgs][D] | NULL, dW [C][D], db [C], dout T [imgs][HW][D],
 *                     dfeat [imgs][D] | NULL};  d = {dt, imgs, D, C, HW};  dW = dz^T feat, db = sum_img dz, and every pixel p < HW of
 *                     dout[img][p] = ((dz W) mask + dfeat) / HW  (without dfeat: ((dz W) / HW) mask; mask, dfeat absent = 1, 0)
 * FM_HD_LOSS_BCE      p = {z [B][C], y [B][C], pos_w HOST, dz [B][C], loss (1 float)};  d = {B, C};  sc = {inv_norm};
 *                     loss = inv_norm sum BCEWithLogits(z, y; pos_w), dz = d loss / d z
 * FM_HD_LOSS_STAGE1   p = {z [2B][C], g [2B][C], y [B][C], active HOST, dz [2B][C], loss};  d = {B, C};  sc = {inv_sup, inv_dis};
 *                     rows r and r + B are the two views of sample r; active classes: inv_sup sum BCE(sigmoid z, y) / 2, the others:
 *                     inv_dis sum (sigmoid z - sigmoid g)^2 / 2
 * FM_HD_LOSS_STAGE2   p = {z [B][C], y [B][C], distill [B][C], dz [B][C], loss};  d = {B, C};  BCE(sigmoid z, y) over the elements with
 *                     distill == 0, divided by their number (none: 0 / 0)
 * FM_HD_LOSS_FIXMATCH p = {z [2B][C] (weak rows, then strong rows), y [B][C], pos_w HOST, pos_wu HOST, active HOST, dz [2B][C], loss};
 *                     d = {B, C, cls_minus_ann (>= 0)};  sc = {inv_sup};  n_neg = the number of classes with active == 0, counted here
 *                     as fm_step_fixmatch does; with n_neg > 0 the kernel divides by n_conf cls_minus_ann, so cls_minus_ann = 0 is
 *                     then FM_ERR_ARG */
enum { FM_HD_AVGPOOL = 0, FM_HD_FC_FWD, FM_HD_FC_BWD, FM_HD_LOSS_BCE, FM_HD_LOSS_STAGE1, FM_HD_LOSS_STAGE2, FM_HD_LOSS_FIXMATCH };
#define FM_HD_NPTR 8
#define FM_HD_NDIM 5
#define FM_HD_NSCAL 2
int fm_debug_head(fm_engine* e, int32_t op, void* const* p, const int32_t* d, const float* sc);

#ifdef __cplusplus
}
#endif
#endif /* FEDMLP_HIP_DEBUG_H */
