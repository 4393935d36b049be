/*
 * fedmlp_hip_rofl.h -- the RoFL client's two entry points of the engine's C ABI (conventions: fedmlp_hip.h).
 *
 * They live in a header of their own, with their own ctypes table (fedmlp_amd/_lib.py: ROFL_SYMBOLS) and their own Python
 * wrappers (fedmlp_amd/engine.py: RoflHeads, a base of Engine): fedmlp_hip.h's entry points are a closed list that the
 * coherence ledger and the refusal table of the test suite enumerate name by name.  The same rules are held for these two by
 * tests/test_rofl_abi_cpu.py (header = table = exports; the wrappers go through Engine._step / Engine._head, which bump the
 * version counters), tests/test_rofl_refusals_gpu.py (every refusal's text) and tests/test_rofl_coherence_gpu.py (the fused step
 * against every first consumer of a derived copy).
 */
#ifndef FEDMLP_HIP_ROFL_H
#define FEDMLP_HIP_ROFL_H

#include "fedmlp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- RoFL (utils/local_training.py:466-626: train_RoFL, RFLloss, get_small_loss_samples) ---------
 * The head of one training batch, with the conventions of fedmlp_hip.h's single-view heads (engine's stream, no synchronisation,
 * no atomics, the same bits from run to run, every element of dz_dev [B][C] written, value and gradient formed in double and
 * rounded once).  It is the first head that reads the pooled FEATURE of the train forward (feat_dev [B][D], a constant of the
 * loss) and that keeps per-client state on the device: centroids_dev [2C][D] (row 2c + t: class c, label value t) and pseudo_dev
 * uint8 [N][C], the round's pseudo-label table, both owned by the caller.  D and C come from the handle.  z_dev, y_dev [B][C];
 * item_dev int32 [B] the rows' positions in the table, distinct within a batch (an item outside [0, N) is never dereferenced:
 * that row stands on its own label).
 *   1. key_i = sum_c BCEWithLogits(pos_weight)(z, y); the n_keep rows of smallest key are kept (ties to the lower row, NaN keys
 *      last).  n_keep = int((1 - forget_rate) * B) is formed by the host.
 *   2. per kept row and class the vote argmax(cos(f[2c], feat_i), cos(f[2c + 1], feat_i)) (a tie gives 0); mask_i = the votes
 *      equal y_i in every class.  Cosine is a.b / (|a| |b|), exactly 0 when a norm is 0.
 *   3. write_labels != 0 (epoch < T_pl): pseudo[item_i] = y_i for the kept rows.  Then new_i = y_i where mask_i, else
 *      pseudo[item_i].
 *   4. loss = mean over n_keep C of BCEWithLogits(pos_weight)(z_i, new_i)
 *           + lambda_cen_eff sum_i mask_i sum_c |feat_i - f[2c + y_ic]|^2 / (n_keep D) / C
 *           + lambda_e sum_i sum_c H(sigmoid z_ic) / (n_keep C), H the binary entropy formed as softplus(z) - z sigmoid(z)
 *      (finite for every z; the reference's fp32 p log p is NaN once p rounds to 0 or 1).  The centroid term has a value and no
 *      gradient.  dz is an exact 0 off the kept rows.  The host forms lambda_cen_eff (lambda_cen epoch / T_pl while epoch < T_pl).
 *   5. AFTER the loss has read them, the centroids move: fh[2c + y_ic] = mean of feat_i over the kept rows (a zero count
 *      divides by 1), s_r = cos(f[r], fh[r]), f[r] = (1 - s_r^2) f[r] + s_r^2 fh[r].
 * keep_dev int32 [B] (may be NULL): bit 0 kept, bit 1 mask.  FM_ERR_ARG: a null pointer, B < 1, B > max_images, n_keep < 1,
 * n_keep > B, N < 1 or N * C >= 2^31, a feature dimension that is no multiple of 4, feat_dev or centroids_dev not 16-byte
 * aligned (the row kernel reads both as float4).  The workspaces (keys, cosine table, distances, keep flags: max_images rows)
 * are allocated at the first RoFL call of a handle.
 * fm_step_rofl: one-view train forward, the head on the engine's logits and pooled feature, backward, Adam.  FM_ERR_ARG under a
 *   requires_grad mask; the bits of fm_forward_train -> fm_loss_rofl -> fm_backward_step. */
int fm_loss_rofl(fm_engine* e, const float* z_dev, const float* feat_dev, const float* y_dev, const int32_t* item_dev, int32_t B,
                 int32_t n_keep, const float* pos_weight_host, float lambda_cen_eff, float lambda_e, int32_t write_labels,
                 float* centroids_dev, uint8_t* pseudo_dev, int64_t N, float* dz_dev, float* loss_dev, int32_t* keep_dev);
int fm_step_rofl(fm_engine* e, const float* x_dev, const float* y_dev, const int32_t* item_dev, int32_t B, int32_t n_keep,
                 const float* pos_weight_host, float lambda_cen_eff, float lambda_e, int32_t write_labels, float* centroids_dev,
                 uint8_t* pseudo_dev, int64_t N, float* loss_dev);

#ifdef __cplusplus
}
#endif

#endif /* FEDMLP_HIP_ROFL_H */
