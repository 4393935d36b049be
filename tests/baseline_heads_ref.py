"""The RSCFed / FedNoRo (LA_KD) / CBAFed loss heads of oracle/steps_ref.py restated dtype-generic, with autograd: the oracle's
functions build their pos_weight tensor in float32 whatever the logits' dtype, so they cannot serve as a float64 yardstick as
they stand.  Each function here is the oracle's torch code with every tensor in `dtype`; tests/test_baseline_heads_cpu.py pins
the float32 results to the oracle's own, bit for bit.  Inputs are numpy arrays / lists; -> (loss, dz) as float64 numpy."""
import numpy as np
import torch
import torch.nn.functional as F


def _t(a, dtype):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)


def _out(loss, z):
    (dz,) = torch.autograd.grad(loss, z)
    return np.float64(loss.detach().numpy()), dz.numpy().astype(np.float64)


def loss_rscfed(z, zt, y, pos_weight, act, neg, bs_norm, annotation_num, dtype=torch.float64):
    """oracle.steps_ref.loss_rscfed"""
    zz = _t(z, dtype).requires_grad_(True)
    l = F.binary_cross_entropy_with_logits(zz, _t(y, dtype), pos_weight=_t(pos_weight, dtype), reduction="none")
    sup = l[:, act].sum() / (bs_norm * annotation_num)
    unsup = F.mse_loss(torch.sigmoid(zz)[:, neg], torch.sigmoid(_t(zt, dtype))[:, neg])
    return _out(sup + unsup, zz)


def loss_la_kd(z, zt, y, act, neg, w_kd, dtype=torch.float64):
    """oracle.steps_ref.loss_la_kd"""
    zz = _t(z, dtype).requires_grad_(True)
    p = torch.sigmoid(zz)
    soft = torch.sigmoid(_t(zt, dtype) / 0.8)
    B = p.shape[0]
    bce = F.binary_cross_entropy(p, _t(y, dtype), reduction="none")[:, act].sum() / (B * len(act))
    kl = F.mse_loss(p, soft, reduction="none")[:, neg].sum() / (B * len(neg))
    return _out(w_kd * kl + (1 - w_kd) * bce, zz)


def loss_cbafed_stage1(z, y, pos_weight, act, bs_norm, annotation_num, dtype=torch.float64):
    """oracle.steps_ref.loss_cbafed_stage1"""
    zz = _t(z, dtype).requires_grad_(True)
    l = F.binary_cross_entropy_with_logits(zz, _t(y, dtype), pos_weight=_t(pos_weight, dtype), reduction="none")
    return _out(l[:, act].sum() / (bs_norm * annotation_num), zz)


def loss_cbafed_stage2(z, labels, idx_neg, loss_w, act, neg, bs_norm, annotation_num, dtype=torch.float64):
    """oracle.steps_ref.loss_cbafed_stage2 on the (labels, idx_neg, loss_w) of oracle.steps_ref.cbafed_stage2_targets.
    loss_w is rounded to float32 first, as the oracle's (and the trainer's) float32 pos_weight tensor holds it."""
    zz = _t(z, dtype).requires_grad_(True)
    pw = _t(np.asarray(loss_w, np.float32), dtype)
    l = F.binary_cross_entropy_with_logits(zz, _t(labels, dtype), pos_weight=pw, reduction="none")
    loss = l[:, act].sum() / (bs_norm * annotation_num)
    for k, i in enumerate(neg):
        if len(idx_neg[k]) != 0:
            loss = loss + l[idx_neg[k], i].sum() / len(idx_neg[k])
    return _out(loss, zz)
