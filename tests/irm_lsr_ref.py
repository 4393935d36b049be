"""torch restatements of the FedLSR / FedIRM two-view loss heads (csrc/heads.hip: k_loss_fedlsr, k_loss_fedirm_sup, k_loss_fedirm_rel)
written from the formulas of include/fedmlp_hip.h, with the gradient by autograd.  Every function takes the kernels' layouts
(z [2B][C] view 1 rows then view 2 rows, y [B][C]) as array-likes, computes in `dtype` (float64 by default: the reference the
kernels are held to; float32: what torch's own fp32 arithmetic gives, the yardstick of tests/test_irm_lsr_heads_gpu.py) on
the CPU and returns numpy float64.  tests/test_irm_lsr_cpu.py pins the building blocks to the reference's own functions
(tests/golden/irm_lsr_kat.npz)."""
import numpy as np
import torch
import torch.nn.functional as F


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a, np.float64)).to(dtype)


def js(p, q):
    """Jensen-Shannon term of FedLSR: KLDivLoss(reduction='mean') is the mean over ALL elements"""
    lm = ((p + q) / 2).log()
    return (F.kl_div(lm, p, reduction="mean") + F.kl_div(lm, q, reduction="mean")) / 2


def anti_sigmoid(p):
    return torch.log(p / (1 - p))


def confuse_matrix(z1, lab):
    """row i: sigmoid((sum_b z1[b, :] lab[b, i]) / (sum_b lab[b, i] + 1e-8) / 2), for any C"""
    # the denominator as the reference forms it: boolean pseudo-labels sum to an int64 count, and count + 1e-8 is then a
    # float32 tensor (the count itself, or 1e-8 for an empty class); float labels stay in their own dtype
    den = (lab.sum(0) + 1e-8).to(z1.dtype)
    num = lab.to(z1.dtype).t() @ z1                           # [C, C]: row i = sum_b lab[b, i] z1[b, :]
    return torch.sigmoid(num / den[:, None] / 2.0)


def kd_loss(Q, P):
    """symmetric kl_div(..., 'batchmean'): the sums divided by the number of rows"""
    return (F.kl_div(Q.log(), P, reduction="batchmean") + F.kl_div(P.log(), Q, reduction="batchmean")) / 2.0


def sigmoid_mse(a, b):
    return (torch.sigmoid(a) - torch.sigmoid(b)) ** 2


def select_rows(z1, up=0.7, down=0.3):
    """the relation phase's rows: every probability > up or < down, and the entropy-style uncertainty < 2; [B] bool"""
    p = torch.sigmoid(z1)
    conf = torch.all((p > up) | (p < down), dim=1)
    unc = -1.0 * (torch.sum(p * torch.log(p + 1e-6), dim=1) + torch.sum((1 - p) * torch.log(1 - p + 1e-6), dim=1))
    return conf & (unc < 2.0)


def _sup(z1, z2, y, pw, active, bs_norm, ann):
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=pw, reduction="none")
    act = [c for c in range(y.shape[1]) if active[c] != 0]
    return (crit(z1, y) + crit(z2, y))[:, act].sum() / (bs_norm * ann)


def _out(loss, zz, extra=()):
    (dz,) = torch.autograd.grad(loss, zz)
    return (float(loss.detach().double()), dz.detach().double().numpy()) + tuple(extra)


def loss_fedlsr(z, y, pw, mix1, beta, dtype=torch.float64, rational=False):
    """-> (loss, dz [2B][C]).  rational=False: the chain the reference writes, sigmoid(2 log(p / (1 - p))); True: the form the
    kernel uses, p^2 / (p^2 + (1 - p)^2) (the same function of p; it differs only in rounding and where p rounds to 1)."""
    zz = _t(z, dtype).requires_grad_(True)
    y, pw = _t(y, dtype), _t(pw, dtype)
    B = y.shape[0]
    z1, z2 = zz[:B], zz[B:]
    q1 = torch.clamp(torch.sigmoid(z1 * 3), min=1e-6, max=1.0)
    q2 = torch.clamp(torch.sigmoid(z2 * 3), min=1e-6, max=1.0)
    p = torch.sigmoid(z1) * mix1 + torch.sigmoid(z2) * (1 - mix1)
    if rational:
        pred_mix = p * p / (p * p + (1 - p) * (1 - p))
    else:
        pred_mix = torch.sigmoid(anti_sigmoid(p) * 2)
    loss = torch.nn.BCEWithLogitsLoss(pos_weight=pw)(pred_mix, y) + js(q1, q2) * beta
    return _out(loss, zz)


def loss_fedirm_sup(z, y, pw, active, ann, bs_norm, dtype=torch.float64):
    """-> (loss, dz [2B][C], relation matrix [C][C] of (z_1, y))"""
    zz = _t(z, dtype).requires_grad_(True)
    y, pw = _t(y, dtype), _t(pw, dtype)
    B = y.shape[0]
    loss = _sup(zz[:B], zz[B:], y, pw, active, bs_norm, ann)
    rel = confuse_matrix(zz[:B].detach(), y)
    return _out(loss, zz, (rel.double().numpy(),))


def loss_fedirm_rel(z, zt, y, pw, active, ann, bs_norm, cw, target, dtype=torch.float64):
    """-> (loss, dz [2B][C], relation matrix [C][C] of (z_1, y), number of selected rows)"""
    zz = _t(z, dtype).requires_grad_(True)
    zt, y, pw, target = _t(zt, dtype), _t(y, dtype), _t(pw, dtype), _t(target, dtype)
    B, C = y.shape
    z1, z2 = zz[:B], zz[B:]
    with torch.no_grad():
        mask = select_rows(z1)
        pseudo = torch.sigmoid(z1)[mask] > 0.5
    if int(mask.sum()) != 0:
        source = confuse_matrix(z1[mask], pseudo)
    else:
        source = 0.5 * torch.ones((C, C), dtype=dtype)
    cons = torch.sum(sigmoid_mse(z1, zt)) / bs_norm
    loss = cw * cons + cw * torch.sum(kd_loss(source, target)) + _sup(z1, z2, y, pw, active, bs_norm, ann)
    rel = confuse_matrix(z1.detach(), y)
    return _out(loss, zz, (rel.double().numpy(), int(mask.sum())))


def selection_margin(z1):
    """how far the relation phase's decisions are from their thresholds (float64): min |p - 0.7|, |p - 0.3|, |p - 0.5| over the
    elements and min |uncertainty - 2| over the rows; a test keeps these above fp32 rounding"""
    z1 = _t(z1, torch.float64)
    p = torch.sigmoid(z1)
    unc = -1.0 * (torch.sum(p * torch.log(p + 1e-6), dim=1) + torch.sum((1 - p) * torch.log(1 - p + 1e-6), dim=1))
    el = torch.minimum(torch.minimum((p - 0.7).abs(), (p - 0.3).abs()), (p - 0.5).abs()).min()
    return float(el), float((unc - 2.0).abs().min())
