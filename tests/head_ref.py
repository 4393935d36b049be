"""float64 restatements of the classifier-head and loss kernels (csrc/heads.hip: k_avgpool, k_fc_fwd, k_fc_bwd, k_loss_bce,
k_loss_stage1, k_loss_stage2, k_loss_fixmatch) in the kernels' own layouts.  tests/test_head_ref_cpu.py pins every function to torch
autograd and to the loss heads of oracle/steps_ref.py; tests/test_head_kernels_gpu.py holds the kernels to them.

The two heads that take BCE on PROBABILITIES (stage 1, stage 2) follow torch's fp32 semantics, which the kernels restate: p is
the fp32 sigmoid, both logarithms are clamped at -100, and the gradient through binary_cross_entropy and sigmoid is
(p - y) / max(p (1 - p), 1e-12) * p (1 - p).  `p32=True` (the default) rounds the float64 sigmoid to fp32 before anything else is
formed from it, so that p = 1 (z >= 17 or so), loss elements of exactly 100 and gradients of exactly 0 come out as they do in fp32;
`p32=False` keeps the float64 sigmoid (what torch computes on float64 tensors)."""
import numpy as np

EPS_PQ = float(np.float32(1e-12))      # the clamp of binary_cross_entropy's backward, as the fp32 constant the kernel holds


def sigmoid(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def one_minus_sigmoid(z):
    return sigmoid(-np.asarray(z, np.float64))


# ---- head --------------------------------------------------------------------------------------------------------------------------
def avgpool(x):
    """x [imgs][HW][C] -> feat [imgs][C]"""
    return np.asarray(x, np.float64).mean(1)


def fc_fwd(feat, W, b):
    """feat [imgs][D], W [C][D], b [C] -> logits [imgs][C]"""
    return np.asarray(feat, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)


def fc_bwd(dz, feat, W, HW, mask=None, dfeat=None):
    """-> dW [C][D], db [C], dpix [imgs][D] = the value every one of the HW pixels of dout[img] carries.  Without dfeat (the fused
    steps): ((dz W) / HW) mask, the dropout multiplier applied to the spread gradient; with dfeat (the autograd path): d loss /
    d feature enters AFTER the dropout multiplier and before the spread: ((dz W) mask + dfeat) / HW."""
    dz, feat, W = (np.asarray(t, np.float64) for t in (dz, feat, W))
    s = dz @ W
    if dfeat is not None:
        if mask is not None:
            s = s * np.asarray(mask, np.float64)
        s = (s + np.asarray(dfeat, np.float64)) / HW
    else:
        s = s / HW
        if mask is not None:
            s = s * np.asarray(mask, np.float64)
    return dz.T @ feat, dz.sum(0), s


# ---- loss elements ------------------------------------------------------------------------------------------------------------------
def bce_logits(z, y, pw):
    """BCEWithLogits with pos_weight, element-wise: l = (1 - y) z + lw softplus(-z), lw = 1 + (pw - 1) y; -> (l, dl / dz)"""
    z, y, pw = (np.asarray(t, np.float64) for t in (z, y, pw))
    lw = 1.0 + (pw - 1.0) * y
    sp = np.log1p(np.exp(-np.abs(z))) + np.maximum(-z, 0.0)
    return (1.0 - y) * z + lw * sp, (1.0 - y) - lw * one_minus_sigmoid(z)


def prob(z, p32=True):
    p = sigmoid(z)
    return p.astype(np.float32).astype(np.float64) if p32 else p


def bce_prob(z, y, p32=True):
    """F.binary_cross_entropy(sigmoid(z), y), element-wise, and its gradient with respect to z; -> (l, dl / dz)"""
    y = np.asarray(y, np.float64)
    p = prob(z, p32)
    q = 1.0 - p if p32 else one_minus_sigmoid(z)
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(p), -100.0), np.maximum(np.log(q), -100.0)
    pq = p * q
    return -(y * lp + (1.0 - y) * lq), (p - y) / np.maximum(pq, EPS_PQ) * pq


# ---- the four loss heads: -> (loss, dz) ------------------------------------------------------------------------------------------------
def loss_bce(z, y, pos_w, inv_norm):
    """z, y [B][C], pos_w [C]"""
    l, d = bce_logits(z, y, np.asarray(pos_w, np.float64)[None, :])
    return l.sum() * inv_norm, d * inv_norm


def loss_stage1(z, g, y, active, inv_sup, inv_dis, p32=True):
    """z (student), g (teacher) [2B][C]: rows r and r + B are the two views of sample r; y [B][C]; active [C] (non-zero = annotated).
    Annotated classes: BCE on probabilities, halved over the views; the others: (sigmoid z - sigmoid g)^2 / 2."""
    z, g, y = (np.asarray(t, np.float64) for t in (z, g, y))
    act = np.asarray(active, np.float64) != 0
    y2 = np.concatenate([y, y], 0)
    l, d = bce_prob(z, y2, p32)
    p, q = sigmoid(z), sigmoid(g)
    e = p - q
    sup = (0.5 * l)[:, act].sum()
    dis = (0.5 * e * e)[:, ~act].sum()
    dz = np.where(act[None, :], 0.5 * d * inv_sup, e * p * one_minus_sigmoid(z) * inv_dis)
    return sup * inv_sup + dis * inv_dis, dz


def loss_stage2(z, y, distill, p32=True):
    """masked BCE on probabilities over the elements with distill == 0, divided by their number; none left: 0 / 0 = NaN, and so is
    every gradient (0 * inf)"""
    sup = (np.asarray(distill, np.float64) == 0).astype(np.float64)
    l, d = bce_prob(z, y, p32)
    den = sup.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        return (l * sup).sum() / den, d * sup * (np.float64(1.0) / den)


def fixmatch_conf(zw, active):
    """the confident rows: every missing-class probability of the weak view above 0.8 or below 0.2; [B] bool"""
    p = sigmoid(zw)
    miss = np.asarray(active, np.float64) == 0
    ok = (p > 0.8) | (p < 0.2)
    return np.all(ok | ~miss[None, :], axis=1)


def loss_fixmatch(z, y, pos_w, pos_wu, active, inv_sup, cls_minus_ann):
    """z [2B][C]: weak rows, then strong rows.  Annotated classes: BCEWithLogits(weak, y; pos_w) inv_sup.  Missing classes of the
    confident rows: BCEWithLogits(strong, [sigmoid(weak) > 0.5]; pos_wu) / (n_conf cls_minus_ann); dropped when no row is
    confident or no class is missing.  dz [2B][C]: the weak half carries the supervised gradient, the strong half the other."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    B = y.shape[0]
    zw, zs = z[:B], z[B:]
    act = np.asarray(active, np.float64) != 0
    conf = fixmatch_conf(zw, active)
    n_idx, n_neg = int(conf.sum()), int((~act).sum())
    use = n_idx > 0 and n_neg > 0
    inv_uns = 1.0 / (n_idx * cls_minus_ann) if use else 0.0
    ls, ds = bce_logits(zw, y, np.asarray(pos_w, np.float64)[None, :])
    hard = (sigmoid(zw) > 0.5).astype(np.float64)
    lu, du = bce_logits(zs, hard, np.asarray(pos_wu, np.float64)[None, :])
    sel = (~act)[None, :] & conf[:, None] & use
    loss = ls[:, act].sum() * inv_sup + (lu * sel).sum() * inv_uns
    return loss, np.concatenate([np.where(act[None, :], ds * inv_sup, 0.0), np.where(sel, du * inv_uns, 0.0)], 0)
