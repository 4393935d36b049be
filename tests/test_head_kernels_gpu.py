"""Kernel-level parity of the classifier head and the loss heads (csrc/heads.hip: k_avgpool, k_fc_fwd, k_fc_bwd, k_loss_bce, k_loss_stage1,
k_loss_stage2, k_loss_fixmatch), each launcher on its own through fm_debug_head, against the float64 restatement in tests/head_ref.py
(pinned to torch autograd and to oracle/steps_ref.py by tests/test_head_ref_cpu.py).  Buffers, canaries and the two input families
are those of tests/test_eff_kernels_gpu.py; worst error / bound ratios go to head_parity.json.

DYADIC: operands are small multiples of 1/2 or 1/4, so every product and partial sum is exact in fp32 and the result must equal the
reference bit for bit (`_exact` asserts the premise on the data used).  The losses enter with z = 0, where sigmoid = 1/2 exactly
(expf(0) = 1) and the gradients are dyadic; the loss value, which carries log 2, is held to its bound.
RANDOM: u = 2^-24; an n-term sum is within (n + c) u sum|terms| plus the terms' own errors, a bf16 store adds half a bf16 ulp.  The
loss elements are propagated operation by operation as (value, absolute error) pairs (`_mul`, `_add`; a product may underflow: + 2^-126).  expf, logf and log1pf: the
ROCm tree on the build machine carries no accuracy table for the device library, so each is ASSUMED within 2 ulp = 4 u relative
(KE, KL, KL1); the recorded ratios show how much of that is used.  Division and the other operations are correctly rounded (u).
So sigmoid(z) = 1 / (1 + expf(-z)) is within p (2 KE (1 - p) + 2) u of p (`_sigf`).

Logit bands of the loss tests.  smooth: |z| <= 8, held to the propagated bound (log(1 - p) amplifies the error of p by 1 / (1 - p):
3000 at z = 8, which the bound states and the kernel is held to).  saturated: |z| in [20, 80], where the fp32 sigmoid is exactly 1
(1 + expf(-z) rounds to 1 for z >= 17, whatever the ulps of expf) or 1 / expf(-z) = e^z up to those ulps: loss elements of 100,
gradients of exactly 0 and the softplus branch have determined values, and the same propagation with the error of p set to 0 at
p = 1 yields them.  mixed: both in one tensor.  |z| in (8, 20) is left out on purpose: where an fp32 sigmoid rounds to 1 differs
between correct implementations (it depends on the last bits of expf), and with it an element jumps between -log(1 - p) ~ 17 and the
clamp's 100."""
import numpy as np
import pytest

from tests import eff_ref as R
from tests import head_ref as H
from tests.test_eff_kernels_gpu import Buf, _canaries, _exact, _parity, DYW, DYC, F32, BF16

pytestmark = pytest.mark.gpu

U = R.U
KE = KL = KL1 = 2           # assumed ulps of expf, logf, log1pf (module docstring)
REPORT = {}
PW = [1.0, 0.05, 37.5]
TINY = 2.0 ** -126          # a product below the smallest normal fp32 number may be flushed to zero (e^-80 squared, say)


@pytest.fixture(scope="module")
def eng():
    """any handle serves: it owns the stream the launchers run on, nothing else"""
    from fedmlp_amd import spec
    from fedmlp_amd.engine import Engine
    e = Engine("Resnet18", 5, 64, 64, 4)
    flat, cnt = spec.init_state("Resnet18", 5, 3)
    e.set_state(flat, cnt)
    yield e
    e.close()


_bits, _within, _check = _parity(REPORT, "head_parity.json")


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _vals(family, rs, shape, bf=False):
    if family == "dyadic":
        return rs.randint(-4, 5, shape) / 2.0
    x = rs.standard_normal(shape)
    return R.bf16_round(x) if bf else _f32(x)


# ---- avgpool ------------------------------------------------------------------------------------------------------------------------
# (imgs, HW, C): 512 / 1280 = two / five trips of the 256 threads; 8: most threads idle; 300: neither a multiple of 256 nor of 64
@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 49, 512), (2, 4, 1280), (1, 1, 8), (2, 9, 300)], ids=str)
def test_avgpool(eng, shape, dt, family):
    """feat = mean over HW: HW - 1 additions and a division: HW u sum|x| / HW.  Dyadic: halves in [-2, 2]; HW a power of two: bit for
    bit; otherwise the division rounds once: feat HW is within 1 ulp (2 u) of the exact sum."""
    imgs, HW, C = shape
    bf = dt == BF16
    rs = np.random.RandomState(10 + HW + C)
    x = _vals(family, rs, shape, bf)
    pool = []
    xb, fb = Buf(eng, x.size, bf, x, pool), Buf(eng, imgs * C, pool=pool)
    eng.debug_head("avgpool", [xb.t, fb.t], [dt, imgs, HW, C])
    name = f"avgpool {shape}{'bf16' if bf else 'f32'}"
    _canaries(pool, name)
    got, want = fb.np((imgs, C)), H.avgpool(x)
    if family == "dyadic":
        _exact(x[0], 1 / 2)
        if HW & (HW - 1) == 0:
            _bits(name, got, want)
        else:
            _within(name + " sum", got.astype(np.float64) * HW, x.sum(1), 2 * U * np.abs(x.sum(1)), family)
    else:
        _within(name, got, want, HW * U * np.abs(x).sum(1) / HW)


# ---- fc -----------------------------------------------------------------------------------------------------------------------------
# (imgs, D, C, HW): imgs 1, 3, 5, 9 = every remainder of the weight gradient's 4-image-lane fold; D = 100: a ragged 64-column block;
# C = 32 = FM_MAXC; C = 1: three of fc_fwd's four waves idle
FC_SHAPES = [(5, 512, 5, 4), (3, 1280, 14, 1), (1, 100, 32, 3), (9, 64, 1, 2)]


def _fc_operands(family, rs, shape):
    imgs, D, C, HW = shape
    if family == "dyadic":
        return (rs.randint(-4, 5, (imgs, D)) / 2.0, rs.choice(DYW, (C, D)), rs.choice(DYC, C), rs.randint(-4, 5, (imgs, C)) / 2.0,
                rs.choice([0.0, 2.0], (imgs, D)), rs.randint(-4, 5, (imgs, D)) / 2.0)
    f = lambda *s: _f32(rs.standard_normal(s))
    return f(imgs, D), f(C, D) / np.sqrt(D), f(C), f(imgs, C), _f32((rs.rand(imgs, D) < 0.8) / 0.8), f(imgs, D)


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("shape", FC_SHAPES, ids=str)
def test_fc_fwd(eng, shape, family):
    """logits = feat W^T + b: D rounded products summed (64 lanes, then the wave) and the bias: (D + 2) u (sum|feat W| + |b|)"""
    imgs, D, C, HW = shape
    rs = np.random.RandomState(20 + D)
    feat, W, b, _, _, _ = _fc_operands(family, rs, shape)
    W = _f32(W)
    pool = []
    bufs = [Buf(eng, t.size, False, t, pool) for t in (feat, W, b)]
    ob = Buf(eng, imgs * C, pool=pool)
    eng.debug_head("fc_fwd", [t.t for t in bufs] + [ob.t], [imgs, D, C])
    _canaries(pool, f"fc_fwd {shape}")
    if family == "dyadic":
        _exact((np.abs(feat).max() * np.abs(W)).T, 1 / 8)
    _check(family, f"fc_fwd {shape}", ob.np((imgs, C)), H.fc_fwd(feat, W, b), (D + 2) * U * (np.abs(feat) @ np.abs(W).T + np.abs(b)))


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", FC_SHAPES, ids=str)
def test_fc_bwd(eng, shape, dt, family):
    """all four (mask, dfeat) arms.  dW = dz^T feat: (imgs + 1) u sum|dz feat|; db: imgs u sum|dz|; s = dz W: (C + 1) u sum|dz W| = e_s.
    Without dfeat: (s inv) mask with inv = fl(1 / HW): (e_s / HW + 2 u |s / HW|) |mask| + u |dout|; with dfeat: (s mask + dfeat) inv:
    (|mask| e_s + u |s mask| + u |s mask + dfeat|) / HW + 2 u |dout| (+ half a bf16 ulp).  Every pixel p < HW of dout[img] must carry the
    same bits.  Dyadic: mask in {0, 2}; HW a power of two: bit for bit; HW = 3: inv is inexact, held to the bound."""
    imgs, D, C, HW = shape
    bf = dt == BF16
    rs = np.random.RandomState(30 + D)
    feat, W, _, dz, mask, dfeat = _fc_operands(family, rs, shape)
    W = _f32(W)
    for use_mask in (False, True):
        for use_dfeat in (False, True):
            name = f"fc_bwd {shape}{'bf16' if bf else 'f32'}{'+mask' if use_mask else ''}{'+dfeat' if use_dfeat else ''}"
            pool = []
            ins = [Buf(eng, t.size, False, t, pool) for t in (dz, feat, W)]
            mb = Buf(eng, mask.size, False, mask, pool) if use_mask else None
            dfb = Buf(eng, dfeat.size, False, dfeat, pool) if use_dfeat else None
            dWb, dbb, dob = Buf(eng, C * D, pool=pool), Buf(eng, C, pool=pool), Buf(eng, imgs * HW * D, bf, pool=pool)
            eng.debug_head("fc_bwd", [t.t for t in ins] + [mb and mb.t, dWb.t, dbb.t, dob.t, dfb and dfb.t], [dt, imgs, D, C, HW])
            _canaries(pool, name)
            m, df = (mask if use_mask else None), (dfeat if use_dfeat else None)
            dW, db, dpix = H.fc_bwd(dz, feat, W, HW, m, df)
            if family == "dyadic":
                _exact(np.abs(dz).max() * np.abs(feat), 1 / 4)
                _exact((np.abs(dz).max() * np.abs(W)), 1 / 8)
            _check(family, name + " dW", dWb.np((C, D)), dW, (imgs + 1) * U * (np.abs(dz).T @ np.abs(feat)))
            _check(family, name + " db", dbb.np((C,)), db, imgs * U * np.abs(dz).sum(0))
            got = dob.np((imgs, HW, D))
            assert (got.view(np.uint32) == got[:, :1].view(np.uint32)).all(), f"{name}: the pixels of an image differ"
            s, es = dz @ W, (C + 1) * U * (np.abs(dz) @ np.abs(W))
            am = np.abs(mask) if use_mask else 1.0
            if use_dfeat:
                bound = (am * es + (U * np.abs(s * am) if use_mask else 0.0) + U * np.abs(dpix * HW)) / HW + 2 * U * np.abs(dpix)
            else:
                bound = (es / HW + 2 * U * np.abs(s / HW)) * am + U * np.abs(dpix)
            fam = family if (HW & (HW - 1) == 0 or family == "random") else "dyadic-within"
            if fam == "dyadic-within":
                _within(name + " dout", got[:, 0], dpix, bound + (R.half_ulp_bf16(np.abs(dpix) + bound) if bf else 0.0), "dyadic")
            else:
                _check(fam, name + " dout", got[:, 0], dpix, bound, bf)


# ---- (value, absolute error) arithmetic of the loss elements -----------------------------------------------------------------------
def _mul(a, b):
    (av, ae), (bv, be) = a, b
    v = av * bv
    return v, np.abs(av) * be + np.abs(bv) * ae + ae * be + U * np.abs(v) + TINY


def _add(a, b):
    v = a[0] + b[0]
    return v, a[1] + b[1] + U * np.abs(v)


def _sigf(z):
    """sigmoidf_ of heads.hip: t = expf(-z) within 2 KE u t, 1 + t and the division one rounding each; t / (1 + t) = 1 - p"""
    p = H.sigmoid(z)
    return p, p * (2 * KE * H.one_minus_sigmoid(z) + 2) * U


def _bce_logits_err(z, y, pw):
    """bce_logits of heads.hip: (l, its error, dz, its error)"""
    lw = 1.0 + (pw - 1.0) * y
    elw = 2 * U * np.abs((pw - 1.0) * y) + U * np.abs(lw)
    t = np.exp(-np.abs(z))
    s1 = np.log1p(t)
    e1 = 2 * KE * U * t / (1 + t) + 2 * KL1 * U * s1                   # log1p is 1 / (1 + t)-Lipschitz
    sp = (s1 + np.maximum(-z, 0.0), e1)
    sp = (sp[0], sp[1] + U * np.abs(sp[0]))
    a = ((1.0 - y) * z, 2 * U * np.abs((1.0 - y) * z))
    l = _add(a, _mul((lw, elw), sp))
    p, ep = _sigf(z)
    om = H.one_minus_sigmoid(z)
    c = _mul((lw, elw), (om, ep + U * om))
    d = (1.0 - y) - c[0]
    return l[0], l[1], d, U * np.abs(1.0 - y) + c[1] + U * np.abs(d)


def _bce_prob_err(z, y):
    """bce_prob of heads.hip against head_ref.bce_prob (p rounded to fp32: one more u p): (l, its error, dz, its error).  Where the
    reference's p is 1 every fp32 sigmoid is (module docstring): the error of p, and of everything formed from it, is 0."""
    l, d = H.bce_prob(z, y)
    p = H.prob(z)
    q = 1.0 - p
    ep = np.where(p == 1.0, 0.0, p * (2 * KE * H.one_minus_sigmoid(z) + 3) * U)
    eq = np.where(p == 1.0, 0.0, ep + U * q)
    with np.errstate(divide="ignore", invalid="ignore"):
        elp = -np.log1p(-np.minimum(ep / p, 0.5)) + 2 * KL * U * np.abs(np.log(p))
        elq = np.where(q > 0, -np.log1p(-np.minimum(eq / np.where(q > 0, q, 1.0), 0.5)) + 2 * KL * U * np.abs(np.log(np.where(q > 0, q, 1.0))), 0.0)
    lp, lq = np.maximum(np.log(p), -100.0), np.where(q > 0, np.maximum(np.log(np.where(q > 0, q, 1.0)), -100.0), -100.0)
    el = y * elp + (1 - y) * elq + 2 * U * (np.abs(y * lp) + np.abs((1 - y) * lq)) + U * np.abs(l)
    A, eA = p - y, ep + U * np.abs(p - y)
    pq, epq = _mul((p, ep), (q, eq))
    Bm = np.maximum(pq, H.EPS_PQ)
    r = A / Bm
    er = eA / Bm + np.abs(A) * epq / (Bm * (Bm - np.minimum(epq, 0.5 * Bm))) + U * np.abs(r)
    dz, edz = _mul((r, er), (pq, epq))
    assert np.allclose(dz, d, rtol=1e-12, atol=0)
    return l, el, d, edz


def _sum_err(terms, errs, n):
    """n-term fp32 sum in any order plus the 10 roundings of the block reduction and the final scale: (n + 10) u sum|t| + sum e"""
    return (n + 10) * U * np.abs(terms).sum() + errs.sum()


def _band(rs, shape, kind):
    """logits of one band, fp32 numbers"""
    smooth = rs.uniform(-8, 8, shape)
    sat = rs.uniform(20, 80, shape) * rs.choice([-1.0, 1.0], shape)
    z = {"smooth": smooth, "saturated": sat, "mixed": np.where(rs.rand(*shape) < 0.5, smooth, sat)}[kind]
    z = _f32(z)
    assert ((np.abs(z) <= 8) | ((np.abs(z) >= 20) & (np.abs(z) <= 80))).all()
    return z


def _labels(rs, B, C):
    return (rs.rand(B, C) < 0.4).astype(np.float64)


def _pw(rs, C):
    pw = rs.choice(PW, C)
    pw[:3] = PW                                   # every value occurs, whatever the draw
    return _f32(pw)


def _active(kind, C):
    return {"all": np.ones(C), "none": np.zeros(C), "alt": (np.arange(C) % 2).astype(np.float64)}[kind]


def _loss_launch(eng, op, dev, host, n_dz, dims, scalars, name):
    """dev: device operands in order, host: {position: list}; the two results are appended; -> (dz, loss)"""
    pool = []
    bufs = [Buf(eng, t.size, False, t, pool) for t in dev]
    dzb, lb = Buf(eng, n_dz, pool=pool), Buf(eng, 1, pool=pool)
    ptrs = [b.t for b in bufs]
    for k in sorted(host):
        ptrs.insert(k, [float(v) for v in host[k]])
    eng.debug_head(op, ptrs + [dzb.t, lb.t], dims, scalars)
    _canaries(pool, name)
    return dzb.np()[:n_dz], float(lb.np()[0])


BC = [(B, C) for B in (1, 7, 52, 128) for C in (5, 14, 32)]      # B C from 5 (below one wave) to 4096 (16 strides of the block)
BANDS = ["smooth", "saturated", "mixed"]


@pytest.mark.parametrize("bc", BC, ids=str)
def test_loss_bce(eng, bc):
    """k_loss_bce in the three bands with pos_weight in {1, 0.05, 37.5}; dyadic: z = 0, y and pos_weight dyadic, inv_norm = 1/64:
    gradients bit for bit.  Bounds: `_bce_logits_err`, scaled by inv_norm (one rounding); the loss: `_sum_err`."""
    B, C = bc
    rs = np.random.RandomState(100 + B + C)
    inv = float(np.float32(1.0 / (B * C)))
    for band in BANDS:
        z, y, pw = _band(rs, (B, C), band), _labels(rs, B, C), _pw(rs, C)
        name = f"loss_bce {bc}{band}"
        dz, loss = _loss_launch(eng, "loss_bce", [z, y], {2: pw}, B * C, [B, C], [inv], name)
        l, el, d, ed = _bce_logits_err(z, y, pw[None, :])
        want_l, want_d = H.loss_bce(z, y, pw, inv)
        _within(name + " dz", dz.reshape(B, C), want_d, ed * inv + U * np.abs(want_d) + TINY)
        _within(name + " loss", loss, want_l, _sum_err(l, el, B * C) * inv + U * abs(want_l))
    z, y, pw = np.zeros((B, C)), rs.choice([0.0, 0.25, 0.5, 1.0], (B, C)), rs.choice([1.0, 0.5, 2.0, 4.0], C)
    dz, loss = _loss_launch(eng, "loss_bce", [z, y], {2: pw}, B * C, [B, C], [1 / 64], f"loss_bce {bc}dyadic")
    want_l, want_d = H.loss_bce(z, y, pw, 1 / 64)
    _exact(want_d.reshape(-1, 1), 2.0 ** -12)
    _bits(f"loss_bce {bc} dz", dz.reshape(B, C), want_d)
    l, el, d, ed = _bce_logits_err(z, y, pw[None, :])
    _within(f"loss_bce {bc} loss", loss, want_l, _sum_err(l, el, B * C) / 64 + U * abs(want_l), "dyadic")


@pytest.mark.parametrize("bc", BC, ids=str)
def test_loss_stage1(eng, bc):
    """k_loss_stage1: rows r and r + B share label row r; teacher logits drawn independently of the student's; active masks all /
    none / alternating (inv_dis = 0 when nothing is missing).  Annotated classes: `_bce_prob_err` halved; the others: e = p - q from
    two `_sigf`, e^2 / 2 and e p (1 - p) by `_mul`.  Dyadic (z = g = 0, every class annotated): gradients (1/2 - y) / 2 inv_sup bit for
    bit."""
    B, C = bc
    rs = np.random.RandomState(200 + B + C)
    bs = B + 3
    for band in BANDS:
        for kind in ("all", "none", "alt"):
            z, g, y, active = _band(rs, (2 * B, C), band), _band(rs, (2 * B, C), band), _labels(rs, B, C), _active(kind, C)
            act = active != 0
            ann, n_neg = max(int(act.sum()), 1), int((~act).sum())
            inv_sup, inv_dis = float(np.float32(1.0 / (bs * ann))), (float(np.float32(1.0 / (bs * n_neg))) if n_neg else 0.0)
            name = f"loss_stage1 {bc}{band}-{kind}"
            dz, loss = _loss_launch(eng, "loss_stage1", [z, g, y], {3: active}, 2 * B * C, [B, C], [inv_sup, inv_dis], name)
            want_l, want_d = H.loss_stage1(z, g, y, active, inv_sup, inv_dis)
            l, el, d, ed = _bce_prob_err(z, np.concatenate([y, y], 0))
            p, q = _sigf(z), _sigf(g)
            e = (p[0] - q[0], p[1] + q[1] + U * np.abs(p[0] - q[0]))
            om = H.one_minus_sigmoid(z)
            t_dis = _mul((0.5 * e[0], 0.5 * e[1]), e)
            d_dis = _mul(_mul(_mul(e, p), (om, p[1] + U * om)), (inv_dis, 0.0))
            ed_all = np.where(act[None, :], 0.5 * ed * inv_sup + U * np.abs(want_d) + TINY, d_dis[1])
            _within(name + " dz", dz.reshape(2 * B, C), want_d, ed_all)
            E1 = _sum_err((0.5 * l)[:, act], (0.5 * el)[:, act], 2 * B * C)
            E2 = _sum_err(t_dis[0][:, ~act], t_dis[1][:, ~act], 2 * B * C)
            _within(name + " loss", loss, want_l, E1 * inv_sup + E2 * inv_dis + 3 * U * abs(want_l))
    z, y = np.zeros((2 * B, C)), rs.choice([0.0, 0.25, 0.5, 1.0], (B, C))
    dz, loss = _loss_launch(eng, "loss_stage1", [z, z, y], {3: np.ones(C)}, 2 * B * C, [B, C], [1 / 16, 0.0], f"loss_stage1 {bc}dyadic")
    want_l, want_d = H.loss_stage1(z, z, y, np.ones(C), 1 / 16, 0.0)
    _bits(f"loss_stage1 {bc} dz", dz.reshape(2 * B, C), want_d)
    l, el, _, _ = _bce_prob_err(z, np.concatenate([y, y], 0))
    _within(f"loss_stage1 {bc} loss", loss, want_l, _sum_err(0.5 * l, 0.5 * el, 2 * B * C) / 16 + 3 * U * abs(want_l), "dyadic")


@pytest.mark.parametrize("bc", BC, ids=str)
def test_loss_stage2(eng, bc):
    """k_loss_stage2 with no, some and all elements distilled.  den = the count (exact), inv = 1 / den (one rounding), dz = d sup inv.
    All distilled: 0 / 0 -- the loss and every gradient are NaN in the kernel as in the reference.  Dyadic: z = 0 and a power-of-two
    count of supervised elements: gradients bit for bit."""
    B, C = bc
    rs = np.random.RandomState(300 + B + C)
    for band in BANDS:
        for frac in (0.0, 0.4, 1.0):
            z, y = _band(rs, (B, C), band), _labels(rs, B, C)
            distill = (rs.rand(B, C) < frac) * rs.choice([1.0, -1.0, 0.5], (B, C)) if frac < 1 else np.ones((B, C))
            name = f"loss_stage2 {bc}{band}-{frac}"
            dz, loss = _loss_launch(eng, "loss_stage2", [z, y, distill], {}, B * C, [B, C], [], name)
            want_l, want_d = H.loss_stage2(z, y, distill)
            if frac == 1.0:
                assert np.isnan(want_l) and np.isnan(want_d).all()
                assert np.isnan(loss) and np.isnan(dz).all(), f"{name}: 0 / 0 must give NaN"
                continue
            sup = (distill == 0).astype(np.float64)
            den = sup.sum()
            if den == 0:
                continue
            l, el, d, ed = _bce_prob_err(z, y)
            _within(name + " dz", dz.reshape(B, C), want_d, ed * sup / den + 2 * U * np.abs(want_d) + TINY)
            _within(name + " loss", loss, want_l, _sum_err(l * sup, el * sup, B * C) / den + U * abs(want_l))
    n = B * C
    keep = 1 << (n.bit_length() - 1)
    z, y = np.zeros((B, C)), rs.choice([0.0, 0.25, 0.5, 1.0], (B, C))
    distill = (np.arange(n) >= keep).astype(np.float64).reshape(B, C)
    dz, loss = _loss_launch(eng, "loss_stage2", [z, y, distill], {}, n, [B, C], [], f"loss_stage2 {bc}dyadic")
    want_l, want_d = H.loss_stage2(z, y, distill)
    _bits(f"loss_stage2 {bc} dz", dz.reshape(B, C), want_d)
    l, el, _, _ = _bce_prob_err(z, y)
    _within(f"loss_stage2 {bc} loss", loss, want_l, _sum_err(l * (distill == 0), el * (distill == 0), n) / keep + U * abs(want_l), "dyadic")


def _fixmatch_weak(rs, B, C, active, case):
    """weak logits: annotated classes smooth; missing classes per case.  thresholds: values at +-(logit 0.8 +- delta) and +-delta,
    delta = 2^-6, on either side of 0.2 / 0.8 / 0.5, and +-30; row 0 confident.  none: every row holds one value inside (0.2, 0.8).
    every: all confident."""
    d, t = 2.0 ** -6, np.log(4.0)
    zw = _band(rs, (B, C), "smooth")
    miss = active == 0
    conf_vals = np.array([t + d, -(t + d), 30.0, -30.0, 75.0])
    all_vals = np.concatenate([conf_vals, [t - d, -(t - d), d, -d]])
    pick = rs.choice(conf_vals if case == "every" else all_vals, (B, C))
    if case == "thresholds":
        pick[0] = rs.choice(conf_vals, C)
    if case == "none" and miss.any():
        pick[:, np.flatnonzero(miss)[0]] = rs.choice([t - d, -(t - d), d, -d], B)
    return _f32(np.where(miss[None, :], pick, zw))


@pytest.mark.parametrize("bc", BC, ids=str)
def test_loss_fixmatch(eng, bc):
    """k_loss_fixmatch.  The gate: weak missing-class logits on either side of all three thresholds (`_fixmatch_weak`; the margin
    |p - threshold| > 1e-3 makes the decision the same in fp32, asserted); cases: thresholds (confident and unconfident rows), no
    confident row, every row confident, no missing class, every class missing.  The strong half of dz must be exactly zero for
    unconfident rows and annotated classes, the weak half for missing classes (their bound is 0).  Supervised part: `_bce_logits_err`
    inv_sup; unsupervised: `_bce_logits_err` on the strong logits with the hard labels, inv_uns = 1 / (n_conf cls_minus_ann) (one
    rounding).  Dyadic, for every B: weak = strong = 0 in annotated classes; a power-of-two number of rows (4 of 7, 32 of 52, 64 of
    128) is confident with +-30 in every missing class, the others hold 0 in one: gradients bit for bit, the strong half of the
    unconfident rows +0, and the loss value s1 inv_sup + s2 inv_uns (it carries log 2) within the bound of the random family."""
    B, C = bc
    rs = np.random.RandomState(400 + B + C)
    bs = B + 1
    for case, kind in (("thresholds", "alt"), ("none", "alt"), ("every", "alt"), ("thresholds", "all"), ("every", "none")):
        active = _active(kind, C)
        act = active != 0
        ann = max(int(act.sum()), 1)
        cma = C - int(act.sum())
        zw, zs = _fixmatch_weak(rs, B, C, active, case), _band(rs, (B, C), "mixed")
        z, y, pw, pwu = np.concatenate([zw, zs], 0), _labels(rs, B, C), _pw(rs, C), _pw(rs, C)[::-1].copy()
        p = H.sigmoid(zw)[:, ~act]
        assert (np.abs(p - 0.8) > 1e-3).all() and (np.abs(p - 0.2) > 1e-3).all()
        conf = H.fixmatch_conf(zw, active)
        assert (np.abs(H.sigmoid(zw)[conf][:, ~act] - 0.5) > 0.29).all()
        if kind == "all":
            assert conf.all()
        elif case == "none":
            assert not conf.any()
        elif case == "every":
            assert conf.all()
        else:
            assert conf[0] and (B < 7 or not conf.all())
        inv_sup = float(np.float32(1.0 / (bs * ann)))
        name = f"loss_fixmatch {bc}{case}-{kind}"
        dz, loss = _loss_launch(eng, "loss_fixmatch", [z, y], {2: pw, 3: pwu, 4: active}, 2 * B * C, [B, C, cma], [inv_sup], name)
        want_l, want_d = H.loss_fixmatch(z, y, pw, pwu, active, inv_sup, cma)
        use = conf.any() and cma > 0
        inv_uns = 1.0 / (conf.sum() * cma) if use else 0.0
        sel = (~act)[None, :] & conf[:, None] & use
        ls, els, ds, eds = _bce_logits_err(zw, y, pw[None, :])
        hard = (H.sigmoid(zw) > 0.5).astype(np.float64)
        lu, elu, du, edu = _bce_logits_err(zs, hard, pwu[None, :])
        ed = np.concatenate([np.where(act[None, :], eds * inv_sup + U * np.abs(want_d[:B]) + TINY, 0.0),
                             np.where(sel, edu * inv_uns + 2 * U * np.abs(want_d[B:]) + TINY, 0.0)], 0)
        got = dz.reshape(2 * B, C)
        _within(name + " dz", got, want_d, ed)
        assert not got[B:][~conf].any() and not got[B:, act].any() and not got[:B, ~act].any()
        E1 = _sum_err(ls[:, act], els[:, act], B * C)
        E2 = _sum_err(lu * sel, elu * sel, B * C)
        _within(name + " loss", loss, want_l, E1 * inv_sup + (E2 + U * np.abs(lu * sel).sum()) * inv_uns + 3 * U * abs(want_l))
    # dyadic: a power-of-two number of rows confident (+-30 in every missing class), scattered among the others, which hold 0
    # (p = 1/2) in their first missing class: inv_uns = 1 / (n_conf 4) and inv_sup = 1/8 are exact, and so is every gradient
    n_conf = 1 << (B.bit_length() - 1)
    n_conf = n_conf // 2 if n_conf == B and B > 1 else n_conf
    active = _active("alt", C)
    act = active != 0
    rows = np.zeros(B, bool)
    rows[rs.permutation(B)[:n_conf]] = True
    zw = np.where(act[None, :], 0.0, rs.choice([30.0, -30.0], (B, C)))
    zw[~rows, np.flatnonzero(~act)[0]] = 0.0
    z = np.concatenate([zw, np.zeros((B, C))], 0)
    y, pw, pwu = rs.choice([0.0, 0.25, 0.5, 1.0], (B, C)), rs.choice([1.0, 0.5, 2.0, 4.0], C), rs.choice([1.0, 0.5, 2.0, 4.0], C)
    conf = H.fixmatch_conf(zw, active)
    assert np.array_equal(conf, rows) and conf.sum() == n_conf and (B < 7 or not conf.all())
    name = f"loss_fixmatch {bc}dyadic"
    dz, loss = _loss_launch(eng, "loss_fixmatch", [z, y], {2: pw, 3: pwu, 4: active}, 2 * B * C, [B, C, 4], [1 / 8], name)
    want_l, want_d = H.loss_fixmatch(z, y, pw, pwu, active, 1 / 8, 4)
    assert want_d[B:][conf][:, ~act].all() and not want_d[B:][~conf].any()
    _exact(want_d.reshape(-1, 1), 2.0 ** -16)
    _bits(f"loss_fixmatch {bc} dz", dz.reshape(2 * B, C), want_d)
    sel = (~act)[None, :] & conf[:, None]
    ls, els, _, _ = _bce_logits_err(zw, y, pw[None, :])
    lu, elu, _, _ = _bce_logits_err(np.zeros((B, C)), (H.sigmoid(zw) > 0.5).astype(np.float64), pwu[None, :])
    E1, E2 = _sum_err(ls[:, act], els[:, act], B * C), _sum_err(lu * sel, elu * sel, B * C)
    _within(f"loss_fixmatch {bc} loss", loss, want_l, E1 / 8 + (E2 + U * np.abs(lu * sel).sum()) / (4 * n_conf) + 3 * U * abs(want_l), "dyadic")


# ---- contract -----------------------------------------------------------------------------------------------------------------------
def test_contract_errors(eng):
    """arguments outside a kernel's contract return FM_ERR_ARG before any launch: the outputs keep their NaN fill"""
    from fedmlp_amd._lib import FmError
    pool = []
    x = Buf(eng, 4096, False, np.ones(4096), pool)
    o1, o2, o3 = Buf(eng, 4096, pool=pool), Buf(eng, 64, pool=pool), Buf(eng, 4096, pool=pool)
    v = [1.0] * 33
    cases = [("avgpool", [x.t, None], [F32, 2, 4, 8]),                                           # missing operand
             ("avgpool", [x.t, o1.t], [2, 2, 4, 8]),                                             # unknown dt
             ("avgpool", [x.t, o1.t], [F32, 2, 0, 8]),                                           # a dimension < 1
             ("fc_fwd", [x.t, x.t, x.t, None], [2, 8, 4]),
             ("fc_fwd", [x.t, x.t, x.t, o1.t], [2, 8, 33]),                                      # C > FM_MAXC
             ("fc_fwd", [x.t, x.t, x.t, o1.t], [0, 8, 4]),
             ("fc_bwd", [x.t, x.t, x.t, None, o1.t, o2.t, None], [F32, 2, 8, 4, 2]),              # dout missing
             ("fc_bwd", [x.t, x.t, x.t, None, o1.t, o2.t, o3.t], [3, 2, 8, 4, 2]),                # unknown dt
             ("fc_bwd", [x.t, x.t, x.t, None, o1.t, o2.t, o3.t], [F32, 2, 8, 33, 2]),             # C > FM_MAXC
             ("fc_bwd", [x.t, x.t, x.t, None, o1.t, o2.t, o3.t], [F32, 2, 8, 4, 0]),              # HW < 1
             ("loss_bce", [x.t, x.t, None, o1.t, o2.t], [4, 5]),                                 # pos_w missing
             ("loss_bce", [x.t, x.t, v, o1.t, o2.t], [4, 33]),
             ("loss_bce", [x.t, x.t, v, o1.t, o2.t], [0, 5]),
             ("loss_stage1", [x.t, x.t, x.t, v, o1.t, None], [4, 5]),                            # loss missing
             ("loss_stage1", [x.t, x.t, x.t, v, o1.t, o2.t], [4, 33]),
             ("loss_stage2", [x.t, x.t, None, o1.t, o2.t], [4, 5]),                              # distill missing
             ("loss_stage2", [x.t, x.t, x.t, o1.t, o2.t], [4, 0]),
             ("loss_fixmatch", [x.t, x.t, v, v, v, o1.t, o2.t], [2049, 1, 1]),                   # B > 2048: the LDS table
             ("loss_fixmatch", [x.t, x.t, v, v, None, o1.t, o2.t], [4, 5, 1]),                   # active missing
             ("loss_fixmatch", [x.t, x.t, v, v, v, o1.t, o2.t], [4, 33, 1]),
             ("loss_fixmatch", [x.t, x.t, v, v, v, o1.t, o2.t], [4, 5, -1]),
             ("loss_fixmatch", [x.t, x.t, v, v, [0.0] + v, o1.t, o2.t], [4, 5, 0])]               # a missing class and cls_minus_ann = 0: 1 / 0
    for op, ptrs, d in cases:
        with pytest.raises(FmError, match="bad argument"):
            eng.debug_head(op, ptrs, d, [1.0, 1.0])
    for b in (o1, o2, o3):
        assert np.isnan(b.np()).all(), "a refused call launched something"
    _canaries(pool, "contract")
    eng.debug_head("loss_fixmatch", [x.t, x.t, v, v, v, o1.t, o2.t], [2048, 1, 1], [1.0])       # the largest B the table holds runs
    assert not np.isnan(o1.np()[:4096]).any() and not np.isnan(o2.np()[:1]).any()
    _canaries(pool, "contract")
