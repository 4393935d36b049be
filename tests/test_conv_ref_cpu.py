"""tests/conv_ref.py (the float64 yardstick of tests/test_eff_conv_f32_gpu.py) pinned to F.conv2d + autograd in float64, the
exactness precondition of every dyadic case asserted on the data the GPU test uses, and the comparator shown to have teeth: the
references of a subtly wrong kernel must fall outside the random-family bounds.  No GPU."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fedmlp_amd import spec
from oracle import efficientnet_ref as O
from tests import conv_ref as CR
from tests import eff_ref as R
from tests import test_eff_kernels_gpu as GEN          # the operand generators and the swish / affine error terms (no GPU at import)

TOL = 1e-12
CONVS = CR.b0_convs()


def _close(name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    assert np.abs(got - want).max() <= TOL * scale, (name, float(np.abs(got - want).max()))


def _beyond(got, want, bound):
    """the comparator of the GPU test (`_within`): is any element further from `want` than its bound?"""
    return bool((np.abs(np.asarray(got, np.float64) - want) > bound).any())


@functools.lru_cache(maxsize=None)
def _sd(family):
    return CR.model_weights(GEN, family)


def test_conv_table():
    """33 convs; 96 x 96 gives maps of 48, 24, 12, 6 and 3; the padded channel counts are multiples of 16"""
    assert len(CONVS) == 33 and CONVS[0]["Kw"] == 48 and (CONVS[0]["hout"], CONVS[-1]["hout"]) == (48, 3)
    assert sorted({c["hout"] for c in CONVS}) == [3, 6, 12, 24, 48]
    assert all(c["cin_p"] % 16 == 0 and c["cout_p"] % 16 == 0 for c in CONVS[1:])
    nf, _ = spec.sizes("Efficient_b0", 5)
    assert sum(int(np.prod(v.shape)) for v in _sd("dyadic").values() if v.dtype == np.float32) == nf


@pytest.mark.parametrize("shape", [(3, 5, 7, 24, 40), (2, 3, 3, 144, 24), (1, 1, 1, 16, 96)], ids=str)
def test_pointwise_against_conv2d(shape):
    N, H, W, cin, cout = shape
    c = dict(cin=cin, cout=cout, k=1, kw_p=1, cin_p=CR.r16(cin), cout_p=CR.r16(cout), Kw=CR.r16(cin))
    rs = np.random.RandomState(sum(shape))
    w4 = rs.standard_normal((cout, cin, 1, 1))
    w = CR.weight_matrix(w4, c).reshape(c["cout_p"], c["Kw"])
    x, dy = rs.standard_normal((N, H, W, c["cin_p"])), rs.standard_normal((N, H, W, c["cout_p"]))
    xt = torch.tensor(x[..., :cin]).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.tensor(w4, requires_grad=True)
    y = F.conv2d(xt, wt)
    y.backward(torch.tensor(dy[..., :cout]).permute(0, 3, 1, 2))
    got = CR.pw_fwd(x, w)                                       # loud pad channels in x: zero weight columns hide them
    _close("fwd", got[..., :cout], y.detach().permute(0, 2, 3, 1).numpy())
    assert not got[..., cout:].any()
    dx = CR.pw_dgrad(dy, w)
    _close("dgrad", dx[..., :cin], xt.grad.permute(0, 2, 3, 1).numpy())
    assert not dx[..., cin:].any()
    xz, dyz = x.copy(), dy.copy()
    xz[..., cin:], dyz[..., cout:] = 0, 0
    dw = CR.pw_wgrad(xz, dyz)
    _close("wgrad", dw[:cout, :cin], wt.grad[:, :, 0, 0].numpy())
    assert not dw[cout:].any() and not dw[:, cin:].any()


@pytest.mark.parametrize("size", [(96, 96), (7, 9), (12, 5), (1, 2)], ids=str)
def test_stem_against_conv2d(size):
    H, W = size
    c = CR.b0_convs(H, W)[0]
    N = 2
    rs = np.random.RandomState(H * 7 + W)
    w4 = rs.standard_normal((32, 3, 3, 3))
    w = CR.weight_matrix(w4, c)
    assert w.shape == (32, 3, 4, 4) and not w[:, :, 3].any() and not w[..., 3].any()
    x, dy = rs.standard_normal((N, H, W, 4)), rs.standard_normal((N, c["hout"], c["wout"], 32))
    (pt, pb), (pl, pr) = O.same_pad(H, 3, 2), O.same_pad(W, 3, 2)
    assert (pt, pl) == (R.same_pad(H, 3, 2), R.same_pad(W, 3, 2)) and c["pad"] == pt
    xt = torch.tensor(x[..., :3]).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.tensor(w4, requires_grad=True)
    y = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt, None, 2)
    y.backward(torch.tensor(dy).permute(0, 3, 1, 2))
    _close("fwd", CR.stem_fwd(x, w, c), y.detach().permute(0, 2, 3, 1).numpy())
    xz = x.copy()
    xz[..., 3] = 0
    dw = CR.stem_wgrad(xz, dy, c)
    _close("wgrad", dw[:, :, :3, :3], wt.grad.permute(0, 2, 3, 1).numpy())
    assert not dw[:, :, 3].any() and not dw[..., 3].any()
    assert CR.conv_wgrad(xz, dy, c).shape == (32, 48)


def test_prologue_and_epilogue_against_torch():
    rs = np.random.RandomState(3)
    N, G, H, W, C = 6, 2, 3, 3, 16
    x, gate = rs.standard_normal((N, H, W, C)), rs.standard_normal((N, C))
    psc, psh = rs.standard_normal((G, C)), rs.standard_normal((G, C))
    xt = torch.tensor(x)
    gt = torch.tensor(gate)[:, None, None, :]
    _close("gate", CR.prologue(x, gate), (xt * gt).numpy())
    sc = torch.tensor(psc).repeat_interleave(N // G, 0)[:, None, None, :]
    sh = torch.tensor(psh).repeat_interleave(N // G, 0)[:, None, None, :]
    _close("affine", CR.prologue(x, gate, psc, psh), (F.silu(xt * sc + sh) * gt).numpy())
    scale, shift, res = rs.standard_normal(C), rs.standard_normal(C), rs.standard_normal(x.shape)
    v = xt * torch.tensor(scale) + torch.tensor(shift)
    _close("act0", CR.epilogue(x, scale, shift, res, 0), (v + torch.tensor(res)).numpy())
    _close("act1", CR.epilogue(x, scale, shift, res, 1), F.relu(v + torch.tensor(res)).numpy())
    _close("act2", CR.epilogue(x, scale, shift, None, 2), F.silu(v).numpy())


def test_arms_of_the_model():
    """the kernel arms the 33 convs reach at these shapes (what the GPU test's coverage assertion relies on): the streaming kernel gets
    M in {16, 32, 48, 80, 144, 240} (and 96, 480, 672, 1152) and K tails 16 .. 240; no conv of EfficientNet-B0 streams with M = 112
    (its 112-row outputs have K = 480 / 672: igemm; the 112-row data gradient has K = 672) and none has min(cout_p, Kw) = 96
    (CC = 6): the padded channel counts are 16, 32, 48, 80, 112, 192, 320 and 6x the real ones"""
    sm = {a[1] for c in CONVS for a in (CR.fwd_arm(c), CR.dgrad_arm(c)) if a[0] == "stream"}
    sk = {a[2] for c in CONVS for a in (CR.fwd_arm(c), CR.dgrad_arm(c)) if a[0] == "stream"}
    assert sm == {16, 32, 48, 80, 96, 144, 240, 480, 672, 1152}
    assert sk >= {16, 32, 48, 80, 112, 144, 240}
    assert {c["cout_p"] for c in CONVS if CR.fwd_arm(c)[0] == "igemm"} == {80, 112, 192, 320, 1280}
    cc = {a[1:3] for a in map(CR.wgrad_arm, CONVS) if a[0] == "skinny"}
    assert cc == {(n, s) for n in (1, 2, 3, 5, 7) for s in (False, True)}
    assert CR.wgrad_arm(CONVS[0]) == ("skinny", 2, True, True)
    assert sum(CR.wgrad_arm(c) == ("generic",) for c in CONVS) == 10
    pc = [CONVS[i] for i in CR.prologue_convs()]
    assert {(c["cin_p"], c["hout"] * c["wout"]) for c in pc if c["role"] == "project"} >= {(32, 2304), (96, 576), (144, 144), (240, 36)}
    assert {c["hout"] for c in pc} == {48, 24, 12, 6, 3} and all(c["cin_p"] <= 256 for c in pc)
    assert len(pc) == 4 + sum(c["k"] == 1 and c["cin_p"] <= 256 and c["hout"] <= 6 for c in CONVS) - 1      # (240 -> 80 at 6 x 6 counts once)


# ---- the dyadic precondition on the data actually used ------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(33))
def test_dyadic_sweep_is_exact(ci):
    """products are multiples of 1/4 and sum|terms| < 2^24 quarters in the forward, the data gradient and the weight gradient; the
    per-group sums of the output and of its squares (multiples of 1/16) stay below 2^24 units too"""
    o = CR.sweep_reference(GEN, "dyadic", ci, _sd("dyadic"))
    assert CR.sweep_exact(o), CONVS[ci]["name"]
    c = o["c"]
    assert not o["y"][..., c["cout"]:].any() and not o["dw"][c["cout"]:].any()
    assert not o["dw"].reshape(c["cout_p"], -1, c["cin_p"])[..., c["cin"]:].any()


@pytest.mark.parametrize("groups", [2, 1])
@pytest.mark.parametrize("ci", CR.prologue_convs())
def test_dyadic_prologue_is_exact(ci, groups):
    """x gate is a multiple of 1/8 below 2 in magnitude with few mantissa bits (a bf16 number: the split forms see it whole); its
    products with the weights are multiples of 1/16"""
    c = CONVS[ci]
    o = CR.operands(GEN, "dyadic", c, ci)
    gate, psc, psh = CR.prologue_operands(GEN, "dyadic", c, ci, groups)
    a = CR.prologue(o["x"], gate)
    assert np.array_equal(R.bf16_round(a), a)
    w = CR.weight_matrix(_sd("dyadic")[c["name"]], c)
    ya = CR.pw_fwd(np.abs(a), np.abs(w))
    assert CR.exact_terms(ya, 1.0 / 16)
    gate, psc, psh = CR.prologue_operands(GEN, "dyadic", c, ci, groups, zero_affine=True)
    assert not CR.prologue(o["x"], gate, psc, psh).any()
    assert len({tuple(g) for g in gate}) == len(gate)


@pytest.mark.parametrize("case", CR.epilogue_cases(), ids=str)
def test_dyadic_epilogue_is_exact(case):
    """y scale + shift + res: multiples of 1/16 whose absolute sum stays below 2^24 units, fused or not"""
    ci, act, res = case
    c = CONVS[ci]
    assert (CR.fwd_arm(c)[0], act) in {("stem", 2), ("stream", 2), ("igemm", 2), ("stream", 0), ("igemm", 0)}
    o = CR.sweep_reference(GEN, "dyadic", ci, _sd("dyadic"))
    scale, shift, r = CR.epilogue_operands(GEN, "dyadic", c, ci, act, res)
    assert CR.exact_terms(o["ya"] * np.abs(scale) + np.abs(shift) + (np.abs(r) if res else 0.0), 1.0 / 16)
    if act == 2:
        assert not CR.epilogue(o["y"], scale, shift, r, act).any()


# ---- the comparator has teeth ------------------------------------------------------------------------------------------------------------
def _lost_pixel(name, ci, n, rand_hit, mutate):
    """A sum over n pixels that loses one of them.  The worst-case bound of the random family, (n + 2) u sum|terms|, is n (n + 2) u times
    an average term: from n (n + 2) u >= 1 on (n >= 4096: the 48 x 48 maps) it may exceed the lost term itself, and the random family
    cannot see the loss.  Those cases rest on the dyadic family, where the same mutant must differ from the reference outright; below
    that size the random bound must catch it.  With the seeds of conv_ref three checks rest on the fallback: the stem's weight
    gradient, the stem's statistics, and the weight gradient of blocks.1's expand conv (all on the 48 x 48 map)."""
    if rand_hit:
        return
    assert n * (n + 2) * CR.U >= 1.0, f"{name}: the random-family bound misses a lost pixel among {n}"
    o = CR.sweep_reference(GEN, "dyadic", ci, _sd("dyadic"))
    got, want = mutate(o)
    assert not np.array_equal(got, want), f"{name}: the dyadic family misses it too"


def _wgrad_lost(o):
    return CR.conv_wgrad(o["xz"], CR.mut_drop_last_pixel(o["dyz"], CR.GROUPS), o["c"]), o["dw"]


def _stats_lost(o):
    return R.bn_stats(CR.mut_drop_last_pixel(o["y"], CR.GROUPS), CR.GROUPS), R.bn_stats(o["y"], CR.GROUPS)


@pytest.mark.parametrize("ci", range(33))
def test_mutants_fail_the_sweep_bounds(ci):
    """random family, every conv: a forward / data gradient without its last 16-k chunk, an output row written one row too far,
    and a weight gradient / statistics without the last pixel of each group fall outside the bounds the GPU test applies (the lost
    pixel on the 48 x 48 maps: see _lost_pixel)"""
    sd = _sd("random")
    o = CR.sweep_reference(GEN, "random", ci, sd)
    c, w = o["c"], o["w"]
    by = CR.dot_bound(c["Kw"], o["ya"])
    assert not _beyond(o["y"], o["y"], by)
    assert _beyond(CR.conv_fwd(o["x"], CR.mut_drop_last_chunk(w), c), o["y"], by), "fwd: last 16-k chunk"
    assert _beyond(CR.mut_row_shift(o["y"], c["cout"]), o["y"], by), "fwd: row shift"
    if c["cin"] != 3:
        bx = CR.dot_bound(c["cout_p"], o["dxa"])
        assert _beyond(CR.pw_dgrad(o["dy"], CR.mut_drop_last_chunk(w, True)), o["dx"], bx), "dgrad: last 16-k chunk"
        assert _beyond(CR.mut_row_shift(o["dx"], c["cin"]), o["dx"], bx), "dgrad: row shift"
    npix = CR.IMGS * c["hout"] * c["wout"]
    bw = CR.dot_bound(npix, o["dwa"])
    assert _beyond(CR.mut_row_shift(o["dw"].T, c["cout"]).T, o["dw"], bw), "wgrad: row shift"
    _lost_pixel("wgrad", ci, npix, _beyond(*_wgrad_lost(o), bw), _wgrad_lost)
    _lost_pixel("statistics", ci, npix // CR.GROUPS, _beyond(*_stats_lost(o), CR.stats_bound(o["y"], CR.GROUPS)), _stats_lost)


@pytest.mark.parametrize("groups", [2, 1])
@pytest.mark.parametrize("ci", CR.prologue_convs())
def test_mutants_fail_the_prologue_bounds(ci, groups):
    """random family, every prologue case: the next image's gate on the last pixel of each image, group 0's psc / psh for group 1,
    and the last 16-k chunk dropped fall outside the bound of the fused forward"""
    c = CONVS[ci]
    o = CR.operands(GEN, "random", c, ci)
    w = CR.weight_matrix(_sd("random")[c["name"]], c).reshape(c["cout_p"], c["Kw"])
    gate, psc, psh = CR.prologue_operands(GEN, "random", c, ci, groups)
    for form in ("gate", "affine"):
        sc, sh = (psc, psh) if form == "affine" else (None, None)
        want = CR.pw_fwd(CR.prologue(o["x"], gate, sc, sh), w)
        b = CR.prologue_bound(GEN, o["x"], gate, sc, sh, w)
        assert _beyond(CR.pw_fwd(CR.mut_gate_next_image(o["x"], gate, sc, sh), w), want, b), (form, "next image's gate")
        assert _beyond(CR.pw_fwd(CR.prologue(o["x"], gate, sc, sh), CR.mut_drop_last_chunk(w)), want, b), (form, "last chunk")
        if form == "affine" and groups > 1:
            assert _beyond(CR.pw_fwd(CR.mut_group0_affine(o["x"], gate, sc, sh), w), want, b), "group 0's affine"
