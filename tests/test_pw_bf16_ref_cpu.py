"""tests/pw_bf16_ref.py (the float64 yardstick of tests/test_pw_bf16_gpu.py) pinned to torch float64 (F.conv2d, autograd, plain
matmul) on the padded layouts, the dyadic preconditions asserted on the data the GPU test uses (every operand and weight a bf16
number, every sum exact in fp32), the launch predicates pinned to the arms the model reaches, and the comparator shown to have
teeth: what a subtly wrong kernel would compute falls outside the bound the GPU test applies to the true result in the random
family, and differs in at least one stored word in the dyadic family.  No GPU."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as CR
from tests import eff_ref as R
from tests import pw_bf16_ref as P
from tests import test_eff_kernels_gpu as GEN          # the operand generators and the swish / affine error terms (no GPU at import)

TOL = 1e-12
CONVS = {s: CR.b0_convs(s, s) for s in P.SIDES}
C96 = CONVS[96]
IMGS, GROUPS = P.IMGS, P.GROUPS


def _close(name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    assert np.abs(got - want).max() <= TOL * scale, (name, float(np.abs(got - want).max()))


def _stored(bound, want, bf=True):
    """the bound the GPU test's _check applies to a stored result: a bf16 store adds half a bf16 ulp of |value| + bound"""
    return bound + (P.hb(np.abs(want) + bound) if bf else 0.0)


def _beyond(got, want, bound):
    return bool((np.abs(np.asarray(got, np.float64) - want) > bound).any())


def _words_differ(got, want):
    """the stored bf16 words of two dyadic results differ somewhere"""
    return not np.array_equal(R.bf16_round(got), R.bf16_round(want))


@functools.lru_cache(maxsize=None)
def _sd(family):
    return CR.model_weights(GEN, family)


@functools.lru_cache(maxsize=4)
def _case(family, ci, side=96):
    return P.sweep_reference(GEN, family, ci, _sd(family), CONVS[side])


# ---- the new reference functions against torch ---------------------------------------------------------------------------------------------
def test_bf16_model_of_the_weights():
    """the shadow is the master rounded to nearest even; pad rows and columns stay zero; dyadic weights are their own shadow"""
    for family in ("dyadic", "random"):
        for c in (C96[0], C96[5], C96[-1]):
            w = P.weights(_sd(family), c)
            m = torch.from_numpy(CR.weight_matrix(_sd(family)[c["name"]], c)).float()
            assert np.array_equal(w.reshape(m.shape), m.to(torch.bfloat16).double().numpy())
            assert P.is_bf16(w) and not w[c["cout"]:].any()
            if family == "dyadic":
                assert np.array_equal(w, P.weights(_sd(family), c, bf=False))
    assert not P.is_bf16(np.array([1.0 + 2.0 ** -9])) and P.is_bf16(np.array([1.0 + 2.0 ** -7, -3.25, 0.0]))


def test_stem_from_nchw_against_conv2d():
    """the stem of a 96 x 64 batch handed over as NCHW: forward and weight gradient against F.conv2d + autograd with TF-"same" padding"""
    H, W = P.STEM_HW
    c = CR.b0_convs(H, W)[0]
    assert (c["hout"], c["wout"], c["Kw"], c["pad"]) == (48, 32, 48, 0) and R.same_pad(W, 3, 2) == c["pad"]
    o = P.operands(GEN, "random", c, 0, imgs=2)
    w4 = np.random.RandomState(5).standard_normal((32, 3, 3, 3))
    w = CR.weight_matrix(w4, c)
    xt = torch.tensor(o["xn"]).requires_grad_(True)
    wt = torch.tensor(w4, requires_grad=True)
    y = F.conv2d(F.pad(xt, (0, 1, 0, 1)), wt, None, 2)
    y.backward(torch.tensor(o["dyz"]).permute(0, 3, 1, 2))
    _close("fwd", CR.stem_fwd(o["x"], w, c), y.detach().permute(0, 2, 3, 1).numpy())
    _close("wgrad", CR.stem_wgrad(o["xz"], o["dyz"], c)[:, :, :3, :3], wt.grad.permute(0, 2, 3, 1).numpy())


def _silu_grad(v):
    s = torch.sigmoid(v)
    return s * (1 + v * (1 - s))


@pytest.mark.parametrize("groups", [1, 2])
def test_exp_bwd_against_autograd(groups):
    """d y_e, dx and dw of the fused expand backward against autograd through a_e = swish(y_e scale + shift), y_e = x W^T, with the
    BatchNorm-backward coefficients as given numbers: d y_e = ca (d a_e swish'(v)) + cb y_e + cc"""
    rs = np.random.RandomState(groups)
    N, HW, L, S = 4, 6, 32, 16
    da, ye, x, res = (rs.standard_normal(s) for s in ((N, HW, L), (N, HW, L), (N, HW, S), (N, HW, S)))
    w, bn = rs.standard_normal((L, S)), rs.standard_normal((5, groups, L))
    dye, dx, dw = P.exp_bwd(da, ye, x, w, bn, res)
    per = lambda v: torch.tensor(v).repeat_interleave(N // groups, 0)[:, None, :]
    yt = torch.tensor(ye, requires_grad=True)
    a = F.silu(yt * per(bn[3]) + per(bn[4]))
    a.backward(torch.tensor(da))                        # yt.grad = da swish'(v) scale; the kernel's d omits the scale factor (it is in ca)
    v = torch.tensor(ye) * per(bn[3]) + per(bn[4])
    want = per(bn[0]) * (torch.tensor(da) * _silu_grad(v)) + per(bn[1]) * torch.tensor(ye) + per(bn[2])
    _close("autograd", (yt.grad).numpy(), (torch.tensor(da) * _silu_grad(v) * per(bn[3])).numpy())
    _close("dye", dye, want.numpy())
    xt, wt = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
    (xt @ wt.T).backward(want)
    _close("dx", dx, (xt.grad + torch.tensor(res)).numpy())
    _close("dw", dw, wt.grad.numpy())
    _close("dx no res", P.exp_bwd(da, ye, x, w, bn)[1], xt.grad.numpy())


@pytest.mark.parametrize("groups", [1, 2])
def test_proj_bwd_against_autograd(groups):
    """the fused project backward against autograd through y_p = (swish(bn1 affine(y_d)) gate) W^T: d a_s, the weight gradient, the
    five per-image sums, and d y_d = ca ((d a_s gate + ds / HW) swish'(v)) + cb y_d + cc"""
    rs = np.random.RandomState(10 + groups)
    N, HW, L, S = 4, 5, 32, 16
    dyp, yd, w = rs.standard_normal((N, HW, S)), rs.standard_normal((N, HW, L)), rs.standard_normal((S, L))
    bn, gate, ds = rs.standard_normal((7, groups, L)), rs.standard_normal((N, L)), rs.standard_normal((N, L))
    got = P.proj_bwd(dyp, yd, w, bn, gate, ds)
    per = lambda v: torch.tensor(v).repeat_interleave(N // groups, 0)[:, None, :]
    yt, gt, wt = torch.tensor(yd, requires_grad=True), torch.tensor(gate, requires_grad=True), torch.tensor(w, requires_grad=True)
    act = F.silu(yt * per(bn[0]) + per(bn[1]))
    a_s = act * gt[:, None, :]
    a_s.retain_grad()
    (a_s @ wt.T).backward(torch.tensor(dyp))
    _close("das", got["das"], a_s.grad.numpy())
    _close("a_s", got["a_s"], a_s.detach().numpy())
    _close("dw", got["dw"], wt.grad.numpy())
    _close("pool5[0] = d gate", got["pool5"][:, 0], gt.grad.numpy())
    v = (yt * per(bn[0]) + per(bn[1])).detach()
    sg, xh, d = _silu_grad(v), (torch.tensor(yd) - per(bn[2])) * per(bn[3]), a_s.grad
    _close("pool5", got["pool5"][:, 1:], torch.stack([(d * sg).sum(1), (d * sg * xh).sum(1), sg.sum(1), (sg * xh).sum(1)], 1).numpy())
    want = per(bn[4]) * ((d * gt.detach()[:, None, :] + torch.tensor(ds)[:, None, :] / HW) * sg) + per(bn[5]) * torch.tensor(yd) + per(bn[6])
    _close("dyd", got["dyd"], want.numpy())
    assert _beyond(P.proj_bwd(dyp, yd, w, bn, gate, ds, hw_div=2 * HW)["dyd"], got["dyd"], 1e-9)


def test_stats_reference_and_bound():
    """acc_stats_bound: with b = 0 it is conv_ref.stats_bound of y; the deviation of the accumulators enters linearly"""
    rs = np.random.RandomState(2)
    y = rs.standard_normal((4, 3, 3, 16))
    _close("b = 0", P.acc_stats_bound(y, 0.0, 2), CR.stats_bound(y, 2))
    b = 1e-3 * np.abs(rs.standard_normal(y.shape))
    d = R.bn_stats(np.abs(y) + b, 2) - R.bn_stats(np.abs(y), 2)
    assert (P.acc_stats_bound(y, b, 2) >= d).all()


def test_unpermute_is_a_permutation():
    y = np.arange(2 * 144, dtype=np.float64).reshape(2, 144)
    m = P.mut_unpermute(y)
    assert np.array_equal(np.sort(m, -1), y) and not np.array_equal(m, y)
    assert np.array_equal(m[:, 128:], y[:, 128:])                   # the odd last row tile (nrt = 1) is stored as it is
    assert m[0, 4] == y[0, 8] and m[0, 16] == y[0, 4]               # (r, i) = (0, 4) holds channel 8; (1, 0) holds channel 4
    assert np.array_equal(P.mut_unpermute(y[:, :16]), y[:, :16])


# ---- the launch predicates ------------------------------------------------------------------------------------------------------------------------
def test_arms_of_the_model():
    """what launch_pw_conv / launch_pw_wgrad / the fused launchers decide for the 33 convs at the two handle sizes, 6 images in 2
    groups -- the sets tests/test_pw_bf16_gpu.py's coverage assertion relies on"""
    arms = [a for s in P.SIDES for a in P.model_arms(CONVS[s], IMGS, GROUPS)]
    st = [a for _, _, a in arms if a and a[0] == "stream"]
    gm = [a for _, _, a in arms if a and a[0] == "gemm"]
    assert {a[1] for a in st} == {(4, 4, 2, 4), (4, 2, 4, 4), (4, 2, 4, 8)}                 # never RT = 2
    assert {(a[1], a[2]) for a in st} >= {(f, m) for f in ((4, 4, 2, 4), (4, 2, 4, 4), (4, 2, 4, 8)) for m in (1, 2)}
    assert {(a[1], a[2], a[3]) for a in st} >= {((4, 4, 2, 4), 1, True), ((4, 2, 4, 4), 1, True), ((4, 2, 4, 4), 2, True)}
    assert {a[5] for a in st} == {1, 2, 3, 4}
    assert any(a[7] == ("full", "rem") and a[6] > 1 for a in st)
    assert {(a[1], a[4]) for a in gm if a[2] == 0} == {(64, 16), (64, 32), (64, 48), (128, 0), (128, 16), (128, 32), (128, 48)}
    assert {(a[2], a[3]) for a in gm} == {(0, 0), (1, 2), (2, 1)}
    wg = [a for _, op, a in arms if op == "wgrad"]
    assert {a[1:3] for a in wg if a[0] == "wave"} == {(2, 1), (6, 1), (6, 2), (9, 2)}
    # the block kernel with CC = 1 has no caller: the two 16-channel GEMMs of the model (32 x 16, 96 x 16) are wave shapes, 32 x 16 with
    # the prologue too
    assert {a[1] for a in wg if a[0] == "block"} == {2, 3, 5, 7, 12, 20}
    assert {a[1:3] for a in wg if a[0] == "block"} == {(2, True)} | {(cc, sw) for cc in (3, 5, 7, 12, 20) for sw in (False, True)}
    assert {a[1] for a in wg if a[0] == "block" and a[3]} == {2, 3, 5, 7} and ("wave", 2, 1, True) in wg
    assert {a[1:] for _, op, a in arms if op == "exp_bwd"} == {(6, 1), (9, 2)}
    assert {a[1:4] for _, op, a in arms if op == "proj_bwd"} == {(2, 1, 1), (3, 2, 2), (3, 2, 3), (3, 3, 3), (3, 3, 5)}
    # K = 1280 is a data gradient only (the head's), plain with K >= 64: pw_gemm takes it before pw_rt is asked
    assert P.pw_rt(1280) == 2 and P.conv_arm(320, 1280, 54, 1, 9, 0)[0] == "gemm"
    assert not any(c["cin_p"] > 1152 for s in P.SIDES for c in CONVS[s])
    # the 96 x 96 handle's first expand conv: 6912 pixels per group, nblk = 7, 14 pixel ranges, two M-tiles
    a = P.conv_arm(96, 16, 6912, 2, 2304, 1)
    assert a[6:] == (2, ("full", "rem")) and P.pw_ppb(6912, 2, 96, 16) == 1024
    # the engine fuses the prologue of blocks 0-10
    assert [P.short(CONVS[96][i]) for i in P.prologue_convs(C96)] == [f"b{i}.proj" for i in range(11)]
    assert P.proj_bwd_nch(240, 48, 6, 144, bf=False) == 0 and P.proj_bwd_nch(240, 48, 6, 144) == 5
    assert P.proj_bwd_nch(144, 48, 6, 9) == 0 and P.exp_bwd_arm(144, 32, 6 * 576, 3 * 576, 2, bf=False) == ("exp_bwd", 9, 2)


# ---- the dyadic preconditions on the data actually used -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(33))
def test_dyadic_sweep_is_exact(ci):
    o = _case("dyadic", ci)
    assert P.sweep_exact(o), C96[ci]["name"]
    c = o["c"]
    assert not o["y"][..., c["cout"]:].any() and not o["dw"][c["cout"]:].any()
    if c["cin"] != 3:
        assert not o["dx"][..., c["cin"]:].any()


def test_dyadic_stem_96x64_is_exact():
    convs = CR.b0_convs(*P.STEM_HW)
    assert P.sweep_exact(P.sweep_reference(GEN, "dyadic", 0, _sd("dyadic"), convs))


@pytest.mark.parametrize("side", P.SIDES)
@pytest.mark.parametrize("groups", [2, 1])
def test_dyadic_prologues_are_exact(side, groups):
    """x gate is a bf16 number (a multiple of 1/8 with few bits), its products with the weights multiples of 1/16; at psc = psh = 0
    the operand is exactly zero"""
    convs = CONVS[side]
    for ci in P.prologue_convs(convs):
        c = convs[ci]
        o = P.operands(GEN, "dyadic", c, ci)
        gate, psc, psh = CR.prologue_operands(GEN, "dyadic", c, ci, groups)
        a = CR.prologue(o["x"], gate)
        assert P.is_bf16(a) and P.is_bf16(CR.prologue(o["xz"], gate))
        w = P.weights(_sd("dyadic"), c)
        assert CR.exact_terms(CR.pw_fwd(np.abs(a), np.abs(w)), 1.0 / 16)
        assert CR.exact_terms(CR.pw_wgrad(np.abs(CR.prologue(o["xz"], gate)), np.abs(o["dyz"])), 1.0 / 16)
        gate, psc, psh = CR.prologue_operands(GEN, "dyadic", c, ci, groups, zero_affine=True)
        assert not CR.prologue(o["x"], gate, psc, psh).any() and len({tuple(g) for g in gate}) == len(gate)


@pytest.mark.parametrize("side,cases", [(96, P.epilogue_cases), (64, P.epilogue_cases_64)])
def test_dyadic_epilogues_are_exact(side, cases):
    convs = CONVS[side]
    for ci, act, res, gated in cases(convs):
        c = convs[ci]
        o = P.sweep_reference(GEN, "dyadic", ci, _sd("dyadic"), convs)
        ya = o["ya"]
        if gated:
            gate, _, _ = CR.prologue_operands(GEN, "dyadic", c, ci, 1)
            ya = CR.pw_fwd(np.abs(CR.prologue(o["x"], gate)), np.abs(o["w"]))
        scale, shift, r = P.epilogue_operands(GEN, "dyadic", c, ci, act, res)
        assert r is None or P.is_bf16(r)
        assert r is None or P.is_bf16(P.epilogue_operands(GEN, "random", c, ci, act, res)[2])
        assert CR.exact_terms(ya * np.abs(scale) + np.abs(shift) + (np.abs(r) if res else 0.0), 1.0 / 64)
        if act == 2:
            assert not CR.epilogue(o["y"], scale, shift, r, act).any()


@pytest.mark.parametrize("side", P.SIDES)
@pytest.mark.parametrize("groups", [2, 1])
def test_dyadic_fused_cases_are_exact(side, groups):
    """the dyadic entry of the fused kernels: scale = shift = 0 and ca = 0, so d y_e = cb y_e + cc and d y_d = cb y_d + cc are bf16
    numbers formed without the sigmoid, a_s = 0 * gate, and the sums that follow are exact"""
    convs = CONVS[side]
    for ci in P.exp_bwd_convs(convs):
        c = convs[ci]
        o = P.fused_operands(GEN, "dyadic", "exp", c, ci, groups, linear=True)
        w = P.weights(_sd("dyadic"), c)
        dye, dx, dw = P.exp_bwd(o["da"], o["ye"], o["x"], w, o["bn"], o["res"])
        assert all(P.is_bf16(o[k]) for k in ("da", "ye", "x", "res")) and P.is_bf16(dye)
        assert CR.exact_terms(np.abs(dye) @ np.abs(w) + np.abs(o["res"]), 1.0 / 16) and CR.exact_terms(CR.pw_wgrad(np.abs(o["x"]), np.abs(dye)), 1.0 / 16)
        assert dx.any() and dw.any()
    for ci in P.proj_bwd_convs(convs):
        c = convs[ci]
        o = P.fused_operands(GEN, "dyadic", "proj", c, ci, groups, linear=True)
        got = P.proj_bwd(o["dyp"], o["yd"], P.weights(_sd("dyadic"), c), o["bn"], o["gate"], o["ds"])
        assert P.is_bf16(o["dyp"]) and P.is_bf16(o["yd"]) and P.is_bf16(got["dyd"]) and got["dyd"].any()
        assert not got["a_s"].any() and not got["dw"].any() and not got["pool5"][:, 0].any()


# ---- the comparator has teeth ------------------------------------------------------------------------------------------------------------------------------
def _lost_pixel(name, n, rand_hit, dyadic_differs):
    """as tests/test_conv_ref_cpu.py: the worst-case bound of a sum over n terms may exceed one lost term from n (n + 2) u >= 1 on;
    those cases rest on the dyadic family"""
    if not rand_hit:
        assert n * (n + 2) * U_ >= 1.0, f"{name}: the random-family bound misses a lost pixel among {n}"
    assert dyadic_differs, f"{name}: the dyadic family misses it"


U_ = R.U


@pytest.mark.parametrize("ci", range(33))
def test_mutants_fail_the_sweep_bounds(ci):
    """every conv of the 96 x 96 sweep: the last 16 K-channels dropped (forward, data gradient), the rows of the M-tile pairs stored
    un-permuted, the residual omitted, and the last pixel of a group lost from the statistics and the weight gradient fall outside the
    bound of the random family and change a stored word of the dyadic family"""
    o, d = _case("random", ci), _case("dyadic", ci)
    c, w = o["c"], o["w"]
    by = _stored(CR.dot_bound(c["Kw"], o["ya"]), o["y"])
    assert not _beyond(R.bf16_round(o["y"]), o["y"], by)
    drop = lambda q: CR.conv_fwd(q["x"], CR.mut_drop_last_chunk(q["w"]), c)
    assert _beyond(drop(o), o["y"], by) and _words_differ(drop(d), d["y"]), "fwd: last 16 K-channels"
    if c["cout_p"] >= 32:               # (a 16-row output is one unpaired row tile: nothing to permute)
        assert _beyond(P.mut_unpermute(o["y"]), o["y"], by) and _words_differ(P.mut_unpermute(d["y"]), d["y"]), "fwd: un-permuted rows"
    if c["cin"] != 3:
        bx = _stored(CR.dot_bound(c["cout_p"], o["dxa"]), o["dx"])
        dropx = lambda q: CR.pw_dgrad(q["dy"], CR.mut_drop_last_chunk(q["w"], True))
        assert _beyond(dropx(o), o["dx"], bx) and _words_differ(dropx(d), d["dx"]), "dgrad: last 16 K-channels"
        if c["cin_p"] >= 32:
            assert _beyond(P.mut_unpermute(o["dx"]), o["dx"], bx) and _words_differ(P.mut_unpermute(d["dx"]), d["dx"]), "dgrad: un-permuted rows"
        bxr = _stored(P.residual_bound(o["dx"] + o["r"], CR.dot_bound(c["cout_p"], o["dxa"])), o["dx"] + o["r"])
        assert _beyond(o["dx"], o["dx"] + o["r"], bxr) and _words_differ(d["dx"], d["dx"] + d["r"]), "dgrad: residual omitted"
    npix = IMGS * c["hout"] * c["wout"]
    lostw = lambda q: CR.conv_wgrad(q["xz"], CR.mut_drop_last_pixel(q["dyz"], GROUPS), c)
    _lost_pixel("wgrad", npix, _beyond(lostw(o), o["dw"], CR.dot_bound(npix, o["dwa"])), not np.array_equal(lostw(d), d["dw"]))
    lost = lambda q: R.bn_stats(CR.mut_drop_last_pixel(q["y"], GROUPS), GROUPS)
    sb = P.acc_stats_bound(o["y"], CR.dot_bound(c["Kw"], o["ya"]), GROUPS)
    assert not _beyond(R.bn_stats(o["y"], GROUPS), R.bn_stats(o["y"], GROUPS), sb)
    _lost_pixel("statistics", npix // GROUPS, _beyond(lost(o), R.bn_stats(o["y"], GROUPS), sb),
                not np.array_equal(lost(d), R.bn_stats(d["y"], GROUPS)))


def test_statistics_of_the_stored_output_fail():
    """Both GEMM kernels sum their fp32 accumulators (the header: "from the fp32 accumulators"), not the bf16 values they store.  The
    sum of the rounded values differs by a random walk of n half-ulps, the worst-case bound grows like n^2 u: the random family sees the
    difference on the 3 x 3 maps (27 pixels per group: asserted for every conv there), the dyadic family -- exact sums, so any
    difference shows -- on every conv whose outputs are not all bf16 numbers"""
    seen = 0
    for ci, c in enumerate(C96):
        d = _case("dyadic", ci)
        if not P.is_bf16(d["y"]):
            assert not np.array_equal(P.mut_stats_of_stored(d["y"], GROUPS), R.bn_stats(d["y"], GROUPS)), P.short(c)
            seen += 1
        if c["hout"] == 3:
            o = _case("random", ci)
            sb = P.acc_stats_bound(o["y"], CR.dot_bound(c["Kw"], o["ya"]), GROUPS)
            assert _beyond(P.mut_stats_of_stored(o["y"], GROUPS), R.bn_stats(o["y"], GROUPS), sb), P.short(c)
    assert seen >= 20, seen


@pytest.mark.parametrize("side", P.SIDES)
@pytest.mark.parametrize("groups", [2, 1])
def test_mutants_fail_the_prologue_bounds(side, groups):
    """every prologue case, forward and weight gradient: the next image's gate row on the last pixels of an image (also a changed
    stored word in the dyadic family), group 0's psc / psh applied to group 1 (random family only: the dyadic entry of the affine form
    is psc = psh = 0 in every group), the last 16 K-channels dropped"""
    convs = CONVS[side]
    for ci in P.prologue_convs(convs):
        c = convs[ci]
        o, d = P.operands(GEN, "random", c, ci), P.operands(GEN, "dyadic", c, ci)
        w, wd = P.weights(_sd("random"), c), P.weights(_sd("dyadic"), c)
        gate, psc, psh = CR.prologue_operands(GEN, "random", c, ci, groups)
        gd, _, _ = CR.prologue_operands(GEN, "dyadic", c, ci, groups)
        assert _words_differ(CR.pw_fwd(P.mut_gate_next_image(d["x"], gd), wd), CR.pw_fwd(CR.prologue(d["x"], gd), wd)), "dyadic: next image's gate"
        for form in ("gate", "affine"):
            sc, sh = (psc, psh) if form == "affine" else (None, None)
            a, da = P.pro_operand(GEN, o["x"], gate, sc, sh)
            want = CR.pw_fwd(a, w)
            b = _stored(P.pro_bound(a, da, w), want)
            assert not _beyond(CR.pw_fwd(R.bf16_round(a), w), want, b)
            assert _beyond(CR.pw_fwd(P.mut_gate_next_image(o["x"], gate, sc, sh), w), want, b), (form, "next image's gate")
            assert _beyond(CR.pw_fwd(a, CR.mut_drop_last_chunk(w)), want, b), (form, "last chunk")
            az, daz = P.pro_operand(GEN, o["xz"], gate, sc, sh)
            wantw, bw = CR.pw_wgrad(az, o["dyz"]), P.pro_wgrad_bound(az, daz, o["dyz"])
            n = IMGS * c["hout"] * c["wout"]
            hit = _beyond(CR.pw_wgrad(P.mut_gate_next_image(o["xz"], gate, sc, sh), o["dyz"]), wantw, bw)
            assert hit or n * (n + 2) * U_ >= 1.0, (form, "wgrad: next image's gate")
            if form == "affine" and groups > 1:
                m = CR.mut_group0_affine(o["x"], gate, sc, sh)
                assert _beyond(CR.pw_fwd(m, w), want, b), "group 0's affine"
                assert _beyond(CR.pw_wgrad(CR.mut_group0_affine(o["xz"], gate, sc, sh), o["dyz"]), wantw, bw), "wgrad: group 0's affine"


@pytest.mark.parametrize("side,cases", [(96, P.epilogue_cases), (64, P.epilogue_cases_64)])
def test_mutants_fail_the_epilogue_bounds(side, cases):
    """the eval epilogue without its residual, and on a convolution that dropped its last 16 K-channels"""
    convs = CONVS[side]
    for ci, act, res, gated in cases(convs):
        c = convs[ci]
        for family in ("random", "dyadic"):
            o = P.sweep_reference(GEN, family, ci, _sd(family), convs)
            y, by = o["y"], CR.dot_bound(c["Kw"], o["ya"])
            if gated:
                gate, _, _ = CR.prologue_operands(GEN, family, c, ci, 1)
                a, da = P.pro_operand(GEN, o["x"], gate)
                y, by = CR.pw_fwd(a, o["w"]), P.pro_bound(a, da, o["w"])
            scale, shift, r = P.epilogue_operands(GEN, family, c, ci, act, res)
            want = CR.epilogue(y, scale, shift, r, act)
            if family == "dyadic":
                if res:
                    assert _words_differ(CR.epilogue(y, scale, shift, None, act), want)
                continue
            b = _stored(CR.epilogue_bound(GEN, y, by, scale, shift, r, act), want)
            assert not _beyond(R.bf16_round(want), want, b)
            if res:
                assert _beyond(CR.epilogue(y, scale, shift, None, act), want, b), (ci, "residual omitted")
            ym = CR.conv_fwd(o["x"] if not gated else a, CR.mut_drop_last_chunk(o["w"]), c)
            assert _beyond(CR.epilogue(ym, scale, shift, r, act), want, b), (ci, "last chunk")


@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("side", P.SIDES)
def test_mutants_fail_the_fused_bounds(side, bf):
    """the fused backward kernels, random family, groups = 2: ds / HW taken with the wrong HW (twice the image), the residual omitted,
    group 0's coefficients applied to group 1, the next image's gate, and the last 16 channels of the inner sum dropped fall outside
    the bounds; the true result rounded the way the kernel rounds its intermediates stays inside.  (The dyadic entry of these kernels
    multiplies the sigmoid path by ca = 0, so ds and the gate do not reach its outputs: these mutations rest on the random family.)"""
    convs = CONVS[side]
    rnd = (lambda t: R.bf16_round(t)) if bf else (lambda t: t)
    for ci in P.exp_bwd_convs(convs):
        c = convs[ci]
        o = P.fused_operands(GEN, "random", "exp", c, ci, 2, bf=bf)
        w = P.weights(_sd("random"), c, bf)
        dye, dx, dw = P.exp_bwd(o["da"], o["ye"], o["x"], w, o["bn"], o["res"])
        bx, bw = P.exp_bwd_bounds(GEN, o["da"], o["ye"], o["x"], w, o["bn"], o["res"], bf)
        bx = _stored(bx, dx, bf)
        assert not _beyond(rnd(dye) @ w + o["res"], dx, bx) and not _beyond(CR.pw_wgrad(o["x"], rnd(dye)), dw, bw)
        assert _beyond(P.exp_bwd(o["da"], o["ye"], o["x"], w, o["bn"])[1], dx, bx), "exp: residual omitted"
        bn0 = o["bn"].copy()
        bn0[:, 1] = bn0[:, 0]
        m = P.exp_bwd(o["da"], o["ye"], o["x"], w, bn0, o["res"])
        assert _beyond(m[1], dx, bx) and _beyond(m[2], dw, bw), "exp: group 0's coefficients"
        wm = w.copy()
        wm[-16:] = 0.0
        assert _beyond(P.exp_bwd(o["da"], o["ye"], o["x"], wm, o["bn"], o["res"])[1], dx, bx), "exp: last 16 channels of the data gradient"
    for ci in P.proj_bwd_convs(convs, bf):
        c = convs[ci]
        o = P.fused_operands(GEN, "random", "proj", c, ci, 2, bf=bf)
        w = P.weights(_sd("random"), c, bf)
        HW = c["hout"] * c["wout"]
        args = (o["dyp"], o["yd"], w, o["bn"], o["gate"])
        want, b = P.proj_bwd(*args, o["ds"]), P.proj_bwd_bounds(GEN, *args, o["ds"], bf)
        bd = _stored(b["dyd"], want["dyd"], bf)
        assert _beyond(P.proj_bwd(*args, o["ds"], hw_div=2 * HW)["dyd"], want["dyd"], bd), "proj: ds / HW with the wrong HW"
        g1 = np.roll(o["gate"], -1, axis=0)
        m = P.proj_bwd(o["dyp"], o["yd"], w, o["bn"], g1, o["ds"])
        assert _beyond(m["dyd"], want["dyd"], bd) and _beyond(m["dw"], want["dw"], b["dw"]), "proj: the next image's gate"
        bn0 = o["bn"].copy()
        bn0[:, 1] = bn0[:, 0]
        m = P.proj_bwd(o["dyp"], o["yd"], w, bn0, o["gate"], o["ds"])
        assert _beyond(m["dyd"], want["dyd"], bd) and _beyond(m["pool5"], want["pool5"], b["pool5"]), "proj: group 0's coefficients"
        wm = w.copy()
        wm[c["cout"] - 1] = 0.0                     # the last real row of the K = S sum that forms d a_s
        m = P.proj_bwd(o["dyp"], o["yd"], wm, o["bn"], o["gate"], o["ds"])
        assert _beyond(m["dyd"], want["dyd"], bd) and _beyond(m["pool5"], want["pool5"], b["pool5"]), "proj: a K-channel of d a_s dropped"
