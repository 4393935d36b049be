"""Kernel-level parity of the bf16 pointwise GEMM family of an EfficientNet-B0 engine with bf16 storage (csrc/pwconv_bf16.hip) -- the
streaming kernel in every form the model launches (<4,4,2>, <4,2,4>, <4,2,4,8> x MODE 0 / 1 / 2 x PRO), the LDS-tiled pw_gemm kernel
(BM 64 / 128, the data gradients and the PRO forms <1, 2> and <2, 1>), the four wave and six block weight-gradient shapes, the
bf16 stem (k_stem_im2col + the same GEMM with K = 48), the fused expand / project backward kernels -- and of the two fp32 fused
twins (projbwd_f32.hip, expbwd_f32.hip), through fm_debug_pw_fwd, fm_debug_pw, fm_debug_exp_bwd and fm_debug_proj_bwd against the
float64 restatement in tests/pw_bf16_ref.py (pinned to torch by tests/test_pw_bf16_ref_cpu.py, which also asserts the dyadic
preconditions on this file's data and shows that the bounds used here reject subtly wrong results).

Handles: 6 images in 2 groups.  96 x 96 in bf16: maps of 48, 24, 12, 6, 3 -- 6912 pixels per group at 48 x 48 give nblk = 7 and 14
pixel ranges (both branches of the block-id remap, two M-tiles), HW = 144 and 36 for the LDS-tiled prologue form, 27 pixels per
group and HW = 9 at the end.  64 x 64 in bf16: HW = 16 < 32 sends the K >= 240 project prologues to the streaming kernel, HW = 64
keeps the LDS-tiled form.  96 x 64 in bf16 for the stem, the only place of this family where H and W enter separately.  96 x 96 in
fp32 for the two fp32 fused twins.  Weights go in through spec.state_dict_to_flat + set_state.

DYADIC: operands are multiples of 1/2 in [-2, 2], weights from DYW, gates and coefficients from DYC: all bf16 numbers, every
product and partial sum exact.  Stored bf16 words (the reference rounds to nearest even), fp32 outputs and folded statistics must
equal the float64 reference BIT FOR BIT.  Sigmoids enter where an exact zero multiplies them (psc = psh = 0, scale = shift = 0,
ca = 0): nothing here relies on the hardware reciprocal returning 0.5 for 2.
RANDOM: standard normal rounded to bf16.  u = 2^-24.  (K + 2) u sum|a b| for a K-term dot product (products of bf16 numbers are
exact in fp32), half a bf16 ulp per bf16 store, the bf16 re-rounding of an operand formed on load carried through the following
sum, statistics against the float64 sums of the unrounded output (the kernels sum their fp32 accumulators): pw_bf16_ref's docstring.
Worst error / bound ratios go to pw_bf16_parity.json beside the other parity reports.

Canaries: every output and workspace sits between sentinel margins and is pre-filled with the sentinel (NaN, bf16 word 0x7FC1)."""
import functools

import numpy as np
import pytest
import torch

from fedmlp_amd import spec
from tests import conv_ref as CR
from tests import eff_ref as R
from tests import pw_bf16_ref as P
from tests import test_eff_kernels_gpu as GEN
from tests.test_eff_kernels_gpu import Buf, WORD, _canaries, _parity

pytestmark = pytest.mark.gpu

REPORT = {}
REPORT_PATH = "pw_bf16_parity.json"
_bits, _within, _check = _parity(REPORT, REPORT_PATH)
IMGS, GROUPS = P.IMGS, P.GROUPS
FAMILIES = ["dyadic", "random"]
CONVS = {96: CR.b0_convs(96, 96), 64: CR.b0_convs(64, 64), "stem": CR.b0_convs(*P.STEM_HW), "f32": CR.b0_convs(96, 96)}
SIZES = {96: (96, 96), 64: (64, 64), "stem": P.STEM_HW, "f32": (96, 96)}
short = P.short


@functools.lru_cache(maxsize=None)
def _sd(family):
    return CR.model_weights(GEN, family)


@functools.lru_cache(maxsize=4)
def _case(family, ci, key=96):
    """operands and float64 results of conv ci, shared read-only by the tests that need them"""
    o = P.sweep_reference(GEN, family, ci, _sd(family), CONVS[key])
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


_LOADED = {}


def _use(e, family):
    if _LOADED.get(id(e)) != family:
        flat, cnt = spec.state_dict_to_flat("Efficient_b0", 5, _sd(family))
        e.set_state(flat, cnt)
        _LOADED[id(e)] = family
    return e


@pytest.fixture(scope="module")
def engs():
    """the four handles of the module docstring, keyed 96, 64, "stem", "f32".  The non-square handle is created like the others:
    the engine takes any in_h, in_w that are multiples of 32"""
    from fedmlp_amd.engine import Engine
    es = {}
    try:
        for key, (H, W) in SIZES.items():
            e = es[key] = Engine("Efficient_b0", 5, H, W, IMGS, precision="fp32" if key == "f32" else "bf16")
            assert e.debug_num_convs() == 33
            for i, c in enumerate(CONVS[key]):
                assert {k: c[k] for k in CR.INFO_KEYS} == e.debug_conv_info(i), (key, i, e.debug_conv_info(i))
        yield es
    finally:
        for e in es.values():
            _LOADED.pop(id(e), None)
            e.close()


def _t(b):
    """what a hook gets: bf16 buffers as bfloat16 tensors"""
    return None if b is None else (b.t.view(torch.bfloat16) if b.bf else b.t)


def _f32(e, a, pool):
    return None if a is None else Buf(e, np.asarray(a).size, False, a, pool)


def _fwd(e, ci, c, x, groups, stats=False, res=None, act=0, x_bf=True, **vec):
    """one fm_debug_pw_fwd launch on canaried buffers: numpy operands in (x bf16, or the stem's fp32 NCHW batch), (out, stats) out"""
    pool = []
    xb = Buf(e, x.size, x_bf, x, pool)
    v = {k: _t(_f32(e, a, pool)) for k, a in vec.items() if a is not None}
    rb = Buf(e, res.size, True, res, pool) if res is not None else None
    yb = Buf(e, IMGS * c["hout"] * c["wout"] * c["cout_p"], True, pool=pool)
    sb = Buf(e, groups * 2 * c["cout_p"], pool=pool) if stats else None
    e.debug_pw_fwd(ci, _t(xb), _t(yb), IMGS, groups, res=_t(rb), act=act, stats=_t(sb), **v)
    _canaries(pool, f"pw_fwd hook, conv {ci}")
    return yb.np((IMGS, c["hout"], c["wout"], c["cout_p"])), (sb.np((groups, 2, c["cout_p"])) if stats else None)


def _pw(e, op, ci, c, x, dy, out_shape, out_bf, groups=1, x_bf=True, **vec):
    """one fm_debug_pw launch (op 1: x = the optional residual; op 2 on the stem: x = the fp32 NCHW batch)"""
    pool = []
    xb = Buf(e, x.size, x_bf, x, pool) if x is not None else None
    db = Buf(e, dy.size, True, dy, pool)
    v = {k: _t(_f32(e, a, pool)) for k, a in vec.items() if a is not None}
    ob = Buf(e, int(np.prod(out_shape)), out_bf, pool=pool)
    e.debug_pw(op, ci, _t(xb), _t(db), _t(ob), IMGS, groups, **v)
    _canaries(pool, f"pw hook op {op}, conv {ci}")
    return ob.np(out_shape)


def _stats_check(family, name, st, y, b, groups):
    ref, sb = R.bn_stats(y, groups), P.acc_stats_bound(y, b, groups)
    _check(family, f"{name} sum", st[:, 0], ref[:, 0], sb[:, 0])
    _check(family, f"{name} sumsq", st[:, 1], ref[:, 1], sb[:, 1])


# ---- one conv, three ops -------------------------------------------------------------------------------------------------------------------
def _sweep(e, family, ci, key=96):
    o = _case(family, ci, key)
    c, name = o["c"], short(o["c"])
    stem = c["cin"] == 3
    _use(e, family)
    npg = IMGS // GROUPS * c["hout"] * c["wout"]
    arms = {"fwd": P.conv_arm(c["cout_p"], c["Kw"], npg, GROUPS, c["hout"] * c["wout"], 1)}
    by = CR.dot_bound(c["Kw"], o["ya"])
    got, st = _fwd(e, ci, c, o["xn"] if stem else o["x"], GROUPS, stats=True, x_bf=not stem)
    tag = arms["fwd"][0]
    _check(family, f"fwd.{tag} {name} y", got, o["y"], by, bf=True)
    assert not got[..., c["cout"]:].any(), f"{name}: a pad channel of y is not zero"
    _stats_check(family, f"stats.{tag} {name}", st, o["y"], by, GROUPS)
    if not stem:
        arms["dgrad"] = P.conv_arm(c["cin_p"], c["cout_p"], IMGS * c["hout"] * c["wout"], 1, c["hout"] * c["wout"], 0)
        bx = CR.dot_bound(c["cout_p"], o["dxa"])
        tag = arms["dgrad"][0]
        got = _pw(e, 1, ci, c, None, o["dy"], o["dx"].shape, True)
        _check(family, f"dgrad.{tag} {name} dx", got, o["dx"], bx, bf=True)
        assert not got[..., c["cin"]:].any(), f"{name}: a pad channel of dx is not zero"
        got = _pw(e, 1, ci, c, o["r"], o["dy"], o["dx"].shape, True)
        _check(family, f"dgrad_res.{tag} {name} dx", got, o["dx"] + o["r"], P.residual_bound(o["dx"] + o["r"], bx), bf=True)
    arms["wgrad"] = P.wgrad_arm(c["cout_p"], c["Kw"])
    got = _pw(e, 2, ci, c, o["xn"] if stem else o["xz"], o["dyz"], o["dw"].shape, False, GROUPS if stem else 1, x_bf=not stem)
    _check(family, f"wgrad.{arms['wgrad'][0]} {name} dw", got, o["dw"], CR.dot_bound(IMGS * c["hout"] * c["wout"], o["dwa"]))
    g4 = got.reshape(c["cout_p"], c["k"], c["kw_p"], c["cin_p"])
    assert not g4[c["cout"]:].any() and not g4[:, :, c["k"]:].any() and not g4[..., c["cin"]:].any(), f"{name}: a pad slot of dw moved"
    return arms


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("ci", range(33))
def test_every_conv(engs, ci, family):
    """All 33 convs on the 96 x 96 handle, 6 images in 2 groups: forward + folded statistics (fm_debug_pw_fwd, the train form),
    data gradient without and with the residual, weight gradient; the stem from its NCHW batch (forward and weight gradient).  The
    forward and the data gradient get finite non-zero pad channels in their operand, which the zero weight columns must hide: the pad
    channels of the results must be exactly 0; pad rows, columns and taps of dw must be exactly 0."""
    print(f"conv {ci} {short(CONVS[96][ci])}: {_sweep(engs[96], family, ci)}")


@pytest.mark.parametrize("family", FAMILIES)
def test_stem_non_square(engs, family):
    """the stem on the 96 x 64 handle (48 x 32 output): k_stem_im2col is where H and W enter separately"""
    _sweep(engs["stem"], family, 0, "stem")


# ---- the eval epilogue ------------------------------------------------------------------------------------------------------------------------
def _epi_cases():
    return [(96,) + t for t in P.epilogue_cases(CONVS[96])] + [(64,) + t for t in P.epilogue_cases_64(CONVS[64])]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", _epi_cases(), ids=lambda p: f"{p[0]}-{short(CONVS[p[0]][p[1]])}-act{p[2]}{'-gate' if p[4] else ''}")
def test_eval_epilogue(engs, case, family):
    """act(conv scale + shift + res) as forward_eval runs it, MODE 2 of both kernels, which no other hook reaches: swish with scale /
    shift on the stem, a K <= 64 expand conv and the head; scale / shift / res on a streaming project conv and on a K > 640 one (the
    8-wave form); the gate prologue + scale / shift / res on block 0's project conv (streaming <4, 4, 2>), on K >= 240, M <= 128 project
    convs at HW = 36 and 64 (pw_gemm <128 | 64, 2, 1>) and at HW = 16 (streaming PRO in the 4- and the 8-wave form).  Dyadic: bit exact
    for act 0, and for act 2 at scale = shift = 0.  Random: conv_ref.epilogue_bound on the convolution's bound, plus the store."""
    key, ci, act, with_res, gated = case
    e = _use(engs[key], family)
    o = _case(family, ci, key)
    c, stem = o["c"], o["c"]["cin"] == 3
    y, by, gate = o["y"], CR.dot_bound(c["Kw"], o["ya"]), None
    if gated:
        gate, _, _ = CR.prologue_operands(GEN, family, c, ci, 1)
        a, da = P.pro_operand(GEN, o["x"], gate)
        y, by = CR.pw_fwd(a, o["w"]), P.pro_bound(a, da, o["w"])
    scale, shift, res = P.epilogue_operands(GEN, family, c, ci, act, with_res)
    got, _ = _fwd(e, ci, c, o["xn"] if stem else o["x"], 1, res=res, act=act, x_bf=not stem, scale=scale, shift=shift, gate=gate)
    want = CR.epilogue(y, scale, shift, res, act)
    arm = P.conv_arm(c["cout_p"], c["Kw"], IMGS * c["hout"] * c["wout"], 1, c["hout"] * c["wout"], 2, 1 if gated else 0)
    _check(family, f"epi.{arm[0]}_act{act}{'_gate' if gated else ''} {key} {short(c)}", got, want,
           CR.epilogue_bound(GEN, y, by, scale, shift, res, act), bf=True)


# ---- operand prologues ---------------------------------------------------------------------------------------------------------------------------
def _pro_cases():
    return [(key, ci) for key in P.SIDES for ci in P.prologue_convs(CONVS[key])]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("groups", [2, 1])
@pytest.mark.parametrize("case", _pro_cases(), ids=lambda p: f"{p[0]}-{short(CONVS[p[0]][p[1]])}")
def test_prologues(engs, case, groups, family):
    """Every project conv whose prologue the engine fuses (blocks 0-10), on both handles, groups 2 and 1, gates different per image,
    psc / psh different per group; forward and weight gradient.  Gate only (no statistics): dyadic bit exact (x gate is a bf16
    number).  psc + psh + gate with statistics: dyadic at psc = psh = 0, where operand, output, statistics and weight gradient are
    exactly 0; random within pw_bf16_ref.pro_bound / pro_wgrad_bound, statistics against the float64 sums of the unrounded output.
    The forward is the streaming kernel with PRO, or pw_gemm <0, 1> / <1, 2> for K >= 240 at HW >= 32; the weight gradient the block
    kernel with PRO (swap: the prologue on the Big operand), for 32 x 16 the wave kernel."""
    key, ci = case
    e = _use(engs[key], family)
    c, name = CONVS[key][ci], f"{key} {short(CONVS[key][ci])} g{groups}"
    o = _case(family, ci, key)
    w, n = o["w"], IMGS * c["hout"] * c["wout"]
    gate, psc, psh = CR.prologue_operands(GEN, family, c, ci, groups, zero_affine=family == "dyadic")
    for form, sc, sh in (("gate", None, None), ("affine", psc, psh)):
        stats = form == "affine"
        a, da = P.pro_operand(GEN, o["x"], gate, sc, sh)
        want, b = CR.pw_fwd(a, w), P.pro_bound(a, da, w)
        arm = P.conv_arm(c["cout_p"], c["cin_p"], n // groups, groups, c["hout"] * c["wout"], int(stats), 2 if stats else 1)
        got, st = _fwd(e, ci, c, o["x"], groups, stats=stats, gate=gate, psc=sc, psh=sh)
        if family == "dyadic" and stats:
            assert not a.any() and not want.any()
        _check(family, f"pro.{form}.{arm[0]} {name} y", got, want, b, bf=True)
        if stats:
            _stats_check(family, f"pro.{form}_stats.{arm[0]} {name}", st, want, b, groups)
        az, daz = P.pro_operand(GEN, o["xz"], gate, sc, sh)
        got = _pw(e, 2, ci, c, o["xz"], o["dyz"], o["dw"].shape, False, groups, gate=gate, psc=sc, psh=sh)
        _check(family, f"pro.{form}.wgrad_{P.wgrad_arm(c['cout_p'], c['cin_p'], True)[0]} {name} dw", got, CR.pw_wgrad(az, o["dyz"]),
               P.pro_wgrad_bound(az, daz, o["dyz"]))


# ---- the fused backward kernels --------------------------------------------------------------------------------------------------------------------
def _fused_keys():
    return [(96, True), (64, True), ("f32", False)]



@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("groups", [2, 1])
@pytest.mark.parametrize("key,bf", _fused_keys(), ids=["bf16-96", "bf16-64", "fp32-96"])
def test_fused_expand_backward(engs, key, bf, groups, family):
    """fm_debug_exp_bwd (pw_exp_bwd_kernel <6, 1> and <9, 2>; the fp32 twin on the fp32 handle) at (96, 16) and (144, 32), with and
    without the residual: dx and dw.  The reference keeps d y_e unrounded; the kernel's bf16 re-rounding of it is carried as a bound
    through both sums (pw_bf16_ref.exp_bwd_bounds).  Dyadic: scale = shift = 0 and ca = 0, so d y_e = cb y_e + cc is formed without
    the sigmoid (whatever it returns is multiplied by an exact zero) and is a bf16 number: dx and dw bit exact."""
    e = _use(engs[key], family)
    for ci in P.exp_bwd_convs(CONVS[key]):
        c = CONVS[key][ci]
        HW, L, S = c["hout"] * c["wout"], c["cout_p"], c["cin_p"]
        assert P.exp_bwd_arm(L, S, IMGS * HW, IMGS // groups * HW, groups, bf) == ("exp_bwd", L // 16, S // 16)
        o = P.fused_operands(GEN, family, "exp", c, ci, groups, bf=bf, linear=family == "dyadic")
        w = P.weights(_sd(family), c, bf)
        for res in (o["res"], None):
            pool = []
            bufs = [Buf(e, o[k].size, bf, o[k], pool) for k in ("da", "ye", "x")]
            rb = Buf(e, res.size, bf, res, pool) if res is not None else None
            bnb = Buf(e, o["bn"].size, False, o["bn"], pool)
            dxb, dwb = Buf(e, IMGS * HW * S, bf, pool=pool), Buf(e, L * S, pool=pool)
            e.debug_exp_bwd(ci, _t(bufs[0]), _t(bufs[1]), _t(bufs[2]), _t(rb), _t(bnb), IMGS, groups, _t(dxb), _t(dwb))
            _canaries(pool, f"exp_bwd conv {ci}")
            _, dx, dw = P.exp_bwd(o["da"], o["ye"], o["x"], w, o["bn"], res)
            bx, bw = P.exp_bwd_bounds(GEN, o["da"], o["ye"], o["x"], w, o["bn"], res, bf)
            name = f"{'bf16' if bf else 'fp32'} {key} {short(c)} g{groups}{' res' if res is not None else ''}"
            _check(family, f"exp_bwd.dx {name}", dxb.np(dx.shape), dx, bx, bf=bf)
            _check(family, f"exp_bwd.dw {name}", dwb.np(dw.shape), dw, bw)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("groups", [2, 1])
@pytest.mark.parametrize("key,bf", _fused_keys(), ids=["bf16-96", "bf16-64", "fp32-96"])
def test_fused_project_backward(engs, key, bf, groups, family):
    """fm_debug_proj_bwd phases 0 and 1 at every shape the launchers accept in the model -- (32, 16), (96, 32), (144, 32), (144, 48) and,
    in bf16, (240, 48) -- including HW = 144 with its ragged 16-pixel tile (96 x 96) and HW = 64 (64 x 64).  The reference keeps d a_s
    and a_s unrounded; the kernel's bf16 re-roundings are carried as bounds (pw_bf16_ref.proj_bwd_bounds).  Dyadic: scale = shift = 0
    and ca = 0 -- swish(0) = 0 * sigmoid is an exact zero, so the first of the five sums and dw are exactly 0 and d y_d = cb y_d + cc
    bit exact; the four sums through swish'(0) = sigmoid(0) are held to the bound (not to 1/2: that would rest on the reciprocal)."""
    e = _use(engs[key], family)
    for ci in P.proj_bwd_convs(CONVS[key], bf):
        c = CONVS[key][ci]
        HW, L, S = c["hout"] * c["wout"], c["cin_p"], c["cout_p"]
        assert P.proj_bwd_arm(L, S, IMGS, HW, bf) is not None
        o = P.fused_operands(GEN, family, "proj", c, ci, groups, bf=bf, linear=family == "dyadic")
        w = P.weights(_sd(family), c, bf)
        pool = []
        db, yb = Buf(e, o["dyp"].size, bf, o["dyp"], pool), Buf(e, o["yd"].size, bf, o["yd"], pool)
        bnb, gb, sb = (Buf(e, o[k].size, False, o[k], pool) for k in ("bn", "gate", "ds"))
        dwb, p5b, dyb = Buf(e, S * L, pool=pool), Buf(e, IMGS * 5 * L, pool=pool), Buf(e, IMGS * HW * L, bf, pool=pool)
        e.debug_proj_bwd(ci, 0, _t(db), _t(yb), _t(bnb), _t(gb), None, IMGS, groups, _t(dwb), _t(p5b))
        e.debug_proj_bwd(ci, 1, _t(db), _t(yb), _t(bnb), _t(gb), _t(sb), IMGS, groups, _t(dyb))
        _canaries(pool, f"proj_bwd conv {ci}")
        want = P.proj_bwd(o["dyp"], o["yd"], w, o["bn"], o["gate"], o["ds"])
        b = P.proj_bwd_bounds(GEN, o["dyp"], o["yd"], w, o["bn"], o["gate"], o["ds"], bf)
        name = f"{'bf16' if bf else 'fp32'} {key} {short(c)} g{groups}"
        p5 = p5b.np(want["pool5"].shape)
        if family == "dyadic":
            _bits(f"proj_bwd.pool5_0 {name}", p5[:, 0], want["pool5"][:, 0])
            _within(f"proj_bwd.pool5 {name}", p5[:, 1:], want["pool5"][:, 1:], b["pool5"][:, 1:], family="dyadic")
        else:
            _within(f"proj_bwd.pool5 {name}", p5, want["pool5"], b["pool5"])
        _check(family, f"proj_bwd.dw {name}", dwb.np(want["dw"].shape), want["dw"], b["dw"])
        _check(family, f"proj_bwd.dyd {name}", dyb.np(want["dyd"].shape), want["dyd"], b["dyd"], bf=bf)


# ---- which instantiations the cases above reach -----------------------------------------------------------------------------------------------------
def _inst(arm):
    """the kernel instantiation of an arm tuple: the template arguments, without the shape-dependent rest"""
    return arm[:4] if arm[0] in ("stream", "gemm") else (arm[:3] if arm[0] in ("exp_bwd", "proj_bwd") else arm)


def _tested_arms():
    """[(arm, K)] of every launch of the tests above, from the same case lists and the restated predicates"""
    out = []
    for c in CONVS[96]:
        M, K, HW = c["cout_p"], c["Kw"], c["hout"] * c["wout"]
        out.append((P.conv_arm(M, K, IMGS // GROUPS * HW, GROUPS, HW, 1), K))
        out.append((P.wgrad_arm(M, K), K))
        if c["cin"] != 3:
            out.append((P.conv_arm(K, M, IMGS * HW, 1, HW, 0), M))
    for key, ci, act, res, gated in _epi_cases():
        c = CONVS[key][ci]
        out.append((P.conv_arm(c["cout_p"], c["Kw"], IMGS * c["hout"] * c["wout"], 1, c["hout"] * c["wout"], 2, int(gated)), c["Kw"]))
    for key, ci in _pro_cases():
        c = CONVS[key][ci]
        HW = c["hout"] * c["wout"]
        for groups in (2, 1):
            out.append((P.conv_arm(c["cout_p"], c["cin_p"], IMGS // groups * HW, groups, HW, 0, 1), c["cin_p"]))
            out.append((P.conv_arm(c["cout_p"], c["cin_p"], IMGS // groups * HW, groups, HW, 1, 2), c["cin_p"]))
        out.append((P.wgrad_arm(c["cout_p"], c["cin_p"], True), c["cin_p"]))
    for key, bf in _fused_keys():
        if not bf:
            continue
        for ci in P.exp_bwd_convs(CONVS[key]):
            c = CONVS[key][ci]
            out.append((P.exp_bwd_arm(c["cout_p"], c["cin_p"], IMGS * c["hout"] * c["wout"], 3 * c["hout"] * c["wout"], 2), c["cout_p"]))
        for ci in P.proj_bwd_convs(CONVS[key]):
            c = CONVS[key][ci]
            out.append((P.proj_bwd_arm(c["cin_p"], c["cout_p"], IMGS, c["hout"] * c["wout"]), c["cout_p"]))
    return out


def test_arm_coverage(engs):
    """From the engine's own conv tables (debug_conv_info, asserted equal to conv_ref.b0_convs by the fixture) and the launch
    predicates restated in pw_bf16_ref: the union of the cases of this file reaches every instantiation the model's graphs can
    launch on the two handles (pw_bf16_ref.model_arms: train and eval forwards with and without the fused prologue, data and weight
    gradients, the fused backward kernels), and in particular
      the streaming kernel <4,4,2>, <4,2,4>, <4,2,4,8> in MODE 0 (K <= 48 data gradients only: <4,4,2>) / 1 / 2, PRO off and on;
      its K % 32 == 16 tails at K = 16, 48, 80, 112, 144, 240; partial last M-tiles with nrt = 1, 2, 3; both branches of the block-id
      remap in one launch with more than one M-tile;
      pw_gemm with BM = 64 and 128, K % 64 in {0, 16, 32, 48}, the PRO forms <1, 2> and <2, 1> (and <0, 1>, which only tests launch);
      all four wave weight-gradient shapes, 32 x 16 also with the prologue; the block kernel with CC = 2, 3, 5, 7, 12, 20, swap both
      ways where the model has both (CC = 2 only swapped), with the prologue at CC = 2, 3, 5, 7;
      both instantiations of pw_exp_bwd_kernel and the five (slice, S) forms of pw_proj_bwd_kernel, one with the ragged last tile.
    Asserted ABSENT, because the predicates show that no convolution of EfficientNet-B0 reaches them (the kernel code stays):
      the RT = 2 streaming form pw_launch_t<2, 2, 4> -- pw_rt keeps it for K = 1280, which only the head's data gradient has, and
      launch_pw_conv hands every plain GEMM with K >= 64 to pw_gemm first;
      the block weight-gradient kernel with CC = 1 -- the two 16-channel GEMMs (32 x 16, 96 x 16) are wave shapes, 32 x 16 with the
      prologue too."""
    for key in P.SIDES:
        assert [engs[key].debug_conv_info(i) for i in range(33)] == [{k: c[k] for k in CR.INFO_KEYS} for c in CONVS[key]]
    tested = _tested_arms()
    assert all(a is not None for a, _ in tested)
    have = {_inst(a) for a, _ in tested}
    model = [a for key in P.SIDES for _, _, a in P.model_arms(CONVS[key], IMGS, GROUPS)]
    assert all(a is not None for a in model)
    missing = {_inst(a) for a in model} - have
    assert not missing, f"instantiations the model launches and no case here reaches: {sorted(missing)}"
    st = [(a, k) for a, k in tested if a[0] == "stream"]
    forms = ((4, 4, 2, 4), (4, 2, 4, 4), (4, 2, 4, 8))
    assert {a[1] for a, _ in st} == set(forms), "the RT = 2 form is expected to be unreachable"
    assert not any(a[0] == "stream" and a[1][0] == 2 for a in model)
    assert {(a[1], a[2], a[3]) for a, _ in st} >= {(f, m, p) for f in forms for m in (1, 2) for p in (False, True)} | {(forms[0], 0, False)}
    assert {k for a, k in st if a[4]} >= {16, 48, 80, 112, 144, 240}
    assert {a[5] for a, _ in st} == {1, 2, 3, 4}
    assert any(a[7] == ("full", "rem") and a[6] > 1 for a, _ in st)
    gm = [a for a, _ in tested if a[0] == "gemm"]
    assert {a[1] for a in gm} == {64, 128} and {a[4] for a in gm} == {0, 16, 32, 48}
    assert {(a[2], a[3]) for a in gm} == {(0, 0), (0, 1), (1, 2), (2, 1)}
    assert {(a[1], a[2], a[3]) for a in gm} >= {(bm, m, p) for bm in (64, 128) for m, p in ((0, 0), (1, 2), (2, 1))}
    wg = [a for a, _ in tested if a[0] in ("wave", "block")]
    assert {a[1:] for a in wg if a[0] == "wave"} == {(2, 1, False), (2, 1, True), (6, 1, False), (6, 2, False), (9, 2, False)}
    assert {a[1:3] for a in wg if a[0] == "block"} == {(2, True)} | {(cc, sw) for cc in (3, 5, 7, 12, 20) for sw in (False, True)}
    assert {a[1] for a in wg if a[0] == "block" and a[3]} == {2, 3, 5, 7}
    assert not any(a[0] == "block" and a[1] == 1 for a in model)
    assert {a[1:3] for a, _ in tested if a[0] == "exp_bwd"} == {(6, 1), (9, 2)}
    pj = [a for a, _ in tested if a[0] == "proj_bwd"]
    assert {a[1:4] for a in pj} == {(2, 1, 1), (3, 2, 2), (3, 2, 3), (3, 3, 3), (3, 3, 5)} and any(a[4] for a in pj)
    REPORT["arm_coverage"] = {"instantiations": sorted(str(i) for i in have)}
    GEN._dump_report(REPORT, REPORT_PATH)


# ---- the hook's contract -----------------------------------------------------------------------------------------------------------------------------
def test_hook_contract(engs):
    """fm_debug_pw_fwd takes the forms the engine's graphs use and nothing else: every other combination raises error -1 before any
    launch (the output stays all-sentinel), sync() reports nothing afterwards, and a plain forward on the same handle is still bit exact"""
    from fedmlp_amd._lib import FmError
    e = _use(engs[96], "dyadic")
    ix = P.index(CONVS[96])
    cs = ix["b1.proj"]
    dev = e.device

    def bad(eng, ci, c, groups=1, act=0, x_f32=False, **kw):
        z = lambda *s: torch.zeros(s, device=dev)
        yb = Buf(eng, IMGS * c["hout"] * c["wout"] * c["cout_p"], True)
        x = z(IMGS, 3, c["hin"], c["win"]) if x_f32 else z(IMGS, c["hin"], c["win"], c["cin_p"]).to(torch.bfloat16)
        shapes = dict(scale=(c["cout_p"],), shift=(c["cout_p"],), res=(IMGS, c["hout"], c["wout"], c["cout_p"]), psc=(groups, c["cin_p"]),
                      psh=(groups, c["cin_p"]), gate=(IMGS, c["cin_p"]), stats=(groups, 2, c["cout_p"]))
        ops = {k: (z(*shapes[k]).to(torch.bfloat16) if k == "res" else z(*shapes[k])) for k in kw}
        with pytest.raises(FmError, match="error -1"):
            eng.debug_pw_fwd(ci, x, _t(yb), IMGS, groups, act=act, **ops)
        torch.cuda.synchronize()
        assert (yb.raw() == WORD).all(), (ci, kw, "something was launched")

    c, c0 = CONVS[96][cs], CONVS[96][0]
    bad(e, cs, c, scale=True)                                                     # half a pair
    bad(e, cs, c, shift=True)
    bad(e, cs, c, 2, gate=True, psc=True, stats=True)
    bad(e, cs, c, 2, gate=True, psh=True, stats=True)
    bad(e, cs, c, 2, psc=True, psh=True, stats=True)                              # psc / psh without a gate
    bad(e, cs, c, res=True)                                                       # res / act without scale and shift
    bad(e, cs, c, act=2)
    bad(e, cs, c, 2, scale=True, shift=True)                                      # groups > 1 with an epilogue
    bad(e, cs, c, 1, scale=True, shift=True, stats=True)                          # statistics with an epilogue
    bad(e, cs, c, 1, scale=True, shift=True, gate=True, psc=True, psh=True)       # the affine prologue under an epilogue
    bad(e, cs, c, 1, act=1, scale=True, shift=True)                               # act = 1: the bf16 kernels have no relu
    bad(e, cs, c, 1, act=3, scale=True, shift=True)
    bad(e, 0, c0, x_f32=True, gate=True)                                          # a prologue on the stem
    bad(e, 0, c0, 2, x_f32=True, gate=True, psc=True, psh=True, stats=True)
    bad(e, 0, c0, x_f32=True, scale=True, shift=True, res=True)                   # a residual on the stem
    ef = engs["f32"]                                                              # a precision-0 handle
    yb = Buf(ef, IMGS * c["hout"] * c["wout"] * c["cout_p"], True)
    with pytest.raises(FmError, match="error -1"):
        ef.debug_pw_fwd(cs, torch.zeros((IMGS, c["hin"], c["win"], c["cin_p"]), device=dev).to(torch.bfloat16), _t(yb), IMGS, 1)
    torch.cuda.synchronize()
    assert (yb.raw() == WORD).all()
    for eng in (e, ef):
        eng.sync()                                                                # no deferred error
    o = _case("dyadic", cs)
    got, st = _fwd(e, cs, c, o["x"], GROUPS, stats=True)
    _bits(f"contract.plain {short(c)} y", got, R.bf16_round(o["y"]))
    _bits(f"contract.plain {short(c)} stats", st, R.bn_stats(o["y"], GROUPS))
    e.sync()
