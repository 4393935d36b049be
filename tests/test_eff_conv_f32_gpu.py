"""Kernel-level parity of the convolution GEMMs of an fp32 EfficientNet-B0 engine -- the streaming 1x1 kernel (csrc/conv1x1.hip, all
its instantiations: statistics on / off, gate prologue 0 / 1 / 2, product forms 0 / 6 / 9), igemm.hip on the K > 256 shapes with
their partial 64- and 128-row tiles and the stream-K fix-up, the skinny and generic weight-gradient kernels (wgrad.hip), the gathered
3x3 stride-2 stem, and conv_fwd's fused eval epilogue of both models -- through fm_debug_conv and fm_debug_conv_fwd against the
float64 restatement in tests/conv_ref.py (pinned to F.conv2d + autograd by tests/test_conv_ref_cpu.py, which also asserts the dyadic
preconditions on this file's data and shows that the bounds used here reject subtly wrong results).

Handles of 96 x 96 inputs and 6 images in 2 groups: maps of 48, 24, 12, 6 and 3, so 27 pixels per group and HW = 9 at the end --
the smallest shapes where a 16-pixel fragment straddles images and every tail arm of the kernels runs.  Weights go in through
spec.state_dict_to_flat + set_state, so they sit in the engine's own padded layout with zero pad rows and columns.

The method, buffers and generators are those of tests/test_eff_kernels_gpu.py.
DYADIC: operands are multiples of 1/2 in [-2, 2], weights from DYW, gates and scales from DYC: every product is exact in every
product form (dyadic bf16 numbers have zero middle and low planes) and every partial sum in any order is exact; outputs, weight
gradients and the folded statistics must equal the float64 reference BIT FOR BIT.  Sigmoids enter at psc = psh = 0 / scale = shift
= 0, where swish(0) = 0 exactly.
RANDOM: standard normal.  u = 2^-24.  A K-term dot product is within (K + 2) u sum|a b| of float64 in every product form
(csrc/split3.h; conv_ref.dot_bound says why partial sums do not add to it); epilogue roundings are counted per operation
(conv_ref.epilogue_bound); an operand formed on load carries its own error through sum |w| da (conv_ref.prologue_bound); the fused
statistics are held against the float64 sums of the output the same launch stored, within (n + 1) u sum|y| and (n + 2) u sum y^2
(n additions, the final rounding of the folded tiles, one more rounding per square: conv_ref.stats_bound).
Worst error / bound ratios go to conv_f32_parity.json beside the other parity reports.

Canaries: every output sits between NaN margins and is pre-filled with NaN."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fedmlp_amd import spec
from tests import conv_ref as CR
from tests import eff_ref as R
from tests import test_eff_kernels_gpu as GEN
from tests.test_local_training_gpu import _dump as _dump_report
from tests.test_eff_kernels_gpu import Buf, _canaries, _parity, _exact, _swish_err, _affine_err, _vals, _wts, _coef  # noqa: F401

pytestmark = pytest.mark.gpu

U = R.U
REPORT = {}
REPORT_PATH = "conv_f32_parity.json"
_bits, _within, _check = _parity(REPORT, REPORT_PATH)
CONVS = CR.b0_convs()
IMGS, GROUPS = CR.IMGS, CR.GROUPS
FAMILIES = ["dyadic", "random"]


def _short(c):
    return c["name"].replace("_blocks.", "b").replace("._expand_conv.weight", ".exp").replace("._project_conv.weight", ".proj") \
        .replace("_conv_stem.weight", "stem").replace("_conv_head.weight", "head")


@functools.lru_cache(maxsize=None)
def _sd(family):
    return CR.model_weights(GEN, family)


@functools.lru_cache(maxsize=4)
def _case(family, ci):
    """operands and float64 results of conv ci, shared (read-only) by the tests that need them while they run one after the
    other: a few cases stay resident, not all 66 (the largest hold tens of MB; recomputing one takes milliseconds)"""
    o = CR.sweep_reference(GEN, family, ci, _sd(family), CONVS)
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


_LOADED = {}


def _use(e, family):
    """the family's weights on handle e (set_state re-lays them out and re-packs the transposed / plane copies)"""
    if _LOADED.get(id(e)) != family:
        flat, cnt = spec.state_dict_to_flat("Efficient_b0", 5, _sd(family))
        e.set_state(flat, cnt)
        _LOADED[id(e)] = family
    return e


def _make_engine(products=None):
    from fedmlp_amd.engine import Engine
    e = Engine("Efficient_b0", 5, CR.SIDE, CR.SIDE, IMGS, products=products)
    assert not e.planes and e.debug_num_convs() == 33
    for i, c in enumerate(CONVS):
        info = e.debug_conv_info(i)
        assert {k: c[k] for k in CR.INFO_KEYS} == info, (i, info)
    return e


@pytest.fixture(scope="module")
def engs():
    """one handle per product form (fm_config.reserved[2]): 6 = the default, 0 = the fp32 matrix pipe, 9"""
    es = {}
    try:
        for p in (6, 0, 9):
            es[p] = _make_engine(p)
            assert es[p].products == p
        yield es
    finally:
        for e in es.values():
            _LOADED.pop(id(e), None)
            e.close()


# ---- one conv, three ops ---------------------------------------------------------------------------------------------------------------
def _arm_name(a):
    return a[0] if a[0] != "skinny" else ("skinny_gather" if a[3] else "skinny")


def _sweep(e, family, ci, ops=("fwd", "dgrad", "wgrad")):
    """forward + statistics, data gradient and weight gradient of conv ci on handle e against the shared reference; returns the arms"""
    o = _case(family, ci)
    c, name = o["c"], _short(o["c"])
    _use(e, family)
    arms = {"fwd": CR.fwd_arm(c), "dgrad": CR.dgrad_arm(c), "wgrad": CR.wgrad_arm(c)}
    if "fwd" in ops:
        pool = []
        xb = Buf(e, o["x"].size, False, o["x"], pool)
        yb, sb = Buf(e, o["y"].size, pool=pool), Buf(e, GROUPS * 2 * c["cout_p"], pool=pool)
        e.debug_conv(0, ci, xb.t, None, yb.t, IMGS, GROUPS, sb.t)
        _canaries(pool, name + " fwd")
        got = yb.np(o["y"].shape)
        tag = _arm_name(arms["fwd"])
        _check(family, f"fwd.{tag} {name} y", got, o["y"], CR.dot_bound(c["Kw"], o["ya"]))
        stored = o["y"] if family == "dyadic" else got.astype(np.float64)
        st, ref, sbnd = sb.np((GROUPS, 2, c["cout_p"])), R.bn_stats(stored, GROUPS), CR.stats_bound(stored, GROUPS)
        _check(family, f"stats.{tag} {name} sum", st[:, 0], ref[:, 0], sbnd[:, 0])
        _check(family, f"stats.{tag} {name} sumsq", st[:, 1], ref[:, 1], sbnd[:, 1])
    if "dgrad" in ops and c["cin"] != 3:
        pool = []
        db = Buf(e, o["dy"].size, False, o["dy"], pool)
        xb = Buf(e, o["dx"].size, pool=pool)
        e.debug_conv(1, ci, None, db.t, xb.t, IMGS)
        _canaries(pool, name + " dgrad")
        _check(family, f"dgrad.{_arm_name(arms['dgrad'])} {name} dx", xb.np(o["dx"].shape), o["dx"], CR.dot_bound(c["cout_p"], o["dxa"]))
    if "wgrad" in ops:
        pool = []
        xb, db = Buf(e, o["xz"].size, False, o["xz"], pool), Buf(e, o["dyz"].size, False, o["dyz"], pool)
        wb = Buf(e, o["dw"].size, pool=pool)
        e.debug_conv(2, ci, xb.t, db.t, wb.t, IMGS)
        _canaries(pool, name + " wgrad")
        got = wb.np(o["dw"].shape)
        _check(family, f"wgrad.{_arm_name(arms['wgrad'])} {name} dw", got, o["dw"], CR.dot_bound(IMGS * c["hout"] * c["wout"], o["dwa"]))
        # the optimizer must not move weights the layout says are zero: pad rows, pad taps and pad channels stay exactly 0
        g4 = got.reshape(c["cout_p"], c["k"], c["kw_p"], c["cin_p"])
        assert not g4[c["cout"]:].any() and not g4[:, :, c["k"]:].any() and not g4[..., c["cin"]:].any(), f"{name}: a pad slot of dw moved"
    return arms


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("ci", range(33))
def test_every_conv(engs, ci, family):
    """All 33 convs on the default handle (six products), 6 images in 2 groups: forward + statistics, weight gradient and data
    gradient (not the stem's: tests/test_input_grad_gpu.py).  The forward and the data gradient get finite non-zero values in the pad
    channels of their operand, which the zero weight columns must hide (the pad channels of the results must be exactly 0: their
    bound is 0); the weight gradient gets zero pad channels and must leave every pad slot exactly 0.  Dyadic: bit exact.  Random:
    (K + 2) u sum|a b| with K = Kw, cout_p and the pixel count; statistics against the stored output (module docstring)."""
    arms = _sweep(engs[6], family, ci)
    print(f"conv {ci} {_short(CONVS[ci])}: {arms}")


def test_arm_coverage(engs):
    """Which kernel each conv takes, from the engine's own conv table and the three `takes` conditions restated in conv_ref
    (conv1x1_stream_takes; launch_wgrad_skinny's S <= 128, CC = ceil(S / 16), swap = Kw > cout_p; else igemm / the generic
    wgrad_kernel), and that the union over test_every_conv's 33 convs covers every arm the model has:
    the streaming kernel with M = 16, 32, 48 (nrt < RT) and the partial last M-tile of 80, 144, 240; its K tails 16 .. 240 including
    K % 32 == 16 (16, 48, 80, 112, 144, 240); the split forms forced off at K = 240; igemm with M = 80, 112, 192, 320, 1280; the skinny
    weight gradient with CC = 1, 2, 3, 5, 7 in both directions; the gathered stem; the generic weight gradient.
    Two arms one might expect do not exist in EfficientNet-B0 and are asserted absent rather than silently skipped: no GEMM streams
    with M = 112 (112-row outputs have K = 480 / 672 and the 112-row data gradient K = 672: all igemm, M = 112 covered there; nrt = 3
    of a last M-tile runs at M = 48 and 240), and no conv has min(cout_p, Kw) in (80, 96], so CC = 6 is never launched (the padded
    channel counts are 16, 32, 48, 80, 112, 192, 320 and the expanded 96 .. 1152)."""
    e = engs[6]
    convs = [e.debug_conv_info(i) for i in range(e.debug_num_convs())]
    gemms = [a for c in convs for a in (CR.fwd_arm(c), CR.dgrad_arm(c)) if a[0] != "stem"]
    stream_m, stream_k = {a[1] for a in gemms if a[0] == "stream"}, {a[2] for a in gemms if a[0] == "stream"}
    assert stream_m >= {16, 32, 48, 80, 144, 240} and 112 not in stream_m, stream_m
    assert stream_k >= {16, 32, 48, 80, 112, 144, 240}, stream_k
    # a streaming GEMM with 192 < K <= 256 exists; that launch_conv1x1_stream then keeps the fp32 pipe is the restated rule
    # (conv_ref.stream_sp), not something a hook reports: nothing here observes which product form the engine picked at K = 240
    assert any(a[0] == "stream" and 192 < a[2] <= 256 and CR.stream_sp(a[2], 6) == 0 for a in gemms)
    assert {a[1] for a in gemms if a[0] == "igemm"} >= {80, 112, 192, 320, 1280}
    wg = [CR.wgrad_arm(c) for c in convs]
    assert {a[1:3] for a in wg if a[0] == "skinny"} == {(cc, sw) for cc in (1, 2, 3, 5, 7) for sw in (False, True)}
    assert not any(80 < min(c["cout_p"], c["Kw"]) <= 96 for c in convs)
    assert wg[0] == ("skinny", 2, True, True) and ("generic",) in wg
    assert {c["hout"] * c["wout"] for c in convs} == {2304, 576, 144, 36, 9}


# ---- product forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("products", [0, 9])
@pytest.mark.parametrize("ci", range(33))
def test_product_forms_dyadic(engs, ci, products):
    """the dyadic sweep on the products = 0 and products = 9 handles: the same bits as the float64 reference, hence as the default form"""
    _sweep(engs[products], "dyadic", ci)


def _form_convs():
    idx = {_short(c): i for i, c in enumerate(CONVS)}
    return [idx[n] for n in ("stem", "b0.proj", "b1.exp", "b5.proj", "b7.proj", "b12.exp", "head")]


@pytest.mark.parametrize("ci", _form_convs())
def test_product_forms_random(engs, ci):
    """test_split_products_are_fp32_accurate's assertion on one conv per arm (stem + gathered wgrad; streaming M = 16 with a swapped
    skinny wgrad; streaming K = 16 / M = 96; K = 240 where the streaming kernel keeps the fp32 pipe; igemm M = 80 with a streaming
    data gradient; K = 192 with an igemm data gradient and the generic wgrad; the head): the relative L2 error against float64 of
    the forms 6 and 9 is <= 1.25 x that of the fp32 matrix pipe + 1e-9, and < 2e-6"""
    o = _case("random", ci)
    c = o["c"]
    errs = {}
    for sp in (0, 9, 6):
        e = _use(engs[sp], "random")
        dev = e.device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
        rel = lambda got, want: float(np.linalg.norm(got.cpu().numpy().astype(np.float64) - want) / np.linalg.norm(want))
        out = torch.full(o["y"].shape, float("nan"), device=dev)
        e.debug_conv(0, ci, t(o["x"]), None, out, IMGS, GROUPS, torch.empty((GROUPS, 2, c["cout_p"]), device=dev))
        r = [rel(out, o["y"])]
        if c["cin"] != 3:
            dx = torch.full(o["dx"].shape, float("nan"), device=dev)
            e.debug_conv(1, ci, None, t(o["dy"]), dx, IMGS)
            r.append(rel(dx, o["dx"]))
        dw = torch.full(o["dw"].shape, float("nan"), device=dev)
        e.debug_conv(2, ci, t(o["xz"]), t(o["dyz"]), dw, IMGS)
        r.append(rel(dw, o["dw"]))
        errs[sp] = r
    print(f"{_short(c)} relative L2 error vs float64 (fwd, [dgrad,] wgrad): {errs}")
    REPORT.setdefault("product_forms/random", {})[_short(c)] = {str(k): v for k, v in errs.items()}
    _dump_report(REPORT, REPORT_PATH)
    for sp in (9, 6):
        for k in range(len(errs[0])):
            assert errs[sp][k] <= 1.25 * errs[0][k] + 1e-9, (sp, k, errs)
            assert errs[sp][k] < 2e-6, (sp, k, errs)


# ---- operand prologues through fm_debug_conv_fwd ---------------------------------------------------------------------------------------------
def _fwd_hook(e, ci, x, c, groups, stats=False, **kw):
    """one fm_debug_conv_fwd launch with NaN-prefilled, canaried buffers; numpy operands in, (out, stats) out"""
    pool = []
    xb = Buf(e, x.size, False, x, pool)
    ops = {k: Buf(e, np.asarray(v).size, False, v, pool).t for k, v in kw.items() if k != "act" and v is not None}
    yb = Buf(e, IMGS * c["hout"] * c["wout"] * c["cout_p"], pool=pool)
    sb = Buf(e, groups * 2 * c["cout_p"], pool=pool) if stats else None
    e.debug_conv_fwd(ci, xb.t, yb.t, IMGS, groups, act=kw.get("act", 0), stats=sb.t if stats else None, **ops)
    _canaries(pool, f"conv_fwd hook, conv {ci}")
    return yb.np((IMGS, c["hout"], c["wout"], c["cout_p"])), (sb.np((groups, 2, c["cout_p"])) if stats else None)


def _materialised(e, ci, c, a, groups):
    """the plain forward on an operand formed beforehand (fp32, by torch on the device): what the fused prologue replaces"""
    out = torch.full((IMGS, c["hout"], c["wout"], c["cout_p"]), float("nan"), device=e.device)
    e.debug_conv_fwd(ci, a.contiguous(), out, IMGS, groups)
    return out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("products", [6, 0, 9])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("groups", [2, 1])
@pytest.mark.parametrize("ci", CR.prologue_convs())
def test_prologues(engs, ci, groups, family, products):
    """GATE = 1 and GATE = 2 of the streaming kernel, which no other hook reaches on an fp32 handle: the project convs with cin_p
    32, 96, 144, 240 (HW = 2304, 576, 144, 36) and every stream-eligible conv on the 6 x 6 and 3 x 3 maps (HW = 36 and 9: a 16-pixel
    fragment straddles images, a block straddles groups' ends), gates different per image, psc / psh different per group.
    Gate only (plain, and under the eval epilogue scale / shift / res when groups = 1): dyadic bit exact.  psc + psh + gate with
    statistics: dyadic at psc = psh = 0, where the operand, the output and the statistics must be exactly 0; random within
    conv_ref.prologue_bound, statistics against the stored output.  How far the fused result is from materialise-then-convolve is
    recorded in the report (pro.*/fused_vs_materialised), not asserted.
    On all three handles, so that GATE = 1 and GATE = 2 run as SP = 6, SP = 9 and SP = 0 at every K and HW (on the products = 6 / 9
    handles K = 240 runs the fp32 pipe anyway); the dyadic bits and the random bound are the same in every product form."""
    e = _use(engs[products], family)
    c, name = CONVS[ci], _short(CONVS[ci])
    o = _case(family, ci)
    x, w = o["x"], o["w"]
    gate, psc, psh = CR.prologue_operands(GEN, family, c, ci, groups, zero_affine=family == "dyadic")
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(e.device)
    per = lambda v: torch.from_numpy(np.ascontiguousarray(CR.per_pixel(v, x), np.float32)).to(e.device)

    # gate only
    a = CR.prologue(x, gate)
    want, bound = CR.pw_fwd(a, w), CR.prologue_bound(GEN, x, gate, None, None, w)
    if family == "dyadic":
        _exact(CR.pw_fwd(np.abs(a), np.abs(w)).reshape(1, -1), 1.0 / 16)
    got, _ = _fwd_hook(e, ci, x, c, groups, gate=gate)
    _check(family, f"pro.gate {name} g{groups}", got, want, bound)
    if family == "random":
        mat = _materialised(e, ci, c, xt * per(gate), groups)
        r = REPORT.setdefault("pro.gate/fused_vs_materialised", {})
        r["max_abs_diff_over_max_abs"] = max(r.get("max_abs_diff_over_max_abs", 0.0), float(np.abs(got - mat).max() / np.abs(want).max()))
    if groups == 1:     # the eval form of a project conv: gate prologue + BN2 affine + skip connection
        scale, shift, res = CR.epilogue_operands(GEN, family, c, ci, 0, True)
        if family == "dyadic":
            _exact((np.abs(want) * np.abs(scale) + np.abs(shift) + np.abs(res)).reshape(1, -1), 1.0 / 64)
        got, _ = _fwd_hook(e, ci, x, c, 1, gate=gate, scale=scale, shift=shift, res=res, act=0)
        _check(family, f"pro.gate_epi {name}", got, CR.epilogue(want, scale, shift, res, 0), CR.epilogue_bound(GEN, want, bound, scale, shift, res, 0))

    # BN1 affine + swish + gate, with statistics
    a = CR.prologue(x, gate, psc, psh)
    want, bound = CR.pw_fwd(a, w), CR.prologue_bound(GEN, x, gate, psc, psh, w)
    got, st = _fwd_hook(e, ci, x, c, groups, stats=True, gate=gate, psc=psc, psh=psh)
    if family == "dyadic":
        assert not a.any() and not want.any()
    _check(family, f"pro.affine {name} g{groups}", got, want, bound)
    stored = want if family == "dyadic" else got.astype(np.float64)
    ref, sbnd = R.bn_stats(stored, groups), CR.stats_bound(stored, groups)
    _check(family, f"pro.affine_stats {name} g{groups} sum", st[:, 0], ref[:, 0], sbnd[:, 0])
    _check(family, f"pro.affine_stats {name} g{groups} sumsq", st[:, 1], ref[:, 1], sbnd[:, 1])
    if family == "random":
        mat = _materialised(e, ci, c, F.silu(xt * per(psc) + per(psh)) * per(gate), groups)
        r = REPORT.setdefault("pro.affine/fused_vs_materialised", {})
        r["max_abs_diff_over_max_abs"] = max(r.get("max_abs_diff_over_max_abs", 0.0), float(np.abs(got - mat).max() / np.abs(want).max()))


# ---- the fused eval epilogue -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", CR.epilogue_cases(), ids=lambda p: f"{_short(CONVS[p[0]])}-act{p[1]}")
def test_eval_epilogue(engs, case, family):
    """act(conv scale + shift + res) as forward_eval runs it: swish with scale / shift on the stem, an expand conv and the head
    (stem kernel, streaming kernel, igemm), scale / shift / res without activation on a streaming and an igemm project conv.
    Dyadic: bit exact for act 0, and for act 2 at scale = shift = 0.  Random: conv_ref.epilogue_bound on top of (K + 2) u sum|a b|."""
    ci, act, with_res = case
    e = _use(engs[6], family)
    o = _case(family, ci)
    c = o["c"]
    scale, shift, res = CR.epilogue_operands(GEN, family, c, ci, act, with_res)
    if family == "dyadic":
        _exact((o["ya"] * np.abs(scale) + np.abs(shift) + (np.abs(res) if with_res else 0.0)).reshape(1, -1), 1.0 / 16)
    got, _ = _fwd_hook(e, ci, o["x"], c, 1, scale=scale, shift=shift, res=res, act=act)
    want = CR.epilogue(o["y"], scale, shift, res, act)
    bound = CR.epilogue_bound(GEN, o["y"], CR.dot_bound(c["Kw"], o["ya"]), scale, shift, res, act)
    _check(family, f"epi.{_arm_name(CR.fwd_arm(c))}_act{act} {_short(c)}", got, want, bound)


RESNET_CASES = [(1, 1, True), (5, 0, False), (7, 0, False)]      # layer1.0.conv1: scale / shift / res / relu; layer2.0.conv1 and its downsample


@pytest.fixture(scope="module")
def resnets():
    """64 x 64 ResNet-18 handles: planes mode (the default) and the fp32 matrix pipe; the three convs under test carry the family's
    weights, set per test"""
    from fedmlp_amd.engine import Engine
    es = {"planes": Engine("Resnet18", 5, 64, 64, IMGS), "products0": Engine("Resnet18", 5, 64, 64, IMGS, products=0)}
    assert es["planes"].planes and not es["products0"].planes and es["products0"].products == 0
    yield es
    for e in es.values():
        _LOADED.pop(id(e), None)
        e.close()


@functools.lru_cache(maxsize=None)
def _resnet_sd(family):
    from tests.test_kernels_gpu import conv_names
    flat, cnt = spec.init_state("Resnet18", 5, 1037)
    sd = spec.flat_to_state_dict("Resnet18", 5, flat, cnt)
    rs = np.random.RandomState(515)
    for ci, _, _ in RESNET_CASES:
        key = conv_names()[ci] + ".weight"
        sd[key] = _wts(family, rs, (sd[key].size,)).reshape(sd[key].shape).astype(np.float32)
    return sd


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mode", ["planes", "products0"])
@pytest.mark.parametrize("case", RESNET_CASES, ids=lambda p: f"conv{p[0]}-act{p[1]}")
def test_eval_epilogue_resnet(resnets, case, mode, family):
    """the same epilogue on ResNet-18 (conv_fwd's planes kernel in the default mode, igemm.hip with products = 0): layer1.0.conv1 with
    scale / shift / res / relu, the stride-2 layer2.0.conv1 and its 1x1 downsample with scale / shift, against F.conv2d in float64.
    Dyadic: bit exact.  Random: (Kw + 2) u sum|x w| through conv_ref.epilogue_bound."""
    from tests.test_kernels_gpu import conv_names
    ci, act, with_res = case
    e = resnets[mode]
    sd = _resnet_sd(family)
    if _LOADED.get(id(e)) != family:
        e.set_state(*spec.state_dict_to_flat("Resnet18", 5, sd))
        _LOADED[id(e)] = family
    c = e.debug_conv_info(ci)
    rs = np.random.RandomState(600 + ci)
    x = _vals(family, rs, (IMGS, c["hin"], c["win"], c["cin_p"]), False)
    scale, shift = _coef(family, rs, (c["cout"],)), _coef(family, rs, (c["cout"],))
    res = _vals(family, rs, (IMGS, c["hout"], c["wout"], c["cout"]), False) if with_res else None
    w = torch.from_numpy(sd[conv_names()[ci] + ".weight"]).double()
    conv = lambda a, b: F.conv2d(torch.from_numpy(a).permute(0, 3, 1, 2), b, None, c["stride"], c["pad"]).permute(0, 2, 3, 1).numpy()
    y, ya = conv(x, w), conv(np.abs(x), w.abs())
    if family == "dyadic":
        _exact(ya.reshape(1, -1), 0.25)
        _exact((ya * np.abs(scale) + np.abs(shift) + (np.abs(res) if with_res else 0.0)).reshape(1, -1), 1.0 / 16)
    assert c["cout_p"] == c["cout"]
    got, _ = _fwd_hook(e, ci, x, c, 1, scale=scale, shift=shift, res=res, act=act)
    want = CR.epilogue(y, scale, shift, res, act)
    bound = CR.epilogue_bound(GEN, y, CR.dot_bound(c["Kw"], ya), scale, shift, res, act)
    _check(family, f"epi.resnet_{mode}_act{act} conv{ci}", got, want, bound)


# ---- stream-K fix-up on EfficientNet shapes ------------------------------------------------------------------------------------------------------
def _streamk_ops():
    """[(conv, ops)]: the forwards (the stem's among them) and data gradients that launch_igemm keeps for igemm.hip"""
    out = []
    for ci, c in enumerate(CONVS):
        ops = tuple(op for op, arm in (("fwd", CR.fwd_arm(c)), ("dgrad", CR.dgrad_arm(c)))
                    if arm[0] == "igemm" or (op == "fwd" and arm[0] == "stem"))
        if ops:
            out.append((ci, ops))
    return out


def _streamk_child():
    """(child process) the dyadic sweep of those, on a fresh default handle; the report stays the parent's: nothing is written"""
    GEN._dump_report = lambda report, path: None
    e = _make_engine()
    try:
        for ci, ops in _streamk_ops():
            _sweep(e, "dyadic", ci, ops)
    finally:
        e.close()
    print(f"ok {sum(len(ops) for _, ops in _streamk_ops())}")


def test_streamk_forced_splits():
    """Stream-K fix-up (partial tiles summed by the last arriver) on EfficientNet shapes -- M = 80, 112, 192, 320 with their partial
    64- and 128-row tiles, K = 320 .. 1280: the persistent grid is forced to odd block counts in a fresh child process per count
    (the override is read once per process), as test_conv_streamk_forced_splits does on ResNet shapes.  Bit exact: partial tiles of
    exact sums add exactly."""
    code = "import sys; sys.path.insert(0, '.'); import tests.test_eff_conv_f32_gpu as T; T._streamk_child()"
    n = sum(len(ops) for _, ops in _streamk_ops())
    assert n == 24, _streamk_ops()          # 12 forwards (10 project convs with K > 256, the head, the stem), 12 data gradients
    for nb in ("7", "61", "509"):
        env = dict(os.environ, FM_IGEMM_BLOCKS=nb)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"ok {n}" in r.stdout, f"FM_IGEMM_BLOCKS={nb}: {r.stdout[-2000:]} {r.stderr[-3000:]}"


# ---- the hook's contract ---------------------------------------------------------------------------------------------------------------------
def test_hook_contract(engs, resnets):
    """fm_debug_conv_fwd takes the three forms the engine's graphs use and nothing else: every other combination returns FM_ERR_ARG
    before any launch (the output stays as it was), never reaches conv_fwd's deferred-error branches, and leaves the handle usable:
    afterwards a plain forward is still bit exact and sync() reports nothing."""
    from fedmlp_amd._lib import FmError
    e = _use(engs[6], "dyadic")
    idx = {_short(c): i for i, c in enumerate(CONVS)}
    cs, ck = idx["b1.proj"], idx["b7.proj"]                  # a streaming project conv; one with K = 480 (igemm)
    dev = e.device

    def bad(eng, ci, c, groups=1, **kw):
        z = lambda *s: torch.zeros(s, device=dev)
        out = torch.full((IMGS, c["hout"], c["wout"], c["cout_p"]), float("nan"), device=dev)
        x = z(IMGS, c["hin"], c["win"], c["cin_p"])
        shapes = dict(scale=(c["cout_p"],), shift=(c["cout_p"],), res=tuple(out.shape), psc=(groups, c["cin_p"]), psh=(groups, c["cin_p"]),
                      gate=(IMGS, c["cin_p"]), stats=(groups, 2, c["cout_p"]))
        ops = {k: (z(*shapes[k]) if v is True else v) for k, v in kw.items()}
        with pytest.raises(FmError, match="error -1"):
            eng.debug_conv_fwd(ci, x, out, IMGS, groups, **ops)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), (ci, kw, "something was launched")

    c, er = CONVS[cs], resnets["products0"]
    bad(e, ck, CONVS[ck], gate=True)                                              # a prologue on a conv the streaming kernel refuses
    bad(e, ck, CONVS[ck], 2, gate=True, psc=True, psh=True, stats=True)
    bad(e, 0, CONVS[0], gate=True)                                                # ... on the stem
    bad(e, cs, c, scale=True)                                                     # half a pair
    bad(e, cs, c, shift=True)
    bad(e, cs, c, 2, gate=True, psc=True, stats=True)
    bad(e, cs, c, 2, gate=True, psh=True, stats=True)
    bad(e, cs, c, 2, psc=True, psh=True, stats=True)                              # psc / psh without a gate
    bad(e, cs, c, 2, scale=True, shift=True)                                      # groups > 1 with an epilogue
    bad(e, cs, c, 1, scale=True, shift=True, stats=True)                          # statistics with an epilogue
    bad(e, cs, c, 2, gate=True, stats=True)                                       # gate alone with statistics
    bad(e, cs, c, 2, gate=True, psc=True, psh=True)                               # the affine form without statistics
    bad(e, cs, c, 1, gate=True, psc=True, psh=True, stats=True, scale=True, shift=True)   # ... with an epilogue
    bad(e, 0, CONVS[0], scale=True, shift=True, res=True)                         # a residual on a stem
    bad(resnets["planes"], 0, er.debug_conv_info(0), scale=True, shift=True, res=True, act=1)
    bad(e, cs, c, res=True)                                                       # res / act without scale and shift
    bad(e, cs, c, act=2)
    bad(e, cs, c, scale=True, shift=True, act=3)
    bad(er, 7, er.debug_conv_info(7), gate=True)                                  # a prologue on a ResNet-18 handle (its 1x1 downsample)
    bad(resnets["planes"], 7, er.debug_conv_info(7), gate=True)
    for eng in (e, er, resnets["planes"]):
        eng.sync()                                                                # no deferred error
    o = _case("dyadic", cs)
    got, st = _fwd_hook(e, cs, o["x"], c, GROUPS, stats=True)
    _bits(f"contract.plain {_short(c)} y", got, o["y"])
    _bits(f"contract.plain {_short(c)} stats", st, R.bn_stats(o["y"], GROUPS))
    e.sync()
