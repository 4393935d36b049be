"""Kernel-level parity of ResNet-18's convolution GEMMs at non-square shapes -- the planes kernels (csrc/pconv.hip in its
tap-row-sharing and per-tap forms with the stream-K fix-up and the planes eval epilogue, pwgrad.hip, pwgrad_ring.hip, stem_rows.hip,
stem_dgrad.hip) and, on a products = 0 handle, igemm.hip with the generic wgrad.hip -- through fm_debug_conv, fm_debug_block_dgrad and
fm_debug_conv_planes against the float64 references of tests/resnet_conv_ref.py (pinned to F.conv2d + autograd by
tests/test_resnet_conv_ref_cpu.py, which also asserts the exactness preconditions of this file's data and shows that these
comparisons reject subtly wrong results).  The method, buffers and generators are those of tests/test_eff_kernels_gpu.py.

Shapes (H x W, images / groups): S1 32 x 224, 4 / 2: stem_rows at Ho = 16, maps 8x56 and 4x28 (ring), 2x14, 1x7.  S2 224 x 32, 4 / 2:
tall maps down to 7x1 -- both halo neighbours of the tap-row-sharing form lie in another row; the stem takes igemm's packed form.
S3 96 x 160, 5 / 1: an odd image count, widths 40, 20, 10, 5.  S4 32 x 32 with 1 and with 3 images: maps 8x8 down to 1x1, fewer pixels
than one 16-row fragment, tilesN = 1 everywhere.

DYADIC and PLANES3 (two arms, see resnet_conv_ref): every product and every partial sum in any order is exact in every product form;
outputs and gradients must equal the float64 reference BIT FOR BIT.  The dyadic statistics too: every tile partial is an fp32 number
(asserted on the data), fm_debug_conv folds the tiles in double and rounds once, so does the reference.  A planes3 output has about
20 significant bits, its square 40: no exact statistics exist there, and that family's statistics are held, like the random one's,
against the float64 sums of the output the same launch stored, within conv_ref.stats_bound.
RANDOM: standard normal; a K-term dot product is within (K + 2) u sum|a b| of float64 in every product form (conv_ref.dot_bound), K =
Kw (forward), the taps of the pixel's parity class x cout (data gradient), imgs hout wout (weight gradient).
Worst error / bound ratios and bit-exact check counts go to resnet_conv_parity.json beside the other parity reports.

Canaries: every output sits between NaN margins and is pre-filled with NaN."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fedmlp_amd import spec
from tests import bn_ref as B
from tests import resnet_conv_ref as RR
from tests import test_eff_kernels_gpu as GEN
from tests.test_eff_kernels_gpu import Buf, _canaries, _parity
from tests.test_local_training_gpu import _dump as _dump_report

pytestmark = pytest.mark.gpu

REPORT = {}
REPORT_PATH = "resnet_conv_parity.json"
_bits, _within, _ = _parity(REPORT, REPORT_PATH)
ARMS = {}                       # (shape, form, op, conv) -> the launcher fm_debug_conv_arm reports
# (shape, form): form = fm_config.reserved[2] (None: the default, six products; 9; 0: the fp32 matrix pipe, not planes mode)
HANDLES = [(s, None) for s in ("S1", "S2", "S3", "S4a", "S4b")] + [("S1", 9), ("S1", 0), ("S2", 0)]
_ENG, _LOADED = {}, {}


def _engine(shape, form):
    """one handle per (H x W, product form), kept for the module (S4a and S4b share theirs)"""
    H, W, _, _, max_imgs = RR.SHAPES[shape]
    key = (H, W, form)
    if key not in _ENG:
        from fedmlp_amd.engine import Engine
        e = Engine("Resnet18", 5, H, W, max_imgs, products=form)
        assert e.planes == (form != 0) and e.products == (6 if form is None else form) and e.debug_num_convs() == 20
        for i, c in enumerate(RR.r18_convs(H, W)):
            assert {k: c[k] for k in RR.INFO_KEYS} == e.debug_conv_info(i), (i, e.debug_conv_info(i))
        _ENG[key] = e
    return _ENG[key]


@pytest.fixture(scope="module", autouse=True)
def _handles():
    yield
    for e in _ENG.values():
        e.close()
    _ENG.clear()
    _LOADED.clear()


@functools.lru_cache(maxsize=None)
def _weights(family):
    return RR.model_weights(GEN, family)


def _use(e, family):
    """the family's weights on handle e (set_state re-lays them out and re-packs the transposed / plane copies)"""
    if _LOADED.get(id(e)) != family:
        e.set_state(*spec.state_dict_to_flat("Resnet18", 5, RR.state_dict(GEN, family)))
        _LOADED[id(e)] = family
    return e


@functools.lru_cache(maxsize=3)
def _case(family, shape, ci):
    o = RR.sweep_reference(GEN, family, shape, ci, _weights(family))
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


def _check(family, name, got, want64, bound):
    """exact families: the same bits (counted in the report under the family's name); random: within the bound"""
    if family == "random":
        return _within(name, got, want64, bound)
    key = name.split(" ")[0]
    before = REPORT.get(key + "/dyadic", {}).get("bit_exact_checks", 0)
    _bits(name, got, want64)
    if family != "dyadic":          # (_bits counts under "dyadic": move this check to its family)
        if before:
            REPORT[key + "/dyadic"]["bit_exact_checks"] = before
        else:
            del REPORT[key + "/dyadic"]
        r = REPORT.setdefault(key + "/" + family, {})
        r["bit_exact_checks"] = r.get("bit_exact_checks", 0) + 1
        _dump_report(REPORT, REPORT_PATH)


def _form_tag(form):
    return "sp6" if form is None else f"sp{form}"


# ---- one conv, three ops ---------------------------------------------------------------------------------------------------------------
def _sweep(e, family, shape, form, ci):
    """forward + statistics, data gradient and weight gradient of conv ci on handle e against the shared reference"""
    imgs, groups = RR.SHAPES[shape][2:4]
    o = _case(family, shape, ci)
    c = o["c"]
    name = f"{c['name']} {shape} {_form_tag(form)}"
    _use(e, family)
    for op in range(3):
        ARMS[(shape, form, op, ci)] = e.debug_conv_arm(op, ci, imgs)
    # forward with folded statistics
    pool = []
    xb = Buf(e, o["x"].size, False, o["x"], pool)
    yb, sb = Buf(e, o["y"].size, pool=pool), Buf(e, groups * 2 * c["cout"], pool=pool)
    e.debug_conv(0, ci, xb.t, None, yb.t, imgs, groups, sb.t)
    _canaries(pool, name + " fwd")
    got = yb.np(o["y"].shape)
    _check(family, f"fwd {name}", got, o["y"], RR.dot_bound(c["Kw"], o["ya"]))
    st = sb.np((groups, 2, c["cout"]))
    if family == "dyadic":
        ref = RR.stats_stored(o["y"])(groups)
        _check(family, f"stats {name} sum", st[:, 0], ref[:, 0], None)
        _check(family, f"stats {name} sumsq", st[:, 1], ref[:, 1], None)
    else:
        stored = got.astype(np.float64)
        ref, sbnd = RR.bn_stats(stored, groups), RR.stats_bound(stored, groups)
        _within(f"stats {name} sum", st[:, 0], ref[:, 0], sbnd[:, 0], family)
        _within(f"stats {name} sumsq", st[:, 1], ref[:, 1], sbnd[:, 1], family)
    # data gradient (the stem: the stem_dgrad kernel)
    pool = []
    db = Buf(e, o["dy"].size, False, o["dy"], pool)
    full = (imgs, c["hin"], c["win"], c["cin"])
    xb = Buf(e, int(np.prod(full)), pool=pool)
    e.debug_conv(1, ci, None, db.t, xb.t, imgs)
    _canaries(pool, name + " dgrad")
    got = xb.np(full)
    if c["k"] == 1 and c["stride"] == 2:        # the only parity class of a stride-2 1x1 conv; nothing else may be touched
        rest = got.copy()
        rest[:, ::2, ::2] = np.nan
        assert np.isnan(rest).all(), f"{name}: the stride-2 1x1 data gradient wrote outside parity class (0, 0)"
    _check(family, f"dgrad {name}", RR.written(got, c), o["dx"], RR.dot_bound(o["dxK"], o["dxa"]))
    # weight gradient
    pool = []
    xb, db = Buf(e, o["xw"].size, False, o["xw"], pool), Buf(e, o["dyw"].size, False, o["dyw"], pool)
    wb = Buf(e, o["dw"].size, pool=pool)
    e.debug_conv(2, ci, xb.t, db.t, wb.t, imgs)
    _canaries(pool, name + " wgrad")
    got = wb.np(o["dw"].shape)
    _check(family, f"wgrad {name}", got, o["dw"], RR.dot_bound(imgs * c["hout"] * c["wout"], o["dwa"]))
    if ci == 0:         # the packed stem: the zero tap slot kw = 7 of every kernel row and the 8 pad columns stay exactly 0
        assert not got[:, :168].reshape(64, 7, 8, 3)[:, :, 7].any() and not got[:, 168:].any(), f"{name}: a pad slot of dw moved"


def _sweep_params():
    """form varies fastest, so that the forms of a (shape, family, conv) share one reference"""
    out = []
    for shape in RR.SHAPES:
        forms = [f for s, f in HANDLES if s == shape]
        for family in RR.FAMILIES:
            for ci in range(20):
                out += [pytest.param(shape, form, family, ci, id=f"{shape}-{_form_tag(form)}-{family}-{RR.conv_names()[ci]}") for form in forms]
    return out


@pytest.mark.parametrize("shape,form,family,ci", _sweep_params())
def test_sweep(shape, form, family, ci):
    """all 20 convs at every shape on the default handle, S1 also with nine products, S1 and S2 also on the fp32 matrix pipe
    (igemm.hip and the generic wgrad.hip): forward with folded statistics, data gradient, weight gradient (module docstring)"""
    _sweep(_engine(shape, form), family, shape, form, ci)


# ---- the grouped data gradient of the stride-2 blocks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [2, 4, 6])
@pytest.mark.parametrize("family", RR.FAMILIES)
@pytest.mark.parametrize("shape", list(RR.SHAPES))
def test_block_dgrad(shape, family, block):
    """fm_debug_block_dgrad: dx = dgrad(conv1; dy1) + dgrad(downsample; dyd) as ONE grouped launch of the per-tap planes kernel.
    Every element is written (NaN prefill); exact families bit exact, random within (K + 2) u sum|a b| with K = both convs' taps of
    the pixel's parity class x cout"""
    imgs = RR.SHAPES[shape][2]
    e = _use(_engine(shape, None), family)
    o = RR.block_reference(GEN, family, shape, block, _weights(family))
    pool = []
    b1, bd = Buf(e, o["dy1"].size, False, o["dy1"], pool), Buf(e, o["dyd"].size, False, o["dyd"], pool)
    xb = Buf(e, o["dx"].size, pool=pool)
    e.debug_block_dgrad(block, b1.t, bd.t, xb.t, imgs)
    e.sync()
    _canaries(pool, f"block {block} {shape}")
    _check(family, f"block_dgrad block{block} {shape}", xb.np(o["dx"].shape), o["dx"], RR.dot_bound(o["K"], o["dxa"]))


# ---- the planes eval epilogue --------------------------------------------------------------------------------------------------------------
def _words(e, a):
    """fp32 NHWC -> the int16 device tensor of its block-major planes, between sentinel margins"""
    w = B.encode_planes(np.asarray(a, np.float32).reshape(-1, a.shape[-1]))
    b = Buf(e, w.size, True)
    b.t.copy_(torch.from_numpy(w.view(np.int16).copy()).to(e.device))
    return b


def _unwords(b, shape):
    """the fp32 values of an output planes buffer: (h + m) + l"""
    P, C = int(np.prod(shape[:-1])), shape[-1]
    return B.planes_sum(*B.decode_planes(b.t.cpu().numpy()[:3 * P * C], P, C)).reshape(shape)


def _planes_call(e, ci, o, imgs, scale, shift, res, res_form, relu, outs):
    c = o["c"]
    pool = []
    xp = _words(e, o["x"]); pool.append(xp)
    sc, sh = Buf(e, scale.size, False, scale, pool), Buf(e, shift.size, False, shift, pool)
    rf = Buf(e, res.size, False, res, pool) if res_form == "f32" else None
    rp = _words(e, res) if res_form == "planes" else None
    if rp is not None:
        pool.append(rp)
    n = o["y"].size
    yb = Buf(e, n, pool=pool) if outs in ("f32", "both") else None
    yp = Buf(e, 3 * n, True, pool=pool) if outs in ("planes", "both") else None
    e.debug_conv_planes(ci, xp.t, imgs, sc.t, sh.t, rf.t if rf else None, rp.t if rp else None, relu, yb.t if yb else None, yp.t if yp else None)
    _canaries(pool, f"conv_planes {c['name']}")
    return (yb.np(o["y"].shape) if yb else None), (_unwords(yp, o["y"].shape) if yp else None)


@pytest.mark.parametrize("case", RR.EPILOGUE_CASES, ids=lambda p: f"{p[0]}-relu{p[1]}-res_{p[2]}-out_{p[3]}")
@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("shape", RR.EPILOGUE_SHAPES)
def test_eval_epilogue_planes(shape, family, case):
    """conv_fwd as forward_eval calls it in planes mode, through fm_debug_conv_planes: planes in; planes-only out, fp32 out, or both
    (then the same floats); the residual as fp32 or as planes.  Operand planes are encoded and output planes decoded on the host
    (bn_ref).  Dyadic: bit exact.  Random: conv_ref.epilogue_bound on top of (Kw + 2) u sum|x w|."""
    name, relu, res_form, outs = case
    imgs = RR.SHAPES[shape][2]
    convs = RR.r18_convs(*RR.SHAPES[shape][:2])
    ci = [c["name"] for c in convs].index(name)
    e = _use(_engine(shape, None), family)
    o = _case(family, shape, ci)
    scale, shift, res = RR.epilogue_operands(GEN, family, shape, ci, o["c"], res_form is not None)
    ARMS[(shape, None, 0, ci)] = e.debug_conv_arm(0, ci, imgs)
    y, yp = _planes_call(e, ci, o, imgs, scale, shift, res, res_form, relu, outs)
    want = RR.epilogue(o["y"], scale, shift, res, relu)
    bound = RR.epilogue_bound(GEN, o["y"], RR.dot_bound(o["c"]["Kw"], o["ya"]), scale, shift, res, relu)
    for tag, got in (("f32", y), ("planes", yp)):
        if got is not None:
            _check(family, f"epi.{tag} {name} {shape}", got, want, bound)
    if outs == "both":
        assert B.same_floats(y, yp), f"{name} {shape}: the planes output is not the fp32 output"


# ---- which launcher ran ----------------------------------------------------------------------------------------------------------------------
def test_arms_are_reached():
    """fm_debug_conv_arm over every case of test_sweep (the conv tables are the engine's own: _engine checks them), and the union
    covers every arm ResNet-18 has.  The tile shapes are restated from the table: pconv's and pwgrad's M tile is 64 rows for 64
    output rows, else 128; pwgrad's N tile is 6 column blocks when k k cin_p / 32 is a multiple of 6 and not of 8, else 8.  Three of
    pwgrad's four tile shapes exist in ResNet-18: every conv with 64 output channels has k k cin_p / 32 = 18, so (64, 8) is asserted
    absent from the model rather than silently skipped."""
    for shape, form in HANDLES:
        e = _engine(shape, form)
        for ci in range(20):
            for op in range(3):
                ARMS.setdefault((shape, form, op, ci), e.debug_conv_arm(op, ci, RR.SHAPES[shape][2]))
    seen = set()
    for (shape, form, op, ci), arm in ARMS.items():
        c = RR.r18_convs(*RR.SHAPES[shape][:2])[ci]
        planes = form != 0
        M = c["cout"] if op == 0 else c["cin"]
        tile = ()
        if arm in ("pconv_ts", "pconv_tap"):
            tile = (64 if M == 64 else 128,)
        if arm == "pwgrad":
            nb = c["k"] * c["k"] * c["cin_p"] // 32
            tile = (64 if c["cout_p"] == 64 else 128, 6 if (nb % 8 != 0 and nb % 6 == 0) else 8)
        seen.add((arm,) + tile)
        if op == 2 and ci > 0:
            ring = planes and c["k"] == 3 and c["stride"] == 1 and 28 <= c["win"] <= 62
            assert (arm == "pwgrad_ring") == ring, (shape, form, c["name"], arm)
            assert arm in (("pwgrad", "pwgrad_ring") if planes else ("wgrad_generic",)), (shape, form, c["name"], arm)
        if ci == 0:
            fwd = "stem_rows" if (planes and c["wout"] == 112) else "igemm_stem"
            assert arm == (fwd, "stem_dgrad", "wgrad_generic")[op], (shape, form, arm)
        elif op < 2:
            assert (arm in ("pconv_ts", "pconv_tap")) == planes and (planes or arm == "igemm"), (shape, form, c["name"], arm)
            if planes:      # tap rows are shared by the 3x3 stride-1 convs and their data gradients
                assert (arm == "pconv_ts") == (c["k"] == 3 and c["stride"] == 1), (shape, form, c["name"], op, arm)
    print(sorted(seen))
    want = {("stem_rows",), ("igemm_stem",), ("igemm",), ("stem_dgrad",), ("wgrad_generic",), ("pwgrad_ring",), ("pconv_ts", 64), ("pconv_ts", 128),
            ("pconv_tap", 64), ("pconv_tap", 128), ("pwgrad", 64, 6), ("pwgrad", 128, 6), ("pwgrad", 128, 8)}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    assert not any(c["cout_p"] == 64 and (c["k"] ** 2 * c["cin_p"] // 32) % 6 != 0 for c in RR.r18_convs(32, 32)[1:])
    REPORT["arms"] = sorted("/".join(str(v) for v in a) for a in seen)
    _dump_report(REPORT, REPORT_PATH)


# ---- stream-K fix-up --------------------------------------------------------------------------------------------------------------------------
def _streamk_child(shape):
    """(child process) the dyadic sweep of a shape on a fresh default handle; the report stays the parent's: nothing is written"""
    GEN._dump_report = lambda report, path: None
    globals()["_dump_report"] = lambda report, path: None
    try:
        for ci in range(20):
            _sweep(_engine(shape, None), "dyadic", shape, None, ci)
    finally:
        for e in _ENG.values():
            e.close()
    print("ok 20")


def test_streamk_forced_splits():
    """The stream-K fix-up of pconv.hip (partial tiles summed by the last arriver) and the ring's split count at non-square shapes:
    the persistent grid is forced to odd block counts in a fresh child process per count (the override is read once per process;
    pwgrad_ring honours it too) and the dyadic sweep of S1 and S3 runs again.  Bit exact: partial tiles of exact sums add exactly."""
    for nb in ("7", "61"):
        for shape in ("S1", "S3"):
            code = f"import sys; sys.path.insert(0, '.'); import tests.test_resnet_conv_gpu as T; T._streamk_child('{shape}')"
            env = dict(os.environ, FM_IGEMM_BLOCKS=nb)
            r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "ok 20" in r.stdout, f"FM_IGEMM_BLOCKS={nb} {shape}: {r.stdout[-2000:]} {r.stderr[-3000:]}"


# ---- the hook's contract ------------------------------------------------------------------------------------------------------------------------
def test_hook_contract():
    """fm_debug_conv_planes takes the forms forward_eval uses and nothing else: both residuals, no output, a stem conv, a products = 0
    handle, relu = 2 and imgs > max_images return FM_ERR_ARG before any launch (the NaN-prefilled outputs stay NaN), sync() reports
    nothing, and a plain forward afterwards is still bit exact."""
    from fedmlp_amd._lib import FmError
    shape = "S1"
    imgs, groups = RR.SHAPES[shape][2:4]
    e, e0 = _use(_engine(shape, None), "dyadic"), _use(_engine(shape, 0), "dyadic")
    ci = RR.conv_names().index("layer1.0.conv2")
    o = _case("dyadic", shape, ci)
    c = o["c"]

    def bad(eng, conv, n=imgs, res=False, resp=False, relu=1, out=True, outp=True):
        cc = RR.r18_convs(*RR.SHAPES[shape][:2])[conv]
        npix_in, npix_out = (imgs + 1) * cc["hin"] * cc["win"], (imgs + 1) * cc["hout"] * cc["wout"]
        dev = eng.device
        xp = torch.zeros(3 * npix_in * max(cc["cin"], 32), dtype=torch.int16, device=dev)
        sc, sh = torch.ones(cc["cout"], device=dev), torch.zeros(cc["cout"], device=dev)
        rf = torch.zeros(npix_out * cc["cout"], device=dev) if res else None
        rp = torch.zeros(3 * npix_out * cc["cout"], dtype=torch.int16, device=dev) if resp else None
        y = torch.full((npix_out * cc["cout"],), float("nan"), device=dev)
        yp = torch.full((3 * npix_out * cc["cout"],), GEN.WORD, dtype=torch.int16, device=dev)
        with pytest.raises(FmError, match="error -1"):
            eng.debug_conv_planes(conv, xp, n, sc, sh, rf, rp, relu, y if out else None, yp if outp else None)
        torch.cuda.synchronize()
        assert torch.isnan(y).all() and (yp == GEN.WORD).all(), (conv, "something was launched")

    bad(e, ci, res=True, resp=True)             # both residual forms
    bad(e, ci, out=False, outp=False)           # no output
    bad(e, 0)                                   # the stem
    bad(e0, ci)                                 # not planes mode
    bad(e, ci, relu=2)
    bad(e, ci, n=imgs + 1)                      # more than max_images
    for eng in (e, e0):
        eng.sync()                              # no deferred error
    pool = []
    xb = Buf(e, o["x"].size, False, o["x"], pool)
    yb, sb = Buf(e, o["y"].size, pool=pool), Buf(e, groups * 2 * c["cout"], pool=pool)
    e.debug_conv(0, ci, xb.t, None, yb.t, imgs, groups, sb.t)
    _canaries(pool, "contract")
    _bits(f"contract.plain {c['name']} y", yb.np(o["y"].shape), o["y"])
    _bits(f"contract.plain {c['name']} stats", sb.np((groups, 2, c["cout"])), RR.stats_stored(o["y"])(groups))
    e.sync()
