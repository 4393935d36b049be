"""Kernel-level parity of what runs between ResNet-18's conv GEMMs -- BatchNorm finalize / apply / backward, the stem max-pool and
its fused backward, and the bf16 plane writers (elementwise.hip, planes_ew.hip) -- each launcher on its own through
fm_debug_ew, against the float64 restatement in tests/bn_ref.py (itself pinned to torch autograd by tests/test_bn_ref_cpu.py).

Two input families.
DYADIC: every operand is a small multiple of a power of two (y, dz, dp multiples of 1/8 in [-4, 4]; per-channel operands from
{0, +-2^-6, +-2^-4, +-1/2, +-1, +-3/2}), so every fp32 product and sum a kernel forms is exact and its output must equal the float64
reference BIT FOR BIT: values, plane words, masks, argmax codes.  (A zero compares equal to a zero of either sign: IEEE maximum
may return either for max(-0, +0).)  `_bits` also asserts that the reference value is an fp32 number, i.e. that the case really
is exact.
RANDOM: standard-normal operands.  With u = 2^-24, a value formed by t rounded fp32 operations is within t u sum|terms| of the
float64 one, a chain of n sequential additions within (n + 2) u sum|terms|; t and n are read off the kernel and stated in each
test.  Discrete decisions are compared where the float64 margin exceeds that bound; the share left out is asserted <= 0.1 %
(tests/test_bn_ref_cpu.py checks the same share on the CPU).  The worst observed error / bound ratio of every random check goes
to the report ew_parity.json, beside the other parity reports; the figures quoted as "measured" below are from there and are not
thresholds."""
import numpy as np
import pytest
import torch

from fedmlp_amd import spec
from tests import bn_ref as R
from tests.test_local_training_gpu import _dump as _dump_report

pytestmark = pytest.mark.gpu

U = R.U
DY = np.array([0.0, 2.0 ** -6, -2.0 ** -6, 2.0 ** -4, -2.0 ** -4, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5], np.float32)
TINY = np.float32(2.0 ** -126)
# both round-to-nearest-even ties of the split (low 16 bits 0x8000 under an even / odd upper half; the same in x - h), the
# smallest normal, values whose m and l / whose l vanish
SPECIAL = np.concatenate([np.array([0x3F808000, 0x3F818000, 0x3F802020, 0x3F802060], np.uint32).view(np.float32),
                          np.array([TINY, 1.0, 3.0, 1.0 + 2.0 ** -10, 0.0, 255.0], np.float32)])
REPORT = {}


def _dump():
    _dump_report(REPORT, "ew_parity.json")


@pytest.fixture(scope="module")
def eng():
    """one 64 x 64 ResNet-18 handle: the owner of the stream the launchers run on, nothing else"""
    from fedmlp_amd.engine import Engine
    e = Engine("Resnet18", 5, 64, 64, 2)
    flat, cnt = spec.init_state("Resnet18", 5, 3)
    e.set_state(flat, cnt)
    yield e
    e.close()


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32))


def _dev(e, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def _nan(e, *shape):
    return torch.full(shape, float("nan"), device=e.device)


def _planes_buf(e, P, C):
    return torch.full((3 * P * C,), 0x7FC1, dtype=torch.int16, device=e.device)      # a NaN pattern no split produces


def _u32(a):
    return _f32(a).view(np.uint32)


def _bits(name, got, want64):
    """dyadic family: got (fp32) == the float64 reference, bit for bit (zeros of either sign equal)"""
    got, want64 = _f32(got.cpu().numpy() if torch.is_tensor(got) else got), np.asarray(want64, np.float64)
    want = want64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), want64), f"{name}: the dyadic case is not exact in fp32"
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = (_u32(got) != _u32(want)) & ~((got == 0) & (want == 0))
    assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} differ, first at {np.argwhere(bad)[0]}: " \
                          f"{got[bad][0]!r} vs {want[bad][0]!r}"


def _within(name, got, want64, bound):
    """random family: |got - want| <= bound elementwise; records the worst error / bound ratio"""
    got = _f32(got.cpu().numpy() if torch.is_tensor(got) else got).astype(np.float64)
    want64, bound = np.asarray(want64, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want64))
    assert got.shape == want64.shape, (name, got.shape, want64.shape)
    err = np.abs(got - want64)
    assert not np.isnan(got).any(), f"{name}: NaN (an element was not written)"
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"{name}: max|err| {err.max():.3e}, worst err/bound {ratio:.3f}")
    REPORT[name] = {"max_abs_err": float(err.max()), "worst_err_over_bound": ratio}
    _dump()
    bad = err > bound
    assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} beyond the bound, worst err/bound {ratio:.3f}"


def _check(family, name, got, want64, bound):
    if family == "dyadic":
        _bits(name, got, want64)
    else:
        _within(name, got, want64, bound)


def _same(name, a, b):
    a, b = (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (a, b))
    assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name}: not bit-identical"


def _check_planes(name, planes, x32, P, C):
    """planes (device int16 words) against the fp32 tensor x32 [P][C] of the same launch: (h + m) + l == x bit for bit, and every
    word equals the reference split at the documented offset"""
    w = planes.cpu().numpy().view(np.uint16)
    x32 = _f32(x32).reshape(P, C)
    h, m, l = R.decode_planes(w, P, C)
    assert R.same_floats(R.planes_sum(h, m, l), x32), f"{name}: (h + m) + l != x"
    want = R.encode_planes(x32)
    bad = w != want
    assert not bad.any(), f"{name}: {bad.sum()} plane words differ from the reference split, first word {np.argwhere(bad)[0]}"


def _vals(family, rs, shape):
    return _f32(rs.randint(-32, 33, shape) / 8.0) if family == "dyadic" else _f32(rs.standard_normal(shape))


def _coef(family, rs, shape, allowed=DY):
    return _f32(rs.choice(allowed, shape)) if family == "dyadic" else _f32(rs.standard_normal(shape))


def _full_mantissa(rs, shape):
    return _f32(rs.standard_normal(shape) * np.exp2(rs.randint(-20, 20, shape)))


def _sprinkle(rs, x):
    """SPECIAL and its negatives at scattered positions of x (in place)"""
    flat = x.reshape(-1)
    sp = np.concatenate([SPECIAL, -SPECIAL])
    pos = rs.choice(flat.size, 4 * sp.size, replace=False)
    flat[pos] = np.tile(sp, 4)
    return pos


# ---- planes round trip ------------------------------------------------------------------------------------------------------
PLANE_SHAPES = [(1, 5, 512), (2, 37, 64), (2, 37, 128)]


@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=str)
def test_planes_round_trip(eng, shape):
    """k_split_planes writes the reference split word for word; k_planes_to_f32 of it is x bit for bit (-0 comes back as +0: its
    sign lives in the h plane only and (-0) + (+0) = +0)"""
    G, pix, C = shape
    P = G * pix
    rs = np.random.RandomState(11)
    x = _full_mantissa(rs, (P, C))
    _sprinkle(rs, x)
    xd, pl, back = _dev(eng, x), _planes_buf(eng, P, C), _nan(eng, P, C)
    eng.debug_ew("split_planes", [xd, pl], [P, C])
    _check_planes("split_planes", pl, x, P, C)
    eng.debug_ew("planes_to_f32", [pl, back], [P, C])
    assert R.same_floats(back.cpu().numpy(), x), "planes_to_f32(split_planes(x)) != x"
    neg0 = _u32(x) == 0x80000000
    assert neg0.sum() == 4 and not _u32(back.cpu().numpy())[neg0].any()          # -0 reads back as +0 (bn_ref.same_floats)


# ---- BatchNorm apply and its plane writer ---------------------------------------------------------------------------------------
def apply_case(family, shape, seed=21):
    G, pix, C = shape
    rs = np.random.RandomState(seed)
    c = {k: _vals(family, rs, (G, pix, C)) for k in ("y", "y2")}
    c["res"] = _vals(family, rs, (G, pix, C)) if family == "dyadic" else _full_mantissa(rs, (G, pix, C))
    for k in ("scale", "shift", "scale2", "shift2"):
        c[k] = _coef(family, rs, (G, C))
    if family == "dyadic":          # channels 0 .. 3 pass y through (scale 1, shift 0): the special values reach the writers
        c["scale"][:, :4], c["shift"][:, :4] = 1.0, 0.0
        c["y"][:, :, :4] = np.resize(np.concatenate([SPECIAL, -SPECIAL]), G * pix * 4).reshape(G, pix, 4)
    return c


APPLY_COMBOS = {"plain_norelu": ((), 0), "plain": ((), 1), "res": (("res",), 1), "resp": (("resp",), 1),
                "y2": (("y2",), 1), "y2_norelu": (("y2",), 0)}


@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=str)
@pytest.mark.parametrize("family", ["dyadic", "random"])
def test_bn_apply_and_planes(eng, family, shape):
    """out = [relu](y scale + shift [+ res] [+ y2 scale2 + shift2]) in every operand combination forward_train uses, fp32 kernel and
    planes kernel.  Random bound: t u sum|terms| with t = 2 (multiply, add; one fused operation rounds less), + 1 for the residual,
    + 3 for the second product, shift and sum.  Measured: worst err / bound 0.59.  The planes of a launch must be the exact
    split of that launch's fp32 output; a planes-only launch (out NULL) writes the same words; the residual read back from planes
    (resp) gives the bits of the fp32 residual."""
    G, pix, C = shape
    P = G * pix
    c = apply_case(family, shape)
    d = {k: _dev(eng, v) for k, v in c.items()}
    d["resp"] = _planes_buf(eng, P, C)
    eng.debug_ew("split_planes", [d["res"], d["resp"]], [P, C])
    for name, (extra, relu) in APPLY_COMBOS.items():
        res = c["res"] if ("res" in extra or "resp" in extra) else None
        y2 = "y2" in extra
        want, mag, _ = R.bn_apply(c["y"], c["scale"], c["shift"], res, c["y2"] if y2 else None, c["scale2"] if y2 else None,
                                  c["shift2"] if y2 else None, relu)
        t = 2 + (1 if res is not None else 0) + (3 if y2 else 0)
        ops = [d["y"], d["scale"], d["shift"], d["res"] if "res" in extra else None] + \
              ([d["y2"], d["scale2"], d["shift2"]] if y2 else [None, None, None])
        dims = [G, pix, C, relu]
        out_p, pl = _nan(eng, G, pix, C), _planes_buf(eng, P, C)
        eng.debug_ew("bn_apply_planes", ops + [out_p, pl, d["resp"] if "resp" in extra else None], dims)
        _check(family, f"bn_apply_planes[{name}]", out_p, want, t * U * mag)
        _check_planes(f"bn_apply_planes[{name}]", pl, out_p.cpu().numpy(), P, C)
        only = _planes_buf(eng, P, C)
        eng.debug_ew("bn_apply_planes", ops + [None, only, d["resp"] if "resp" in extra else None], dims)
        _same(f"bn_apply_planes[{name}] planes only", only, pl)
        if "resp" in extra:
            with_res = _nan(eng, G, pix, C)
            eng.debug_ew("bn_apply_planes", [d["y"], d["scale"], d["shift"], d["res"], None, None, None, with_res,
                                             _planes_buf(eng, P, C), None], dims)
            _same("bn_apply_planes: resp against res", out_p, with_res)
        else:
            out_f = _nan(eng, G, pix, C)
            eng.debug_ew("bn_apply", ops + [out_f], dims)
            _check(family, f"bn_apply[{name}]", out_f, want, t * U * mag)
            if family == "dyadic":
                _same(f"bn_apply against bn_apply_planes [{name}]", out_f, out_p)


# ---- BatchNorm finalize -----------------------------------------------------------------------------------------------------
def _finalize(eng, stats, G, tiles, C, count, gamma, beta, rm, rv, eps, mom, skip=None):
    """-> dict of host arrays; stats gets the fold area behind it; run_mean / run_var are copies"""
    ws = torch.zeros(G * tiles * 2 * C + G * 32 * 2 * C, device=eng.device)
    ws[:G * tiles * 2 * C] = _dev(eng, stats).reshape(-1)
    o = {k: _nan(eng, G, C) for k in ("mean", "istd", "scale", "shift")}
    rmd, rvd = _dev(eng, rm), _dev(eng, rv)
    sk = None if skip is None else torch.tensor([skip], dtype=torch.int32, device=eng.device)
    eng.debug_ew("bn_finalize", [ws, _dev(eng, gamma), _dev(eng, beta), rmd, rvd, o["mean"], o["istd"], o["scale"], o["shift"], sk],
                 [G, tiles, C, count], [eps, mom])
    o = {k: v.cpu().numpy() for k, v in o.items()}
    if rm is not None:
        o["run_mean"], o["run_var"] = rmd.cpu().numpy(), rvd.cpu().numpy()
    return o


FIN_SHAPES = [(C, tiles, G) for C in (24, 64, 96) for tiles in (1, 3, 64, 65, 100) for G in (1, 2)]


def test_bn_finalize_dyadic(eng):
    """mean in {0, +-1/2, 1, -3/2}, var + eps in {1/4, 1, 4} with eps = 2^-10, count = 2 (so the unbiased variance 2 var is exact
    too), momentum 1/8, the sums dealt to the tiles in multiples of 1/16: every quantity the kernel forms is exact -- all outputs
    and both running statistics, moved once per group in group order, bit for bit.  Channel 1 has s2 / n < mean^2 (the clamp:
    istd = 1 / sqrt(eps) = 32); then count = 1, *skip = 1 and run_mean = NULL."""
    eps, mom, n = 2.0 ** -10, 0.125, 2
    rs = np.random.RandomState(31)
    for C, tiles, G in FIN_SHAPES:
        mu = rs.choice(_f32([0, 0.5, -0.5, 1, -1.5]), (G, C)).astype(np.float64)
        var = rs.choice([0.25, 1.0, 4.0], (G, C)) - eps
        tot = np.stack([n * mu, n * (var + mu * mu)], 1)                 # [G][2][C]
        tot[:, 1, 1] = n * mu[:, 1] ** 2 - 0.125                         # the clamp channel
        stats = rs.randint(-64, 65, (G, tiles, 2, C)) / 16.0
        stats[:, 0] += tot - stats.sum(1)
        stats = _f32(stats)
        assert np.array_equal(stats.astype(np.float64).sum(1), tot)
        gamma, beta = _coef("dyadic", rs, C), _coef("dyadic", rs, C)
        rm, rv = _f32(rs.randint(-8, 9, C) / 8.0), _f32(rs.randint(1, 17, C) / 8.0)
        want = R.bn_finalize(stats, n, gamma, beta, eps, mom, rm, rv)
        assert want["istd"][0, 1] == 32.0
        got = _finalize(eng, stats, G, tiles, C, n, gamma, beta, rm, rv, eps, mom)
        for k in ("mean", "istd", "scale", "shift", "run_mean", "run_var"):
            _bits(f"bn_finalize C{C} tiles{tiles} G{G} {k}", got[k], want[k])
    # count = 1: variance 0 and no unbiased factor; skip = 1 / run_mean NULL: outputs written, running statistics untouched
    one = _f32(rs.randint(-16, 17, (G, 1, 2, C)) / 8.0)
    one[:, :, 1] = one[:, :, 0] ** 2
    want = R.bn_finalize(one, 1, gamma, beta, eps, mom, rm, rv)
    got = _finalize(eng, one, G, 1, C, 1, gamma, beta, rm, rv, eps, mom, skip=0)
    for k in ("mean", "istd", "scale", "shift", "run_mean", "run_var"):
        _bits(f"bn_finalize count 1 {k}", got[k], want[k])
    want = R.bn_finalize(stats, n, gamma, beta, eps, mom, rm, rv, skip=True)
    for label, kw in (("skip", dict(rm=rm, rv=rv, skip=1)), ("no running statistics", dict(rm=None, rv=None))):
        got = _finalize(eng, stats, G, tiles, C, n, gamma, beta, eps=eps, mom=mom, **kw)
        for k in ("mean", "istd", "scale", "shift"):
            _bits(f"bn_finalize {label} {k}", got[k], want[k])
        if kw["rm"] is not None:
            _same("run_mean under skip", got["run_mean"], rm)
            _same("run_var under skip", got["run_var"], rv)


def finalize_bounds(stats, count, want, gamma, beta, rm, rv, mom, folded):
    """fp32 error bounds of k_bn_finalize's outputs from its own roundings (the sums themselves are taken in double: 2^-53 terms
    are covered by the 1e-12 slack).  f = 1 when the tile partials are first folded to fp32 chunk sums (tiles > 64), else 0.
    mean: f + 1 roundings of sum|s1| / n.   var: f roundings of sum|s2| / n and of 2 |mean| sum|s1| / n.
    istd = (var + eps)^-1/2: |d istd| = istd / (2 (var + eps)) |d var|, + 1 rounding.   scale = gamma istd: + 1.
    shift = beta - mean scale: 2 operations on (|beta| + |mean scale|), + the operands' errors.
    running statistics, per group: (1 - momentum), two products, one sum = 4 operations on the terms' magnitudes (5 for the
    variance, whose unbiased value is rounded to fp32 first), errors carried from group to group with factor (1 - momentum) < 1."""
    st = np.abs(stats.astype(np.float64)).sum(1)
    a1, a2 = st[:, 0] / count, st[:, 1] / count
    mean, istd, scale = want["mean"], want["istd"], want["scale"]
    slack = 1e-12
    b = {"mean": (folded + 1) * U * a1 + slack * a1}
    dvar = folded * U * (a2 + 2 * np.abs(mean) * a1) + slack * (a2 + mean * mean)
    veps = 1.0 / (istd * istd)
    b["istd"] = istd / (2 * veps) * dvar + U * istd
    b["scale"] = np.abs(gamma)[None] * b["istd"] + U * np.abs(scale)
    b["shift"] = 2 * U * (np.abs(beta)[None] + np.abs(mean * scale)) + np.abs(scale) * b["mean"] + np.abs(mean) * b["scale"]
    if rm is not None:
        unb = want["var"] * (count / (count - 1.0) if count > 1 else 1.0)
        b["run_mean"] = (4 * U * (np.abs(rm)[None] + np.abs(mean)) + mom * b["mean"]).sum(0)
        b["run_var"] = (5 * U * (np.abs(rv)[None] + unb) + mom * dvar * unb / np.maximum(want["var"], 1e-30)).sum(0)
    return b


def test_bn_finalize_random(eng):
    """statistics of N(0.3, 1.7^2) activations, fp32 tile partials, count = the pixels per group, eps 1e-5, momentum 0.1;
    bounds: finalize_bounds.  Measured: worst err / bound 0.97 (mean and istd, a single rounding each), 0.48 (shift), 0.46 / 0.15
    (running mean / variance)."""
    eps, mom = float(np.float32(1e-5)), float(np.float32(0.1))
    rs = np.random.RandomState(32)
    worst = {}
    for C, tiles, G in FIN_SHAPES:
        pix = max(2 * tiles, 37)
        x = rs.standard_normal((G, pix, C)) * 1.7 + 0.3
        stats = _f32(R.tile_stats(x, tiles))
        gamma, beta = _f32(rs.standard_normal(C)), _f32(rs.standard_normal(C))
        rm, rv = _f32(rs.standard_normal(C)), _f32(rs.uniform(0.5, 2.0, C))
        want = R.bn_finalize(stats, pix, gamma, beta, eps, mom, rm, rv)
        got = _finalize(eng, stats, G, tiles, C, pix, gamma, beta, rm, rv, eps, mom)
        bound = finalize_bounds(stats, pix, want, gamma, beta, rm, rv, mom, 1 if tiles > 64 else 0)
        for k, bk in bound.items():
            err = np.abs(got[k].astype(np.float64) - want[k])
            assert (err <= bk).all(), f"bn_finalize C{C} tiles{tiles} G{G} {k}: worst err/bound {(err / bk).max():.3f}"
            worst[k] = max(worst.get(k, 0.0), float((err / bk).max()))
    print("bn_finalize random, worst err/bound:", worst)
    REPORT["bn_finalize"] = {"worst_err_over_bound": worst}
    _dump()


@pytest.mark.parametrize("family", ["dyadic", "random"])
def test_bn_finalize_frozen_and_eval_affine(eng, family):
    """frozen: every group gets mean = run_mean, istd = (run_var + eps)^-1/2 (double, one rounding), scale = gamma istd (+ 1),
    shift = beta - mean scale (2 operations + the scale's error); reads and writes no running statistic.  eval affine: the same
    scale / shift formed in fp32: sqrtf(rv + eps) and the division are 3 roundings of the scale, then as above.  Dyadic:
    run_var + eps in {1/4, 1, 4} with eps = 2^-10.  Measured: worst err / bound 0.83 (frozen istd, one rounding), 0.54 (eval scale)."""
    rs = np.random.RandomState(33)
    for C, G in ((24, 1), (64, 2), (96, 2)):
        if family == "dyadic":
            eps = 2.0 ** -10
            gamma, beta, rm = _coef(family, rs, C), _coef(family, rs, C), _f32(rs.randint(-16, 17, C) / 8.0)
            rv = _f32(rs.choice([0.25, 1.0, 4.0], C) - eps)
        else:
            eps = float(np.float32(1e-5))
            gamma, beta, rm = (_f32(rs.standard_normal(C)) for _ in range(3))
            rv = _f32(rs.uniform(0.01, 3.0, C))
        want = R.bn_frozen(G, gamma, beta, rm, rv, eps)
        o = {k: _nan(eng, G, C) for k in ("mean", "istd", "scale", "shift")}
        rmd, rvd = _dev(eng, rm), _dev(eng, rv)
        for skip in (None, torch.tensor([1], dtype=torch.int32, device=eng.device)):
            eng.debug_ew("bn_finalize_frozen", [_dev(eng, gamma), _dev(eng, beta), rmd, rvd, o["mean"], o["istd"], o["scale"],
                                                o["shift"], skip], [G, C], [eps])
            bi = U * want["istd"] * 1.001
            bs = np.abs(gamma) * bi + U * np.abs(want["scale"])
            bound = {"mean": 0.0 * bi, "istd": bi, "scale": bs,
                     "shift": 2 * U * (np.abs(beta) + np.abs(want["mean"] * want["scale"])) + np.abs(want["mean"]) * bs}
            for k in o:
                _check(family, f"bn_finalize_frozen C{C} {k}", o[k], want[k], bound[k])
        _same("run_mean after the frozen finalize", rmd, rm)
        _same("run_var after the frozen finalize", rvd, rv)
        sc, sh = _nan(eng, C), _nan(eng, C)
        eng.debug_ew("bn_eval_affine", [_dev(eng, gamma), _dev(eng, beta), rmd, rvd, sc, sh], [C], [eps])
        bs = 3 * U * np.abs(want["scale"][0]) * 1.001
        _check(family, f"bn_eval_affine C{C} scale", sc, want["scale"][0], bs)
        _check(family, f"bn_eval_affine C{C} shift", sh, want["shift"][0],
               2 * U * (np.abs(beta) + np.abs(rm * want["scale"][0])) + np.abs(rm) * bs)


# ---- stem max-pool ----------------------------------------------------------------------------------------------------------
POOL_HW = [(8, 8), (8, 12)]
POOL_G, POOL_IPG, POOL_C = 2, 3, 64
STEM_GAMMA = _f32([0.0, 2.0 ** -6, 1.0 / 16, -0.5, 1.5])
STEM_BETA = _f32([-1.0, 0.0, 0.5])


def stem_case(family, hw, seed=41):
    """y [6][H][W][64]; channel c: gamma = STEM_GAMMA[c % 5] (0, the gather arm's 2^-6, the fast arm's first value 1/16, -1/2,
    3/2) -- in the random family from channel 10 on N(0, 1) --, beta = STEM_BETA[(c / 5) % 3]; mean, istd per group; scale =
    gamma istd and shift = beta - mean scale (fp32).  Dyadic: istd in {1/2, 1}, mean in {0, +-1/2, 1}; y takes few values in
    channels 0 .. 9 (ties everywhere) and is constant in image 0 of channel 7 (all-equal windows under a nonzero scale)."""
    H, W = hw
    G, ipg, C = POOL_G, POOL_IPG, POOL_C
    rs = np.random.RandomState(seed)
    y = _vals(family, rs, (G * ipg, H, W, C))
    gamma, beta = STEM_GAMMA[np.arange(C) % 5].copy(), STEM_BETA[(np.arange(C) // 5) % 3].copy()
    if family == "dyadic":
        y[..., :10] = rs.randint(-1, 2, y[..., :10].shape)
        y[0, :, :, 7] = 1.0
        mean, istd = _f32(rs.choice([0, 0.5, -0.5, 1], (G, C))), _f32(rs.choice([0.5, 1.0], (G, C)))
    else:
        gamma[10:], beta[10:] = _f32(rs.standard_normal(C - 10)), _f32(rs.standard_normal(C - 10))
        mean, istd = _f32(rs.standard_normal((G, C)) * 0.3), _f32(rs.uniform(0.5, 2.0, (G, C)))
    scale = _f32(gamma[None] * istd)
    shift = _f32(beta[None] - mean.astype(np.float64) * scale)
    dp = _vals(family, rs, (G * ipg, H // 2, W // 2, C))
    ca, cb, cc = (_coef(family, rs, (G, C)) for _ in range(3))
    return dict(y=y, gamma=gamma, beta=beta, mean=mean, istd=istd, scale=scale, shift=shift, dp=dp, ca=ca, cb=cb, cc=cc)


def pool_sure(pre, e, code):
    """where the max-pool's choice cannot depend on fp32 rounding: with every window value known to lie in relu([pre - e, pre + e]),
    each other inside position is either surely smaller than the winner, or surely EQUAL to it (both intervals are the same
    point: values clamped to 0 by the ReLU, or formed without rounding) and later in (kh, kw) order"""
    N, H, W, C = pre.shape
    lo, hi = (np.full((N, H + 2, W + 2, C), -np.inf) for _ in range(2))
    lo[:, 1:-1, 1:-1], hi[:, 1:-1, 1:-1] = np.maximum(pre - e, 0.0), np.maximum(pre + e, 0.0)
    win = lambda a, j: a[:, j // 3:j // 3 + H:2, j % 3:j % 3 + W:2]
    lo_w, hi_w = (np.select([code == j for j in range(9)], [win(a, j) for j in range(9)]) for a in (lo, hi))
    sure = np.ones(code.shape, bool)
    for j in range(9):
        lo_j, hi_j = win(lo, j), win(hi, j)
        sure &= (hi_j < lo_w) | (code == j) | ((lo_j == hi_j) & (lo_w == hi_w) & (lo_j == lo_w) & (j > code))
    return sure


def pool_reference(c, ipg=POOL_IPG):
    """pooled, code, the fp32 bound of a pooled value (2 rounded operations on |y scale| + |shift| -- none where scale = 0: the
    product and the sum are then exact --, the largest over the window) and which codes are compared (pool_sure)"""
    pooled, code, _, pre = R.stem_pool(c["y"], c["scale"], c["shift"], ipg)
    g = np.arange(c["y"].shape[0]) // ipg
    sc = R.f64(c["scale"])[g][:, None, None]
    e = 2 * U * np.where(sc == 0, 0.0, np.abs(R.f64(c["y"]) * sc) + np.abs(R.f64(c["shift"]))[g][:, None, None])
    return pooled, code, R.pool_choice(e)[0], pool_sure(pre, e, code)


@pytest.mark.parametrize("hw", POOL_HW, ids=str)
@pytest.mark.parametrize("family", ["dyadic", "random"])
def test_stem_pool(eng, family, hw):
    """pooled = maxpool3x3s2p1(relu(y scale + shift)) and the argmax code, fp32 kernel and planes kernel, 6 images in 2 groups.
    Dyadic: values and codes bit for bit, ties included (the first inside position wins: code 4 at the top-left corner of an
    all-equal map, 3 / 1 along the top row / left column, 0 inside).  Random: a pooled value is within 2 u (|y scale| + |shift|)
    of the reference (max is 1-Lipschitz); codes compared where no rounding can change the choice (pool_sure).  Measured: worst
    err / bound 0.49, nothing left out.  Also the plain max-pool (scale NULL) and the forms without idx / without pooled."""
    H, W = hw
    G, ipg, C = POOL_G, POOL_IPG, POOL_C
    N, Hp, Wp = G * ipg, H // 2, W // 2
    P = N * Hp * Wp
    c = stem_case(family, hw)
    pooled, code, bound, sure = pool_reference(c)
    if family == "dyadic":
        assert code[0, 0, 0, 7] == 4 and code[0, 0, 1, 7] == 3 and code[0, 1, 0, 7] == 1 and code[0, 1, 1, 7] == 0
        sure[:] = True
    assert (~sure).mean() <= 1e-3
    yd, scd, shd = _dev(eng, c["y"]), _dev(eng, c["scale"]), _dev(eng, c["shift"])
    dims = [G, ipg, H, W, C]
    idx = lambda: torch.full((N, Hp, Wp, C), 0xEE, dtype=torch.uint8, device=eng.device)
    po, io = _nan(eng, N, Hp, Wp, C), idx()
    eng.debug_ew("stem_pool", [yd, scd, shd, po, io], dims)
    pp, ip, pl = _nan(eng, N, Hp, Wp, C), idx(), _planes_buf(eng, P, C)
    eng.debug_ew("stem_pool_planes", [yd, scd, shd, pp, ip, pl], dims)
    for name, pv, iv in (("stem_pool", po, io), ("stem_pool_planes", pp, ip)):
        _check(family, f"{name} pooled", pv, pooled, bound)
        got = iv.cpu().numpy()
        assert np.array_equal(got[sure], code[sure]), f"{name}: {(got != code)[sure].sum()} argmax codes differ"
    _check_planes("stem_pool_planes", pl, pp.cpu().numpy(), P, C)
    if family == "dyadic":
        _same("stem_pool against stem_pool_planes", po, pp)
    # the forms that write only what they were asked to
    p2 = _nan(eng, N, Hp, Wp, C)
    eng.debug_ew("stem_pool", [yd, scd, shd, p2, None], dims)
    _same("stem_pool without idx", p2, po)
    p3, i3, pl3 = _nan(eng, N, Hp, Wp, C), idx(), _planes_buf(eng, P, C)
    eng.debug_ew("stem_pool_planes", [yd, scd, shd, p3, None, pl3], dims)
    _same("stem_pool_planes without idx: pooled", p3, pp)
    _same("stem_pool_planes without idx: planes", pl3, pl)
    pl4 = _planes_buf(eng, P, C)
    eng.debug_ew("stem_pool_planes", [yd, scd, shd, None, i3, pl4], dims)
    _same("stem_pool_planes without pooled: idx", i3, ip)
    _same("stem_pool_planes without pooled: planes", pl4, pl)
    # plain max-pool of the eval path: no arithmetic, so values and codes are exact in both families
    plain, pcode, _, _ = R.stem_pool(c["y"])
    for op, extra in (("stem_pool", []), ("stem_pool_planes", [_planes_buf(eng, P, C)])):
        pv, iv = _nan(eng, N, Hp, Wp, C), idx()
        eng.debug_ew(op, [yd, None, None, pv, iv] + extra, dims)
        _bits(f"{op} plain", pv, plain)
        assert np.array_equal(iv.cpu().numpy(), pcode), f"{op} plain: argmax codes"


# ---- stem: fused max-pool + BatchNorm backward ------------------------------------------------------------------------------
def _nblk(n):
    return max(1, min(1024, -(-n // 64)))


def block_of_pixel(n, C):
    """block that sums pixel p of a group of n in the two reduce kernels: tiles of 8 * (256 / (C / 4)) pixels dealt round-robin"""
    TP = 8 * (256 // (C // 4))
    return (np.arange(n) // TP) % _nblk(n)


def chain_length(n, C):
    """sequential fp32 additions behind one partial sum: a thread adds 8 pixels per tile of its block, then lane 0 adds the other
    256 / (C / 4) - 1 threads' sums"""
    P = 256 // (C // 4)
    TP = 8 * P
    tiles = -(-n // TP)
    return 8 * -(-tiles // _nblk(n)) + P - 1


def block_sums(terms, n, C):
    """terms [G][n][C] -> [G][nblk][C] summed per block"""
    blk = block_of_pixel(n, C)
    out = np.zeros((terms.shape[0], _nblk(n), C))
    for b in range(_nblk(n)):
        out[:, b] = terms[:, blk == b].sum(1)
    return out


def stem_bwd_reference(c, pooled32, code, ipg=POOL_IPG):
    """the float64 composite behind k_stem_pool_bn_reduce / _apply, from the pooled values and codes the kernels are fed: the
    per-pooled-position terms of s1 and s2 (xhat of y at the argmax), the magnitudes for the s2 bound, the dense dy"""
    y, dp = R.f64(c["y"]), R.f64(c["dp"])
    N, H, W, C = y.shape
    G = N // ipg
    g = np.arange(N) // ipg
    on = pooled32 > 0
    d = np.where(on, dp, 0.0)
    ya = R.gather_argmax(y, code)
    mu, istd = R.f64(c["mean"])[g][:, None, None], R.f64(c["istd"])[g][:, None, None]
    sc, be, ga = R.f64(c["scale"])[g][:, None, None], R.f64(c["beta"]), R.f64(c["gamma"])
    xh = (ya - mu) * istd
    fast = np.abs(ga) >= 0.0625
    # magnitude of the terms behind d * xhat: fast arm (pooled - beta) / gamma with pooled = y scale + (beta - mean scale), 7
    # roundings (scale, mean scale, shift, the pooled value, the difference, the division, the product with d); gather arm
    # (y - mean) istd d, 3 roundings
    with np.errstate(divide="ignore", invalid="ignore"):
        mfast = np.abs(d) * (np.abs(ya * sc) + np.abs(mu * sc) + np.abs(be)) / np.abs(ga)
    mag2 = np.where(fast, 7 * np.where(fast, mfast, 0.0), 3 * np.abs(d) * (np.abs(ya) + np.abs(mu)) * istd)
    dense = R.pool_route(dp, pooled32, code, H, W)
    dy, dymag = R.bn_bwd_apply(dense.reshape(G, -1, C), y.reshape(G, -1, C), c["ca"], c["cb"], c["cc"])
    sh = lambda a: a.reshape(G, -1, C)
    return sh(d), sh(d * xh), sh(np.abs(d)), sh(np.abs(d * xh)), sh(mag2), dy, dymag


@pytest.mark.parametrize("hw", POOL_HW, ids=str)
@pytest.mark.parametrize("family", ["dyadic", "random"])
def test_stem_pool_bn_backward(eng, family, hw):
    """k_stem_pool_bn_reduce / _apply fed the reference's pooled values (rounded to fp32) and codes.
    reduce: part[g][block] = (sum d, sum d xhat) over the block's pooled positions, d = dp where pooled > 0, xhat of y at the
    argmax -- by the gather for |gamma| < 1/16 (gamma 0 and 2^-6), from (pooled - beta) / gamma from exactly 1/16 on.  Chain:
    n = 8 ceil(tiles / blocks) + 256 / (C / 4) - 1 = 8 + 15 = 23 additions (C = 64, one tile per block): bound (n + 2) u sum|d| for
    s1, (n + 2) u sum|d xhat| + u sum(term magnitudes x their roundings, 7 fast / 3 gather; stem_bwd_reference) for s2.
    Measured: worst err / bound 0.04 (s1), 0.03 (s2).
    apply: dy = ca (sum of the window gradients that chose the position) + cb y + cc at every dense position, the last row and
    column included: at most 3 additions + 4 operations: 7 u sum|terms|.  Measured: worst err / bound 0.37.
    Dyadic: all of it bit for bit, and bit-identical to the unfused k_stem_pool_bwd -> k_bn_bwd_reduce / k_bn_bwd_apply."""
    H, W = hw
    G, ipg, C = POOL_G, POOL_IPG, POOL_C
    N, Hp, Wp = G * ipg, H // 2, W // 2
    npool, nb = ipg * Hp * Wp, _nblk(ipg * Hp * Wp)
    c = stem_case(family, hw)
    pooled, code, _, _ = pool_reference(c)
    pooled32 = _f32(pooled)
    t1, t2, a1, a2, mag2, dy_want, dymag = stem_bwd_reference(c, pooled32, code)
    d = {k: _dev(eng, v) for k, v in c.items()}
    pd, cd = _dev(eng, pooled32), _dev(eng, code)
    dims = [G, ipg, H, W, C]
    part = _nan(eng, G, nb, 2, C)
    eng.debug_ew("stem_pool_bn_reduce", [d["dp"], pd, cd, d["y"], d["mean"], d["istd"], part, d["gamma"], d["beta"]], dims)
    n = chain_length(npool, C)
    assert n == 23
    got = part.cpu().numpy()
    _check(family, "stem_pool_bn_reduce s1", got[:, :, 0], block_sums(t1, npool, C), (n + 2) * U * block_sums(a1, npool, C))
    _check(family, "stem_pool_bn_reduce s2", got[:, :, 1], block_sums(t2, npool, C),
           (n + 2) * U * block_sums(a2, npool, C) + U * block_sums(mag2, npool, C))
    dy = _nan(eng, N, H, W, C)
    eng.debug_ew("stem_pool_bn_apply", [d["dp"], pd, cd, d["y"], d["ca"], d["cb"], d["cc"], dy], dims)
    _check(family, "stem_pool_bn_apply dy", dy.reshape(G, -1, C), dy_want, 7 * U * dymag)
    # the unfused order on the same inputs
    dense = _nan(eng, N, H, W, C)
    eng.debug_ew("stem_pool_bwd", [d["dp"], pd, cd, dense], [N, H, W, C])
    _check(family, "stem_pool_bwd", dense, R.pool_route(c["dp"], pooled32, code, H, W),
           3 * U * R.pool_route(np.abs(c["dp"]), pooled32, code, H, W))
    if family == "dyadic":
        pix = ipg * H * W
        part2, dy2 = _nan(eng, G, _nblk(pix), 2, C), _nan(eng, N, H, W, C)
        eng.debug_ew("bn_bwd_reduce", [dense, None, d["y"], d["mean"], d["istd"], part2, None, None, None], [G, pix, C])
        eng.debug_ew("bn_bwd_apply", [dense, None, d["y"], d["ca"], d["cb"], d["cc"], dy2, None, None, None], [G, pix, C])
        _same("fused against unfused dy", dy, dy2)
        fin = []
        for pt, blocks in ((part, nb), (part2, _nblk(pix))):
            o = {k: _nan(eng, *s) for k, s in (("ca", (G, C)), ("cb", (G, C)), ("cc", (G, C)), ("dgamma", (C,)), ("dbeta", (C,)))}
            eng.debug_ew("bn_bwd_finalize", [pt, d["gamma"], d["mean"], d["istd"], o["ca"], o["cb"], o["cc"], o["dgamma"], o["dbeta"]],
                         [G, blocks, C, 64, 0])
            fin.append(o)
        for k in fin[0]:
            _same(f"fused against unfused {k}", fin[0][k], fin[1][k])
        _bits("stem dgamma", fin[0]["dgamma"], t2.sum((0, 1)))
        _bits("stem dbeta", fin[0]["dbeta"], t1.sum((0, 1)))


# ---- BatchNorm backward -----------------------------------------------------------------------------------------------------
BWD_SHAPES = [(2, 37, 64), (1, 200, 128), (1, 9, 512), (1, 64 * 65, 64)]


def bwd_case(family, shape, seed=51):
    """dz, y [G][pix][C]; the forward's scale / shift (the mask source msc / msh), mean, istd, gamma and the apply coefficients.
    Dyadic: istd in {1/2, 1} (3/2 in channel 1), mean in {0, +-1/2, 1}; channel 0 is the identity (scale 1, shift 0, mean 0, istd 1,
    cb 0) with positive dz and y >= 0 (so its sums cannot cancel down to the tiny term), and holds z = the smallest normal at pixel
    1 (dz = 1 there) and z = exactly 0 at pixel 0; scale 0 / shift 0 channels make more
    exact zeros."""
    G, pix, C = shape
    rs = np.random.RandomState(seed)
    c = dict(dz=_vals(family, rs, shape), y=_vals(family, rs, shape))
    for k in ("scale", "shift", "ca", "cb", "cc", "gamma"):
        c[k] = _coef(family, rs, (G, C) if k != "gamma" else C)
    if family == "dyadic":
        c["mean"], c["istd"] = _f32(rs.choice([0, 0.5, -0.5, 1], (G, C))), _f32(rs.choice([0.5, 1.0], (G, C)))
        c["istd"][:, 1] = 1.5
        for k, v in (("scale", 1), ("shift", 0), ("mean", 0), ("istd", 1), ("cb", 0)):
            c[k][:, 0] = v
        c["dz"][:, :, 0], c["y"][:, :, 0] = np.abs(c["dz"][:, :, 0]) + 0.125, np.abs(c["y"][:, :, 0])
        c["y"][:, 0, 0], c["y"][:, 1, 0], c["dz"][:, 1, 0] = 0.0, TINY, 1.0
    else:
        c["mean"], c["istd"] = _f32(rs.standard_normal((G, C)) * 0.3), _f32(rs.uniform(0.5, 2.0, (G, C)))
    return c


@pytest.mark.parametrize("shape", BWD_SHAPES, ids=str)
@pytest.mark.parametrize("family", ["dyadic", "random"])
def test_bn_backward(eng, family, shape):
    """k_bn_bwd_reduce -> k_bn_bwd_finalize (batch and frozen) -> k_bn_bwd_apply(_planes) with the three ReLU-mask sources, all of
    the same z = relu(fma(y, scale, shift)) (k_bn_apply's own output): fp32 z, the h plane of split(z), mask_scale / mask_shift.
    The three give bit-identical partials, dyh and dy in both families.
    reduce: s1 = sum dyh, s2 = sum dyh xhat per block; chain n = 8 ceil(tiles / blocks) + 256 / (C / 4) - 1 additions (23, 15, 9
    and 23 for the four shapes); bound (n + 2) u sum|dyh| and (n + 2 + 3) u sum|dyh xhat| (xhat = (y - mean) istd and the product:
    3 more roundings per term).  Measured: worst err / bound 0.14.
    finalize, from the kernel's own partials (summed in double; pix = 4160 folds 65 blocks through fp32 chunk sums: 1 rounding):
    dgamma / dbeta 1 + fold roundings; ca = gamma istd 1; cb = -ca istd (s2 / count): 3 + the sum's; cc = -cb mean - ca (s1 /
    count): 4 on |cb mean| + |ca s1 / count|, + |mean| x cb's error.  Two groups are summed into dgamma / dbeta.  Dyadic: count
    = 64 (s / count exact).  Measured: worst err / bound 0.95 (ca, a single rounding).
    apply: dy = ca dyh + cb y + cc: 4 operations; dyh_out is dz under the mask, exactly; the planes of dy are the exact split of
    the fp32 dy of the same launch, and a planes-only launch writes the same words.  Measured: worst err / bound 0.61."""
    G, pix, C = shape
    P = G * pix
    c = bwd_case(family, shape)
    d = {k: _dev(eng, v) for k, v in c.items()}
    z = _nan(eng, G, pix, C)
    eng.debug_ew("bn_apply", [d["y"], d["scale"], d["shift"], None, None, None, None, z], [G, pix, C, 1])
    zh = _planes_buf(eng, P, C)
    eng.debug_ew("split_planes", [z, zh], [P, C])
    z32 = z.cpu().numpy()
    zref, zmag, _ = R.bn_apply(c["y"], c["scale"], c["shift"])
    _check(family, "z", z, zref, 2 * U * zmag)
    if family == "dyadic":
        assert z32[0, 0, 0] == 0 and z32[0, 1, 0] == TINY and (z32 == 0).mean() > 0.3
    dyh = np.where(z32 > 0, c["dz"], np.float32(0)).astype(np.float64)
    xh = (R.f64(c["y"]) - R.f64(c["mean"])[:, None]) * R.f64(c["istd"])[:, None]
    s1, s2, a1, a2 = (block_sums(t, pix, C) for t in (dyh, dyh * xh, np.abs(dyh), np.abs(dyh * xh)))
    nb, n = _nblk(pix), chain_length(pix, C)
    assert n == {64: 23, 128: 15, 512: 9}[C]
    sources = {"z": [z, None, None, None], "zh": [None, None, None, zh], "msc": [None, d["scale"], d["shift"], None]}
    parts = {}
    for name, (zz, msc, msh, zp) in sources.items():
        parts[name] = torch.full((G * nb * 2 * C + G * 32 * 2 * C,), float("nan"), device=eng.device)
        eng.debug_ew("bn_bwd_reduce", [d["dz"], zz, d["y"], d["mean"], d["istd"], parts[name], msc, msh, zp], [G, pix, C])
    got = parts["z"][:G * nb * 2 * C].reshape(G, nb, 2, C).cpu().numpy()
    _check(family, f"bn_bwd_reduce {shape} s1", got[:, :, 0], s1, (n + 2) * U * a1)
    _check(family, f"bn_bwd_reduce {shape} s2", got[:, :, 1], s2, (n + 5) * U * a2)
    for name in ("zh", "msc"):
        _same(f"bn_bwd_reduce partials, mask from {name} against z", parts[name][:G * nb * 2 * C], parts["z"][:G * nb * 2 * C])
    # finalize on the kernel's own partials
    count = 64 if family == "dyadic" else pix
    p64 = got.astype(np.float64)
    f = 1 if nb > 64 else 0
    S1, S2, A1, A2 = p64[:, :, 0].sum(1), p64[:, :, 1].sum(1), np.abs(p64[:, :, 0]).sum(1), np.abs(p64[:, :, 1]).sum(1)
    for frozen in (0, 1):
        want = R.bn_bwd_coeffs(S1, S2, count, c["gamma"], c["mean"], c["istd"], bool(frozen))
        o = {k: _nan(eng, *s) for k, s in (("ca", (G, C)), ("cb", (G, C)), ("cc", (G, C)), ("dgamma", (C,)), ("dbeta", (C,)))}
        eng.debug_ew("bn_bwd_finalize", [parts["z"], d["gamma"], d["mean"], d["istd"], o["ca"], o["cb"], o["cc"], o["dgamma"],
                                         o["dbeta"]], [G, nb, C, count, frozen])
        slack = 1 + 1e-6
        mu, istd, ca = np.abs(R.f64(c["mean"])), R.f64(c["istd"]), np.abs(want["ca"])
        bcb = (3 * U * np.abs(want["cb"]) + (f + 1) * U * ca * istd * A2 / count) * slack
        bound = {"ca": U * ca, "cb": bcb * (1 - frozen), "dgamma": (f + 1) * U * A2.sum(0) * slack, "dbeta": (f + 1) * U * A1.sum(0) * slack,
                 "cc": (1 - frozen) * (4 * U * (np.abs(want["cb"]) * mu + ca * np.abs(S1) / count) + mu * bcb
                                       + (f + 1) * U * ca * A1 / count) * slack}
        for k in o:
            _check(family, f"bn_bwd_finalize {shape} frozen={frozen} {k}", o[k], want[k], bound[k])
        if frozen:
            assert not o["cb"].any() and not o["cc"].any()
    # apply
    want, mag = R.bn_bwd_apply(dyh, c["y"], c["ca"], c["cb"], c["cc"])
    co = [d["ca"], d["cb"], d["cc"]]
    outs = {}
    for name, (zz, msc, msh, zp) in sources.items():
        dy, dyh_o, pl = _nan(eng, G, pix, C), _nan(eng, G, pix, C), _planes_buf(eng, P, C)
        eng.debug_ew("bn_bwd_apply_planes", [d["dz"], zz, d["y"]] + co + [dy, dyh_o, msc, msh, pl, zp], [G, pix, C])
        outs[name] = (dy, dyh_o, pl)
        if name != "zh":
            dy_f, dyh_f = _nan(eng, G, pix, C), _nan(eng, G, pix, C)
            eng.debug_ew("bn_bwd_apply", [d["dz"], zz, d["y"]] + co + [dy_f, dyh_f, msc, msh], [G, pix, C])
            _check(family, f"bn_bwd_apply {shape} [{name}]", dy_f, want, 4 * U * mag)
            _same(f"bn_bwd_apply dyh_out [{name}]", dyh_f.cpu().numpy(), dyh.astype(np.float32))
            if family == "dyadic":
                _same(f"bn_bwd_apply against bn_bwd_apply_planes [{name}]", dy_f, dy)
    dy, dyh_o, pl = outs["z"]
    _check(family, f"bn_bwd_apply_planes {shape}", dy, want, 4 * U * mag)
    _same("bn_bwd_apply_planes dyh_out", dyh_o.cpu().numpy(), dyh.astype(np.float32))
    _check_planes("bn_bwd_apply_planes", pl, dy.cpu().numpy(), P, C)
    for name in ("zh", "msc"):
        for what, a, b in zip(("dy", "dyh_out", "planes"), outs[name], outs["z"]):
            _same(f"bn_bwd_apply_planes {what}, mask from {name} against z", a, b)
    only = _planes_buf(eng, P, C)
    eng.debug_ew("bn_bwd_apply_planes", [d["dz"], z, d["y"]] + co + [None, None, None, None, only, None], [G, pix, C])
    _same("bn_bwd_apply_planes planes only", only, pl)


# ---- contract ---------------------------------------------------------------------------------------------------------------
def test_arguments_outside_a_kernels_contract_are_refused(eng):
    from fedmlp_amd._lib import FmError
    x = torch.zeros(4096, device=eng.device)
    b = torch.zeros(4096, dtype=torch.uint8, device=eng.device)
    for op, ptrs, dims in (("split_planes", [x, x], [4, 48]),                              # C % 32
                           ("bn_apply_planes", [x, x, x, None, None, None, None, x, x, None], [1, 4, 48, 1]),
                           ("bn_apply", [x, x, x, None, None, None, None, x], [1, 4, 6, 1]),          # C % 4
                           ("bn_apply", [x, x, x, None, None, None, None, None], [1, 4, 8, 1]),       # out missing
                           ("bn_bwd_apply_planes", [x, x, x, x, x, x, x, None, None, None, x, None], [1, 4, 16]),
                           ("stem_pool", [x, x, x, x, b], [1, 1, 7, 8, 8]),                           # odd H
                           ("stem_pool_planes", [x, x, x, x, b, x], [1, 1, 8, 5, 32]),                # odd W
                           ("stem_pool_bn_apply", [x, x, b, x, x, x, x, x], [1, 1, 8, 7, 8]),
                           ("bn_bwd_reduce", [x, x, x, x, x, x, None, None, None], [1, 4, 24])):      # C not a power of two
        with pytest.raises(FmError, match="bad argument"):
            eng.debug_ew(op, ptrs, dims)


# ---- the share of discrete decisions the random family leaves out (also run on the CPU: tests/test_bn_ref_cpu.py) -----------
def left_out_shares():
    out = {}
    for hw in POOL_HW:
        out[f"stem_pool {hw}"] = float((~pool_reference(stem_case("random", hw))[3]).mean())
    return out
