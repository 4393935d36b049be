"""Kernel-level parity of the EfficientNet-B0 depthwise-convolution and squeeze-excite kernels (csrc/effnet.hip), each launcher on its
own through fm_debug_eff, against the float64 restatement in tests/eff_ref.py (pinned to torch autograd by
tests/test_eff_ref_cpu.py).  Workspace sizes come from fm_debug_eff_ws; nothing here guesses them.

Two input families.
DYADIC: activations are multiples of 1/2 in [-2, 2], depthwise weights from {0, +-1/2, +-1, +-2}, per-channel operands from
{0, +-1/4, +-1/2, +-1}: every product and every partial sum in any order is exact in fp32 (`_exact` asserts sum|terms| < 2^24 units
on the data actually used) and all operands are bf16 numbers.  Outputs, stored bf16 words (the reference rounds to nearest even),
fused (sum, sumsq) partials after summing the tiles, pooling sums and weight gradients must equal the reference BIT FOR BIT.  Ops
with a sigmoid enter with their linear parts: act = 0, pooling sums, and scale = shift = 0 / rpre = 0, where swish(0) = 0 and
swish'(0) = 1/2 exactly (exp2(0) = 1 and rcp(2) = 1/2 are exact on the hardware units too).
RANDOM: standard-normal operands (bf16 storage: rounded to bf16 first).  u = 2^-24.  A KxK depthwise value is within
(K K + 1) u sum|x w| of the float64 one, an n-term sum within (n + c) u sum|terms| (c = the roundings per term, stated per test),
plus sum of the terms' own errors; a bf16 store adds half a bf16 ulp of the result.  Where sigmoid enters: hardware exp and rcp are
1 ulp = 2 u relative each (head of effnet.hip), exp's argument -v log2(e) carries 2 u |v|, so with s = sigmoid(v)
|ds| <= s ((1 - s)(2 + 2|v|) + 3) u  (`_sig_err`), propagated through v s (`_swish_err`) and s (1 + v (1 - s)) (`_swish_grad_err`) term
by term as ABSOLUTE errors (swish' crosses zero near v = -1.28).  Fused statistics are sums of the values the kernel STORED, so in
this family their reference is the float64 sum over the stored output of the same launch (itself held to its own bound); later
stages of the squeeze-excite backward are likewise held against the float64 function of the stage's stored inputs.
Worst error / bound ratios go to eff_parity.json beside the other parity reports.

Canaries: every output and workspace sits between sentinel margins (NaN, bf16 word 0x7FC1) and is pre-filled with the sentinel;
`_canaries` asserts the margins afterwards, an unwritten element is a NaN and fails the comparison, and a workspace whose size
fm_debug_eff_ws reports as 0 (request declined) must stay untouched."""
import numpy as np
import pytest
import torch

from fedmlp_amd import spec
from tests import eff_ref as R
from tests.test_local_training_gpu import _dump as _dump_report

pytestmark = pytest.mark.gpu

U = R.U
M = 64                      # margin elements on either side of every buffer
WORD = 0x7FC1               # bf16 NaN pattern no kernel produces
REPORT = {}
F32, BF16 = 0, 1
DYW = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
DYC = np.array([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0])


@pytest.fixture(scope="module")
def eng():
    """one small EfficientNet-B0 handle: the owner of the stream the launchers run on, nothing else"""
    from fedmlp_amd.engine import Engine
    e = Engine("Efficient_b0", 5, 64, 64, 8)
    flat, cnt = spec.init_state("Efficient_b0", 5, 3)
    e.set_state(flat, cnt)
    yield e
    e.close()


# ---- buffers with canaries ---------------------------------------------------------------------------------------------------------
class Buf:
    """n elements (fp32, or bf16 words) between two sentinel margins; `t` is what a kernel gets"""

    def __init__(self, e, n, bf=False, init=None, pool=None):
        self.n, self.bf, self.declined = max(int(n), 16), bf, int(n) == 0
        if bf:
            self.full = torch.full((self.n + 2 * M,), WORD, dtype=torch.int16, device=e.device)
        else:
            self.full = torch.full((self.n + 2 * M,), float("nan"), device=e.device)
        self.t = self.full[M:M + self.n]
        if init is not None:
            a = np.ascontiguousarray(np.asarray(init, np.float32)).reshape(-1)
            assert a.size == max(int(n), 1), (a.size, n)
            src = torch.from_numpy(R.bf16_words(a).view(np.int16).copy()) if bf else torch.from_numpy(a)
            self.t[:a.size].copy_(src.to(e.device))
        if pool is not None:
            pool.append(self)

    def raw(self):
        a = self.full.cpu().numpy()
        return a.view(np.uint16) if self.bf else a.view(np.uint32)

    def np(self, shape=None):
        a = self.t.cpu().numpy()
        a = R.bf16_decode(a) if self.bf else a
        return a if shape is None else a[:int(np.prod(shape))].reshape(shape)

    def check(self, name):
        w, s = self.raw(), (WORD if self.bf else 0x7FC00000)
        assert (w[:M] == s).all() and (w[M + self.n:] == s).all(), f"{name}: a margin was written"
        if self.declined:
            assert (w == s).all(), f"{name}: a declined request wrote to its workspace"


def _canaries(pool, name):
    for i, b in enumerate(pool):
        b.check(f"{name}[buffer {i}]")


def _parity(report, path):
    """(_bits, _within, _check) recording into `report`, which is written to `path` beside the other parity reports after every
    check (tests/test_head_kernels_gpu.py keeps a report of its own through the same three)"""

    def _rec(key, err, bound):
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        r = report.setdefault(key, {})
        r["max_abs_err"] = max(r.get("max_abs_err", 0.0), float(err.max()))
        r["worst_err_over_bound"] = max(r.get("worst_err_over_bound", 0.0), ratio)
        _dump_report(report, path)
        return ratio

    def _bits(name, got, want64):
        got64, want64 = np.asarray(got).astype(np.float64), np.asarray(want64, np.float64)
        got, want = got64.astype(np.float32), want64.astype(np.float32)
        assert np.array_equal(got.astype(np.float64), got64, equal_nan=True)
        assert np.array_equal(want.astype(np.float64), want64), f"{name}: the dyadic case is not exact in fp32"
        assert got.shape == want.shape, (name, got.shape, want.shape)
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~((got == 0) & (want == 0))
        assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} differ, first at {np.argwhere(bad)[0]}: " \
                              f"{got[bad][0]!r} vs {want[bad][0]!r}"
        r = report.setdefault(name.split(" ")[0] + "/dyadic", {})
        r["bit_exact_checks"] = r.get("bit_exact_checks", 0) + 1
        _dump_report(report, path)

    def _within(name, got, want64, bound, family="random"):
        got = np.asarray(got).astype(np.float64)
        want64 = np.asarray(want64, np.float64)
        bound = np.broadcast_to(np.asarray(bound, np.float64), want64.shape)
        assert got.shape == want64.shape, (name, got.shape, want64.shape)
        assert not np.isnan(got).any(), f"{name}: NaN (an element was not written)"
        err = np.abs(got - want64)
        ratio = _rec(name.split(" ")[0] + "/" + family, err, bound)
        print(f"{name}: max|err| {err.max():.3e}, worst err/bound {ratio:.3f}")
        assert not (err > bound).any(), f"{name}: {(err > bound).sum()} of {err.size} beyond the bound, worst err/bound {ratio:.3f}"

    def _check(family, name, got, want64, bound, bf=False):
        """bf: `got` was stored as bf16 -- the dyadic reference is rounded to nearest even, the random bound gains half a bf16 ulp"""
        if family == "dyadic":
            _bits(name, got, R.store(want64, bf))
        else:
            _within(name, got, want64, bound + (R.half_ulp_bf16(np.abs(want64) + bound) if bf else 0.0))

    return _bits, _within, _check


_bits, _within, _check = _parity(REPORT, "eff_parity.json")


def _exact(terms, unit):
    """every partial sum of `terms` in any order is an fp32 number: sum|terms| < 2^24 units"""
    t = np.abs(np.asarray(terms, np.float64))
    assert np.array_equal(np.round(t / unit), t / unit) and t.sum(0).max() / unit < 2 ** 24, "dyadic case too large to be exact"


def _sig_err(v):
    s = R.sigmoid(v)
    return s * ((1.0 - s) * (2.0 + 2.0 * np.abs(v)) + 3.0) * U


def _swish_err(v, dv=0.0):
    return np.abs(v) * _sig_err(v) + U * np.abs(R.swish(v)) + 1.1 * dv


def _swish_grad_err(v, dv=0.0):
    s, ds = R.sigmoid(v), _sig_err(v)
    t = 1.0 - s
    p = v * t
    ep = np.abs(v) * (ds + U * t) + U * np.abs(p)
    q = 1.0 + p
    return np.abs(q) * ds + s * (ep + U * np.abs(q)) + U * np.abs(s * q) + 0.6 * dv


def _affine_err(y, sc, sh):
    """rounding of v = y sc + sh (two operations, or one fused)"""
    return 2.0 * U * (np.abs(y * sc) + np.abs(sh))


def _vals(family, rs, shape, bf):
    if family == "dyadic":
        return rs.randint(-4, 5, shape) / 2.0
    x = rs.standard_normal(shape)
    return R.bf16_round(x) if bf else x.astype(np.float32).astype(np.float64)


def _wts(family, rs, shape):
    if family == "dyadic":
        w = rs.choice(DYW, shape)
        w[0], w[-1] = 2.0, -1.0                  # no symmetry under the 180-degree rotation
        return w
    return rs.standard_normal(shape).astype(np.float32).astype(np.float64)


def _coef(family, rs, shape, pos=False):
    if family == "dyadic":
        c = rs.choice(DYC, shape)
        return np.abs(c) + 0.25 if pos else c
    c = rs.standard_normal(shape).astype(np.float32).astype(np.float64)
    return np.abs(c) + 0.1 if pos else c


# ---- launch arithmetic restated (effnet.hip), to say which arm a shape hits ------------------------------------------------------------
def _rowu(K, s, Hi, Wi, pad_t, pad_l, generic=False):
    """the row-uniform kernels take TF-"same" padding of any size at stride 1 and of even sizes at stride 2 (dw_blk_ok + the size
    test of dw_fwd_t / dw_dgrad_t)"""
    pt = (K - 1) // 2 if s == 1 else (K - 2) // 2
    return (not generic) and pad_t == pt and pad_l == pt and (s == 1 or (Hi % 2 == 0 and Wi % 2 == 0))


def _stats_rowgroups(steps, nchunk, groups):
    target = max(1, 3072 // (nchunk * groups))
    for d in range(min(target, steps), 0, -1):
        if steps % d == 0:
            return d if (4 * d >= target or d == steps) else 0
    return 0


def _stats_served(dgrad, K, s, N, Hi, Wi, C, pad_t, pad_l, groups, generic=False):
    if not _rowu(K, s, Hi, Wi, pad_t, pad_l, generic):
        return False
    spi = (Hi + 1) // 2 if s == 1 else (Hi if dgrad else Hi // 2)
    W = Wi if (s == 1 or dgrad) else Wi // 2
    nchunk = (((W + 3) // 4) * (C // 4) + 63) // 64
    return (N * spi) % groups == 0 and _stats_rowgroups(N * spi // groups, nchunk, groups) > 0


def _dims(dt, N, Hi, Wi, C, K, s, act=0, groups=1, pads=None):
    pt, pl = pads if pads is not None else (R.same_pad(Hi, K, s), R.same_pad(Wi, K, s))
    return [dt, N, Hi, Wi, R.out_size(Hi, s), R.out_size(Wi, s), C, K, s, pt, pl, act, groups]


# Shapes (N, H, W, C), the smallest that reach each arm of the launch code:
#  (2, 7, 7, 16)    W % 4 = 3, odd H (the lower row of the last pair is missing); WB Q = 8 < 64: one ragged chunk.  Stride 2: 7 -> 4,
#                   pad_t = (K-1)/2 differs from the even case: generic kernels.  98 output pixels: dw_wgrad_blocks = 1
#  (2, 5, 10, 100)  W % 4 = 2, odd H; WB Q = 75: two chunks, the second ragged; C % 8 != 0 (bf16 pieces are 8 bytes here).  Stride 2:
#                   odd H: generic
#  (1, 1, 3, 8)     H = 1, W < 4
#  (2, 6, 9, 8)     W % 4 = 1.  Stride 2: odd W: generic
#  (3, 8, 12, 24)   even: the row-uniform stride-2 kernels (Wo = 6: a partial column block; dgrad: WB = 3)
#  (9, 16, 12, 16)  72 row steps at stride 1.  Without a request: 5 row groups -> the XCD order pads the grid to 8 groups of 4 (27
#                   early-returning blocks); with the statistics request (rpb = 1): 72 row groups = 18 XCD groups, padded to 24: three
#                   batches, 24 padding blocks.  1728 output pixels: 13 weight-gradient blocks of 133, the last one ragged (132)
DW_SHAPES = [(2, 7, 7, 16), (2, 5, 10, 100), (1, 1, 3, 8), (2, 6, 9, 8), (3, 8, 12, 24), (9, 16, 12, 16)]
KS = [(3, 1), (3, 2), (5, 1), (5, 2)]


def _dw_fwd_case(eng, family, dt, K, s, shape, seed, act=0, affine=False, request=None, groups=1, generic=False, pads=None):
    """one k_dw_fwd launch checked against the reference; request None / "stats" / "pool"; returns the served flag"""
    N, H, W, C = shape
    bf = dt == BF16
    rs = np.random.RandomState(seed)
    x, w = _vals(family, rs, shape, bf), _wts(family, rs, (K * K, C))
    d = _dims(dt, N, H, W, C, K, s, act, groups, pads)
    Ho, Wo, pt, pl = d[4], d[5], d[9], d[10]
    name = f"dw_fwd K{K}s{s}{'bf16' if bf else 'f32'}{shape}{request or ''}{'g' if generic else ''}"
    pool = []
    xb, wb = Buf(eng, x.size, bf, x, pool), Buf(eng, w.size, False, w, pool)
    yb = Buf(eng, N * Ho * Wo * C, bf, pool=pool)
    sc = sh = None
    if affine:
        sc, sh = _coef(family, rs, (C,)), _coef(family, rs, (C,))
    scb = Buf(eng, C, False, sc, pool) if affine else None
    shb = Buf(eng, C, False, sh, pool) if affine else None
    ws = eng.debug_eff_ws("dw_fwd", d)
    recb = stb = plb = None
    if request == "stats":
        recb, stb = Buf(eng, ws[0], pool=pool), Buf(eng, ws[1], pool=pool)
        assert ws[1] == groups * 8 * 2 * C
    elif request == "pool":
        recb, plb = Buf(eng, ws[2], pool=pool), Buf(eng, ws[3], pool=pool)
    served = eng.debug_eff("dw_fwd", [xb.t, wb.t, yb.t, scb and scb.t, shb and shb.t, recb and recb.t, stb and stb.t, plb and plb.t], d)
    _canaries(pool, name)
    conv = R.dw_fwd(x, w, K, s, pt, pl)
    bound = (K * K + 1) * U * R.dw_fwd(np.abs(x), np.abs(w), K, s, pt, pl)
    want = conv
    if affine:
        v = conv * sc + sh
        dv = bound * np.abs(sc) + _affine_err(conv, sc, sh)
        want = R.act(v, act)
        bound = _swish_err(v, dv) if act == 2 else dv
    if family == "dyadic":
        _exact(np.abs(x).max() * np.abs(w), 1 / 8)
    got = yb.np((N, Ho, Wo, C))
    _check(family, name + " y", got, want, bound, bf)
    stored = R.store(want, bf) if family == "dyadic" else got.astype(np.float64)
    if request == "stats":
        assert served == (ws[0] > 0), (name, served, ws)
        if served:
            assert N % groups == 0
            st = stb.np((groups, 8, 2, C)).astype(np.float64).sum(1)
            ref = R.bn_stats(stored, groups)
            n = N * Ho * Wo // groups
            g = R.group_rows(np.abs(stored), groups)
            if family == "dyadic":
                _exact(g[0] ** 2, 1 / 64)
            _check(family, name + " sum", st[:, 0], ref[:, 0], n * U * g.sum(1))
            _check(family, name + " sumsq", st[:, 1], ref[:, 1], (n + 1) * U * (g * g).sum(1))
        else:
            assert np.isnan(stb.np()).all(), f"{name}: a declined request wrote stats_out"
    if request == "pool":
        assert served == (ws[2] > 0), (name, served, ws)
        if served:
            ref = R.pool_sums(stored)
            _check(family, name + " pool", plb.np((N, C)), ref, Ho * Wo * U * R.pool_sums(np.abs(stored)))
        else:
            assert np.isnan(plb.np()).all()
    return served


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("ks", KS, ids=lambda p: f"K{p[0]}s{p[1]}")
def test_dw_fwd(eng, ks, dt, family):
    """y = conv(x, w) at every shape of DW_SHAPES, plain and with the train-mode statistics request (groups = 1).  Random bound:
    (K K + 1) u sum|x w| (+ half a bf16 ulp); statistics over n stored values: n u sum|y| and (n + 1) u sum y^2.  The served flag must
    be what the launch arithmetic gives, and a served request must come with a non-zero record size from fm_debug_eff_ws.
    Worst ratios: eff_parity.json (dw_fwd/random)."""
    K, s = ks
    for i, shape in enumerate(DW_SHAPES):
        N, H, W, C = shape
        assert not _dw_fwd_case(eng, family, dt, K, s, shape, 100 + i)
        served = _dw_fwd_case(eng, family, dt, K, s, shape, 100 + i, request="stats")
        assert served == _stats_served(False, K, s, N, H, W, C, R.same_pad(H, K, s), R.same_pad(W, K, s), 1), (shape, served)
        assert served == _rowu(K, s, H, W, R.same_pad(H, K, s), R.same_pad(W, K, s))       # groups = 1: every row-uniform launch serves


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_dw_fwd_generic_forced(eng, monkeypatch, dt, family):
    """FM_DW_GENERIC=1 sends even shapes through the generic per-pixel kernels; they decline every request"""
    monkeypatch.setenv("FM_DW_GENERIC", "1")
    for K, s in KS:
        assert not _dw_fwd_case(eng, family, dt, K, s, (3, 8, 12, 24), 150, request="stats", generic=True)
    assert not _dw_fwd_case(eng, family, dt, 3, 1, (2, 6, 5, 8), 151, generic=True, pads=(0, 2))     # not TF-"same": generic anyway


# (K, s, shape, groups, served) -- the flag of each is derived by hand from dw_rowu_launch / dw_stats_rowgroups:
#  (4, 8, 8, 16) groups 2: 16 steps, 8 per group, target 1536 -> d = 8 = all of them: served
#  (3, 2, 8, 16) groups 2: HB = 1: 3 steps do not split into 2 groups: declined
#  (53, 1, 128, 512): WB Q = 4096 lanes = 64 chunks, target 3072 / 64 = 48; 53 steps (prime, above the target): the only divisor <= 48
#                     is 1 and 4 * 1 < 48: dw_stats_rowgroups returns 0: declined
#  stride 2 (4, 8, 8, 16) groups 2: 16 output rows, 8 per group: served
STATS_CASES = [(3, 1, (9, 16, 12, 16), 1, True), (5, 1, (4, 8, 8, 16), 2, True), (3, 2, (4, 8, 8, 16), 2, True),
               (3, 1, (3, 2, 8, 16), 2, False), (3, 1, (53, 1, 128, 512), 1, False)]


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_dw_fwd_stats_request(eng, dt, family):
    """the statistics request in its served (groups 1 and 2) and both declined arms; the flag is asserted against STATS_CASES"""
    for i, (K, s, shape, groups, want) in enumerate(STATS_CASES):
        N, H, W, C = shape
        assert _stats_served(False, K, s, N, H, W, C, R.same_pad(H, K, s), R.same_pad(W, K, s), groups) == want
        got = _dw_fwd_case(eng, family, dt, K, s, shape, 200 + i, request="stats", groups=groups)
        assert got == want, (shape, groups, got)


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_dw_fwd_eval_epilogue_and_pooling(eng, dt, family):
    """the eval forward: y = act(conv scale + shift) with the per-image pooling sums of the stored y (ST = 3).  H = 36: 18 row pairs
    (stride 1) / 18 output rows (stride 2) per image, dw_pool_rpb falls back to 9 (two blocks per image); H = 34 at stride 1: 17 pairs,
    rpb = 1.  Dyadic: act = 0 (the affine is exact); random: swish, bound = _swish_err(v, |scale| conv bound + 2 u (|conv scale| +
    |shift|)); pooling over n stored values: n u sum|y|.  Odd sizes at stride 2 run the generic kernel, which declines."""
    act = 0 if family == "dyadic" else 2
    for i, (K, s, shape) in enumerate([(3, 1, (3, 36, 6, 16)), (5, 2, (3, 36, 6, 16)), (5, 1, (2, 34, 5, 8)), (3, 2, (2, 7, 7, 16))]):
        served = _dw_fwd_case(eng, family, dt, K, s, shape, 300 + i, act=act, affine=True, request="pool")
        assert served == _rowu(K, s, shape[1], shape[2], R.same_pad(shape[1], K, s), R.same_pad(shape[2], K, s))
    if family == "random":
        _dw_fwd_case(eng, family, dt, 3, 1, (2, 7, 7, 16), 310, act=1, affine=True)           # relu epilogue, no request


# ---- data gradient -----------------------------------------------------------------------------------------------------------------
def _dw_dgrad_case(eng, family, dt, K, s, shape, seed, ye=False, groups=1, generic=False):
    N, H, W, C = shape
    bf = dt == BF16
    rs = np.random.RandomState(seed)
    d = _dims(dt, N, H, W, C, K, s, 0, groups)
    Ho, Wo, pt, pl = d[4], d[5], d[9], d[10]
    dy, w = _vals(family, rs, (N, Ho, Wo, C), bf), _wts(family, rs, (K * K, C))
    name = f"dw_dgrad K{K}s{s}{'bf16' if bf else 'f32'}{shape}{'ye' if ye else ''}{'g' if generic else ''}"
    pool = []
    dyb, wb, dxb = Buf(eng, dy.size, bf, dy, pool), Buf(eng, w.size, False, w, pool), Buf(eng, N * H * W * C, bf, pool=pool)
    ptrs = [dyb.t, wb.t, dxb.t]
    ws = eng.debug_eff_ws("dw_dgrad", d)
    if ye:
        yev = _vals(family, rs, shape, bf)
        mean, istd = _coef(family, rs, (groups, C)), _coef(family, rs, (groups, C), pos=True)
        # dyadic: scale = shift = 0, where swish'(0) = 1/2 exactly: the sums are linear in the stored dx
        scale = np.zeros((groups, C)) if family == "dyadic" else _coef(family, rs, (groups, C))
        shift = np.zeros((groups, C)) if family == "dyadic" else _coef(family, rs, (groups, C))
        yeb = Buf(eng, yev.size, bf, yev, pool)
        q = [Buf(eng, groups * C, False, a, pool) for a in (mean, istd, scale, shift)]
        recb, stb = Buf(eng, ws[0], pool=pool), Buf(eng, ws[1], pool=pool)
        ptrs += [yeb.t] + [b.t for b in q] + [recb.t, stb.t]
    served = eng.debug_eff("dw_dgrad", ptrs, d)
    _canaries(pool, name)
    want = R.dw_dgrad(dy, w, K, s, pt, pl, H, W)
    bound = (K * K + 1) * U * R.dw_dgrad(np.abs(dy), np.abs(w), K, s, pt, pl, H, W)
    got = dxb.np(shape)
    _check(family, name + " dx", got, want, bound, bf)
    if not ye:
        assert not served
        return served
    assert served == (ws[0] > 0) == _stats_served(True, K, s, N, H, W, C, pt, pl, groups, generic), (name, served, ws)
    if not served:
        assert np.isnan(stb.np()).all(), f"{name}: a declined request wrote stats_out"
        return served
    stored = R.store(want, bf) if family == "dyadic" else got.astype(np.float64)
    ref = R.bn0_bwd_sums(stored, yev, mean, istd, scale, shift, groups)
    st = stb.np((groups, 8, 2, C)).astype(np.float64).sum(1)
    # bound: term t1 = dx sg with |d sg| from _swish_grad_err (v = ye scale + shift carries 2 u (|ye scale| + |shift|)), t2 = t1 xhat
    # with xhat = (ye - mean) istd within 2 u |xhat|; n-term sums: n u sum|t| + sum of the terms' errors
    dxg, yg = R.group_rows(stored, groups), R.group_rows(yev, groups)
    sc, sh, mu, isd = (a[:, None, :] for a in (scale, shift, mean, istd))
    v = yg * sc + sh
    sg, esg = R.swish_grad(v), _swish_grad_err(v, _affine_err(yg, sc, sh))
    xh = (yg - mu) * isd
    t1, e1 = dxg * sg, np.abs(dxg) * esg + U * np.abs(dxg * sg)
    e2 = np.abs(xh) * e1 + np.abs(t1) * 2 * U * np.abs(xh) + U * np.abs(t1 * xh)
    n = N * H * W // groups
    if family == "dyadic":
        _exact(t1[0] * np.abs(xh[0]).max(), 1 / 256)
    _check(family, name + " S1", st[:, 0], ref[:, 0], n * U * np.abs(t1).sum(1) + e1.sum(1))
    _check(family, name + " S2", st[:, 1], ref[:, 1], n * U * np.abs(t1 * xh).sum(1) + e2.sum(1))
    return served


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("ks", KS, ids=lambda p: f"K{p[0]}s{p[1]}")
def test_dw_dgrad(eng, ks, dt, family):
    """dx at every shape of DW_SHAPES (shape = the INPUT's): stride 1 is the forward kernel with the rotated kernel (`flip`) -- the
    weights are not symmetric under the rotation --, stride 2 the row-uniform kernel at even sizes and the generic one at odd sizes.
    Random bound: (K K + 1) u sum|dy w| (+ half a bf16 ulp).  Worst ratios: eff_parity.json (dw_dgrad/random)."""
    K, s = ks
    for i, shape in enumerate(DW_SHAPES):
        _dw_dgrad_case(eng, family, dt, K, s, shape, 400 + i)


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_dw_dgrad_bn0_sums(eng, monkeypatch, dt, family):
    """the data gradient with ye and the BN quad (ST = 2): served with groups 1 and 2 at both strides, declined where the steps do
    not split into the groups, at odd stride-2 sizes and in the forced generic kernels.  S1, S2 against float64 (kernels.h:
    k_chan_reduce mode 1 with swish); bound in _dw_dgrad_case."""
    cases = [(3, 1, (2, 7, 7, 16), 1, True), (5, 1, (4, 5, 10, 100), 2, True), (3, 2, (3, 8, 12, 24), 1, True),
             (5, 2, (4, 8, 12, 24), 2, True), (3, 1, (3, 2, 8, 16), 2, False), (3, 2, (2, 7, 7, 16), 1, False)]
    for i, (K, s, shape, groups, want) in enumerate(cases):
        assert _dw_dgrad_case(eng, family, dt, K, s, shape, 500 + i, ye=True, groups=groups) == want, (K, s, shape, groups)
    monkeypatch.setenv("FM_DW_GENERIC", "1")
    for K, s in KS:
        assert not _dw_dgrad_case(eng, family, dt, K, s, (3, 8, 12, 24), 520, ye=True, generic=True)


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------
def _dw_wgrad_case(eng, family, dt, K, s, shape, seed, pads=None):
    N, H, W, C = shape
    bf = dt == BF16
    rs = np.random.RandomState(seed)
    d = _dims(dt, N, H, W, C, K, s, pads=pads)
    Ho, Wo, pt, pl = d[4], d[5], d[9], d[10]
    x, dy = _vals(family, rs, shape, bf), _vals(family, rs, (N, Ho, Wo, C), bf)
    name = f"dw_wgrad K{K}s{s}{'bf16' if bf else 'f32'}{shape}"
    ws = eng.debug_eff_ws("dw_wgrad", d)
    assert ws[1] == K * K * C and ws[0] > 0
    pool = []
    dyb, xb = Buf(eng, dy.size, bf, dy, pool), Buf(eng, x.size, bf, x, pool)
    pb, ob = Buf(eng, ws[0], pool=pool), Buf(eng, ws[1], pool=pool)
    eng.debug_eff("dw_wgrad", [dyb.t, xb.t, pb.t, ob.t], d)
    _canaries(pool, name)
    want = R.dw_wgrad(dy, x, K, s, pt, pl)
    if family == "dyadic":
        _exact(R.dw_wgrad(np.abs(dy), np.abs(x), K, s, pt, pl), 1 / 4)
    _check(family, name, ob.np((K * K, C)), want, (N * Ho * Wo + 1) * U * R.dw_wgrad(np.abs(dy), np.abs(x), K, s, pt, pl))


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("ks", KS, ids=lambda p: f"K{p[0]}s{p[1]}")
def test_dw_wgrad(eng, monkeypatch, ks, dt, family):
    """dw [K*K][C] at every shape of DW_SHAPES.  The five kernels (dw_wgrad_full / dw_wgrad_t): dw_rowu_wgrad_kernel (bf16, and fp32
    5x5, at TF-"same" sizes the row-uniform test accepts), dw_wgrad_blk2_kernel (fp32 3x3 stride 1), dw_wgrad_blk_kernel (fp32 3x3
    stride 2, even sizes), dw_wgrad_kernel<3> / <5> (odd sizes at stride 2, FM_DW_GENERIC, other paddings).  An n-pixel sum of
    rounded products: (n + 1) u sum|dy x|.  Worst ratios: eff_parity.json (dw_wgrad/random)."""
    K, s = ks
    for i, shape in enumerate(DW_SHAPES):
        _dw_wgrad_case(eng, family, dt, K, s, shape, 600 + i)
    monkeypatch.setenv("FM_DW_GENERIC", "1")
    _dw_wgrad_case(eng, family, dt, K, s, (3, 8, 12, 24), 650)
    _dw_wgrad_case(eng, family, dt, K, s, (9, 16, 12, 16), 651)                 # generic kernel, 13 blocks, ragged last one


# ---- squeeze-excite ----------------------------------------------------------------------------------------------------------------
# (imgs, ipg, HW, C, Cs): HW 49 / 196 / 1030 give 1 / 3 / 16 pooling chunks (196 = 3 * 66 - 2, 1030 = 16 * 65 - 10: ragged last chunks);
# Cs 4, 6, 10, 48 (B0's 6 and 10 are no multiples of the 4 rows a wave takes); imgs = 2 groups of 3 / 5 images; C = 1152 makes the
# pooling kernels loop over channel pieces (Q = 288 > 256 lanes)
SE_SHAPES = [(6, 3, 49, 32, 4), (6, 3, 196, 144, 6), (2, 1, 1030, 32, 10), (10, 5, 49, 1152, 48)]


def _se_weights(family, rs, C, Cs):
    if family == "dyadic":
        return rs.choice(DYC, (Cs, C)), rs.choice(DYC, Cs), rs.choice(DYC, (Cs, C)), rs.choice(DYC, C)
    f = lambda *sh: (rs.standard_normal(sh) / np.sqrt(sh[-1])).astype(np.float32).astype(np.float64)
    return f(Cs, C), f(Cs), (rs.standard_normal((Cs, C)) / np.sqrt(Cs)).astype(np.float32).astype(np.float64), f(C)


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SE_SHAPES, ids=str)
def test_se_fwd_and_scale(eng, shape, dt, family):
    """k_se_fwd with and without scale / shift on load and with `pooled`, then k_se_scale.  Dyadic: the pooling partials (summed over the
    chunks) and, without scale / shift, out = a gate for a dyadic gate are bit-exact.  Random bounds: pooled sum over HW values:
    HW u sum|A| + sum _swish_err; sq = sum / HW: + 2 u |sq|; rpre: (C + 2) u (sum|W1 sq| + |b1|) + sum|W1| d sq;  r = swish(rpre);
    t = b2 + W2 r: (Cs + 2) u (sum|W2 r| + |b2|) + sum|W2| d r;  gate: _sig_err(t) + d t / 4;  out = A gate: |gate| d A + u |out|
    (+ half a bf16 ulp).  Worst ratios: eff_parity.json (se_fwd/random, se_scale/random)."""
    N, ipg, HW, C, Cs = shape
    G, bf = N // ipg, dt == BF16
    rs = np.random.RandomState(700 + C + HW)
    a = _vals(family, rs, (N, HW, C), bf)
    W1, b1, W2t, b2 = _se_weights(family, rs, C, Cs)
    variants = [("plain", False, False), ("pooled", False, True)] + ([("affine", True, False)] if family == "random" else [])
    for vname, affine, pooled in variants:
        name = f"se_fwd {shape}{'bf16' if bf else 'f32'}{vname}"
        scale = _coef(family, rs, (G, C)) if affine else None
        shift = _coef(family, rs, (G, C)) if affine else None
        d = [dt, N, HW, C, Cs, ipg if affine else 1, int(pooled)]
        ws = eng.debug_eff_ws("se_fwd", d)
        nch = max(1, min(16, HW // 64))
        assert ws[0] == (N * C if pooled else N * nch * C)
        A = R.se_input(a, scale, shift, ipg)
        dA = _swish_err(a * R.per_image(scale, ipg, N) + R.per_image(shift, ipg, N),
                        _affine_err(a, R.per_image(scale, ipg, N), R.per_image(shift, ipg, N))) if affine else np.zeros_like(A)
        pool = []
        ab = Buf(eng, a.size, bf, a, pool)
        wbs = [Buf(eng, t.size, False, t, pool) for t in (W1, b1, W2t, b2)]
        pw = Buf(eng, ws[0], False, R.pool_sums(A) if pooled else None, pool)
        scb = Buf(eng, G * C, False, scale, pool) if affine else None
        shb = Buf(eng, G * C, False, shift, pool) if affine else None
        sqb, rpb, gtb = Buf(eng, N * C, pool=pool), Buf(eng, N * Cs, pool=pool), Buf(eng, N * C, pool=pool)
        eng.debug_eff("se_fwd", [None if pooled else ab.t, scb and scb.t, shb and shb.t, pw.t] + [b.t for b in wbs] +
                      [sqb.t, rpb.t, gtb.t], d)
        _canaries(pool, name)
        psum = R.pool_sums(A)
        if pooled:
            psum = psum.astype(np.float32).astype(np.float64)                # what the workspace held
            epool = np.zeros_like(psum)
        else:
            got_pool = pw.np((N, nch, C)).astype(np.float64).sum(1)
            epool = HW * U * R.pool_sums(np.abs(A)) + dA.sum(1)
            if family == "dyadic":
                _exact(A[0], 1 / 2)
            _check(family, name + " pool", got_pool, psum, epool)
        sq, rpre, gate = R.se_fwd(A, W1, b1, W2t, b2, pooled=psum)
        esq = epool / HW + 2 * U * np.abs(sq)
        erp = (C + 2) * U * (np.abs(sq) @ np.abs(W1).T + np.abs(b1)) + esq @ np.abs(W1).T
        r = R.swish(rpre)
        er = _swish_err(rpre, erp)
        t = r @ W2t + b2
        et = (Cs + 2) * U * (np.abs(r) @ np.abs(W2t) + np.abs(b2)) + er @ np.abs(W2t)
        _within(name + " sq", sqb.np((N, C)), sq, esq, family)
        _within(name + " rpre", rpb.np((N, Cs)), rpre, erp, family)
        _within(name + " gate", gtb.np((N, C)), gate, _sig_err(t) + 0.25 * et, family)
        if HW & (HW - 1) == 0 and family == "dyadic" and not pooled:
            _bits(name + " sq", sqb.np((N, C)), sq)
        if pooled:
            continue
        # k_se_scale with this launch's operands; the gate is its own operand here
        gt = np.abs(_coef(family, rs, (N, C))) if family == "dyadic" else R.sigmoid(rs.standard_normal((N, C))).astype(np.float32).astype(np.float64)
        gb, ob = Buf(eng, N * C, False, gt, pool), Buf(eng, a.size, bf, pool=pool)
        eng.debug_eff("se_scale", [ab.t, scb and scb.t, shb and shb.t, gb.t, ob.t], [dt, N, HW, C, 1, ipg if affine else 1, 0])
        _canaries(pool, name + " scale")
        want = R.se_scale(A, gt)
        _check(family, f"se_scale {shape}{vname}", ob.np((N, HW, C)), want, gt[:, None, :] * dA + U * np.abs(want), bf)


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SE_SHAPES + [(33, 33, 49, 32, 6)], ids=str)
def test_se_bwd_bn1(eng, shape, dt, family):
    """k_se_bwd_bn1, stage by stage.  pool_ws [imgs][nch][5][C] (nch from fm_debug_eff_ws) summed over the chunks against the five
    float64 per-image sums; then dgp, drp, ds and the BN1 partials against the float64 function of the STORED stage inputs (pool
    records, gate, dgp, drp, ds as the kernel left them).  (33, 33, 49, 32, 6): ipg = 33 gives two BN1 splits of 17 and 16 images.
    Dyadic: scale = shift = 0, where A = 0 and sg = 1/2: the five sums are linear and bit-exact; dgp = 0.  Bounds, with n = HW and the
    per-element errors dA = _swish_err, dsg = _swish_grad_err (v carries 2 u (|y scale| + |shift|)), xh within 2 u |xh|:
    R: n u sum|d A| + sum(|d| dA + u |d A|); P1: n u sum|d sg| + sum(|d| dsg + u |d sg|); P2: ... times |xh| + 3 u |d sg xh|; Q1: n u sum sg +
    sum dsg; Q2: n u sum|sg xh| + sum(|xh| dsg + 3 u |sg xh|).  dgp = R g (1 - g): (nch + 4) u sum_k|R_k| g (1 - g);
    drp = (W2 dgp) swish'(rpre): (C + 2) u sum|W2 dgp| |swish'| + |W2 dgp| _swish_grad_err(rpre); ds = W1^T drp: (Cs + 1) u sum|W1 drp|;
    S = sum_img (g P + ds / HW Q): (ipg + nch + 5) u sum_img (g sum_k|P_k| + |ds| / HW sum_k|Q_k|).
    The same launch with dout = NULL and nch_ready = nch (the engine's call after the fused project-conv backward, which leaves the
    records itself) must reproduce dgp, drp, ds and the partials bit for bit from the records of the first launch.
    Worst ratios: eff_parity.json (se_bwd_bn1/random)."""
    N, ipg, HW, C, Cs = shape
    G, bf = N // ipg, dt == BF16
    rs = np.random.RandomState(800 + C + HW)
    y, dout = _vals(family, rs, (N, HW, C), bf), _vals(family, rs, (N, HW, C), bf)
    W1, _, W2t, _ = _se_weights(family, rs, C, Cs)
    dy = family == "dyadic"
    scale = np.zeros((G, C)) if dy else _coef(family, rs, (G, C))
    shift = np.zeros((G, C)) if dy else _coef(family, rs, (G, C))
    mean, istd = _coef(family, rs, (G, C)), _coef(family, rs, (G, C), pos=True)
    gate = np.abs(rs.choice(DYC, (N, C))) if dy else R.sigmoid(rs.standard_normal((N, C))).astype(np.float32).astype(np.float64)
    rpre = np.zeros((N, Cs)) if dy else rs.standard_normal((N, Cs)).astype(np.float32).astype(np.float64)
    d = [dt, N, HW, C, Cs, ipg, 0]
    ws = eng.debug_eff_ws("se_bwd_bn1", d)
    nch, splits = ws[0] // (N * 5 * C), ws[2]
    assert ws[0] == N * nch * 5 * C and ws[1] == G * splits * 2 * C and splits == max(1, min(32, ipg // 16))
    assert nch == max(1, min(max(1, min(16, HW // 64)), max(HW // 512, 2)))
    name = f"se_bwd_bn1 {shape}{'bf16' if bf else 'f32'}"
    pool = []
    ins = [Buf(eng, t.size, b, t, pool) for t, b in ((dout, bf), (y, bf), (scale, 0), (shift, 0), (mean, 0), (istd, 0))]
    pw = Buf(eng, ws[0], pool=pool)
    ins2 = [Buf(eng, t.size, False, t, pool) for t in (gate, rpre, W1, W2t)]
    outs = [Buf(eng, n, pool=pool) for n in (N * C, N * Cs, N * C, ws[1])]
    eng.debug_eff("se_bwd_bn1", [b.t for b in ins] + [pw.t] + [b.t for b in ins2] + [b.t for b in outs], d)
    _canaries(pool, name)
    rec = pw.np((N, nch, 5, C)).astype(np.float64)
    p5 = rec.sum(1)
    sc, sh, mu, isd = (R.per_image(t, ipg, N) for t in (scale, shift, mean, istd))
    v = y * sc + sh
    dv = _affine_err(y, sc, sh)
    A, sg, xh = R.swish(v), R.swish_grad(v), (y - mu) * isd
    dA, dsg = _swish_err(v, dv), _swish_grad_err(v, dv)
    ref5 = R.se_bwd_bn1(dout, y, scale, shift, mean, istd, ipg, gate, rpre, W1, W2t)[0]
    ad = np.abs(dout)
    terms = [dout * A, dout * sg, dout * sg * xh, sg, sg * xh]
    errs = [ad * dA + U * np.abs(terms[0]), ad * dsg + U * np.abs(terms[1]),
            (ad * dsg + U * np.abs(terms[1])) * np.abs(xh) + 3 * U * np.abs(terms[2]), dsg, np.abs(xh) * dsg + 3 * U * np.abs(terms[4])]
    if dy:
        _exact(np.abs(dout[0]) * np.abs(xh[0]).max(), 1 / 256)
    for k, nm in enumerate(("R", "P1", "P2", "Q1", "Q2")):
        _check(family, f"{name} {nm}", p5[:, k], ref5[:, k], HW * U * np.abs(terms[k]).sum(1) + errs[k].sum(1))
    dgp_g, drp_g, ds_g = outs[0].np((N, C)), outs[1].np((N, Cs)), outs[2].np((N, C))
    bn_g = outs[3].np((G, splits, 2, C)).astype(np.float64).sum(1)
    arec = np.abs(rec).sum(1)
    gg = gate * (1 - gate)
    _within(name + " dgp", dgp_g, p5[:, 0] * gg, (nch + 4) * U * arec[:, 0] * gg, family)
    dg64 = dgp_g.astype(np.float64)
    dot, adot = dg64 @ W2t.T, np.abs(dg64) @ np.abs(W2t).T
    sgr = R.swish_grad(rpre)
    _within(name + " drp", drp_g, dot * sgr, (C + 2) * U * adot * np.abs(sgr) + np.abs(dot) * _swish_grad_err(rpre), family)
    dr64 = drp_g.astype(np.float64)
    _within(name + " ds", ds_g, dr64 @ W1, (Cs + 1) * U * (np.abs(dr64) @ np.abs(W1)), family)
    dsv = ds_g.astype(np.float64) / HW
    for k, nm in ((0, "S1"), (1, "S2")):
        want = (gate * p5[:, 1 + k] + dsv * p5[:, 3 + k]).reshape(G, ipg, C).sum(1)
        bnd = (ipg + nch + 5) * U * (gate * arec[:, 1 + k] + np.abs(dsv) * arec[:, 3 + k]).reshape(G, ipg, C).sum(1)
        _within(f"{name} {nm}", bn_g[:, k], want, bnd, family)
    if dy:
        assert not dgp_g.any() and not drp_g.any() and not ds_g.any()                   # R = 0 exactly
    # dout = NULL, nch_ready = nch: pool_ws is an input
    outs2 = [Buf(eng, n, pool=pool) for n in (N * C, N * Cs, N * C, ws[1])]
    d2 = [dt, N, HW, C, Cs, ipg, nch]
    assert eng.debug_eff_ws("se_bwd_bn1", d2) == ws
    eng.debug_eff("se_bwd_bn1", [None] + [b.t for b in ins[1:]] + [pw.t] + [b.t for b in ins2] + [b.t for b in outs2], d2)
    _canaries(pool, name + " nch_ready")
    for a, b in zip(outs, outs2):
        assert np.array_equal(a.np().view(np.uint32), b.np().view(np.uint32)), f"{name}: nch_ready launch differs"


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("shape", [(6, 32, 4), (7, 144, 6), (40, 32, 10), (10, 1152, 48), (37, 64, 8)], ids=str)
def test_se_wgrad(eng, shape, family):
    """the contiguous range [dW1 | db1 padded to 4 | dW2 | db2] (imgs, C, Cs): 16 image splits (imgs 6, 7, 10: most splits empty;
    37: ragged; 40: more than one 16-image tile never, three images per split).  The Cs of the cases cover spec.b0_blocks()'s squeezed
    widths that are not multiples of 4 (6 and 10); the pad slots after db1 must hold +0 (the arena keeps every tensor 16-byte
    aligned and Adam must leave the pad zero).  Dyadic: rpre = 0, swish(0) = 0: dW2 = 0 and dW1, db1, db2 bit-exact.  Random: sums
    over imgs terms in 16 slabs: (imgs + 18) u sum|terms|, + sum |dgp| _swish_err(rpre) for dW2.
    Worst ratios: eff_parity.json (se_wgrad/random)."""
    N, C, Cs = shape
    cs_b0 = {max(1, cin // 4) for (_, _, _, cin, _) in spec.b0_blocks()}
    assert {6, 10} <= cs_b0 and max(cs_b0) == 48
    rs = np.random.RandomState(900 + N + C)
    dy = family == "dyadic"
    dgp, drp, sq = (_vals(family, rs, sh, False) for sh in ((N, C), (N, Cs), (N, C)))
    rpre = np.zeros((N, Cs)) if dy else _vals(family, rs, (N, Cs), False)
    ws = eng.debug_eff_ws("se_wgrad", [N, C, Cs])
    o_b1, o_w2, o_b2, n = R.se_range_offsets(C, Cs)
    assert ws[1] == n and ws[0] == 16 * n
    pool = []
    ins = [Buf(eng, t.size, False, t, pool) for t in (dgp, drp, rpre, sq)]
    pb, ob = Buf(eng, ws[0], pool=pool), Buf(eng, ws[1], pool=pool)
    eng.debug_eff("se_wgrad", [b.t for b in ins] + [pb.t, ob.t], [N, C, Cs])
    _canaries(pool, f"se_wgrad {shape}")
    got = ob.np()
    want = R.se_wgrad(dgp, drp, rpre, sq)
    bound = np.zeros(n)
    k = (N + 18) * U
    bound[:o_b1] = k * (np.abs(drp).T @ np.abs(sq)).reshape(-1)
    bound[o_b1:o_b1 + Cs] = k * np.abs(drp).sum(0)
    sw = R.swish(rpre)
    bound[o_w2:o_b2] = (k * (np.abs(sw).T @ np.abs(dgp)) + _swish_err(rpre).T @ np.abs(dgp)).reshape(-1)
    bound[o_b2:] = k * np.abs(dgp).sum(0)
    if dy:
        _exact(np.abs(drp).max() * np.abs(sq), 1 / 4)
    _check(family, f"se_wgrad {shape}", got, want, bound)
    pad = got[o_b1 + Cs:o_w2]
    assert pad.size == (-Cs) % 4 and not pad.view(np.uint32).any(), "pad slots after db1 are not +0"


# ---- BN + activation passes --------------------------------------------------------------------------------------------------------
# (groups, images per group, HW, C) -- Q = C / (4 NV) 16-byte pieces per pixel, NV = 2 when both types are bf16, else 1:
#  (2, 3, 6, 16)    Q = 4 / 2: tiny, two groups, HW = 6 divides nothing else
#  (1, 2, 49, 100)  fp32 only (C % 8 != 0).  Q = 25: the rows form runs T = 250 threads (6 idle) and a block covers 4 rows = 1000
#                   pieces.  2450 pieces = 2 blocks + 450: the last block's first row is full and its second ends at thread 200
#  (1, 3, 49, 100)  3675 pieces = 3 blocks + 675: ends inside the THIRD row (thread 175): the tail breaks at k = 3
#  (1, 4, 49, 100)  4900 pieces = 4 blocks + 900: ends inside the FOURTH row (thread 150): no row is skipped, the last is partial
#  (1, 5, 9, 24)    bf16 only: Q = 3, T = 255, a block covers 1020 pieces; 135 pieces end inside the first row
#  (1, 19, 9, 24)   bf16 only: 513 pieces end inside the third row (thread 3);  (1, 29, 9, 24): 783 pieces, the fourth (thread 18)
#                   (`_arm_asserts` holds each of these rows with `_tail_row`)
#  (3, 1, 5, 672)   Q = 168 > 128 (84 in bf16): one pixel row per block in the rows form and in chan_reduce, 88 idle threads
#  (1, 2, 4, 1152)  fp32 Q = 288 > 256: the rows form is declined and chan_reduce's threads 0 .. 31 make a second trip over the
#                   channel pieces; bf16 Q = 144
#  (2, 4, 64, 32)   256 pixels per group: 4 chan_reduce blocks per group, pixel tiles dealt round-robin
BN_SHAPES = [(2, 3, 6, 16), (1, 2, 49, 100), (1, 3, 49, 100), (1, 4, 49, 100), (1, 5, 9, 24), (1, 19, 9, 24), (1, 29, 9, 24),
             (3, 1, 5, 672), (1, 2, 4, 1152), (2, 4, 64, 32)]
# row of the rows form's last block in which the piece count ends (0 = first), for the shapes whose Q does not divide 256
TAIL_ROWS = {(1, 2, 49, 100): (25, 1), (1, 3, 49, 100): (25, 2), (1, 4, 49, 100): (25, 3),
             (1, 5, 9, 24): (3, 0), (1, 19, 9, 24): (3, 2), (1, 29, 9, 24): (3, 3)}
BN_TYPES = [(F32, F32), (BF16, BF16), (F32, BF16)]
EW_R = 4


def _bn_cases():
    for k, sh in enumerate(BN_SHAPES):
        for ty, ta in BN_TYPES:
            if (ty, ta) == (F32, F32) and sh[3] == 24:
                continue
            if (ty, ta) == (BF16, BF16) and sh[3] % 8:
                continue
            if (ty, ta) == (F32, BF16) and k not in (0, len(BN_SHAPES) - 1):
                continue
            yield pytest.param(sh, ty, ta, id=f"{sh}-{'f32' if ty == F32 else 'bf16'}.{'f32' if ta == F32 else 'bf16'}")


def _rows_on(C, ty, ta, mode, bit):
    """ew_rows_on of effnet.hip restated: the rows form runs when the pass's bit is set in FM_EW_ROWS (both types bf16) /
    FM_EW_ROWS_F32 (otherwise) and a pixel has 1 .. 256 pieces"""
    nv = 2 if (ty == BF16 and ta == BF16) else 1
    Q = C // (4 * nv)
    return bool(int(mode) & bit) and 1 <= Q <= 256, Q


def _tail_row(pix, Q):
    """row (0 .. EW_R - 1) of the rows form's last block in which the last piece lies, and whether it fills that row"""
    T = (256 // Q) * Q
    rem = (pix * Q - 1) % (EW_R * T) + 1
    return (rem - 1) // T, rem % T == 0


def _set_rows(monkeypatch, mode):
    monkeypatch.setenv("FM_EW_ROWS", mode)
    monkeypatch.setenv("FM_EW_ROWS_F32", mode)


def _arm_asserts(shape, ty, ta, mode, bit):
    G, ipg, HW, C = shape
    on, Q = _rows_on(C, ty, ta, mode, bit)
    assert on == (mode == "3" and Q <= 256)
    if shape == (1, 2, 4, 1152):
        assert (Q, on) == ((288, False) if ta == F32 else (144, mode == "3"))
    if shape in TAIL_ROWS:
        assert ty == ta and 256 % Q and (Q, _tail_row(ipg * HW, Q)) == (TAIL_ROWS[shape][0], (TAIL_ROWS[shape][1], False))   # ends INSIDE that row
    if shape == (3, 1, 5, 672) and ta == F32:
        assert Q == 168 and 256 // Q == 1
    return on


def _bn_operands(family, rs, shape, ty, ta, backward):
    G, ipg, HW, C = shape
    n = ipg * HW
    dy = family == "dyadic"
    o = {"y": _vals(family, rs, (G, n, C), ty == BF16), "x": _vals(family, rs, (G, n, C), ta == BF16)}       # x: res, or a / dz
    o["scale"], o["shift"] = _coef(family, rs, (G, C)), _coef(family, rs, (G, C))
    o["rowscale"] = rs.choice([0.0, 2.0] if dy else [0.0, 1.25], (G, ipg))              # stochastic depth: 0 or 1 / keep
    if backward:
        o["mean"], o["istd"] = _coef(family, rs, (G, C)), _coef(family, rs, (G, C), pos=True)
        o["ca"], o["cb"], o["cc"] = (_coef(family, rs, (G, C)) for _ in range(3))
        if dy:
            o["gate"] = np.abs(rs.choice(DYC, (G, ipg, C)))
            # dsv / HW must be exact: HW a power of two and dsv a multiple of HW / 16; otherwise 0
            o["dsv"] = rs.choice(DYC, (G, ipg, C)) * HW / 4 if HW & (HW - 1) == 0 else np.zeros((G, ipg, C))
        else:
            o["gate"] = R.sigmoid(rs.standard_normal((G, ipg, C))).astype(np.float32).astype(np.float64)
            o["dsv"] = rs.standard_normal((G, ipg, C)).astype(np.float32).astype(np.float64)
    return o


def _dyh_terms(family, o, shape, a, rowscaled, gated):
    """(kw of the reference, dyh, its absolute error bound) for the operands o.  d = x gate + dsv (1 / HW): roundings of 1 / HW, the
    two products and the sum; times swish'(v) (`_swish_grad_err`, v within `_affine_err`), times rowscale: one rounding each"""
    G, ipg, HW, C = shape
    sc, sh = (o["scale"], o["shift"]) if not (family == "dyadic" and a == 2) else (np.zeros((G, C)), np.zeros((G, C)))
    kw = dict(scale=sc, shift=sh, rowscale=o["rowscale"] if rowscaled else None, gate=o["gate"] if gated else None,
              dsv=o["dsv"] if gated else None)
    d, e = o["x"], np.zeros_like(o["x"])
    if gated:
        g, dv = R._per_pixel(o["gate"], HW), R._per_pixel(o["dsv"], HW) / HW
        d = o["x"] * g + dv
        e = U * np.abs(o["x"] * g) + 2 * U * np.abs(dv) + U * np.abs(d)
    if a == 2:
        v = o["y"] * sc[:, None, :] + sh[:, None, :]
        sg = R.swish_grad(v)
        e = np.abs(sg) * e + np.abs(d) * _swish_grad_err(v, _affine_err(o["y"], sc[:, None, :], sh[:, None, :])) + U * np.abs(d * sg)
        d = d * sg
    if rowscaled:
        r = R._per_pixel(o["rowscale"], HW)
        d, e = d * r, r * e + U * np.abs(d * r)
    return kw, sc, sh, d, e


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("mode", ["0", "3"], ids=["piece", "rows"])
@pytest.mark.parametrize("shape,ty,ta", _bn_cases())
def test_bnact_apply(eng, monkeypatch, shape, ty, ta, mode, family):
    """out = act(y scale + shift) rowscale[img] + res through k_bnact_apply in the one-piece form (FM_EW_ROWS = FM_EW_ROWS_F32 = 0) and
    the rows form (3), with and without res and rowscale (0 or 1 / keep), act 0 / 1 / 2 (dyadic: 0 and 1, the affine is exact).
    Random bound: v within `_affine_err`, swish within `_swish_err`, one rounding for the rowscale product and one for the residual
    sum (+ half a bf16 ulp for a bf16 out).  Worst ratios: eff_parity.json (bnact_apply/random)."""
    G, ipg, HW, C = shape
    _set_rows(monkeypatch, mode)
    on = _arm_asserts(shape, ty, ta, mode, 1)
    rs = np.random.RandomState(1000 + C + HW)
    o = _bn_operands(family, rs, shape, ty, ta, False)
    d = [ty, ta, G, ipg * HW, HW, C, 0, 0]
    assert eng.debug_eff_ws("bnact_apply", d) == [0, 0, 0, 0]
    for a in ((0, 1) if family == "dyadic" else (0, 1, 2)):
        for with_res, with_rs in ((False, False), (True, False), (False, True), (True, True)):
            name = f"bnact_apply {shape}{ty}{ta}{'rows' if on else 'piece'} act{a}{'+res' if with_res else ''}{'*rs' if with_rs else ''}"
            pool = []
            yb = Buf(eng, o["y"].size, ty == BF16, o["y"], pool)
            scb, shb = Buf(eng, G * C, False, o["scale"], pool), Buf(eng, G * C, False, o["shift"], pool)
            rb = Buf(eng, o["x"].size, ta == BF16, o["x"], pool) if with_res else None
            rsb = Buf(eng, G * ipg, False, o["rowscale"], pool) if with_rs else None
            ob = Buf(eng, o["y"].size, ta == BF16, pool=pool)
            d[7] = a
            eng.debug_eff("bnact_apply", [yb.t, scb.t, shb.t, rb and rb.t, rsb and rsb.t, ob.t], d)
            _canaries(pool, name)
            sc, sh = o["scale"][:, None, :], o["shift"][:, None, :]
            v = o["y"] * sc + sh
            want = R.bnact_apply(o["y"], o["scale"], o["shift"], HW, a, o["x"] if with_res else None, o["rowscale"] if with_rs else None)
            dv = _affine_err(o["y"], sc, sh)
            bound = _swish_err(v, dv) if a == 2 else dv
            if with_rs:
                r = R._per_pixel(o["rowscale"], HW)
                bound = r * bound + U * np.abs(R.act(v, a) * r)
            if with_res:
                bound = bound + U * np.abs(want)
            if family == "dyadic":
                _exact(np.abs(o["y"]).max() * np.abs(o["scale"]) * 2 + 4, 1 / 16)
            _check(family, name, ob.np((G, ipg * HW, C)), want, bound, ta == BF16)


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("shape,ty,ta", _bn_cases())
def test_chan_reduce(eng, shape, ty, ta, family):
    """k_chan_reduce, `part` summed over its bn_bwd_blocks(pix) blocks in float64.  Mode 0: (sum y, sum y^2) over n = pix values: n u
    sum|y| and (n + 1) u sum y^2.  Mode 1: (sum dyh, sum dyh xhat) with act 0 / 2, with and without rowscale and gate + dsv: n u sum|t|
    + sum of the terms' errors (`_dyh_terms`; xhat = (y - mean) istd within 2 u |xhat|, the product one more rounding).  Dyadic:
    act 2 enters with scale = shift = 0 (swish' = 1/2 exactly), dsv only where HW is a power of two.  The size of `part` comes from
    fm_debug_eff_ws and is asserted against the launch arithmetic.  Worst ratios: eff_parity.json (chan_reduce/random)."""
    G, ipg, HW, C = shape
    n = ipg * HW
    nblk = max(1, min(1024, -(-n // 64)))
    rs = np.random.RandomState(1100 + C + HW)
    o = _bn_operands(family, rs, shape, ty, ta, True)
    d = [ty, ta, G, n, HW, C, 0, 0]
    ws = eng.debug_eff_ws("chan_reduce", d)
    assert ws == [G * nblk * 2 * C, 0, 0, 0]
    tag = f"chan_reduce {shape}{ty}{ta}"
    pool = []
    yb = Buf(eng, o["y"].size, ty == BF16, o["y"], pool)
    pb = Buf(eng, ws[0], pool=pool)
    eng.debug_eff("chan_reduce", [None, yb.t, None, None, None, None, None, pb.t], d)
    _canaries(pool, tag)
    got = pb.np((G, nblk, 2, C)).astype(np.float64).sum(1)
    ref = R.chan_reduce(o["y"], 0)
    ay = np.abs(o["y"])
    if family == "dyadic":
        _exact(o["y"][0] ** 2, 1 / 4)
    _check(family, tag + " sum", got[:, 0], ref[:, 0], n * U * ay.sum(1))
    _check(family, tag + " sumsq", got[:, 1], ref[:, 1], (n + 1) * U * (ay * ay).sum(1))
    ab = Buf(eng, o["x"].size, ta == BF16, o["x"], pool)
    vb = {k: Buf(eng, o[k].size, False, o[k], pool) for k in ("mean", "istd", "rowscale", "gate", "dsv")}
    xh = (o["y"] - o["mean"][:, None, :]) * o["istd"][:, None, :]
    for a in (0, 2):
        for rowscaled, gated in ((False, False), (True, False), (False, True), (True, True)):
            name = f"{tag} act{a}{'*rs' if rowscaled else ''}{'+se' if gated else ''}"
            kw, sc, sh, t1, e1 = _dyh_terms(family, o, shape, a, rowscaled, gated)
            scb, shb = Buf(eng, G * C, False, sc, pool), Buf(eng, G * C, False, sh, pool)
            pb = Buf(eng, ws[0], pool=pool)
            d[6], d[7] = 1, a
            eng.debug_eff("chan_reduce", [ab.t, yb.t, vb["mean"].t, vb["istd"].t, scb.t if a == 2 else None, shb.t if a == 2 else None,
                                          vb["rowscale"].t if rowscaled else None, pb.t, vb["gate"].t if gated else None,
                                          vb["dsv"].t if gated else None], d)
            _canaries(pool, name)
            got = pb.np((G, nblk, 2, C)).astype(np.float64).sum(1)
            ref = R.chan_reduce(o["y"], 1, HW, a, d=o["x"], mean=o["mean"], istd=o["istd"], **kw)
            e2 = np.abs(xh) * e1 + np.abs(t1) * 2 * U * np.abs(xh) + U * np.abs(t1 * xh)
            if family == "dyadic":
                _exact(t1[0] * np.abs(xh[0]).max(), 2.0 ** -10)
            _check(family, name + " S1", got[:, 0], ref[:, 0], n * U * np.abs(t1).sum(1) + e1.sum(1))
            _check(family, name + " S2", got[:, 1], ref[:, 1], n * U * np.abs(t1 * xh).sum(1) + e2.sum(1))


@pytest.mark.parametrize("family", ["dyadic", "random"])
@pytest.mark.parametrize("mode", ["0", "3"], ids=["piece", "rows"])
@pytest.mark.parametrize("shape,ty,ta", _bn_cases())
def test_bnact_bwd_apply(eng, monkeypatch, shape, ty, ta, mode, family):
    """dy = ca dyh + cb y + cc through k_bnact_bwd_apply in both forms, act 0 / 2, with and without rowscale and gate + dsv; dz is
    stored as the activations are (ta), y and dy as the raw convolution output (ty).  Random bound: |ca| times the error of dyh
    (`_dyh_terms`) plus 3 u (|ca dyh| + |cb y| + |cc|) for the two products and two sums (+ half a bf16 ulp for a bf16 dy).
    Worst ratios: eff_parity.json (bnact_bwd_apply/random)."""
    G, ipg, HW, C = shape
    _set_rows(monkeypatch, mode)
    on = _arm_asserts(shape, ty, ta, mode, 2)
    rs = np.random.RandomState(1200 + C + HW)
    o = _bn_operands(family, rs, shape, ty, ta, True)
    d = [ty, ta, G, ipg * HW, HW, C, 0, 0]
    pool = []
    zb, yb = Buf(eng, o["x"].size, ta == BF16, o["x"], pool), Buf(eng, o["y"].size, ty == BF16, o["y"], pool)
    vb = {k: Buf(eng, o[k].size, False, o[k], pool) for k in ("ca", "cb", "cc", "rowscale", "gate", "dsv")}
    ca, cb, cc = (o[k][:, None, :] for k in ("ca", "cb", "cc"))
    for a in (0, 2):
        for rowscaled, gated in ((False, False), (True, False), (False, True), (True, True)):
            name = f"bnact_bwd_apply {shape}{ty}{ta}{'rows' if on else 'piece'} act{a}{'*rs' if rowscaled else ''}{'+se' if gated else ''}"
            kw, sc, sh, t1, e1 = _dyh_terms(family, o, shape, a, rowscaled, gated)
            scb, shb = Buf(eng, G * C, False, sc, pool), Buf(eng, G * C, False, sh, pool)
            ob = Buf(eng, o["y"].size, ty == BF16, pool=pool)
            d[7] = a
            eng.debug_eff("bnact_bwd_apply", [zb.t, yb.t, vb["ca"].t, vb["cb"].t, vb["cc"].t, scb.t if a == 2 else None,
                                              shb.t if a == 2 else None, vb["rowscale"].t if rowscaled else None, ob.t,
                                              vb["gate"].t if gated else None, vb["dsv"].t if gated else None], d)
            _canaries(pool, name)
            want = R.bnact_bwd_apply(o["x"], o["y"], o["ca"], o["cb"], o["cc"], HW, a, **kw)
            bound = np.abs(ca) * e1 + 3 * U * (np.abs(ca * t1) + np.abs(cb * o["y"]) + np.abs(cc))
            if family == "dyadic":
                _exact(np.abs(ca * t1)[0] + np.abs(cb * o["y"])[0] + np.abs(cc)[0], 2.0 ** -12)
            _check(family, name, ob.np((G, ipg * HW, C)), want, bound, ty == BF16)


# ---- contract -----------------------------------------------------------------------------------------------------------------------
def test_contract_errors(eng):
    """arguments outside a kernel's contract return FM_ERR_ARG before any launch: the outputs keep their NaN fill"""
    from fedmlp_amd._lib import FmError
    pool = []
    good = _dims(F32, 1, 4, 4, 8, 3, 1)
    x, w = Buf(eng, 128, False, np.ones(128), pool), Buf(eng, 72, False, np.ones(72), pool)
    y, rec, st = Buf(eng, 128, pool=pool), Buf(eng, 4096, pool=pool), Buf(eng, 128, pool=pool)

    def bad_dims(**kw):
        d = list(good)
        for k, v in kw.items():
            d[int(k[1:])] = v
        return d
    cases = [("dw_fwd", [x.t, w.t, y.t], bad_dims(d6=6)),               # C % 4
             ("dw_fwd", [x.t, w.t, y.t], bad_dims(d7=4)),               # K
             ("dw_fwd", [x.t, w.t, y.t], bad_dims(d7=7)),
             ("dw_fwd", [x.t, w.t, y.t], bad_dims(d1=0)),               # a dimension < 1
             ("dw_fwd", [x.t, w.t, y.t], bad_dims(d8=3)),               # stride
             ("dw_fwd", [x.t, w.t, y.t], bad_dims(d4=3)),               # Ho
             ("dw_fwd", [x.t, w.t, y.t], bad_dims(d9=3)),               # pad_t
             ("dw_fwd", [x.t, w.t, y.t], bad_dims(d0=2)),               # dt
             ("dw_fwd", [x.t, w.t, y.t], bad_dims(d12=0)),              # groups
             ("dw_fwd", [x.t, None, y.t], good),                        # missing operand
             ("dw_fwd", [x.t, w.t, y.t, x.t], good),                    # scale without shift
             ("dw_fwd", [x.t, w.t, y.t, None, None, rec.t], good),      # rec without a result
             ("dw_fwd", [x.t, w.t, y.t, None, None, None, st.t], good),  # a result without rec
             ("dw_dgrad", [x.t, w.t, y.t, x.t], good),                  # ye without the BN quad
             ("dw_dgrad", [x.t, w.t, None], good),
             ("dw_wgrad", [x.t, x.t, rec.t, None], good),
             ("se_fwd", [x.t, None, None, rec.t, w.t, w.t, w.t, w.t, y.t, y.t, None], [F32, 1, 4, 8, 2, 1, 0]),
             ("se_fwd", [x.t, None, None, rec.t, w.t, w.t, w.t, w.t, y.t, y.t, st.t], [F32, 1, 4, 6, 2, 1, 0]),       # C % 4
             ("se_fwd", [x.t, None, None, rec.t, w.t, w.t, w.t, w.t, y.t, y.t, st.t], [BF16, 1, 4, 12, 2, 1, 0]),     # bf16: C % 8
             ("se_fwd", [x.t, None, None, rec.t, w.t, w.t, w.t, w.t, y.t, y.t, st.t], [F32, 3, 4, 8, 2, 2, 0]),       # imgs % ipg
             ("se_fwd", [None, None, None, rec.t, w.t, w.t, w.t, w.t, y.t, y.t, st.t], [F32, 1, 4, 8, 2, 1, 0]),      # a missing, not pooled
             ("se_scale", [x.t, None, None, None, y.t], [F32, 1, 4, 8, 1, 1, 0]),
             ("se_bwd_bn1", [None] + [x.t] * 5 + [rec.t] + [x.t] * 4 + [y.t, y.t, y.t, st.t], [F32, 1, 4, 8, 2, 1, 0]),  # dout, no records
             ("se_wgrad", [x.t, x.t, x.t, x.t, rec.t, y.t], [1, 8, 49]),                                              # Cs > 48
             ("se_wgrad", [x.t, x.t, x.t, x.t, rec.t, None], [1, 8, 2]),
             # BN + activation passes: d = {ty, ta, groups, pix_per_group, HW, C, mode, act}; x: 128 elements = 1 x 16 x 8
             ("bnact_apply", [x.t, w.t, w.t, None, None, y.t], [F32, F32, 1, 16, 4, 6, 0, 0]),                          # C % 4
             ("bnact_apply", [x.t, w.t, w.t, None, None, y.t], [BF16, BF16, 1, 8, 4, 12, 0, 0]),                        # both bf16: C % 8
             ("bnact_apply", [x.t, w.t, w.t, None, None, y.t], [F32, F32, 1, 16, 3, 8, 0, 0]),                          # pix % HW
             ("bnact_apply", [x.t, w.t, w.t, None, None, y.t], [BF16, F32, 1, 16, 4, 8, 0, 0]),                         # (bf16, f32)
             ("bnact_apply", [x.t, w.t, w.t, None, None, y.t], [F32, 2, 1, 16, 4, 8, 0, 0]),                            # unknown type
             ("bnact_apply", [x.t, w.t, w.t, None, None, y.t], [F32, F32, 1, 16, 4, 8, 0, 3]),                          # act
             ("bnact_apply", [x.t, w.t, w.t, None, None, y.t], [F32, F32, 0, 16, 4, 8, 0, 0]),                          # a dimension < 1
             ("bnact_apply", [x.t, w.t, None, None, None, y.t], [F32, F32, 1, 16, 4, 8, 0, 0]),                         # shift missing
             ("bnact_apply", [x.t, w.t, w.t, None, None, None], [F32, F32, 1, 16, 4, 8, 0, 0]),                         # out missing
             ("chan_reduce", [None, x.t, None, None, None, None, None, None], [F32, F32, 1, 16, 4, 8, 0, 0]),           # part missing
             ("chan_reduce", [None, x.t, w.t, w.t, None, None, None, st.t], [F32, F32, 1, 16, 4, 8, 1, 0]),             # mode 1 without a
             ("chan_reduce", [x.t, x.t, w.t, w.t, None, None, None, st.t], [F32, F32, 1, 16, 4, 8, 1, 2]),              # act 2, no scale / shift
             ("chan_reduce", [x.t, x.t, w.t, w.t, None, None, None, st.t], [F32, F32, 1, 16, 4, 8, 1, 1]),              # act 1 in a backward pass
             ("chan_reduce", [x.t, x.t, w.t, w.t, None, None, None, st.t, x.t, None], [F32, F32, 1, 16, 4, 8, 1, 0]),   # gate without dsv
             ("chan_reduce", [None, x.t, None, None, None, None, None, st.t], [F32, F32, 1, 16, 4, 8, 2, 0]),           # mode
             ("bnact_bwd_apply", [x.t, x.t, w.t, w.t, w.t, None, None, None, y.t, None, x.t], [F32, F32, 1, 16, 4, 8, 0, 0]),   # dsv without gate
             ("bnact_bwd_apply", [x.t, x.t, w.t, w.t, w.t, w.t, None, None, y.t], [F32, F32, 1, 16, 4, 8, 0, 2]),       # act 2, no shift
             ("bnact_bwd_apply", [x.t, x.t, w.t, w.t, None, None, None, None, y.t], [F32, F32, 1, 16, 4, 8, 0, 0]),     # cc missing
             ("bnact_bwd_apply", [x.t, x.t, w.t, w.t, w.t, None, None, None, None], [F32, F32, 1, 16, 4, 8, 0, 0])]     # dy missing
    for op, ptrs, d in cases:
        with pytest.raises(FmError, match="bad argument"):
            eng.debug_eff(op, ptrs, d)
    with pytest.raises(FmError, match="bad argument"):
        eng.debug_eff_ws("dw_wgrad", bad_dims(d7=4))
    with pytest.raises(FmError, match="bad argument"):
        eng.debug_eff_ws("se_fwd", [F32, 1, 0, 8, 2, 1, 0])
    with pytest.raises(FmError, match="bad argument"):
        eng.debug_eff_ws("chan_reduce", [F32, F32, 1, 16, 3, 8, 0, 0])
    for b in (y, rec, st):
        assert np.isnan(b.np()).all(), "a refused call launched something"
    _canaries(pool, "contract")
    assert eng.debug_eff("dw_fwd", [x.t, w.t, y.t], good) is False and not np.isnan(y.np()).any()           # and the good call runs
