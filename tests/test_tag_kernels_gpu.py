"""Kernel-level parity of the kernels that give FedMLP its name -- proto_accumulate_kernel, cos_tag_kernel, count_sign_kernel,
rank_select_kernel, count_sign_rows_kernel, rank_select_rows_kernel (the tail of csrc/heads.hip) and the host part of
fm_proto_finalize -- through fm_proto_*, fm_cos_tag, fm_select_topk and fm_select_topk_rows, which take caller tensors (no debug
hook), against the float64 / exact-integer restatements of tests/tag_ref.py (pinned to oracle/steps_ref.py and the reference's
kat.json by tests/test_tag_ref_cpu.py, which also asserts the data preconditions relied on here and shows that every comparison
below rejects a subtly wrong kernel).  These kernels make DISCRETE decisions (which samples get pseudo-labels), so selections and
counts are compared exactly.

Three handles (tag_ref.HANDLES): ResNet-18 C = 5 (D = 512), EfficientNet-B0 fp32 C = 5 (D = 1280), ResNet-18 C = 32 (FM_MAX_CLASSES:
the by-value ClassVec full, every class listed in one fm_cos_tag call).

COSINE.  N in {1, 3, 4, 5, 257} (4 samples per block: below, at, over one block; 65 blocks with a ragged last one).
 DYADIC: entries in {0, +-2^k} with 4^m nonzeros per row -- norms are powers of two, dot products small integers times a power of
 two: sim must equal float64 BIT FOR BIT whatever the order or the formula.
 RANDOM (standard normal, and its ReLU: real features are non-negative): |got - ref| <= bound, derived from the kernel as written,
 in units of u = 2^-24.  A dot product or squared norm of D terms passes D/64 per-lane additions, 6 tree levels and 1 product:
 g = (D/64 + 7) u times sum|terms| (15 u at D = 512, 27 u at D = 1280; an fma only removes a rounding).  A norm is a square root of
 such a sum: g/2 + u, and sqrtf contributes twice (|f| and |p|); then one product |f| |p| (u), one reciprocal (u), one multiply (u):
 each cosine is within g sum|f p| / (|f| |p|) + (g + 5 u) |cos|; the subtraction adds u |sim|.  No measured tolerance enters.  The
 library is built with `hipcc -O3` and no fast-math flag (the Makefile's one compile line), which keeps fp32 division and square
 root correctly rounded, as the count assumes.  Wherever |ref| > bound the SIGN (the clean / noise decision) must agree; at most 2 %
 of the elements may be undecided (a condition on the generators, asserted on the CPU side too).
 Scaling all features by 2^20 or 2^-20 leaves sim bit-identical.  An all-zero feature row gives NaN in every listed class and leaves
 its neighbours' bits alone; a NaN or all-zero prototype pair gives a NaN row and leaves the other classes' bits alone.
 sim sits between NaN margins and is pre-filled with NaN: exactly n_cls x N elements are written.

PROTOTYPES.  One pass = five fm_proto_accumulate calls of B = 1, 255, 256, 257, 600 rows (the counting loops stride by 256).
 Labels hold 0, 1 and a 0.5 that must land in neither row; class 2 is active AND negative; class 0 is active without positives
 (0/0 = NaN unguarded, the zero row under the guard); the last class is active; inactive rows stay exactly zero.
 INTEGER-valued features: every row sum is exact in any order, so the finalized rows are np.float32(sum) / np.float32(count) bit for
 bit (a wrong count shows as well).  RANDOM features: within (n_rows + n_calls + 1) u sum|f| / count of float64, plus u |mean| for
 the division.  t = count / n_local is compared exactly with the integer reference: every logit is further from the L / U band than
 fp32 sigmoid can err (tag_ref.logit_margin, from `_sig_err`), plus the exact edges z = 0 with L = 0.5 / U = 0.5 (not counted), +-inf
 (counted) and NaN (not counted).  fm_proto_reset between the passes must clear all three accumulators.

SELECTION.  fm_select_topk and fm_select_topk_rows, EACH against tag_ref.select (not against one another), N and pool sizes in
 {1, 63, 64, 255, 256, 257, 1025} (256 threads per block), value families distinct / heavy ties / mixed +-0.0 / +-inf / denormals /
 all >= 0 / all < 0, thresholds whose double product thr * count sits a hair under or over an integer (100 non-negatives and 100
 negatives: 0.29 -> 28, 0.57 -> 56, 0.07 -> 7), 1.0 and one that gives k = 0; pools as permutations, a reversed whole row, a short pool
 beside a long one, an empty pool between others, a stride larger than every pool, a fully-NaN class.  PARTLY-NaN rows (an all-zero
 feature row makes one): NaN elements are never selected and the rest is ranked as if they were absent; two successive calls agree.
 The host pick tables are pre-filled with a sentinel: nothing beyond the reported counts is written.

Bit-exact check counts and worst error / bound ratios go to tag_parity.json beside the other parity reports."""
import ctypes as C

import numpy as np
import pytest
import torch

from fedmlp_amd import _lib, spec
from tests import tag_ref as T
from tests.test_eff_kernels_gpu import Buf, _canaries, _parity

pytestmark = pytest.mark.gpu

REPORT = {}
_bits, _within, _ = _parity(REPORT, "tag_parity.json")
SENT = -7                   # host pick tables are pre-filled with it
THRS = ((0.29, 0.57), (1.0, 1.0), (0.005, 0.005))


@pytest.fixture(scope="module")
def engs():
    """the three handles, built on first use: owners of the accumulators and of the stream the launches run on"""
    from fedmlp_amd.engine import Engine
    made = {}

    def get(name):
        if name not in made:
            model, n_cls, hw, D = T.HANDLES[name]
            e = Engine(model, n_cls, hw, hw, 8)
            flat, cnt = spec.init_state(model, n_cls, 3)
            e.set_state(flat, cnt)
            assert e.feature_dim == D
            made[name] = e
        return made[name]

    yield get
    for e in made.values():
        e.close()


def _dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(e.device)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ---- cosine tagging ------------------------------------------------------------------------------------------------------------------------
def _cos(e, f, proto, classes, name):
    """one fm_cos_tag launch through the C ABI into a caller buffer between NaN margins -> sim [n_cls, N]"""
    N, n_cls = f.shape[0], len(classes)
    pool = []
    fb, pb, sb = Buf(e, f.size, init=f, pool=pool), Buf(e, proto.size, init=proto, pool=pool), Buf(e, n_cls * N, pool=pool)
    cls = (C.c_int32 * n_cls)(*[int(c) for c in classes])
    e._enqueue()
    _lib.check(e.lib.fm_cos_tag(e.h, C.c_void_p(fb.t.data_ptr()), N, C.c_void_p(pb.t.data_ptr()), cls, n_cls, C.c_void_p(sb.t.data_ptr())))
    torch.cuda.synchronize()
    _canaries(pool, name)
    got = sb.np()
    assert np.isnan(got[n_cls * N:]).all(), f"{name}: more than n_cls x N elements were written"
    return got[:n_cls * N].reshape(n_cls, N)


@pytest.mark.parametrize("family", T.COS_FAMILIES)
@pytest.mark.parametrize("handle", list(T.HANDLES))
def test_cos_tag(engs, handle, family):
    e = engs(handle)
    _, n_classes, _, D = T.HANDLES[handle]
    for N in T.COS_N:
        f, proto = T.cos_case(family, D, n_classes, N, 100 + N)
        for i, classes in enumerate(T.class_lists(n_classes)):
            name = f"cos[{handle},N{N},list{i}] {family}"
            got = _cos(e, f, proto, classes, name)
            want, bound = T.cos_diff(f, proto, classes)
            if family == "dyadic":
                _bits(name, got, want)
                continue
            _within(name, got, want, bound, family)
            assert T.undecided(want, bound) <= 0.02, name
            decided = np.abs(want) > bound
            assert (np.signbit(got[decided]) == np.signbit(want[decided])).all(), f"{name}: a decided sign differs"


@pytest.mark.parametrize("handle", list(T.HANDLES))
def test_cos_tag_scaling_is_bit_identical(engs, handle):
    e = engs(handle)
    _, n_classes, _, D = T.HANDLES[handle]
    classes = T.class_lists(n_classes)[1]
    for family in ("normal", "relu"):
        f, proto = T.cos_case(family, D, n_classes, 257, 31)
        base = _cos(e, f, proto, classes, "cos_scale")
        assert np.isfinite(base).all()
        for sc in (2.0 ** 20, 2.0 ** -20):
            assert _same_bits(_cos(e, f * sc, proto, classes, "cos_scale"), base), (handle, family, sc)


@pytest.mark.parametrize("handle", list(T.HANDLES))
def test_cos_tag_zero_and_nan_rows(engs, handle):
    e = engs(handle)
    _, n_classes, _, D = T.HANDLES[handle]
    classes = T.class_lists(n_classes)[1]
    f, proto = T.cos_case("relu", D, n_classes, 9, 77)
    base = _cos(e, f, proto, classes, "cos_zero")
    # all-zero feature rows: the first of a block, the last of a block, the last sample (alone in its block)
    fz = f.copy()
    fz[[0, 3, 8]] = 0.0
    got = _cos(e, fz, proto, classes, "cos_zero")
    assert np.isnan(got[:, [0, 3, 8]]).all() and _same_bits(np.delete(got, [0, 3, 8], 1), np.delete(base, [0, 3, 8], 1))
    want, _ = T.cos_diff(fz, proto, classes)
    assert np.array_equal(np.isnan(want), np.isnan(got))
    # a NaN element in one prototype row of class a, an all-zero pair for class b: their rows are NaN, every other class keeps its bits
    a, b = classes[0], classes[-1]
    pz = proto.copy()
    pz[2 * a + 1, D // 2] = np.nan
    pz[2 * b:2 * b + 2] = 0.0
    got = _cos(e, f, pz, classes, "cos_nan_proto")
    bad = np.array([c in (a, b) for c in classes])
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all() and _same_bits(got[~bad], base[~bad])
    want, _ = T.cos_diff(f, pz, classes)
    assert np.array_equal(np.isnan(want), np.isnan(got))


# ---- prototype pass and finalize -------------------------------------------------------------------------------------------------------------
def _mask(n, members):
    return [1.0 if c in members else 0.0 for c in range(n)]


def _proto_run(e, batches, n_classes, active, negative, band, n_local, guard):
    for f, z, y in batches:
        e.proto_accumulate(_dev(e, f), _dev(e, z), _dev(e, y), _mask(n_classes, active), _mask(n_classes, negative), *band)
    return e.proto_finalize(guard, n_local, _mask(n_classes, active))


@pytest.mark.parametrize("family", ("int", "normal"))
@pytest.mark.parametrize("handle", list(T.HANDLES))
def test_proto_pass(engs, handle, family):
    e = engs(handle)
    _, n_classes, _, D = T.HANDLES[handle]
    n_local = sum(T.PROTO_B)
    for seed, (band, guard) in enumerate(zip(T.PROTO_BANDS, (False, True))):
        batches, active, negative = T.proto_case(family, D, n_classes, band, 40 + seed)
        e.proto_reset()
        t, proto = _proto_run(e, batches, n_classes, active, negative, band, n_local, guard)
        p = T.proto_pass(batches, n_classes, active, negative, *band, n_local, guard)
        name = f"proto[{handle},L{band[0]},guard{int(guard)}] {family}"
        print(name, "t counts", p.tcount, "row counts", [p.count[2 * c + v] for c in active for v in (0, 1)])
        assert np.array_equal(t, p.t), (name, t * n_local, p.tcount)
        idle = [r for c in range(n_classes) if c not in active for r in (2 * c, 2 * c + 1)]
        assert not proto[idle].any(), f"{name}: an inactive row was written"
        assert p.count[1] == 0
        if guard:
            assert not proto[1].any(), f"{name}: the guarded empty row is not zero"
        else:
            assert np.isnan(proto[1]).all(), f"{name}: 0 / 0 is not NaN"
        rows = [r for c in active for r in (2 * c, 2 * c + 1) if p.count[r]]
        assert len(rows) == 2 * len(active) - 1
        if family == "int":
            _bits(name, proto[rows], np.stack([T.finalized_f32(p.sum[r], p.count[r]) for r in rows]))
        else:
            _within(name, proto[rows], p.proto[rows], T.proto_bound(p, len(batches))[rows], family)


def test_proto_reset_clears_all_three_accumulators(engs):
    e = engs("r18")
    n_classes, D = 5, 512
    band = T.PROTO_BANDS[1]
    batches, active, negative = T.proto_case("int", D, n_classes, band, 9)
    e.proto_reset()
    t, proto = _proto_run(e, batches[:3], n_classes, active, negative, band, 512, False)
    assert t[negative].all() and np.isfinite(proto[0]).all() and proto[0].any()
    e.proto_reset()
    t, proto = e.proto_finalize(False, 512, _mask(n_classes, active))
    assert not t.any(), "the t counts survived fm_proto_reset"
    rows = [r for c in active for r in (2 * c, 2 * c + 1)]
    assert np.isnan(proto[rows]).all(), "row sums or row counts survived fm_proto_reset (0 / 0 must be NaN)"
    t, proto = e.proto_finalize(True, 512, _mask(n_classes, active))
    assert not proto.any() and not t.any()
    # and a pass after the reset is a pass on its own
    t, proto = _proto_run(e, batches[3:], n_classes, active, negative, band, 857, True)
    p = T.proto_pass(batches[3:], n_classes, active, negative, *band, 857, True)
    assert np.array_equal(t, p.t)
    rows = [r for r in rows if p.count[r]]
    _bits("proto_reset[r18] int", proto[rows], np.stack([T.finalized_f32(p.sum[r], p.count[r]) for r in rows]))


# ---- selection -------------------------------------------------------------------------------------------------------------------------------
def _topk(e, v, ct, nt):
    """fm_select_topk through the C ABI with sentinel-filled pick tables of N entries"""
    n = len(v)
    sim = _dev(e, v)
    cap = max(n, 1)
    top, bot = (C.c_int32 * cap)(*([SENT] * cap)), (C.c_int32 * cap)(*([SENT] * cap))
    nt_, nb_ = C.c_int32(), C.c_int32()
    e._enqueue()
    _lib.check(e.lib.fm_select_topk(e.h, C.c_void_p(sim.data_ptr()), n, float(ct), float(nt), cap, top, C.byref(nt_), bot, C.byref(nb_)))
    assert all(x == SENT for x in top[nt_.value:]) and all(x == SENT for x in bot[nb_.value:]), "written beyond the reported count"
    return list(top[:nt_.value]), list(bot[:nb_.value])


def _rows(e, sims, pools, ct, nt, stride=None):
    """fm_select_topk_rows through the C ABI: pools[k] = positions into row k in pool order (None = the whole row, allowed only when
    every pool is None), any stride >= the longest pool"""
    sims = np.asarray(sims, np.float32)
    n_cls, N = sims.shape
    sizes = [N if p is None else len(p) for p in pools]
    rows = None
    if any(p is not None for p in pools):
        stride = max(max(sizes), 1) if stride is None else stride
        flat = np.full((n_cls, stride), 0, np.int32)
        for k, p in enumerate(pools):
            flat[k, :sizes[k]] = np.arange(N) if p is None else np.asarray(p, np.int32)
        rows = flat.ctypes.data_as(C.POINTER(C.c_int32))
    else:
        stride = N
    cap = int(max(ct, nt, 0.0) * max(sizes)) + 1
    pn = (C.c_int32 * n_cls)(*sizes)
    top, bot = (C.c_int32 * (n_cls * cap))(*([SENT] * (n_cls * cap))), (C.c_int32 * (n_cls * cap))(*([SENT] * (n_cls * cap)))
    nt_, nb_ = (C.c_int32 * n_cls)(), (C.c_int32 * n_cls)()
    sd = _dev(e, sims)
    e._enqueue()
    _lib.check(e.lib.fm_select_topk_rows(e.h, C.c_void_p(sd.data_ptr()), N, n_cls, rows, pn, stride, float(ct), float(nt), cap, top, nt_,
                                         bot, nb_))
    out = []
    for k in range(n_cls):
        assert all(x == SENT for x in top[k * cap + nt_[k]:(k + 1) * cap]) and all(x == SENT for x in bot[k * cap + nb_[k]:(k + 1) * cap]), \
            "written beyond the reported count"
        out.append((list(top[k * cap:k * cap + nt_[k]]), list(bot[k * cap:k * cap + nb_[k]])))
    return out


@pytest.mark.parametrize("family", T.SELECT_FAMILIES)
def test_select_value_families(engs, family):
    """both entry points against the reference at every size; the rows call takes the seven sizes as seven pools of one launch"""
    e = engs("r18")
    rs = np.random.RandomState(11)
    nmax = max(T.SELECT_N)
    sims = np.stack([T.select_values(family, rs, nmax) for _ in T.SELECT_N])
    pools = [[int(r) for r in rs.permutation(nmax)[:n]] for n in T.SELECT_N]
    for ct, nt in THRS:
        for k, n in enumerate(T.SELECT_N):
            v = sims[k][pools[k]]
            assert _topk(e, v, ct, nt) == T.select(v, ct, nt), (family, n, ct, nt)
        assert _rows(e, sims, pools, ct, nt) == T.select_rows(sims, pools, ct, nt), (family, ct, nt)
    whole = [None] * len(T.SELECT_N)
    assert _rows(e, sims, whole, 1.0, 1.0) == T.select_rows(sims, whole, 1.0, 1.0), family


def test_select_thresholds_a_hair_from_an_integer(engs):
    """k = int(thr * count) in double, truncated: 100 values >= 0 and 100 < 0"""
    e = engs("r18c32")
    rs = np.random.RandomState(12)
    v = T.hundred_hundred(rs)
    sims = np.full((2, 257), 0.5, np.float32)
    pool = [int(r) for r in rs.permutation(257)[:200]]
    sims[1, pool] = v
    for thr, k in T.THRESHOLD_KS:
        for ct, nt in ((thr, thr), (thr, 1.0), (1.0, thr)):
            top, bot = _topk(e, v, ct, nt)
            assert (len(top), len(bot)) == (k if ct == thr else 100, k if nt == thr else 100), (thr, len(top), len(bot))
            assert (top, bot) == T.select(v, ct, nt)
            got = _rows(e, sims, [pool[:50], pool], ct, nt)
            assert got == T.select_rows(sims, [pool[:50], pool], ct, nt) and got[1] == (top, bot)


def test_select_rows_pools(engs):
    e = engs("r18c32")
    rs = np.random.RandomState(13)
    N = 300
    sims = (rs.randint(-6, 7, (7, N)) / 8.0).astype(np.float32)            # heavy ties
    sims[5] = np.nan                                                        # a class nobody annotates
    pools = [[int(r) for r in rs.permutation(N)],                           # a permutation of the whole row
             list(range(N - 1, -1, -1)),                                    # the reversed whole row
             [int(r) for r in rs.permutation(N)[:3]],                       # a short pool: maxn comes from another class
             [],                                                            # an empty pool between non-empty ones
             [int(r) for r in rs.permutation(N)[:257]],
             list(range(N)),                                                # fully NaN
             [int(r) for r in rs.randint(0, N, 64)]]                        # positions may repeat
    for ct, nt in THRS + ((0.3, 0.5),):
        want = T.select_rows(sims, pools, ct, nt)
        assert want[3] == ([], []) and want[5] == ([], [])
        assert _rows(e, sims, pools, ct, nt) == want, (ct, nt)
        assert _rows(e, sims, pools, ct, nt, stride=N + 37) == want, (ct, nt, "stride")
    # all 32 classes of the full-width handle in one call
    sims = (rs.randint(-6, 7, (32, 65)) / 8.0).astype(np.float32)
    pools = [[int(r) for r in rs.permutation(65)[:1 + 2 * k]] for k in range(32)]
    assert _rows(e, sims, pools, 0.57, 0.29) == T.select_rows(sims, pools, 0.57, 0.29)


NAN_CASES = {"one": lambda n: [n // 2], "several": lambda n: sorted({1 % n, n // 3, n // 2, n - 2 if n > 1 else 0}),
             "first": lambda n: [0], "last": lambda n: [n - 1], "first_and_last": lambda n: [0, n - 1]}


@pytest.mark.parametrize("where", list(NAN_CASES))
def test_select_partly_nan_rows(engs, where):
    """a NaN similarity (an all-zero feature row makes one) is never selected and is ranked nowhere: the picks are those of the row
    without its NaN elements, mapped back to positions, from both entry points, and the same on a second call"""
    e = engs("r18")
    rs = np.random.RandomState(14)
    sizes = (5, 64, 257, 1025)
    nmax = max(sizes)
    for family in ("distinct", "ties"):
        rows = [T.with_nans(T.select_values(family, rs, n), NAN_CASES[where](n)) for n in sizes]
        sims = np.zeros((len(sizes), nmax), np.float32)
        pools = []
        for k, r in enumerate(rows):
            p = [int(x) for x in rs.permutation(nmax)[:len(r)]]
            sims[k, p] = r
            pools.append(p)
        for ct, nt in ((1.0, 1.0), (0.29, 0.57)):
            for r in rows:
                want = T.select(r, ct, nt)
                assert all(not np.isnan(r[i]) for i in want[0] + want[1])
                first, second = _topk(e, r, ct, nt), _topk(e, r, ct, nt)
                assert first == want, (where, family, len(r), ct, nt)
                assert second == first
            want = T.select_rows(sims, pools, ct, nt)
            first, second = _rows(e, sims, pools, ct, nt), _rows(e, sims, pools, ct, nt)
            assert first == want, (where, family, ct, nt)
            assert second == first
