"""tests/tag_ref.py (the float64 / exact-integer yardstick of tests/test_tag_kernels_gpu.py) pinned to oracle/steps_ref.py on NaN-free
data and to the reference-generated tests/golden/kat.json; the data preconditions of the GPU file asserted on the generators it
imports (exactness of the dyadic families, the margin of every logit from the L / U decision band, the share of sign-undecided
similarities); and the comparisons shown to have teeth: each listed mutation, applied to a numpy fp32 emulation of the kernels, fails
the check the GPU file applies, while the unmutated emulation passes it.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import steps_ref as O
from tests import tag_ref as T
from tests import test_eff_kernels_gpu as GEN          # `_sig_err` (no GPU at import)
from tests.helpers import load_golden

f32 = np.float32


@pytest.fixture(scope="module")
def kat():
    return load_golden("kat.json")


# ---- the comparators of the GPU file -----------------------------------------------------------------------------------------------------
def _beyond(got, want, bound):
    """`_within`: a NaN (an unwritten element) or an element further from `want` than its bound"""
    got = np.asarray(got, np.float64)
    return bool(np.isnan(got).any() or (np.abs(got - want) > bound).any())


def _differs(got, want):
    """`_bits`: any element with different fp32 bits (signed zeros alike)"""
    got, want = np.asarray(got, np.float64).astype(f32), np.asarray(want, np.float64).astype(f32)
    return bool(((got.view(np.uint32) != want.view(np.uint32)) & ~((got == 0) & (want == 0))).any())


# ---- pinning -----------------------------------------------------------------------------------------------------------------------------
def test_cos_diff_pinned_to_the_oracle_and_the_kat(kat):
    rs = np.random.RandomState(0)
    for D, relu in ((512, False), (1280, True), (16, False)):
        f, proto = T.random_rows(rs, 37, D, relu), T.random_rows(rs, 10, D, relu)
        classes = [3, 0, 4, 3]
        sim, bound = T.cos_diff(f, proto, classes)
        for k, c in enumerate(classes):
            want = O.cosine_diff(torch.tensor(f), torch.tensor(proto[2 * c]), torch.tensor(proto[2 * c + 1])).numpy()
            assert np.abs(sim[k] - want).max() < 1e-13
        assert (bound > 0).all() and bound.max() < (D + 2) * T.U * 2.1         # tighter than the loose (D + 2) u per cosine
    g = kat["cosine"]
    proto = np.stack([np.asarray(g["p0"], np.float64), np.asarray(g["p1"], np.float64)])
    sim, _ = T.cos_diff(np.asarray(g["f"], np.float64), proto, [0])
    np.testing.assert_allclose(sim[0], np.asarray(g["sim"], np.float64), rtol=0, atol=1e-6)
    sim, _ = T.cos_diff([[1., 2, 3], [0, -1, .5], [2, 0, 0]], [[1., 0, 0], [0., 1, 1]], [0])
    np.testing.assert_allclose(sim[0], np.asarray(kat["cosine_survey"]["sim"], np.float64), rtol=0, atol=1e-6)


def test_cos_diff_zero_norms_are_nan():
    f = np.array([[1.0, 2.0], [0.0, 0.0], [3.0, -1.0]])
    proto = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [0.0, 0.0], [np.nan, 1.0], [1.0, 1.0]])
    sim, bound = T.cos_diff(f, proto, [0, 1, 2])
    assert np.isnan(sim[:, 1]).all() and np.isnan(sim[1]).all() and np.isnan(sim[2]).all()
    assert np.isfinite(sim[0, [0, 2]]).all() and np.isfinite(bound[0, [0, 2]]).all()


def test_select_pinned_to_the_oracle_and_the_kat(kat):
    g = kat["topk"]
    lst = g["lst"]
    n_clean, n_noise = sum(v >= 0 for v in lst), sum(v < 0 for v in lst)
    for kt in range(n_clean + 1):
        for kb in range(n_noise + 1):
            top, bot = T.select(lst, (kt + 0.5) / n_clean, (kb + 0.5) / n_noise)
            assert top == g["max"][str(kt)] and bot == g["min"][str(kb)]
    rs = np.random.RandomState(1)
    for family in T.SELECT_FAMILIES:
        for n in (1, 64, 257):
            v = T.select_values(family, rs, n)
            for ct, nt in ((0.005, 0.01), (0.3, 0.5), (1.0, 1.0)):
                top, bot = T.select(v, ct, nt)
                lst = [float(x) for x in v]
                kt, kb = int(1 * ct * int((v >= 0).sum())), int(1 * nt * int((v < 0).sum()))
                assert top == O.max_m_indices(lst, kt) and bot == O.min_n_indices(lst, kb), (family, n)
                pool = list(rs.permutation(1000)[:n])
                ctop, cbot = O.select_for_class(v, pool, ct, nt)
                assert ctop == [int(pool[j]) for j in top]
                assert cbot == ([int(pool[j]) for j in bot] if top else [])            # the clean-list-twice quirk is the caller's
    sims = rs.randint(-3, 4, (3, 50)) / 4.0
    pools = [None, [7, 3, 49, 0, 3], []]
    got = T.select_rows(sims, pools, 0.5, 1.0)
    assert got[0] == T.select(sims[0], 0.5, 1.0) and got[1] == T.select(sims[1][[7, 3, 49, 0, 3]], 0.5, 1.0) and got[2] == ([], [])


def test_select_contract_for_nan():
    """the reference gives garbage on NaN keys (the issue's example); ours: NaN elements are never selected and the others keep the
    order they have without them"""
    lst = [.1, float("nan"), .5, .3, float("nan"), .9]
    assert O.max_m_indices(lst, 3) == [0, 1, 2]                                 # why the reference is no guide here
    assert T.select(lst, 1.0, 1.0) == ([5, 2, 3, 0], [])
    assert T.select(lst, 0.75, 1.0) == ([5, 2, 3], [])
    assert T.select([float("nan"), -1.0, 2.0, -3.0, float("nan")], 1.0, 1.0) == ([2], [3, 1])
    assert T.select([float("nan")] * 4, 1.0, 1.0) == ([], [])
    assert T.select([-0.0, 0.0, -0.0], 1.0, 1.0) == ([0, 1, 2], [])
    assert [int(1 * t * 100) for t, _ in T.THRESHOLD_KS] == [k for _, k in T.THRESHOLD_KS]
    assert 0.29 * 100 < 29 and 0.57 * 100 < 57 and 0.07 * 100 > 7                 # a hair under / over an integer in double


def test_proto_pass_pinned_to_the_oracle():
    """integer-valued features: the oracle's fp32 accumulators are exact, so sums and means agree to the last fp32 bit of the oracle;
    normal features: to fp32 accuracy.  Labels hold 0.5, a class is active and negative, a class has no positives."""
    for family, tol in (("int", 0.0), ("normal", 2e-6)):
        batches, active, negative = T.proto_case(family, 24, 5, (0.3, 0.7), 4)
        clean = [(f, np.nan_to_num(z, nan=1.0, posinf=9.0, neginf=-9.0), y) for f, z, y in batches]    # the oracle pin is NaN-free
        tb = [(torch.tensor(f, dtype=torch.float32), torch.tensor(z, dtype=torch.float32), torch.tensor(y, dtype=torch.float32)) for f, z, y in clean]
        for guard in (False, True):
            p = T.proto_pass(clean, 5, active, negative, 0.3, 0.7, 1369, guard)
            t, proto = O.prototype_pass(tb, 5, active, negative, 0.3, 0.7, 1369, guard)
            np.testing.assert_array_equal(p.t, t)
            want = proto.numpy().astype(np.float64)
            if tol == 0.0:
                np.testing.assert_array_equal(T.finalized_f32(p.sum[0], p.count[0]), proto.numpy()[0])
                np.testing.assert_array_equal(T.finalized_f32(p.sum[9], p.count[9]), proto.numpy()[9])
            np.testing.assert_allclose(p.proto, want, rtol=2e-6 if tol == 0.0 else 0, atol=tol * np.abs(p.abs).max(), equal_nan=True)
            assert np.isnan(p.proto[1]).all() != guard and p.count[1] == 0
            assert not p.proto[[2, 3, 6, 7]].any() and p.count[2] == 0
            assert sum(p.count[0:2]) < 1369                                    # the 0.5 labels are in neither row


# ---- preconditions of the GPU file ---------------------------------------------------------------------------------------------------------
def test_sig_err_is_the_one_of_the_eff_file():
    z = np.linspace(-30, 30, 241)
    np.testing.assert_allclose(T.sig_err(z), GEN._sig_err(z), rtol=1e-12, atol=0)


@pytest.mark.parametrize("handle", list(T.HANDLES))
def test_cosine_preconditions(handle):
    """dyadic cases are exact in fp32 (and not trivially zero); at most 2 % of the random similarities are sign-undecided"""
    _, C, _, D = T.HANDLES[handle]
    for N in T.COS_N:
        f, proto = T.cos_case("dyadic", D, C, N, 100 + N)
        for classes in T.class_lists(C):
            assert T.dyadic_exact(f, proto, classes), (handle, N, classes)
        sim, _ = T.cos_diff(f, proto, T.class_lists(C)[1])
        assert np.count_nonzero(sim) > 0.4 * sim.size or N < 4
        assert (f[:, -1] != 0).all() and (proto[:, -1] != 0).all()            # the last column takes part in every product
        for family in ("normal", "relu"):
            f, proto = T.cos_case(family, D, C, N, 100 + N)
            for classes in T.class_lists(C):
                sim, bound = T.cos_diff(f, proto, classes)
                assert np.isfinite(sim).all() and T.undecided(sim, bound) <= 0.02, (handle, family, N)
                assert bound.max() < 1e-4 * np.abs(sim).max() or N < 4          # the bound resolves the values it judges


@pytest.mark.parametrize("handle", list(T.HANDLES))
def test_proto_preconditions(handle):
    """every finite logit but the exact edge z = 0 is further from the band than the fp32 sigmoid can err; the integer family's sums
    are exact in fp32 in any order; every membership case the GPU test names is present"""
    _, C, _, D = T.HANDLES[handle]
    for band in T.PROTO_BANDS:
        for family in ("int", "normal"):
            batches, active, negative = T.proto_case(family, D, C, band, 7)
            assert [b[0].shape[0] for b in batches] == list(T.PROTO_B)
            assert set(active) & set(negative) and C - 1 in active
            edges = 0
            for f, z, y in batches:
                zz = z[:, negative]
                fin = np.isfinite(zz) & (zz != 0)
                assert (T.logit_margin(zz[fin], *band) > 1.0).all()
                edges += int((zz == 0).sum()) + int(np.isnan(zz).sum()) + int(np.isinf(zz).sum())
                assert set(np.unique(y)) <= {0.0, 0.5, 1.0}
            assert edges == 4 * len(negative)
            p = T.proto_pass(batches, C, active, negative, *band, 1369, False)
            assert p.count[1] == 0 and min(p.count[2 * c] for c in active) > 0 and p.count[2 * (C - 1) + 1] > 0
            assert all(p.count[2 * c] + p.count[2 * c + 1] < 1369 for c in active)       # 0.5 labels
            assert all(0 < p.tcount[c] < 1369 for c in negative)
            if family == "int":
                assert np.array_equal(np.round(p.abs), p.abs) and p.abs.max() < 2 ** 24


def test_select_preconditions():
    rs = np.random.RandomState(2)
    v = T.hundred_hundred(rs)
    assert int((v >= 0).sum()) == 100 and int((v < 0).sum()) == 100 and len(np.unique(v)) < 100
    for family in T.SELECT_FAMILIES:
        v = T.select_values(family, rs, 257)
        assert not np.isnan(v).any()
        if family == "zeros":
            assert (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any()
        if family == "denormal":
            assert ((v != 0) & (np.abs(v) < np.finfo(f32).tiny)).any()
        if family == "distinct":
            assert len(np.unique(v)) == 257
        if family == "inf":
            assert np.isposinf(v).any() and np.isneginf(v).any()


# ---- fp32 emulations of the kernels, with their mutants -----------------------------------------------------------------------------------
def _wave_dot(a, b):
    """sum_d a[.., d] b[.., d] as cos_tag_kernel forms it: lane l adds its terms d = l, l + 64, .. in order, then a 6-level tree"""
    t = (a.astype(f32) * b.astype(f32)).astype(f32)
    pad = (-t.shape[-1]) % 64
    t = np.concatenate([t, np.zeros(t.shape[:-1] + (pad,), f32)], -1).reshape(t.shape[:-1] + (-1, 64))
    acc = np.zeros(t.shape[:-2] + (64,), f32)
    for s in range(t.shape[-2]):
        acc = (acc + t[..., s, :]).astype(f32)
    d = 32
    while d >= 1:
        acc = (acc + acc[..., np.arange(64) ^ d]).astype(f32)
        d >>= 1
    return acc[..., 0]


def _cos_emul(f, proto, classes, mut=None):
    f, proto = np.asarray(f, f32), np.asarray(proto, f32)
    D = f.shape[1]
    out = np.empty((len(classes), f.shape[0]), f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        fn = np.sqrt(_wave_dot(f, f))
        for k, c in enumerate(classes):
            p0, p1 = proto[2 * c], proto[(2 * c + 2) % proto.shape[0] if mut == "row" else 2 * c + 1]
            cs = []
            for p in (p0, p1):
                dot = _wave_dot(f[:, :D - 1], p[None, :D - 1]) if mut == "last" else _wave_dot(f, p[None])
                den = (fn * np.sqrt(_wave_dot(p, p))).astype(f32)
                if mut == "eps":
                    den = np.maximum(den, f32(1e-8))
                cs.append((dot * (f32(1.0) / den)).astype(f32))
            out[k] = cs[0] - cs[1]
    return out


def _select_emul(values, clean_thr, noise_thr, mut=None):
    """count_sign_kernel + fm_select_topk's k + rank_select_kernel, element by element in the order a GPU might run them"""
    v = np.asarray(values, f32)
    n = len(v)
    n_clean = int((v > 0).sum()) if mut == "gt" else int((v >= 0).sum())
    n_noise = int((v < 0).sum())
    if mut == "round":
        kt, kb = int(round(clean_thr * n_clean)), int(round(noise_thr * n_noise))
    elif mut == "f32":
        kt, kb = int(f32(clean_thr) * f32(n_clean)), int(f32(noise_thr) * f32(n_noise))
    else:
        kt, kb = int(1 * clean_thr * n_clean), int(1 * noise_thr * n_noise)
    top, bot = [-1] * kt, [-1] * kb
    order = sorted(range(n), key=lambda i: bool(np.isnan(v[i])))            # the NaN elements' stores land last
    for i in order:
        if np.isnan(v[i]) and mut != "nan":
            continue
        tie = (np.arange(n) > i) if mut == "last" else (np.arange(n) < i)
        with np.errstate(invalid="ignore"):
            rd = int(((v > v[i]) | ((v == v[i]) & tie)).sum())
            ra = int(((v < v[i]) | ((v == v[i]) & tie)).sum())
        if rd < kt:
            top[rd] = i
        if ra < kb:
            bot[ra] = i
    return top, bot


def _proto_emul(batches, C, active, negative, L, U_, n_local, guard, mut=None):
    D = batches[0][0].shape[1]
    psum, pcnt, tcnt = np.zeros((2 * C, D), f32), [0] * (2 * C), [0] * C
    L, U_ = f32(L), f32(U_)
    for feat, z, y in batches:
        feat, z, y = np.asarray(feat, f32), np.asarray(z, f32), np.asarray(y, f32)
        for c in active:
            for v in (0, 1):
                m = (y[:, c] != 0) if (mut == "ne0" and v == 1) else (y[:, c] == f32(v))
                s = np.zeros(D, f32)
                for row in feat[m]:
                    s = (s + row).astype(f32)
                psum[2 * c + v] = (psum[2 * c + v] + s).astype(f32)
                pcnt[2 * c + v] += int(m.sum())
        with np.errstate(over="ignore", invalid="ignore"):
            p = (f32(1) / (f32(1) + np.exp(-z).astype(f32))).astype(f32)
            for c in negative:
                lo = (p[:, c] <= L) if mut == "le" else (p[:, c] < L)
                tcnt[c] += int((lo | (p[:, c] > U_)).sum())
    proto = psum.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in active:
            for r in (2 * c, 2 * c + 1):
                if not (guard and pcnt[r] == 0):
                    proto[r] = proto[r] / f32(pcnt[r])
    return np.array(tcnt, np.float64) / float(n_local), proto, pcnt


# ---- the checks have teeth -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (512, 1280))
def test_cosine_checks_pass_the_emulation_and_reject_the_mutants(D):
    C, N = 5, 37
    classes = T.class_lists(C)[1]
    fd, pd = T.cos_case("dyadic", D, C, N, 5)
    wd, _ = T.cos_diff(fd, pd, classes)
    assert not _differs(_cos_emul(fd, pd, classes), wd)
    worst = 0.0
    for family in ("normal", "relu"):
        f, p = T.cos_case(family, D, C, N, 5)
        want, bound = T.cos_diff(f, p, classes)
        got = _cos_emul(f, p, classes)
        assert not _beyond(got, want, bound)
        worst = max(worst, float((np.abs(got - want) / bound).max()))
        for mut in ("last", "row"):
            assert _beyond(_cos_emul(f, p, classes, mut), want, bound), (family, mut)
        # scaling: bit-identical for the true form; the zero row: NaN for the true form, a number under an eps clamp
        for sc in (2.0 ** 20, 2.0 ** -20):
            assert np.array_equal(_cos_emul(f * sc, p, classes), got)
        fz = f.copy()
        fz[3] = 0.0
        assert np.isnan(_cos_emul(fz, p, classes)[:, 3]).all() and not np.isnan(_cos_emul(fz, p, classes, "eps")[:, 3]).any()
    print(f"D = {D}: the fp32 emulation's worst error / bound = {worst:.4f}")
    assert worst < 0.25                                                     # the bound is a worst case: real rounding stays far inside
    for mut in ("last", "row"):
        assert _differs(_cos_emul(fd, pd, classes, mut), wd), mut


SEL = ((0.29, 0.57), (0.07, 1.0), (1.0, 0.29), (0.005, 0.005))


def test_selection_checks_pass_the_emulation_and_reject_the_mutants():
    rs = np.random.RandomState(3)
    hh = T.hundred_hundred(rs)
    zeros = T.select_values("zeros", rs, 257)
    ties = T.select_values("ties", rs, 257)
    nan1 = T.with_nans(T.select_values("distinct", rs, 64), [17])
    for v in (hh, zeros, ties, nan1, T.with_nans(ties, [0, 256, 100])):
        for ct, nt in SEL:
            assert _select_emul(v, ct, nt) == T.select(v, ct, nt)

    def caught(mut, v, thrs=SEL):
        return any(_select_emul(v, ct, nt, mut) != T.select(v, ct, nt) for ct, nt in thrs)

    assert caught("gt", zeros) and not caught("gt", hh[hh != 0])            # `>` for `>=`: seen through the +-0.0 family alone
    assert caught("last", ties) and caught("last", zeros)
    assert caught("round", hh, ((0.29, 0.57),)) and caught("f32", hh, ((0.29, 0.29),))
    assert int(f32(0.29) * f32(100)) == 29 and int(0.29 * 100) == 28
    assert caught("nan", nan1, ((1.0, 1.0),)) and caught("nan", T.with_nans(hh, [0]), ((0.29, 0.57),))


def test_prototype_checks_pass_the_emulation_and_reject_the_mutants():
    C, D, n_local = 5, 40, 1369
    for band in T.PROTO_BANDS:
        for family in ("int", "normal"):
            batches, active, negative = T.proto_case(family, D, C, band, 11)
            p = T.proto_pass(batches, C, active, negative, *band, n_local, False)
            t, proto, cnt = _proto_emul(batches, C, active, negative, *band, n_local, False)
            assert np.array_equal(t, p.t) and cnt == p.count
            rows = [r for c in active for r in (2 * c, 2 * c + 1) if p.count[r]]
            if family == "int":
                for r in rows:
                    assert not _differs(proto[r], T.finalized_f32(p.sum[r], p.count[r]))
            else:
                assert not _beyond(proto[rows], p.proto[rows], T.proto_bound(p, len(batches))[rows])
            t, proto, cnt = _proto_emul(batches, C, active, negative, *band, n_local, False, "ne0")
            assert cnt != p.count                                              # label != 0 for == 1: the 0.5 labels enter row 1
            r = 2 * (C - 1) + 1
            if family == "int":
                assert _differs(proto[r], T.finalized_f32(p.sum[r], p.count[r]))
            else:
                assert _beyond(proto[r], p.proto[r], T.proto_bound(p, len(batches))[r])
            t, _, _ = _proto_emul(batches, C, active, negative, *band, n_local, False, "le")
            assert np.array_equal(t, p.t) == (band[0] != 0.5)                  # p <= L for p < L: seen at z = 0, L = 0.5 alone
