"""Float64 / exact-integer restatements of the prototype pass, cosine tagging and clean / noisy selection (the tail of csrc/heads.hip
and fm_proto_finalize), the yardstick of tests/test_tag_kernels_gpu.py, with the operand generators that file uses.  Written from
the formulas; tests/test_tag_ref_cpu.py pins it to oracle/steps_ref.py and to the reference-generated tests/golden/kat.json.  numpy
only, no GPU.

The one place where the contract is OURS and not the reference's: a NaN similarity is never selected.  The pick is what the row gives
with its NaN elements removed, mapped back to positions (Python's sorted() with NaN keys returns garbage, so the reference is no
guide there)."""
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff


def sigmoid(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(v))
        return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sig_err(v):
    """|fp32 sigmoid - float64 sigmoid| for 1 / (1 + exp(-v)) with exp within 1 ulp and argument error 2 u |v|: the `_sig_err` of
    tests/test_eff_kernels_gpu.py restated (tests/test_tag_ref_cpu.py asserts the two agree)"""
    s = sigmoid(v)
    return s * ((1.0 - s) * (2.0 + 2.0 * np.abs(v)) + 3.0) * U


# ---- prototype + t pass ----------------------------------------------------------------------------------------------------------------
def proto_pass(batches, C, active, negative, L, U_, n_local, guard):
    """batches = [(feat [b, D], logits [b, C], labels [b, C])]; active / negative = lists of class indices; L, U_ as the kernel gets
    them (fp32).  Row 2c + v of an active class c sums the features whose label[c] == v EXACTLY (0.5 is in neither row); t counts
    p < L or p > U_ over the negative classes (a NaN logit in neither).  -> sum, abs (sum|f|), count, tcount, t = tcount / n_local,
    proto = sum / count (0 / 0 = NaN; under `guard` a row without members stays zero)."""
    D = np.asarray(batches[0][0]).shape[1]
    L, U_ = float(np.float32(L)), float(np.float32(U_))
    s, a = np.zeros((2 * C, D)), np.zeros((2 * C, D))
    cnt, tc = [0] * (2 * C), [0] * C
    for feat, logits, labels in batches:
        feat, logits, labels = (np.asarray(t, np.float64) for t in (feat, logits, labels))
        p = sigmoid(logits)
        for c in active:
            for v in (0, 1):
                m = labels[:, c] == float(v)
                cnt[2 * c + v] += int(m.sum())
                s[2 * c + v] += feat[m].sum(0)
                a[2 * c + v] += np.abs(feat[m]).sum(0)
        for c in negative:
            with np.errstate(invalid="ignore"):
                tc[c] += int(((p[:, c] < L) | (p[:, c] > U_)).sum())
    proto = s.copy()
    for c in active:
        for r in (2 * c, 2 * c + 1):
            if guard and cnt[r] == 0:
                continue
            proto[r] = s[r] / cnt[r] if cnt[r] else np.nan
    return SimpleNamespace(sum=s, abs=a, count=cnt, tcount=tc, t=np.array(tc, np.float64) / float(n_local), proto=proto)


def finalized_f32(row_sum, count):
    """what fm_proto_finalize stores when the fp32 row sum is exact: one fp32 division"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(row_sum, np.float64).astype(np.float32) / np.float32(count)


def proto_bound(p, n_calls):
    """|fp32 finalized row - p.proto|: a row sum is n_rows additions inside the calls (n_rows = the row's count), one per call onto
    the accumulator, and one to spare: (n_rows + n_calls + 1) u sum|f| before the division, then one rounding for it"""
    n = np.array(p.count, np.float64)[:, None]
    return ((n + n_calls + 1) * U * p.abs / np.maximum(n, 1.0)) * (1 + U) + U * np.abs(np.nan_to_num(p.proto))


# ---- cosine tagging --------------------------------------------------------------------------------------------------------------------
def cos_gamma(D):
    """roundings a term of a D-term dot product / squared norm passes in cos_tag_kernel: D / 64 per-lane additions, 6 tree levels,
    1 product (an fma only removes one)"""
    return (math.ceil(D / 64) + 6 + 1) * U


def cos_diff(f, proto, classes):
    """sim[k, n] = cos(f_n, proto[2c]) - cos(f_n, proto[2c + 1]), c = classes[k], in float64 and in the kernel's form
    d * (1 / (|f| |p|)) so that a zero norm gives 0 * inf = NaN; with the per-element bound of the fp32 kernel:
      each cosine: g S / (|f| |p|) for the dot product (S = sum|f p|, g = cos_gamma) + (g + 5 u) |cos|: the two square roots carry
      g / 2 + u each (sqrtf contributes twice), their product, the reciprocal and the multiply one u each;
      the subtraction: u |sim|.
    A factor 1 + 2^-10 covers the second-order terms."""
    f, proto = np.asarray(f, np.float64), np.asarray(proto, np.float64)
    g = cos_gamma(f.shape[1])
    fn = np.sqrt((f * f).sum(1))
    sim, bound = np.empty((len(classes), f.shape[0])), np.empty((len(classes), f.shape[0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, c in enumerate(classes):
            cs, es = [], []
            for p in (proto[2 * c], proto[2 * c + 1]):
                den = fn * np.sqrt((p * p).sum())
                cos = (f @ p) * (1.0 / den)
                cs.append(cos)
                es.append(g * (np.abs(f) @ np.abs(p)) * (1.0 / den) + (g + 5 * U) * np.abs(cos))
            sim[k] = cs[0] - cs[1]
            bound[k] = (es[0] + es[1] + U * np.abs(sim[k])) * (1 + 2.0 ** -10)
    return sim, bound


def undecided(sim, bound):
    """share of the finite elements whose sign (the clean / noise decision) the bound leaves open"""
    ok = np.isfinite(sim)
    return float((np.abs(sim[ok]) <= bound[ok]).mean()) if ok.any() else 0.0


# ---- selection -------------------------------------------------------------------------------------------------------------------------
def select(values, clean_thr, noise_thr):
    """-> (top, bot): positions of the k_top largest (descending) and the k_bot smallest (ascending) fp32 values, stable (the first
    position wins ties, -0.0 ties with +0.0), NaN elements never picked; k = int(1 * thr * count) in Python double with
    count = #(v >= 0) / #(v < 0) (-0.0 >= 0; NaN in neither)"""
    v = [float(x) for x in np.asarray(values, np.float32).reshape(-1)]
    n_clean = sum(1 for x in v if x >= 0)
    n_noise = sum(1 for x in v if x < 0)
    kt, kb = int(1 * clean_thr * n_clean), int(1 * noise_thr * n_noise)
    keep = [i for i, x in enumerate(v) if x == x]
    top = sorted(keep, key=lambda i: v[i], reverse=True)[:kt]        # sorted() is stable, also under reverse
    bot = sorted(keep, key=lambda i: v[i])[:kb]
    return top, bot


def select_rows(sims, pools, clean_thr, noise_thr):
    """per class k: select() over sims[k][pools[k]] (None = the whole row); picks are positions INSIDE the pool"""
    sims = np.asarray(sims, np.float32)
    out = []
    for k, p in enumerate(pools):
        row = sims[k] if p is None else sims[k][np.asarray(p, np.int64)] if len(p) else sims[k][:0]
        out.append(select(row, clean_thr, noise_thr))
    return out


# ---- generators (shared by the GPU file and the CPU preconditions) ---------------------------------------------------------------------
DY_POOL = 100               # dyadic rows draw their nonzero columns from this many columns and the LAST one


def dyadic_rows(rs, n, D, cols=None):
    """n rows of D entries in {0, +-2^k}: one k in [-4, 4] per row, exactly 4^m nonzeros (m in 0..3, cycling with the row), the last
    column always among them.  |row| = 2^(m + k), dot products of two such rows are 2^(k + k') times an integer of at most 64:
    cosines are small dyadic rationals, exact in fp32 whatever the order or the formula.  `cols`: the column pool (shared between
    features and prototypes so that the supports overlap)."""
    if cols is None:
        cols = dyadic_cols(rs, D)
    out = np.zeros((n, D))
    for i in range(n):
        m, k = i % 4, int(rs.randint(-4, 5))
        pick = np.concatenate([[D - 1], rs.choice(cols, 4 ** m - 1, replace=False)]) if m else np.array([D - 1])
        out[i, pick.astype(np.int64)] = rs.choice([-1.0, 1.0], pick.size) * 2.0 ** k
    return out


def dyadic_cols(rs, D):
    return rs.choice(D - 1, DY_POOL, replace=False)


def dyadic_exact(f, proto, classes):
    """the preconditions of bit equality: every row holds 4^m nonzeros of one magnitude 2^k, and the reference is an fp32 number"""
    for rows in (np.asarray(f, np.float64), np.asarray(proto, np.float64)):
        for r in rows:
            nz = np.abs(r[r != 0])
            if nz.size == 0:
                continue
            lk = math.log2(nz[0])
            if not ((nz == nz[0]).all() and nz.size in (1, 4, 16, 64) and lk == int(lk)):
                return False
    sim, _ = cos_diff(f, proto, classes)
    fin = np.isfinite(sim)
    return bool(np.array_equal(sim[fin].astype(np.float32).astype(np.float64), sim[fin]))


def random_rows(rs, n, D, relu=False):
    x = rs.standard_normal((n, D)).astype(np.float32).astype(np.float64)
    return np.maximum(x, 0.0) if relu else x


def proto_labels(rs, B, C):
    """0, 1 and a 0.5 that belongs to neither row; the first rows (when there are enough) hold one of each in every class"""
    y = rs.choice([0.0, 1.0, 0.5], (B, C), p=[0.5, 0.35, 0.15])
    if B >= 3:
        y[0], y[1], y[2] = 0.0, 1.0, 0.5
    return y


def logit_margin(z, L, U_):
    """distance of float64 sigmoid(z) from the fp32 thresholds, in units of the fp32 sigmoid's error bound (+ u): > 1 means the
    kernel's p < L / p > U decision cannot differ from the reference's"""
    z = np.asarray(z, np.float64)
    s = sigmoid(z)
    d = np.minimum(np.abs(s - float(np.float32(L))), np.abs(s - float(np.float32(U_))))
    return d / (2.0 * sig_err(z) + U)


def safe_logits(rs, shape, L, U_):
    """2 N(0, 1) logits, those inside the band where fp32 sigmoid could flip the decision replaced by 8.0"""
    z = (2.0 * rs.standard_normal(shape)).astype(np.float32).astype(np.float64)
    z[logit_margin(z, L, U_) <= 4.0] = 8.0
    return z


SELECT_FAMILIES = ("distinct", "ties", "zeros", "inf", "denormal", "allpos", "allneg")


def select_values(family, rs, n):
    if family == "distinct":
        v = (rs.permutation(n) - n // 2 + 0.5) / n
    elif family == "ties":
        v = rs.randint(-3, 4, n) / 4.0
    elif family == "zeros":
        v = rs.choice([0.0, -0.0, 1.0, -1.0], n, p=[0.35, 0.35, 0.15, 0.15])
    elif family == "inf":
        v = rs.standard_normal(n)
        v[rs.uniform(size=n) < 0.2] = np.inf
        v[rs.uniform(size=n) < 0.2] = -np.inf
    elif family == "denormal":
        v = rs.randint(-5, 6, n) * 2.0 ** -149
    elif family == "allpos":
        v = np.abs(rs.standard_normal(n)) + 0.1
    elif family == "allneg":
        v = -np.abs(rs.standard_normal(n)) - 0.1
    else:
        raise ValueError(family)
    return v.astype(np.float32)


def hundred_hundred(rs):
    """exactly 100 values >= 0 and 100 values < 0, shuffled, with ties: thr * 100 sits a hair under / over an integer in double for
    thr = 0.29 (k = 28), 0.57 (56), 0.07 (7)"""
    v = np.concatenate([rs.randint(0, 30, 100) / 32.0, -(rs.randint(1, 30, 100) / 32.0)])
    return v[rs.permutation(200)].astype(np.float32)


THRESHOLD_KS = ((0.29, 28), (0.57, 56), (0.07, 7), (1.0, 100), (0.005, 0))


def with_nans(v, where):
    v = np.array(v, np.float32)
    v[list(where)] = np.nan
    return v


# ---- the cases of the GPU file -----------------------------------------------------------------------------------------------------------
HANDLES = {"r18": ("Resnet18", 5, 64, 512), "eff": ("Efficient_b0", 5, 64, 1280), "r18c32": ("Resnet18", 32, 32, 512)}
COS_N = (1, 3, 4, 5, 257)                     # 4 samples per block: below, at and over a block, and 65 blocks (the last one ragged)
COS_FAMILIES = ("dyadic", "normal", "relu")
PROTO_B = (1, 255, 256, 257, 600)             # the calls of one pass: the counting loops stride by 256 threads
PROTO_BANDS = ((0.5, 0.7), (0.3, 0.5))        # z = 0 sits exactly on L, then exactly on U: counted in neither pass
SELECT_N = (1, 63, 64, 255, 256, 257, 1025)


def class_lists(C):
    """one class; all C classes unsorted; a repeated class"""
    every = [int(c) for c in np.random.RandomState(C).permutation(C)]
    if every == sorted(every):
        every = every[::-1]
    return [[C - 2], every, [2, C - 1, 2]]


def cos_case(family, D, C, N, seed):
    rs = np.random.RandomState(seed)
    if family == "dyadic":
        cols = dyadic_cols(rs, D)
        return dyadic_rows(rs, N, D, cols), dyadic_rows(rs, 2 * C, D, cols)
    relu = family == "relu"
    return random_rows(rs, N, D, relu), random_rows(rs, 2 * C, D, relu)


def proto_case(family, D, C, band, seed):
    """-> batches (one per PROTO_B), active, negative.  Class 2 is active AND negative, class 0 is active without positives, the last
    class is active; features are small integers ("int": sums exact in any order) or standard normal.  The 255-row call carries the
    logit edges z = 0 (p = 1/2 exactly: expf(-0) = 1), +inf (p = 1), -inf (p = 0) and NaN in every negative class."""
    rs = np.random.RandomState(seed)
    active, negative = [0, 2, C - 1], [1, 2, 3]
    batches = []
    for B in PROTO_B:
        f = rs.randint(-8, 9, (B, D)).astype(np.float64) if family == "int" else random_rows(rs, B, D)
        y = proto_labels(rs, B, C)
        y[:, 0] = np.where(y[:, 0] == 1.0, 0.0, y[:, 0])
        z = safe_logits(rs, (B, C), *band)
        if B == 255:
            z[:4, negative] = np.array([0.0, np.inf, -np.inf, np.nan])[:, None]
        batches.append((f, z, y))
    return batches, active, negative
