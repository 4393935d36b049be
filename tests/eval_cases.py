"""Seeded inputs of the evaluation-metric fixtures (tests/golden/rank_metrics.json holds the expectations; the arrays are
rebuilt from these generators, which is smaller than storing them).  numpy's RandomState streams are stable across numpy
versions; every case carries a checksum of its bytes in the fixture, so a generator that drifts is reported as such."""
import hashlib

import numpy as np

# the sizes at which the kernel takes another path: the 64-lane wave, the 256-positive block, the 2048-score LDS tile
# (fedmlp_amd/csrc/kernels.h: FM_METRICS_ROWS / FM_METRICS_BP / FM_METRICS_TILE), each with its neighbours
TILE = 2048
SIZES = (2, 3, 63, 64, 65, 255, 256, 257, TILE + 1, 5000)
CLASSES = (1, 5, 32)
FAMILIES = ("uniform", "five_level", "all_equal", "sigmoid", "signed_zero")
PREVALENCES = (0.02, 0.3, 0.9)
THRESHOLD = 0.5


def scores(rs, family, n):
    """one column of fp32 scores"""
    if family == "uniform":
        return rs.uniform(size=n).astype(np.float32)
    if family == "five_level":                    # exact 0.0 and 1.0, tie groups of n / 5
        return rs.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32), size=n)
    if family == "all_equal":                     # one tie group; nothing is predicted at the 0.5 threshold
        rs.uniform(size=n)
        return np.full(n, 0.5, np.float32)
    if family == "sigmoid":                       # sigmoid of N(0, 12^2) logits: saturates to ties at 1.0 and near 0
        z = (12.0 * rs.standard_normal(n)).astype(np.float32).astype(np.float64)
        return (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    if family == "signed_zero":                   # -0.0 == +0.0 under the IEEE compare; a bit-pattern sort would split them
        return rs.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), size=n)
    raise ValueError(family)


def labels(rs, n, prev, degenerate_ok=False):
    """one column of 0/1 labels at prevalence `prev`, redrawn until it has a positive and a negative"""
    for _ in range(100000):
        y = (rs.uniform(size=n) < prev).astype(np.float32)
        if degenerate_ok or 0 < y.sum() < n:
            return y
    raise RuntimeError("no two-class column")


def make_case(n, C, family, prev, seed):
    """(y, p): fp32 [n, C]; every column has both classes"""
    rs = np.random.RandomState(seed)
    y = np.stack([labels(rs, n, prev) for _ in range(C)], 1)
    p = np.stack([scores(rs, family, n) for _ in range(C)], 1)
    return np.ascontiguousarray(y), np.ascontiguousarray(p)


def case_list():
    """every size x family; the class count and the prevalence rotate, so each size and each family sees all of them"""
    out = []
    for si, n in enumerate(SIZES):
        for fi, family in enumerate(FAMILIES):
            out.append({"name": f"n{n}_{family}", "n": n, "C": CLASSES[(si + fi) % 3], "family": family,
                        "prev": PREVALENCES[(2 * si + fi) % 3], "seed": 7000 + len(out)})
    return out


def degenerate_list():
    """inputs only: columns without positives / without negatives, N = 1; the expectation is the host functions'"""
    out = []
    for n, family, seed in ((1, "uniform", 1), (1, "five_level", 2), (5, "uniform", 3), (64, "five_level", 4),
                            (257, "sigmoid", 5), (300, "all_equal", 6)):
        out.append({"name": f"deg_n{n}_{family}", "n": n, "family": family, "seed": 9000 + seed})
    return out


def make_degenerate(n, family, seed):
    """(y, p) fp32 [n, 4]: column 0 has no positives, column 1 no negatives, columns 2 and 3 are drawn at 0.3 / 0.9 (with
    n = 1 every column is one-class)"""
    rs = np.random.RandomState(seed)
    y = np.stack([np.zeros(n, np.float32), np.ones(n, np.float32), labels(rs, n, 0.3, True), labels(rs, n, 0.9, True)], 1)
    p = np.stack([scores(rs, family, n) for _ in range(4)], 1)
    return np.ascontiguousarray(y), np.ascontiguousarray(p)


def checksum(y, p):
    return hashlib.sha1(y.tobytes() + p.tobytes()).hexdigest()[:16]


def counts_of(y, p, threshold=THRESHOLD):
    """int64 [C, 4] {tp, npos, npred, tn} with pred = p > threshold"""
    yt, pred = y != 0, p > threshold
    return np.stack([(yt & pred).sum(0), yt.sum(0), pred.sum(0), (~yt & ~pred).sum(0)], 1).astype(np.int64)


# ---- the valloss fixture: a linear stub net over a tiny dataset ------------------------------------------------------
VALLOSS = {"N": 230, "C": 3, "F": 6, "batch_size": 2, "data_seed": 31, "torch_seed": 1234}


def valloss_problem():
    """(x fp32 [N, F], targets fp32 [N, C], W fp32 [F, C]); the stub net's logits are x @ W"""
    v = VALLOSS
    rs = np.random.RandomState(v["data_seed"])
    x = rs.standard_normal((v["N"], v["F"])).astype(np.float32)
    t = (rs.uniform(size=(v["N"], v["C"])) < 0.4).astype(np.float32)
    W = rs.standard_normal((v["F"], v["C"])).astype(np.float32)
    return x, t, W
