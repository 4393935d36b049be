"""Kernel-level parity of the RSCFed / FedNoRo (LA_KD) / CBAFed loss heads (csrc/heads.hip: k_loss_rscfed, k_loss_lakd,
k_loss_cbafed) through Engine.loss_rscfed / loss_lakd / loss_cbafed, against oracle/steps_ref.py's head arithmetic in its
dtype-generic restatement tests/baseline_heads_ref.py (pinned to the oracle's float32 results by tests/test_baseline_heads_cpu.py).

Bound: the rule of tests/test_irm_lsr_heads_gpu.py.  Per tensor and per case d = max |torch-CPU fp32 autograd - float64| on the
same inputs, floored at 2^-24 max|tensor|, and the kernel may be 4 d from the float64 result.  d, the worst error and the worst
error / bound per head go to baseline_heads_parity.json.

Shapes: B in {1, 3, 64, 67} x C in {2, 5, 14, 32}: C = 2 is one active and one missing class, C = 32 is FM_MAX_CLASSES, B C runs
from below one 256-thread pass to far above it.  Active sets: one class, and two where C >= 5.  Logits: the smooth band |z| <= 8
of tests/test_head_kernels_gpu.py; LA_KD also with |z| up to 120, where the -100 clamp binds.

CBAFed stage 2 decides on the device what the trainer decided on the host, so counts and weights are compared EXACTLY with
oracle.steps_ref.cbafed_stage2_targets.  That can hold only when no probability sits within rounding of a threshold: the inputs
are built (and checked, in float64) to keep every sigmoid(z) at least 1e-5 from tao[i] and 1 - tao[i]."""
import numpy as np
import pytest
import torch

from oracle import steps_ref as O
from tests import baseline_heads_ref as R
from tests.test_local_training_gpu import _dump

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
REPORT = {}
CASES = [(B, C, ann) for B in (1, 3, 64, 67) for C in (2, 5, 14, 32) for ann in ((1, 2) if C >= 5 else (1,))]
BS = 32                                            # args.batch_size of the normalisation (not the actual B)
_ENG = {}


@pytest.fixture(scope="module")
def engines():
    """a handle per class count (the heads take C from the handle); it owns the stream the launches run on, nothing else"""
    from fedmlp_amd import spec
    from fedmlp_amd.engine import Engine

    def get(C):
        if C not in _ENG:
            e = Engine("Resnet18", C, 32, 32, 4)
            e.set_state(*spec.init_state("Resnet18", C, 3))
            _ENG[C] = e
        return _ENG[C]
    yield get
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _sets(C, ann):
    act = [C // 2] if ann == 1 else [0, C - 1]
    neg = [c for c in range(C) if c not in act]
    return act, neg, [1.0 if c in act else 0.0 for c in range(C)]


def _pw(rs, C):
    return _f32(rs.choice([1.0, 0.05, 37.5, 6.4], C))


def _within(name, got, want, f32):
    """the module docstring's bound; records d and the ratio"""
    got, want, f32 = (np.asarray(a, np.float64) for a in (got, want, f32))
    assert got.shape == want.shape == f32.shape, (name, got.shape, want.shape)
    assert np.isfinite(f32).all(), f"{name}: the fp32 reference is not finite on these inputs"
    assert np.isfinite(got).all(), f"{name}: not finite (an element was not written?)"
    d = max(float(np.abs(f32 - want).max()), U * float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    ratio = err / (4 * d) if d > 0 else (0.0 if err == 0 else np.inf)
    key = name.split(" ")[0] + "/" + name.split(" ")[-1]
    r = REPORT.setdefault(key, {"torch_fp32_distance": 0.0, "max_abs_err": 0.0, "worst_err_over_bound": 0.0})
    r["torch_fp32_distance"] = max(r["torch_fp32_distance"], d)
    r["max_abs_err"] = max(r["max_abs_err"], err)
    r["worst_err_over_bound"] = max(r["worst_err_over_bound"], ratio)
    _dump(REPORT, "baseline_heads_parity.json")
    print(f"{name}: torch fp32 distance {d:.3e}, max|err| {err:.3e}, err / (4 d) {ratio:.3f}")
    assert err <= 4 * d, f"{name}: max|err| {err:.3e} beyond 4 x {d:.3e}"


@pytest.mark.parametrize("case", CASES, ids=str)
def test_loss_rscfed(engines, case):
    B, C, ann = case
    eng = engines(C)
    rs = np.random.RandomState(100 + 31 * B + 7 * C + ann)
    act, neg, am = _sets(C, ann)
    z, zt = _f32(rs.uniform(-8, 8, (B, C))), _f32(rs.uniform(-8, 8, (B, C)))
    y, pw = (rs.rand(B, C) < 0.4).astype(np.float64), _pw(rs, C)
    want = R.loss_rscfed(z, zt, y, pw, act, neg, BS, ann)
    f32 = R.loss_rscfed(z, zt, y, pw, act, neg, BS, ann, dtype=torch.float32)
    dz, loss = eng.loss_rscfed(_dev(z), _dev(zt), _dev(y), pw, am, ann, BS)
    dz2, loss2 = eng.loss_rscfed(_dev(z), _dev(zt), _dev(y), pw, am, ann, BS)
    assert np.array_equal(_bits(dz), _bits(dz2)) and np.array_equal(_bits(loss), _bits(loss2))     # run to run
    _within(f"rscfed {case} loss", loss.cpu().numpy()[0], want[0], f32[0])
    _within(f"rscfed {case} dz", dz.cpu().numpy(), want[1], f32[1])


def _lakd(eng, case, z, zt, y, name):
    B, C, ann = case
    act, neg, am = _sets(C, ann)
    for w_kd in (float(np.float32(0.8 * 0.0067)), 0.5):
        want = R.loss_la_kd(z, zt, y, act, neg, w_kd)
        f32 = R.loss_la_kd(z, zt, y, act, neg, w_kd, dtype=torch.float32)
        dz, loss = eng.loss_lakd(_dev(z), _dev(zt), _dev(y), am, w_kd)
        dz2, loss2 = eng.loss_lakd(_dev(z), _dev(zt), _dev(y), am, w_kd)
        assert np.array_equal(_bits(dz), _bits(dz2)) and np.array_equal(_bits(loss), _bits(loss2))     # run to run
        _within(f"{name} {case} loss", loss.cpu().numpy()[0], want[0], f32[0])
        _within(f"{name} {case} dz", dz.cpu().numpy(), want[1], f32[1])
    return want


@pytest.mark.parametrize("case", CASES, ids=str)
def test_loss_lakd(engines, case):
    B, C, ann = case
    rs = np.random.RandomState(200 + 31 * B + 7 * C + ann)
    z, zt = _f32(rs.uniform(-8, 8, (B, C))), _f32(rs.uniform(-8, 8, (B, C)))
    _lakd(engines(C), case, z, zt, (rs.rand(B, C) < 0.4).astype(np.float64), "lakd")


def test_loss_lakd_clamp_binds(engines):
    """|z| up to 120: sigmoid(z) rounds to 1 (or 0), log(0) = -inf is clamped at -100 and the element's gradient is 0"""
    case = (67, 14, 2)
    B, C, _ = case
    rs = np.random.RandomState(300)
    z = _f32(rs.uniform(-120, 120, (B, C)))
    zt = _f32(rs.uniform(-120, 120, (B, C)))
    y = (rs.rand(B, C) < 0.5).astype(np.float64)
    z[0, 0], y[0, 0] = 120.0, 0.0                  # an active element (class 0) whose log(1 - p) is -inf in both dtypes
    z[1, 0], y[1, 0] = -120.0, 1.0
    want = _lakd(engines(C), case, z, zt, y, "lakd_clamp")
    assert want[0] > 100.0 * 0.5 * 2 / (B * 2)      # the two clamped elements are in the loss: (1 - w_kd) 100 each / (B |active|)


# ---- CBAFed ---------------------------------------------------------------------------------------------------------------------
def _logit(p):
    return np.log(p / (1 - p))


KINDS = ("clean_only", "none", "all", "random")


def _stage2_inputs(rs, B, C, act, neg, variant):
    """logits, labels and tao for stage 2.  The k-th missing class is built as KINDS[(k + variant) % 4]:
    clean_only: every row below 1 - tao or between the thresholds, at least one below (noise = 0, clean > 0: weight 1);
    none: every row between the thresholds (no pseudo row: the term is skipped, weight 1);
    all: every row beyond a threshold, row 0 above tao with y = 0 (a label that becomes 1);
    random: |z| <= 8 as drawn.
    Offending logits (a probability within 1e-5 of a threshold, in float64) are redrawn until none is left."""
    tao = _f32(rs.uniform(0.55, 0.95, C))
    z = _f32(rs.uniform(-8, 8, (B, C)))
    y = (rs.rand(B, C) < 0.4).astype(np.float64)
    kinds = {}
    for k, i in enumerate(neg):
        kind = KINDS[(k + variant) % 4]
        kinds[i] = kind
        hi = _logit(tao[i]) + rs.uniform(0.5, 3.0, B)
        lo = _logit(1 - tao[i]) - rs.uniform(0.5, 3.0, B)
        mid = rs.uniform(-0.1, 0.1, B)
        if kind == "clean_only":
            pick = rs.rand(B) < 0.5
            pick[0] = True
            z[:, i] = _f32(np.where(pick, lo, mid))
        elif kind == "none":
            z[:, i] = _f32(mid)
        elif kind == "all":
            pick = rs.rand(B) < 0.5
            pick[0] = True
            z[:, i] = _f32(np.where(pick, hi, lo))
            y[0, i] = 0.0
    for _ in range(100):
        p = 1.0 / (1.0 + np.exp(-z))
        bad = np.zeros_like(z, bool)
        for i in neg:
            bad[:, i] = (np.abs(p[:, i] - tao[i]) < 1e-5) | (np.abs(p[:, i] - (1 - tao[i])) < 1e-5)
        if not bad.any():
            break
        z = np.where(bad, _f32(rs.uniform(-8, 8, z.shape)), z)
    p = 1.0 / (1.0 + np.exp(-z))
    for i in neg:                                   # the float64 check the exact comparisons below rest on
        assert (np.abs(p[:, i] - tao[i]) >= 1e-5).all() and (np.abs(p[:, i] - (1 - tao[i])) >= 1e-5).all()
    return z, y, tao, kinds


@pytest.mark.parametrize("case", CASES, ids=str)
def test_loss_cbafed_warmup(engines, case):
    B, C, ann = case
    eng = engines(C)
    rs = np.random.RandomState(400 + 31 * B + 7 * C + ann)
    act, neg, am = _sets(C, ann)
    z, y, pw = _f32(rs.uniform(-8, 8, (B, C))), (rs.rand(B, C) < 0.4).astype(np.float64), _pw(rs, C)
    want = R.loss_cbafed_stage1(z, y, pw, act, BS, ann)
    f32 = R.loss_cbafed_stage1(z, y, pw, act, BS, ann, dtype=torch.float32)
    pw_d = _dev(pw)
    counts = torch.arange(7, 7 + C + 1, dtype=torch.int64, device="cuda")
    pw0, c0 = pw_d.clone(), counts.clone()
    dz, loss = eng.loss_cbafed(_dev(z), _dev(y), am, ann, BS, None, pw_d, counts)
    dz2, loss2 = eng.loss_cbafed(_dev(z), _dev(y), am, ann, BS, None, pw_d)            # counts may be absent in the warm-up
    assert np.array_equal(_bits(dz), _bits(dz2)) and np.array_equal(_bits(loss), _bits(loss2))
    assert np.array_equal(_bits(pw_d), _bits(pw0)) and torch.equal(counts, c0)         # the warm-up only reads the weights
    assert (dz.cpu().numpy()[:, neg] == 0).all()                                       # exact zeros outside the loss
    _within(f"cbafed_warmup {case} loss", loss.cpu().numpy()[0], want[0], f32[0])
    _within(f"cbafed_warmup {case} dz", dz.cpu().numpy(), want[1], f32[1])


@pytest.mark.parametrize("case", CASES, ids=str)
def test_loss_cbafed_stage2(engines, case):
    B, C, ann = case
    eng = engines(C)
    act, neg, am = _sets(C, ann)
    seen = set()
    for variant in range(4):
        rs = np.random.RandomState(500 + 31 * B + 7 * C + ann + 1000 * variant)
        z, y, tao, kinds = _stage2_inputs(rs, B, C, act, neg, variant)
        pw = _pw(rs, C)
        # the host decisions, on torch's fp32 probabilities as the trainer made them
        prob = torch.sigmoid(torch.tensor(z, dtype=torch.float32))
        labels, idx_neg, loss_w, n_pseudo = O.cbafed_stage2_targets(prob, torch.tensor(y, dtype=torch.float32), neg,
                                                                    [float(t) for t in tao], [float(v) for v in pw])
        for k, i in enumerate(neg):                 # the inputs contain what they were built to contain
            hi = prob[:, i] > float(tao[i])
            lo = prob[:, i] < 1 - float(tao[i])
            assert not bool((hi & lo).any())
            if kinds[i] == "clean_only":
                assert int(hi.sum()) == 0 and int(lo.sum()) > 0 and loss_w[i] == 1
            elif kinds[i] == "none":
                assert n_pseudo[k] == 0 and loss_w[i] == 1
            elif kinds[i] == "all":
                assert n_pseudo[k] == B
                assert bool(hi[0]) and y[0, i] == 0.0 and float(labels[0, i]) == 1.0     # a hi row whose y was 0
            seen.add(kinds[i])
        want = R.loss_cbafed_stage2(z, labels.numpy(), idx_neg, loss_w, act, neg, BS, ann)
        f32 = R.loss_cbafed_stage2(z, labels.numpy(), idx_neg, loss_w, act, neg, BS, ann, dtype=torch.float32)
        y_d, pw_d = _dev(y), _dev(pw)
        y0 = y_d.clone()
        counts = torch.zeros(C + 1, dtype=torch.int64, device="cuda")
        dz, loss = eng.loss_cbafed(_dev(z), y_d, am, ann, BS, tao, pw_d, counts)
        assert np.array_equal(_bits(y_d), _bits(y0))                                   # the labels are formed in registers
        # exact: the weights, class_num_list and data_num
        want_pw = np.asarray(loss_w, np.float32)
        assert np.array_equal(pw_d.cpu().numpy().view(np.uint32), want_pw.view(np.uint32)), (pw_d.cpu().numpy(), want_pw)
        want_counts = np.zeros(C + 1, np.int64)
        for k, i in enumerate(neg):
            want_counts[i] = n_pseudo[k]
        want_counts[act] = B
        want_counts[C] = sum(n_pseudo) + B * ann
        assert np.array_equal(counts.cpu().numpy(), want_counts), (counts.cpu().numpy(), want_counts)
        # dz is exactly 0 outside the loss: the missing classes' rows that are neither hi nor lo
        out = np.ones((B, C), bool)
        out[:, act] = False
        for k, i in enumerate(neg):
            out[idx_neg[k].numpy(), i] = False
        assert (dz.cpu().numpy()[out] == 0).all()
        # a second call: the same bits (the weights it rewrites are the ones it finds), counts accumulate
        dz2, loss2 = eng.loss_cbafed(_dev(z), y_d, am, ann, BS, tao, pw_d, counts)
        assert np.array_equal(_bits(dz), _bits(dz2)) and np.array_equal(_bits(loss), _bits(loss2))
        assert np.array_equal(counts.cpu().numpy(), 2 * want_counts)
        _within(f"cbafed_stage2 {case} v{variant} loss", loss.cpu().numpy()[0], want[0], f32[0])
        _within(f"cbafed_stage2 {case} v{variant} dz", dz.cpu().numpy(), want[1], f32[1])
    assert seen >= {"clean_only", "none", "all"}, seen


def test_heads_need_an_active_and_a_missing_class(engines):
    from fedmlp_amd._lib import FmError
    C, B = 5, 3
    eng = engines(C)
    z = torch.zeros((B, C), device="cuda")
    pw = torch.ones(C, device="cuda")
    counts = torch.zeros(C + 1, dtype=torch.int64, device="cuda")
    for am in ([1.0] * C, [0.0] * C):
        with pytest.raises(FmError):
            eng.loss_rscfed(z, z, z, [1.0] * C, am, 1, BS)
        with pytest.raises(FmError):
            eng.loss_lakd(z, z, z, am, 0.5)
        with pytest.raises(FmError):
            eng.loss_cbafed(z, z, am, 1, BS, None, pw)
        with pytest.raises(FmError):
            eng.loss_cbafed(z, z, am, 1, BS, [0.7] * C, pw, counts)
    assert int(counts.sum()) == 0
