"""Kernel-level parity of the RoFL head (csrc/heads.hip: rofl_rows_kernel, rofl_select_kernel, rofl_centroid_kernel) through
Engine.loss_rofl, against tests/rofl_ref.py (pinned to the reference's own functions by tests/test_rofl_cpu.py).

The head makes discrete decisions (which rows are kept, how each kept row votes), so the inputs are BUILT to keep them away from
a tie, and that margin is asserted in float64 before the engine is called: every row's every |cos_0 - cos_1| >= 1e-4, and the
gap of the per-row loss across the keep boundary >= 1e-4 of the loss.  A seed that misses a margin is redrawn (at most 20 times;
a case that cannot meet them fails).  The centroids are scaled rows of an orthogonal matrix; a row's feature is the sum of the
centroids it should vote for, plus noise.  Half of the kept rows vote their labels (mask = 1), the others differ from their
labels in exactly one class; one class carries label 0 in every row, so the mean feature of its label-1 centroid has a zero
count: cosine 0, centroid unchanged.

Exact: the keep flags (kept set and mask), the label table afterwards (untouched rows included), zeros of dz off the kept rows,
and the bits of every output from run to run.  Bounded, by the rule of tests/test_baseline_heads_gpu.py: per tensor,
d = max |rofl_ref at float32 - rofl_ref at float64| on the same inputs, floored at 2^-24 max|tensor|; the kernel may be 4 d from
the float64 result.  d, the worst error and the worst ratio per tensor go to rofl_parity.json."""
import numpy as np
import pytest
import torch

from tests import rofl_ref as R
from tests.test_local_training_gpu import _dump

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
REPORT = {}
MAXB = 67
LAM_CEN, LAM_E = 0.75, float(np.float32(0.8))
_ENG = {}


@pytest.fixture(scope="module")
def engines():
    """a handle per (model, class count): the head takes C and D from the handle and its stream; B <= max_images"""
    from fedmlp_amd import spec
    from fedmlp_amd.engine import Engine

    def get(C, model="Resnet18"):
        if (model, C) not in _ENG:
            e = Engine(model, C, 32, 32, MAXB)
            e.set_state(*spec.init_state(model, C, 3))
            _ENG[(model, C)] = e
        return _ENG[(model, C)]
    yield get
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _within(name, got, want, f32):
    got, want, f32 = (np.asarray(a, np.float64) for a in (got, want, f32))
    assert got.shape == want.shape == f32.shape, (name, got.shape, want.shape)
    assert np.isfinite(f32).all(), f"{name}: the fp32 reference is not finite on these inputs"
    assert np.isfinite(got).all(), f"{name}: not finite (an element was not written?)"
    d = max(float(np.abs(f32 - want).max()), U * float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    ratio = err / (4 * d) if d > 0 else (0.0 if err == 0 else np.inf)
    r = REPORT.setdefault(name.split(" ")[0] + "/" + name.split(" ")[-1], {"torch_fp32_distance": 0.0, "max_abs_err": 0.0, "worst_err_over_bound": 0.0})
    r["torch_fp32_distance"] = max(r["torch_fp32_distance"], d)
    r["max_abs_err"] = max(r["max_abs_err"], err)
    r["worst_err_over_bound"] = max(r["worst_err_over_bound"], ratio)
    _dump(REPORT, "rofl_parity.json")
    print(f"{name}: torch fp32 distance {d:.3e}, max|err| {err:.3e}, err / (4 d) {ratio:.3f}")
    assert err <= 4 * d, f"{name}: max|err| {err:.3e} beyond 4 x {d:.3e}"


def _inputs(B, C, D, n, seed, zmax=8.0):
    """float32-representable inputs as float64 torch tensors (the module docstring's construction)"""
    g = torch.Generator().manual_seed(seed)
    f32 = lambda t: t.float().double()                                            # noqa: E731
    z = f32((2 * torch.rand((B, C), generator=g, dtype=torch.float64) - 1) * zmax)
    y = (torch.rand((B, C), generator=g) < 0.4).double()
    empty = C // 2
    y[:, empty] = 0.0                                                             # nobody carries label 1 of this class
    w = torch.tensor([1.0, 5.0, 2.5, 37.5], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=g)]
    q, _ = torch.linalg.qr(torch.randn((D, 2 * C), generator=g, dtype=torch.float64))
    f_k = f32(q.T * (0.5 + 1.5 * torch.rand((2 * C, 1), generator=g, dtype=torch.float64)))
    keep = R.kept_rows(R.row_loss(z, y, w), n)
    vote = y.clone()
    for k, i in enumerate(torch.nonzero(keep).flatten().tolist()):
        if k % 2:                                                                 # every other kept row: one class disagrees
            c = int(torch.randint(0, C, (1,), generator=g))
            vote[i, c] = 1 - vote[i, c]
    own = f_k[2 * torch.arange(C)[None, :] + vote.long()]                         # [B, C, D]
    feat = f32(own.sum(1) + 0.02 * torch.randn((B, D), generator=g, dtype=torch.float64))
    N = B + 5
    item = torch.randperm(N, generator=g)[:B].to(torch.int32)
    pseudo = (torch.rand((N, C), generator=g) < 0.5).to(torch.uint8)
    return z, feat, y, item, w, f_k, pseudo, vote, empty


def _drawn(B, C, D, n, base, zmax=8.0):
    for k in range(20):
        inp = _inputs(B, C, D, n, base + 1000 * k, zmax)
        z, feat, y, _, w, f_k = inp[:6]
        vote_margin, gap = R.margins(z, feat, y, n, w, f_k, every_row=True)
        if vote_margin >= 1e-4 and gap >= 1e-4:
            return inp
    pytest.fail(f"no seed gives the margins for B = {B}, C = {C}, n_keep = {n}: last {vote_margin:.2e}, {gap:.2e}")


def _call(eng, z, feat, y, item, n, w, write_labels, f_k, pseudo, lam_cen=LAM_CEN, lam_e=LAM_E):
    """-> dz, loss, keep, f_k after, table after (device tensors; the inputs are copied, so a second call starts alike)"""
    fk_d, ps_d = f_k.float().cuda().contiguous(), pseudo.cuda().contiguous()
    keep = torch.full((y.shape[0],), -1, dtype=torch.int32, device="cuda")
    dz, loss = eng.loss_rofl(z.float().cuda(), feat.float().cuda(), y.float().cuda(), item.cuda(), n, w.tolist(), lam_cen, lam_e,
                             write_labels, fk_d, ps_d, keep=keep)
    return dz, loss, keep, fk_d, ps_d


def _check(eng, name, inp, n, write_labels, structure=True):
    z, feat, y, item, w, f_k, pseudo, vote, empty = inp
    B, C = y.shape
    want = R.head(z, feat, y, item, n, w, LAM_CEN, LAM_E, write_labels, f_k, pseudo)
    f32 = R.head(z.float(), feat.float(), y.float(), item, n, w.float(), LAM_CEN, LAM_E, write_labels, f_k.float(), pseudo)
    keep, mask = want["keep"], want["mask"]
    assert torch.equal(f32["keep"], keep) and torch.equal(f32["mask"], mask)
    if structure:                                  # the construction did what the docstring says
        assert torch.equal(mask, keep & (vote == y).all(1)) and int(keep.sum()) == n
        assert int(mask.sum()) == (n + 1) // 2
        assert torch.equal(want["f_k"][2 * empty + 1], f_k[2 * empty + 1])
    a = _call(eng, z, feat, y, item, n, w, write_labels, f_k, pseudo)
    b = _call(eng, z, feat, y, item, n, w, write_labels, f_k, pseudo)
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v))                                 # run to run
    dz, loss, kflags, fk_after, table = a
    assert np.array_equal(kflags.cpu().numpy(), (keep.int() + 2 * mask.int()).numpy())
    assert np.array_equal(table.cpu().numpy(), want["pseudo"].numpy())
    if write_labels:
        assert np.array_equal(table.cpu().numpy()[item.long()[keep]], y[keep].to(torch.uint8).numpy())
    else:
        assert np.array_equal(table.cpu().numpy(), pseudo.numpy())
    assert not dz.cpu()[~keep].any() and np.array_equal(_bits(dz.cpu()[~keep]), np.zeros((B - n, C), np.uint32))
    if structure:
        assert np.array_equal(_bits(fk_after[2 * empty + 1]), _bits(f_k.float()[2 * empty + 1]))
    _within(f"{name} loss", loss.cpu().numpy()[0], want["loss"].numpy(), f32["loss"].numpy())
    _within(f"{name} dz", dz.cpu().numpy(), want["dz"].numpy(), f32["dz"].numpy())
    _within(f"{name} f_k", fk_after.cpu().numpy(), want["f_k"].numpy(), f32["f_k"].numpy())
    assert not np.array_equal(_bits(fk_after), _bits(f_k.float()))                # the centroids moved


CASES = [(B, C, fr, wl) for B in (3, 64, 67) for C in (2, 5, 14, 32) for fr in (0.2, 0.0) for wl in (False, True)]


@pytest.mark.parametrize("case", CASES, ids=str)
def test_loss_rofl(engines, case):
    B, C, fr, wl = case
    n = R.n_keep(fr, B)
    inp = _drawn(B, C, 512, n, 7 + 31 * B + 5 * C + int(10 * fr) + wl)
    _check(engines(C), f"resnet18 {case}", inp, n, wl)


@pytest.mark.parametrize("wl", [False, True])
def test_loss_rofl_efficientnet_feature(engines, wl):
    """D = 1280: five float4 passes per lane in the row kernel, five per thread in the centroid kernel"""
    B, C = 67, 5
    n = R.n_keep(0.2, B)
    eng = engines(C, "Efficient_b0")
    assert eng.feature_dim == 1280
    _check(eng, f"efficient_b0 {(B, C, 0.2, wl)}", _drawn(B, C, 1280, n, 901 + wl), n, wl)


def test_loss_rofl_saturated_logits(engines):
    """|z| up to 120, where fp32 p log p is NaN: every output finite and within the bound of the float64 softplus form"""
    B, C = 67, 14
    n = R.n_keep(0.2, B)
    inp = _drawn(B, C, 512, n, 4242, zmax=120.0)
    assert float(inp[0].abs().max()) > 100
    _check(engines(C), f"saturated {(B, C)}", inp, n, True)


def test_ties_go_to_the_lower_row_and_nan_last(engines):
    """rows 3 and 5 have bit-equal inputs and sit on the two sides of the keep boundary: row 3 is kept.  Then row 0's logits
    are NaN: it sorts last, is not kept, and its dz is an exact 0 while every other output stays finite"""
    B, C, n = 8, 5, 5
    z, feat, y, item, w, f_k, pseudo, _, _ = _inputs(B, C, 512, n, 77)
    y[:] = 0.0
    z[:] = torch.tensor([-3.0, -2.0, -1.0, 0.5, 2.0, 0.5, -4.0, 3.0], dtype=torch.float64)[:, None]     # key = C softplus(z)
    feat[5] = feat[3]
    eng = engines(C)
    dz, loss, keep, _, _ = _call(eng, z, feat, y, item, n, w, True, f_k, pseudo)
    assert (keep.cpu().numpy() & 1).tolist() == [1, 1, 1, 1, 0, 0, 1, 0]
    assert torch.equal(R.kept_rows(R.row_loss(z, y, w), n), (keep.cpu() & 1).bool())
    z[0] = float("nan")
    dz, loss, keep, fk_after, _ = _call(eng, z, feat, y, item, n, w, True, f_k, pseudo)
    assert (keep.cpu().numpy() & 1).tolist() == [0, 1, 1, 1, 0, 1, 1, 0]
    assert not dz.cpu()[0].any() and bool(torch.isfinite(dz).all()) and bool(torch.isfinite(loss).all())
    assert bool(torch.isfinite(fk_after).all())


def test_a_zero_centroid_has_cosine_zero(engines):
    """a centroid row of zeros (round 0, a label value the client never saw): its cosine is exactly 0, so the vote goes to the
    other row when that one's cosine is positive and to 0 when it is negative -- the float64 restatement decides the same"""
    B, C, n = 8, 5, 8
    z, feat, y, item, w, f_k, pseudo, _, _ = _inputs(B, C, 512, n, 99)
    f_k[2 * 1 + 1] = 0.0
    want = R.head(z, feat, y, item, n, w, LAM_CEN, LAM_E, False, f_k, pseudo)
    t = R.cos_table(feat, f_k)
    assert bool((t[:, 3] == 0).all()) and float(t[:, 2].abs().min()) >= 1e-4
    dz, loss, keep, fk_after, _ = _call(engines(C), z, feat, y, item, n, w, False, f_k, pseudo)
    assert np.array_equal(keep.cpu().numpy(), (want["keep"].int() + 2 * want["mask"].int()).numpy())
    assert bool(torch.isfinite(fk_after).all()) and bool(torch.isfinite(loss).all())


@pytest.mark.parametrize("what,text", [("n_keep_0", "n_keep < 1"), ("n_keep_big", "n_keep > B"), ("null_centroids", "bad argument: null$"),
                                       ("big_batch", "B exceeds max_images")])
def test_refusals(engines, what, text):
    from fedmlp_amd._lib import FmError
    B, C = (MAXB + 1 if what == "big_batch" else 8), 5
    z, feat, y, item, w, f_k, pseudo, _, _ = _inputs(B, C, 512, 6, 5)
    n = {"n_keep_0": 0, "n_keep_big": B + 1}.get(what, 6)
    fk_d, ps_d = f_k.float().cuda(), pseudo.cuda()
    with pytest.raises(FmError, match=text):
        engines(C).loss_rofl(z.float().cuda(), feat.float().cuda(), y.float().cuda(), item.cuda(), n, w.tolist(), LAM_CEN, LAM_E, True,
                             None if what == "null_centroids" else fk_d, ps_d)
    assert torch.equal(fk_d.cpu(), f_k.float()) and torch.equal(ps_d.cpu(), pseudo)          # nothing was enqueued
