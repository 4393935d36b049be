"""The FixMatch strong view without a GPU: the numpy restatement (tests/strong_ref.py) against Pillow's and the reference's own
outputs (tests/golden/augment_strong_pil.npz, made by tests/golden/make_strong_golden.py), the coverage the fixture must have,
the host-side draws (fedmlp_amd.augment.draw_strong) and the dataset switch.  The kernel's side is tests/test_augment_strong_gpu.py."""
import os

import numpy as np
import torch

from fedmlp_amd import augment as A
from tests import strong_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_strong_pil.npz")


def fixture_cases():
    """[(image, weak matrix, flip, [(op name or Skip, v, sign)] * 2, corners, out_u8, out_f32)] of the fixture"""
    g = np.load(GOLD)
    H, W = g["images"].shape[2:]
    cases = []
    for i in range(len(g["op"])):
        slots = [(R.OPS[g["op"][i, s]] if g["apply"][i, s] else R.SKIP, int(g["v"][i, s]), int(g["sign"][i, s])) for s in range(2)]
        cases.append((g["images"][g["image_index"][i]], g["matrices"][i], int(g["flips"][i]), slots,
                      R.cutout_corners(float(g["cut"][i, 0]), float(g["cut"][i, 1]), H, W), g["out_u8"][i], g["out_f32"][i]))
    return cases


def fixture_symbolic():
    g = np.load(GOLD)
    return {k: g[k] for k in ("op", "v", "apply", "sign", "cut")}


def test_fixture_is_no_larger_than_the_weak_fixture():
    assert os.path.getsize(GOLD) <= 401164


def test_restatement_equals_pillow_on_every_fixture_case():
    cases = fixture_cases()
    assert len(cases) >= 16
    for img, m, flip, slots, corners, out_u8, out_f32 in cases:
        u8 = R.strong_u8(img, m, flip, slots, corners)
        np.testing.assert_array_equal(u8, out_u8, err_msg=str(slots))                          # byte for byte, every pixel
        f32 = R.normalise(u8, A.IMAGENET_MEAN, A.IMAGENET_STD)
        np.testing.assert_array_equal(f32.view(np.int32), out_f32.view(np.int32), err_msg=str(slots))      # bit for bit


def test_fixture_covers_the_pool():
    g = np.load(GOLD)
    H, W = g["images"].shape[2:]
    cases = fixture_cases()
    applied = [(name, v, sign, s) for c in cases for s, (name, v, sign) in enumerate(c[3]) if name != R.SKIP]
    for op in R.OPS:
        vs = {v for name, v, _, _ in applied if name == op}
        assert len(vs) >= 2 and 1 in vs and 9 in vs, (op, vs)
    for op in R.SIGNED:
        assert {sign for name, _, sign, _ in applied if name == op} == {-1, 1}, op
    for family in (R.GEOMETRIC, R.HISTOGRAM, ("Sharpness",)):
        assert {s for name, _, _, s in applied if name in family} == {0, 1}, family          # in each slot position
    chains = {(c[3][0][0], c[3][1][0]) for c in cases}
    assert any(a in R.GEOMETRIC and b == "AutoContrast" for a, b in chains)
    assert any(a in R.GEOMETRIC and b == "Equalize" for a, b in chains)
    assert any(a == b and a != R.SKIP for a, b in chains)                                      # the same op twice
    assert (R.SKIP, R.SKIP) in chains
    corners = [c[4] for c in cases]
    assert any(x0 == 0 and y0 == 0 for x0, y0, _, _ in corners)                                # clipped at the left / top border
    assert any(x1 == W and y1 == H for _, _, x1, y1 in corners)                                # clipped at the right / bottom border
    assert {c[2] for c in cases} == {0, 1}                                                     # weak flip on and off
    # the inputs are structured: no histogram op of the fixture is the identity on the image it met
    for img, m, flip, slots, corners, _, _ in cases:
        a = R.strong_u8(img, m, flip, [], (0, 0, -1, -1))
        for name, v, sign in slots:
            b = R.apply_op(a, name, v, sign)
            if name in R.HISTOGRAM:
                assert not np.array_equal(a, b), name
            a = b


def test_records_reproduce_the_fixture_from_its_symbolic_draws():
    g = np.load(GOLD)
    H, W = g["images"].shape[2:]
    rec = A.strong_records(fixture_symbolic(), H, W)
    assert rec.dtype == np.int32 and rec.shape == (len(g["op"]), A.STRONG_RECORD) and A.STRONG_RECORD * 4 % 16 == 0
    for i, (_, _, _, slots, corners, _, _) in enumerate(fixture_cases()):
        assert tuple(rec[i, 16:20]) == tuple(corners)
        for s, (name, v, sign) in enumerate(slots):
            sl = rec[i, 8 * s:8 * s + 8]
            if name == R.SKIP:
                assert sl[0] == A.STRONG_SKIP and not sl[1:].any()
                continue
            assert A.STRONG_OPS[sl[0]] == name
            if name in ("Brightness", "Color", "Contrast", "Sharpness"):
                assert sl[1:2].view(np.float32)[0] == R.blend_factor(v)
            elif name == "Posterize":
                assert sl[1] == R.posterize_mask(v)
            elif name == "Solarize":
                assert sl[1] == R.solarize_threshold(v)
            elif name in R.GEOMETRIC:
                from oracle.augment_ref import fixed_coeffs
                assert list(sl[1:7]) == fixed_coeffs(R.geometric_matrix(name, v, sign, H, W))
            assert sl[7] == 0


def test_draw_strong_semantics():
    H, W, B = 224, 224, 4096
    sym = A.draw_strong_symbolic(B, H, W, torch.Generator().manual_seed(3))
    assert sym["op"].shape == (B, 2) and sym["op"].min() == 0 and sym["op"].max() == 13
    assert sym["v"].min() == 1 and sym["v"].max() == 9                       # randint(1, m): m itself never comes
    assert set(np.unique(sym["apply"])) == {0, 1} and set(np.unique(sym["sign"])) == {-1, 1}
    assert 0.45 < sym["apply"].mean() < 0.55                                 # a fair coin
    assert (sym["cut"] >= 0).all() and (sym["cut"][:, 0] < W).all() and (sym["cut"][:, 1] < H).all()
    rec = A.strong_records(sym, H, W)
    np.testing.assert_array_equal(rec, A.draw_strong(B, H, W, torch.Generator().manual_seed(3)))       # same seed, same records
    assert not np.array_equal(rec, A.draw_strong(B, H, W, torch.Generator().manual_seed(4)))
    x0, y0, x1, y1 = rec[:, 16], rec[:, 17], rec[:, 18], rec[:, 19]
    assert (x0 >= 0).all() and (y0 >= 0).all() and (x0 < W).all() and (y0 < H).all()
    assert (x1 > x0).all() and (x1 <= W).all() and (y1 > y0).all() and (y1 <= H).all() and ((x1 - x0) <= 16).all()
    skipped = rec[:, 0] == A.STRONG_SKIP
    np.testing.assert_array_equal(skipped, sym["apply"][:, 0] == 0)
    np.testing.assert_array_equal(rec[~skipped, 0], sym["op"][~skipped, 0])
    np.testing.assert_array_equal(A.skip_strong(2, (1, 2, 3, 4)),
                                  np.asarray([[14] + [0] * 7 + [14] + [0] * 7 + [1, 2, 3, 4]] * 2, np.int32))


class FakeEngine:
    """the Engine surface CachedAugmentedViews uses; logs which entry a batch went through"""

    def __init__(self, hw):
        self.in_h = self.in_w = hw
        self.device = torch.device("cpu")
        self.log = []

    def augment(self, cache, idx, params, mean, std):
        self.log.append("augment")
        assert params.shape == (idx.shape[0], 8)
        return torch.zeros((idx.shape[0], 3, self.in_h, self.in_w))

    def augment_strong(self, cache, idx, params, strong, mean, std):
        self.log.append("augment_strong")
        assert params.shape == (idx.shape[0], 8) and strong.shape == (idx.shape[0], 20) and strong.dtype == torch.int32
        return torch.ones((idx.shape[0], 3, self.in_h, self.in_w))


def _dataset(**kw):
    rs = np.random.RandomState(0)
    return A.AugmentedDataset(rs.randint(0, 256, size=(6, 3, 32, 32)).astype(np.uint8), np.zeros((6, 2), np.float32),
                              generator=torch.Generator().manual_seed(1), **kw)


def test_dataset_without_strong_never_takes_the_strong_path():
    eng = FakeEngine(32)
    for ds in (_dataset(), _dataset(strong=False), _dataset(train=False), _dataset(train=False, strong=True)):
        for key in ("image", "image_aug_1", "image_aug_2"):
            ds.device_batch(eng, key, [0, 3, 5])
    assert eng.log == ["augment"] * 12


def test_dataset_with_strong_sends_only_the_second_view_through_it():
    eng = FakeEngine(32)
    ds = _dataset(strong=True)
    out = [ds.device_batch(eng, key, [1, 2]) for key in ("image", "image_aug_1", "image_aug_2")]
    assert eng.log == ["augment", "augment", "augment_strong"] and float(out[2].sum()) == 2 * 3 * 32 * 32
    # a weak-only dataset and a strong one consume the weak stream alike up to the strong draw: the first view is unchanged
    a, b = _dataset(), _dataset(strong=True)
    seen = []
    for ds in (a, b):
        e = FakeEngine(32)
        e.augment = lambda cache, idx, params, mean, std, seen=seen: seen.append(params.clone()) or torch.zeros(1)
        ds.device_batch(e, "image_aug_1", [0, 1, 2])
    assert torch.equal(seen[0], seen[1])
