"""The FixMatch strong view on the GPU: fm_augment_strong against Pillow's and the reference's own outputs
(tests/golden/augment_strong_pil.npz) and against the numpy restatement (tests/strong_ref.py, itself pinned to the fixture by
tests/test_augment_strong_cpu.py) -- equality everywhere, no tolerance -- and wired into train_FixMatch."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_strong_pil.npz")
SEED_224 = 0               # chosen on the CPU: at B = 128 this seed applies all 14 ops in each slot (asserted below)


def structured_images(n, H, W, seed):
    """ramps mixed with a little noise, every second one squeezed into a narrow range: histograms that AutoContrast / Equalize change"""
    rs = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = []
    for i in range(n):
        ramp = np.stack([xs * 255.0 / (W - 1), ys * 255.0 / (H - 1), ((xs * (i + 1) + ys) % 256).astype(np.float64)])
        a = np.clip(ramp * 0.85 + rs.randint(0, 40, size=ramp.shape), 0, 255)
        out.append(a * 0.5 + 40 if i % 2 else a)
    return np.stack(out).astype(np.uint8)


def run(eng, imgs, sel, params, strong):
    from fedmlp_amd.augment import IMAGENET_MEAN, IMAGENET_STD
    dev = eng.device
    return eng.augment_strong(torch.from_numpy(imgs).to(dev), torch.as_tensor(sel, dtype=torch.int32, device=dev),
                              torch.from_numpy(params).to(dev), torch.from_numpy(strong).to(dev), IMAGENET_MEAN, IMAGENET_STD)


def test_strong_is_bit_exact_with_pillow_fixture():
    from fedmlp_amd.engine import get_engine
    from fedmlp_amd.augment import fixed_point_params, strong_records
    g = np.load(GOLD)
    H, W = g["images"].shape[2:]
    N = len(g["op"])
    eng = get_engine("Resnet18", 5, H, W, N)
    params = np.asarray([fixed_point_params(g["matrices"][i], g["flips"][i]) for i in range(N)], np.int32)
    strong = strong_records({k: g[k] for k in ("op", "v", "apply", "sign", "cut")}, H, W)
    out = run(eng, g["images"], g["image_index"], params, strong).cpu().numpy()
    for i in range(N):                                           # what Pillow + ToTensor + Normalize produced, bit for bit, every case
        np.testing.assert_array_equal(out[i], g["out_f32"][i], err_msg=f"case {i}: ops {g['op'][i]} apply {g['apply'][i]}")


def test_strong_equals_restatement_at_224_on_the_benchmarked_batch():
    from fedmlp_amd.engine import get_engine
    from fedmlp_amd.augment import (draw_matrices, draw_strong_symbolic, fixed_point_params, strong_records, IMAGENET_MEAN,
                                    IMAGENET_STD)
    from tests import strong_ref as R
    H = W = 224
    B = 128
    gen = torch.Generator().manual_seed(SEED_224)
    mats, flips = draw_matrices(B, H, W, gen)
    sym = draw_strong_symbolic(B, H, W, gen)
    for s in range(2):                                           # the batch cannot pass by drawing little
        assert set(sym["op"][sym["apply"][:, s] == 1, s]) == set(range(14)), s
    imgs = structured_images(8, H, W, 7)
    sel = np.random.RandomState(1).randint(0, len(imgs), size=B)
    params = np.asarray([fixed_point_params(mats[b], flips[b]) for b in range(B)], np.int32)
    eng = get_engine("Resnet18", 5, H, W, B)
    strong = strong_records(sym, H, W)
    out = run(eng, imgs, sel, params, strong).cpu().numpy()
    again = run(eng, imgs, sel, params, strong).cpu().numpy()
    np.testing.assert_array_equal(out.view(np.int32), again.view(np.int32))          # the histogram path is order-independent
    for b in range(B):
        slots = [(R.OPS[sym["op"][b, s]] if sym["apply"][b, s] else R.SKIP, int(sym["v"][b, s]), int(sym["sign"][b, s]))
                 for s in range(2)]
        want = R.strong_ref(imgs[sel[b]], mats[b], flips[b], slots, tuple(strong[b, 16:20]), IMAGENET_MEAN, IMAGENET_STD)
        np.testing.assert_array_equal(out[b], want, err_msg=f"sample {b}: {slots}")


def test_both_slots_skipped_is_the_weak_view_with_a_grey_rectangle():
    from fedmlp_amd.engine import get_engine
    from fedmlp_amd.augment import draw_params, skip_strong, IMAGENET_MEAN, IMAGENET_STD
    H = W = 224
    B = 6
    eng = get_engine("Resnet18", 5, H, W, B)
    imgs = structured_images(4, H, W, 2)
    sel = [3, 0, 1, 1, 2, 0]
    params = draw_params(B, H, W, torch.Generator().manual_seed(9))
    strong = skip_strong(B, (0, 0, 0, 0))
    strong[:, 16:20] = [[0, 0, 16, 16], [100, 50, 116, 66], [215, 210, 224, 224], [0, 208, 8, 224], [223, 0, 224, 16], [60, 60, 76, 76]]
    dev = eng.device
    weak = eng.augment(torch.from_numpy(imgs).to(dev), torch.as_tensor(sel, dtype=torch.int32, device=dev),
                       torch.from_numpy(params).to(dev), IMAGENET_MEAN, IMAGENET_STD).cpu().numpy()
    out = run(eng, imgs, sel, params, strong).cpu().numpy()
    grey = ((np.float32(127) / np.float32(255) - np.asarray(IMAGENET_MEAN, np.float32)) / np.asarray(IMAGENET_STD, np.float32))
    for b in range(B):
        x0, y0, x1, y1 = strong[b, 16:20]
        inside = np.zeros((H, W), bool)
        inside[y0:y1 + 1, x0:x1 + 1] = True
        assert inside.any()
        np.testing.assert_array_equal(out[b][:, ~inside], weak[b][:, ~inside])
        for c in range(3):
            np.testing.assert_array_equal(out[b][c][inside], np.full(int(inside.sum()), grey[c], np.float32))


def test_batch_larger_than_the_handle_is_refused_with_an_error_code():
    from fedmlp_amd.engine import Engine
    from fedmlp_amd._lib import FmError
    from fedmlp_amd.augment import draw_params, draw_strong
    HW = 64
    eng = Engine("Resnet18", 5, HW, HW, 8)
    try:
        imgs = structured_images(3, HW, HW, 4)
        for B, ok in ((8, True), (9, False)):
            g = torch.Generator().manual_seed(B)
            args = (imgs, np.arange(B) % 3, draw_params(B, HW, HW, g), draw_strong(B, HW, HW, g))
            if ok:
                assert torch.isfinite(run(eng, *args)).all()
            else:
                with pytest.raises(FmError, match="max_images"):
                    run(eng, *args)
        torch.cuda.synchronize()
    finally:
        eng.close()


def test_fixmatch_trains_on_the_strong_view():
    """LocalUpdate.train_FixMatch on AugmentedDataset(strong=True): the second view is the strong one (it differs from the first and
    every sample carries the 127-grey rectangle), and a round returns a finite loss."""
    from fedmlp_amd.augment import AugmentedDataset, IMAGENET_MEAN, IMAGENET_STD
    from fedmlp_amd.model import build_model
    from fedmlp_amd.local_training import LocalUpdate
    from tests.helpers import make_args
    from tests.synth import class_lists
    C, HW, N = 4, 64, 48
    rs = np.random.RandomState(3)
    imgs = structured_images(N, HW, HW, 11)
    targets = (rs.uniform(size=(N, C)) < 0.3).astype(np.float32)
    targets[0, :] = 1
    ds = AugmentedDataset(imgs, targets, train=True, generator=torch.Generator().manual_seed(5), strong=True)
    args = make_args(n_classes=C, batch_size=16)
    pos, neg = class_lists(targets, C)
    net = build_model(make_args(n_classes=C, pretrained=0, batch_size=16))
    loc = LocalUpdate(args, 1, ds, list(range(N)), pos, neg, active_class_list=[1])
    eng = loc._bind(net, "image_aug_1")
    which = list(range(12))
    v1 = loc._images(eng, "image_aug_1", which)
    v2 = loc._images(eng, "image_aug_2", which)
    assert v2.shape == (12, 3, HW, HW) and v2.is_cuda and not torch.equal(v1, v2)
    grey = ((np.float32(127) / np.float32(255) - np.asarray(IMAGENET_MEAN, np.float32)) / np.asarray(IMAGENET_STD, np.float32))
    v2 = v2.cpu().numpy()
    for b in range(len(which)):
        is_grey = (v2[b, 0] == grey[0]) & (v2[b, 1] == grey[1]) & (v2[b, 2] == grey[2])
        ys, xs = np.nonzero(is_grey)
        # a filled rectangle of the cutout's size (17 x 17 inclusive, less where the right / bottom border clips it, never less
        # than 9 x 9) lies among the grey pixels
        best = max((int(is_grey[y:y + 17, x:x + 17].all()) * min(17, HW - y) * min(17, HW - x) for y, x in zip(ys, xs)), default=0)
        assert best >= 9 * 9, (b, best)
    ret = loc.train_FixMatch(0, net)
    assert np.isfinite(ret[1])
