#!/usr/bin/env python3
"""Golden vectors for the FixMatch strong view, produced by PILLOW and by THE REFERENCE'S OWN op functions in the
build container (Pillow 12.2; neither is available to the GPU tests).

The reference's utils/FixMatch.py is loaded by path and its pool functions and CutoutAbs are called on seeded uint8
images, after the weak Image.transform(AFFINE, NEAREST, fill 0) + flip of make_augment_golden.py.  random.random and
np.random.uniform are pinned for each call, so the recorded sign and cutout position are the ones used.  Each case is
a chain (slot 0, slot 1, cutout) as RandAugmentMC.__call__ (utils/FixMatch.py:212-219) would run it for that draw.
Writes tests/golden/augment_strong_pil.npz: input images, per case the image index, weak matrix, flip, the symbolic
draw (op index in fixmatch_augment_pool() order, v, apply coin, sign, cutout floats), the uint8 result and the
normalised fp32 result.
usage: python tests/golden/make_strong_golden.py /path/to/reference/utils/FixMatch.py"""
import importlib.util
import os
import sys
from unittest import mock

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fedmlp_amd.augment import inverse_affine_matrix, IMAGENET_MEAN, IMAGENET_STD   # noqa: E402

H, W = 64, 96
AC, BR, CO, CT, EQ, ID, PO, RO, SH, SX, SY, SO, TX, TY = range(14)
MUST_CHANGE = (AC, EQ, CT)
# (image, weak (angle, tx, ty), flip, slot 0, slot 1, cutout (x0, y0) draws); a slot is (op, v, sign) or
# (op, v, sign, False) for a slot whose coin said "do not apply"
CASES = [
    (1, (4.0, 1, -1), 0, (RO, 1, -1), (AC, 9, 1), (40.3, 30.9)),        # geometric -> AutoContrast: the fill enters the histogram
    (0, (-7.5, -2, 1), 1, (SX, 9, 1), (EQ, 1, 1), (70.2, 12.5)),        # geometric -> Equalize
    (1, (10.0, 1, -1), 0, (AC, 1, 1), (RO, 9, 1), (20.0, 50.0)),        # histogram op first, geometric second
    (2, (-3.0, 0, 0), 1, (EQ, 9, 1), (SX, 1, -1), (55.5, 33.3)),
    (0, (2.0, 2, 1), 0, (SH, 1, 1), (CT, 9, 1), (10.1, 40.7)),          # Sharpness first
    (1, (-9.0, -1, 0), 1, (CT, 1, 1), (SH, 9, 1), (80.9, 20.2)),        # Sharpness second, Contrast first
    (2, (0.0, 0, 0), 0, (BR, 1, 1), (BR, 9, 1), (48.0, 32.0)),          # the same op twice; Pillow's scale-only weak path
    (0, (6.0, 1, 1), 1, (CO, 1, 1), (PO, 1, 1), (30.6, 8.4)),
    (2, (-5.0, -1, -1), 0, (PO, 9, 1), (CO, 9, 1), (60.0, 45.0)),
    (0, (8.0, 0, 1), 1, (SO, 1, 1), (SO, 9, 1), (25.5, 25.5)),
    (2, (-1.0, 2, 0), 0, (SY, 1, -1), (SY, 9, 1), (66.6, 36.6)),
    (0, (3.0, -2, -1), 1, (TX, 1, -1), (TX, 9, 1), (35.0, 15.0)),
    (1, (-6.0, 1, 1), 0, (TY, 9, -1), (TY, 1, 1), (75.0, 48.0)),
    (2, (5.0, 0, -1), 1, (ID, 1, 1), (ID, 9, 1), (50.0, 10.0)),
    (0, (-2.0, 1, 0), 0, (CT, 5, 1, False), (RO, 4, -1, False), (3.7, 5.2)),     # both skipped; cutout clipped left / top
    (1, (7.0, -1, 1), 1, (SH, 3, 1, False), (PO, 5, 1), (93.8, 61.4)),           # cutout clipped right / bottom
]


def images():
    rs = np.random.RandomState(20241)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ramp = np.stack([xs * 255.0 / (W - 1), ys * 255.0 / (H - 1), (xs + ys) * 255.0 / (W + H - 2)])
    a = np.clip(ramp * 0.9 + rs.randint(0, 4, size=ramp.shape), 0, 255)              # a ramp mixed with noise
    b = a * 0.5 + 40                                                                  # a narrow range
    c = np.clip(96 + 64 * np.sin(xs / 7.0)[None] * np.cos(ys / 5.0)[None] * np.asarray([1.0, 0.6, -0.8])[:, None, None]
                + rs.randint(0, 3, size=ramp.shape), 0, 255)                         # smooth blobs, per-channel range
    return np.stack([a, b, c]).astype(np.uint8)


def main():
    spec = importlib.util.spec_from_file_location("reference_fixmatch", sys.argv[1])
    fm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fm)
    pool = fm.fixmatch_augment_pool()
    assert [f.__name__ for f, _a, _b in pool] == ["AutoContrast", "Brightness", "Color", "Contrast", "Equalize", "Identity",
                                                  "Posterize", "Rotate", "Sharpness", "ShearX", "ShearY", "Solarize",
                                                  "TranslateX", "TranslateY"]
    imgs = images()
    mean = np.asarray(IMAGENET_MEAN, np.float32)[:, None, None]
    std = np.asarray(IMAGENET_STD, np.float32)[:, None, None]
    rec = {k: [] for k in ("image_index", "matrices", "flips", "op", "v", "apply", "sign", "cut", "out_u8", "out_f32")}
    for ii, (angle, tx, ty), flip, s0, s1, cut in CASES:
        m = inverse_affine_matrix((W * 0.5, H * 0.5), angle, (tx, ty))
        pil = Image.fromarray(imgs[ii].transpose(1, 2, 0)).transform((W, H), Image.AFFINE, m, Image.NEAREST, fillcolor=0)
        if flip:
            pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
        ops, vs, aps, sgs = [], [], [], []
        for slot in (s0, s1):
            op, v, sign = slot[:3]
            apply = len(slot) < 4
            if apply:
                fn, max_v, bias = pool[op]
                before = np.array(pil)
                with mock.patch("random.random", return_value=0.25 if sign < 0 else 0.75):
                    pil = fn(pil, v=v, max_v=max_v, bias=bias)
                if op in MUST_CHANGE:
                    assert not np.array_equal(before, np.array(pil)), (fn.__name__, "left its input unchanged")
            ops.append(op); vs.append(v); aps.append(int(apply)); sgs.append(sign)
        with mock.patch("numpy.random.uniform", side_effect=list(cut)):
            pil = fm.CutoutAbs(pil, int(32 * 0.5))
        a = np.array(pil).transpose(2, 0, 1)
        t = ((a.astype(np.float32) / np.float32(255.0) - mean) / std).astype(np.float32)
        for k, val in zip(rec, (ii, m, flip, ops, vs, aps, sgs, cut, a, t)):
            rec[k].append(val)
    dt = {"image_index": np.int32, "matrices": np.float64, "flips": np.int32, "op": np.int32, "v": np.int32,
          "apply": np.int32, "sign": np.int32, "cut": np.float64, "out_u8": np.uint8, "out_f32": np.float32}
    out = os.path.join(ROOT, "tests", "golden", "augment_strong_pil.npz")
    np.savez_compressed(out, images=imgs, **{k: np.asarray(v, dt[k]) for k, v in rec.items()})
    print("wrote augment_strong_pil.npz", len(CASES), "cases,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
