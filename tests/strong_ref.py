"""Numpy restatement of the FixMatch strong view (TEST SUPPORT ONLY): the 14 ops of the reference's
fixmatch_augment_pool() (utils/FixMatch.py:147-163) and CutoutAbs (:46-59) on uint8 [3,H,W] images, written from
Pillow's arithmetic:

* ImageEnhance.{Brightness, Color, Contrast, Sharpness}: Image.blend(degenerate, image, factor), libImaging/Blend.c
  for 0 <= factor <= 1: (UINT8)((int)d + alpha * ((int)x - (int)d)) with alpha a C float, product and sum rounded
  separately, the cast truncating.  Degenerates: black; convert("L") (libImaging/Convert.c
  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16); the constant int(mean(L) + 0.5) (ImageStat, a double mean);
  ImageFilter.SMOOTH (libImaging/Filter.c 3x3, kernel (1,1,1,1,5,1,1,1,1)/13, offset 0, +0.5 and truncation, the
  border row / column copied).  The smoothed value is T/13 + 0.5 with T an integer; its distance to the nearest
  integer is at least 1/26, far above fp32 rounding, so floor((2T + 13) / 26) is the same number.
* ImageOps.{autocontrast, equalize, posterize, solarize}: per-channel 256-entry LUTs (ImageOps.py).
* Image.rotate (Image.py: matrix of round(cos, 15) / round(sin, 15) about (W/2, H/2)) and Image.transform(AFFINE)
  for ShearX/Y, TranslateX/Y: NEAREST through the 16.16 fixed-point walk that oracle.augment_ref already restates.
* ImageDraw.rectangle: both corners inclusive.

Pinned by tests/golden/augment_strong_pil.npz (outputs of Pillow and of the reference's own op functions).
"""
import math

import numpy as np

from oracle.augment_ref import affine_nearest_u8

OPS = ("AutoContrast", "Brightness", "Color", "Contrast", "Equalize", "Identity", "Posterize", "Rotate",
       "Sharpness", "ShearX", "ShearY", "Solarize", "TranslateX", "TranslateY")
SKIP = "Skip"
SIGNED = ("Rotate", "ShearX", "ShearY", "TranslateX", "TranslateY")
GEOMETRIC = SIGNED
HISTOGRAM = ("AutoContrast", "Equalize", "Contrast")
CUTOUT = 16
GREY = 127


def blend_factor(v):
    return np.float32(float(v) * 0.9 / 10 + 0.05)


def _blend(d, x, f):
    d = d.astype(np.float32)
    t = np.float32(f) * (x.astype(np.float32) - d)                 # fp32 product, rounded
    return (d + t).astype(np.uint8)                                # fp32 sum, rounded, then truncated


def luma(img):
    r, g, b = (img[c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def smooth(img):
    a = img.astype(np.int64)
    out = a.copy()
    t = sum(a[:, 1 + dy:a.shape[1] - 1 + dy, 1 + dx:a.shape[2] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    t = t + 4 * a[:, 1:-1, 1:-1]
    out[:, 1:-1, 1:-1] = (2 * t + 13) // 26
    return out.astype(np.uint8)


def autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.asarray([min(max(int(ix * scale + offset), 0), 255) for ix in range(256)], np.uint8)


def equalize_lut(h):
    nz = [int(v) for v in h if v]
    if len(nz) <= 1:
        return np.arange(256, dtype=np.uint8)
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return np.arange(256, dtype=np.uint8)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(n // step)
        n += int(h[i])
    return np.minimum(np.asarray(lut, np.int64), 255).astype(np.uint8)      # Image.point clips the table to 8 bits


def _per_channel_lut(img, make):
    return np.stack([make(np.bincount(img[c].ravel(), minlength=256))[img[c]] for c in range(3)])


def rotate_matrix(deg, H, W):
    """Image.rotate(deg) for an angle that is no multiple of 90: the matrix it hands to transform(AFFINE)"""
    angle = -math.radians(deg % 360.0)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
         round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def geometric_matrix(op, v, sign, H, W):
    """the AFFINE matrix of a geometric op of the pool at magnitude v with its sign coin (sign = -1: the coin was < 0.5)"""
    if op == "Rotate":
        return rotate_matrix(sign * int(v * 30 / 10), H, W)
    s = sign * (float(v) * 0.3 / 10)
    if op == "ShearX":
        return [1, s, 0, 0, 1, 0]
    if op == "ShearY":
        return [1, 0, 0, s, 1, 0]
    if op == "TranslateX":
        return [1, 0, int(s * W), 0, 1, 0]
    if op == "TranslateY":
        return [1, 0, 0, 0, 1, int(s * H)]
    raise ValueError(op)


def posterize_mask(v):
    return ~(2 ** (8 - (int(v * 4 / 10) + 4)) - 1) & 0xFF


def solarize_threshold(v):
    return 256 - int(v * 256 / 10)


def apply_op(img, op, v, sign):
    """one op of the pool on uint8 [3,H,W] -> uint8 [3,H,W]"""
    _, H, W = img.shape
    if op in (SKIP, "Identity"):
        return img.copy()
    if op == "AutoContrast":
        return _per_channel_lut(img, autocontrast_lut)
    if op == "Equalize":
        return _per_channel_lut(img, equalize_lut)
    if op == "Brightness":
        return _blend(np.zeros_like(img), img, blend_factor(v))
    if op == "Color":
        return _blend(np.broadcast_to(luma(img), img.shape), img, blend_factor(v))
    if op == "Contrast":
        mean = int(float(luma(img).astype(np.int64).sum()) / (H * W) + 0.5)
        return _blend(np.full_like(img, mean), img, blend_factor(v))
    if op == "Sharpness":
        return _blend(smooth(img), img, blend_factor(v))
    if op == "Posterize":
        return img & np.uint8(posterize_mask(v))
    if op == "Solarize":
        return np.where(img < solarize_threshold(v), img, 255 - img).astype(np.uint8)
    return affine_nearest_u8(img, geometric_matrix(op, v, sign, H, W))


def cutout_corners(x0f, y0f, H, W, v=CUTOUT):
    """CutoutAbs' corner arithmetic on its two uniform draws"""
    x0 = int(max(0, x0f - v / 2.))
    y0 = int(max(0, y0f - v / 2.))
    return x0, y0, int(min(W, x0 + v)), int(min(H, y0 + v))


def cutout(img, corners):
    x0, y0, x1, y1 = corners
    out = img.copy()
    out[:, y0:y1 + 1, x0:x1 + 1] = GREY                            # inclusive corners; numpy clips at the border
    return out


def normalise(u8, mean, std):
    t = u8.astype(np.float32) / np.float32(255.0)
    mean = np.asarray(mean, np.float32)[:, None, None]
    std = np.asarray(std, np.float32)[:, None, None]
    return ((t - mean) / std).astype(np.float32)


def strong_u8(img, weak_matrix, flip, slots, corners):
    """weak affine + flip, the op slots [(op, v, sign), ...] in order, cutout: uint8 [3,H,W]"""
    a = affine_nearest_u8(img, weak_matrix)
    if flip:
        a = np.ascontiguousarray(a[:, :, ::-1])
    for op, v, sign in slots:
        a = apply_op(a, op, v, sign)
    return cutout(a, corners)


def strong_ref(img, weak_matrix, flip, slots, corners, mean, std):
    return normalise(strong_u8(img, weak_matrix, flip, slots, corners), mean, std)
