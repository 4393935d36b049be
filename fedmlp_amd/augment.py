"""Host side of the HBM-resident input pipeline.

The reference's train transform (dataset/dataset.py:40-53) is
Resize(224) -> RandomAffine(degrees=10, translate=(0.02, 0.02)) -> RandomHorizontalFlip ->
ToTensor -> Normalize(ImageNet mean/std), applied on PIL images by DataLoader workers, once per
view and per __getitem__ (dataset/all_dataset.py:66-91).  Resize precedes every random op, so
caching the resized uint8 pixels in HBM is exact; the random draws happen here (torchvision 0.13's
RandomAffine.get_params / RandomHorizontalFlip semantics and its _get_inverse_affine_matrix, restated:
torchvision is not vendored in the reference), the pixel work is the engine's fm_augment kernel, which
is bit-exact with Pillow's fixed-point nearest-neighbour affine (checked against Pillow's own outputs,
tests/golden/augment_pil.npz).  The ORDER of the reference's draws (worker-seeded RNG streams) is not
reproducible by construction: "parity unpinned" for that part only.

The FixMatch pair (dataset/dataset.py:63-77) adds RandAugmentMC(n=2, m=10) (utils/FixMatch.py:205-219) to the second
view: two ops of a pool of 14, each applied on a fair coin at a magnitude v in 1..9, then a 16-pixel grey cutout.
draw_strong() makes those draws and packs what does not depend on pixels into the int32[20] record of
fm_augment_strong (include/fedmlp_hip.h); the pixel work, histograms included, is the engine's, bit-exact with
Pillow 12.2 (tests/golden/augment_strong_pil.npz).
"""
import math

import numpy as np
import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def inverse_affine_matrix(center, angle, translate):
    """torchvision.transforms.functional._get_inverse_affine_matrix with scale 1, shear 0."""
    rot = math.radians(angle)
    cx, cy = center
    tx, ty = translate
    a, b, c, d = math.cos(rot), -math.sin(rot), math.sin(rot), math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def _fix16(v):
    t = float(v) * 65536.0 + 0.5                # Geometry.c FIX(): FLOOR(v * 65536.0 + 0.5)
    return int(t) if t >= 0.0 else int(math.floor(t))


def fixed_point_params(matrix, flip):
    """6 doubles + flip -> the int32[8] record fm_augment takes (include/fedmlp_hip.h)."""
    a0, a1, a2, a3, a4, a5 = [float(v) for v in matrix[:6]]
    return [_fix16(a0), _fix16(a1), _fix16(a2 + a0 * 0.5 + a1 * 0.5), _fix16(a3), _fix16(a4),
            _fix16(a5 + a3 * 0.5 + a4 * 0.5), int(bool(flip)), 0]


def draw_matrices(B, H, W, generator=None, degrees=10.0, translate=(0.02, 0.02), p_flip=0.5):
    """One RandomAffine + RandomHorizontalFlip draw per sample: (matrices [B,6] float64, flips [B]).
    angle ~ U(-deg, deg); tx, ty = round(U(-t*W, t*W)), round(U(-t*H, t*H)); flip ~ U(0,1) < p."""
    u = torch.rand((B, 4), generator=generator).numpy().astype(np.float64)
    mats = np.zeros((B, 6), np.float64)
    flips = np.zeros(B, np.int32)
    for b in range(B):
        angle = -degrees + 2 * degrees * u[b, 0]
        tx = int(round(-translate[0] * W + 2 * translate[0] * W * u[b, 1]))
        ty = int(round(-translate[1] * H + 2 * translate[1] * H * u[b, 2]))
        mats[b] = inverse_affine_matrix((W * 0.5, H * 0.5), angle, (tx, ty))
        flips[b] = 1 if u[b, 3] < p_flip else 0
    return mats, flips


def draw_params(B, H, W, generator=None, **kw):
    """[B,8] int32 parameter records of one draw per sample."""
    mats, flips = draw_matrices(B, H, W, generator, **kw)
    return np.asarray([fixed_point_params(mats[b], flips[b]) for b in range(B)], dtype=np.int32)


def identity_params(B):
    """the test-time transform (dataset/dataset.py:55-60: Resize -> ToTensor -> Normalize): no affine, no flip"""
    return np.asarray([fixed_point_params([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], 0)] * B, dtype=np.int32)


# ---- the strong view: RandAugmentMC(n=2, m=10) + CutoutAbs(16), utils/FixMatch.py:147-163, :205-219 ----------------
STRONG_OPS = ("AutoContrast", "Brightness", "Color", "Contrast", "Equalize", "Identity", "Posterize", "Rotate",
              "Sharpness", "ShearX", "ShearY", "Solarize", "TranslateX", "TranslateY")   # fixmatch_augment_pool() order
STRONG_SKIP = len(STRONG_OPS)                  # op code of a slot whose coin came up >= 0.5
STRONG_SLOTS = 2
STRONG_RECORD = 8 * STRONG_SLOTS + 4           # int32 per sample: two slots of 8, then the cutout corners
CUTOUT_ABS = 16


def _f32_bits(f):
    return int(np.asarray(f, np.float32).view(np.int32))


def rotate_matrix(deg, H, W):
    """Image.rotate(deg) (NEAREST, no expand): cos / sin rounded to 15 places, about (W/2, H/2)"""
    angle = -math.radians(deg % 360.0)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
         round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def strong_slot(op, v, sign, H, W):
    """one applied op of the pool -> the 8 int32 of its slot: {op code, parameter(s), 0 ...}"""
    name = STRONG_OPS[op]
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        par = [_f32_bits(float(v) * 0.9 / 10 + 0.05)]                  # _float_parameter(v, 0.9) + 0.05, a C float in blend
    elif name == "Posterize":
        par = [~(2 ** (8 - (int(v * 4 / 10) + 4)) - 1) & 0xFF]          # ImageOps.posterize keeps int(v*4/10) + 4 bits
    elif name == "Solarize":
        par = [256 - int(v * 256 / 10)]
    elif name == "Rotate":
        par = fixed_point_params(rotate_matrix(sign * int(v * 30 / 10), H, W), 0)[:6]
    elif name in ("ShearX", "ShearY", "TranslateX", "TranslateY"):
        s = sign * (float(v) * 0.3 / 10)
        m = {"ShearX": [1, s, 0, 0, 1, 0], "ShearY": [1, 0, 0, s, 1, 0], "TranslateX": [1, 0, int(s * W), 0, 1, 0],
             "TranslateY": [1, 0, 0, 0, 1, int(s * H)]}[name]
        par = fixed_point_params(m, 0)[:6]
    else:
        par = []
    return ([int(op)] + par + [0] * 8)[:8]


def cutout_corners(x0f, y0f, H, W, v=CUTOUT_ABS):
    """CutoutAbs (utils/FixMatch.py:46-59) on its two uniform draws: corners of an INCLUSIVE rectangle"""
    x0 = int(max(0, x0f - v / 2.))
    y0 = int(max(0, y0f - v / 2.))
    return [x0, y0, int(min(W, x0 + v)), int(min(H, y0 + v))]


def strong_records(sym, H, W):
    """symbolic draw (draw_strong_symbolic) -> [B,20] int32 records of fm_augment_strong"""
    op, v, ap, sg, cut = sym["op"], sym["v"], sym["apply"], sym["sign"], sym["cut"]
    B, n = op.shape
    assert n <= STRONG_SLOTS, "fm_augment_strong carries two op slots"
    rec = np.zeros((B, STRONG_RECORD), np.int32)
    for b in range(B):
        for s in range(STRONG_SLOTS):
            if s < n and ap[b, s]:
                rec[b, 8 * s:8 * s + 8] = strong_slot(int(op[b, s]), int(v[b, s]), int(sg[b, s]), H, W)
            else:
                rec[b, 8 * s] = STRONG_SKIP
        rec[b, 8 * STRONG_SLOTS:] = cutout_corners(float(cut[b, 0]), float(cut[b, 1]), H, W)
    return rec


def draw_strong_symbolic(B, H, W, generator=None, n=2, m=10):
    """RandAugmentMC.__call__ (utils/FixMatch.py:212-219) per sample: n ops uniformly with replacement from the pool,
    v = randint(1, m) (1..m-1), a fair coin for applying each, the sign coin of Rotate / Shear / Translate
    (random() < 0.5 -> negative), CutoutAbs' x0 ~ U(0, W), y0 ~ U(0, H).
    Returns {"op" [B,n] 0..13, "v" [B,n], "apply" [B,n] 0/1, "sign" [B,n] +1/-1, "cut" [B,2] float64}."""
    op = torch.randint(0, len(STRONG_OPS), (B, n), generator=generator).numpy().astype(np.int32)
    v = torch.randint(1, m, (B, n), generator=generator).numpy().astype(np.int32)
    u = torch.rand((B, 2 * n + 2), generator=generator, dtype=torch.float64).numpy()
    return {"op": op, "v": v, "apply": (u[:, :n] < 0.5).astype(np.int32),
            "sign": np.where(u[:, n:2 * n] < 0.5, -1, 1).astype(np.int32),
            "cut": u[:, 2 * n:] * np.asarray([W, H], np.float64)}


def draw_strong(B, H, W, generator=None, n=2, m=10):
    """[B,20] int32 strong records of one RandAugmentMC(n, m) + CutoutAbs(16) draw per sample"""
    return strong_records(draw_strong_symbolic(B, H, W, generator, n, m), H, W)


def skip_strong(B, corners):
    """records with both slots skipped and the given cutout corners (x0, y0, x1, y1): strong = weak + cutout"""
    rec = np.zeros((B, STRONG_RECORD), np.int32)
    rec[:, 0:8 * STRONG_SLOTS:8] = STRONG_SKIP
    rec[:, 8 * STRONG_SLOTS:] = np.asarray(corners, np.int32)
    return rec


class CachedAugmentedViews:
    """Per-client uint8 cache in HBM (N x 3 x H x W bytes: 752 MB for 5 000 ICH images) that hands out
    freshly augmented views of a batch (dataset/all_dataset.py:66-78) without touching the host pixels."""

    def __init__(self, engine, images_u8, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.engine = engine
        self.cache = torch.as_tensor(images_u8, dtype=torch.uint8).to(engine.device).contiguous()
        self.mean, self.std = mean, std

    def view(self, sample_idx, params):
        idx = torch.as_tensor(list(sample_idx), dtype=torch.int32, device=self.engine.device)
        p = torch.from_numpy(np.ascontiguousarray(params, dtype=np.int32)).to(self.engine.device)
        return self.engine.augment(self.cache, idx, p, self.mean, self.std)

    def view_strong(self, sample_idx, params, strong):
        """the FixMatch strong view: the weak records plus the [B,20] records of draw_strong"""
        dev = self.engine.device
        idx = torch.as_tensor(list(sample_idx), dtype=torch.int32, device=dev)
        p = torch.from_numpy(np.ascontiguousarray(params, dtype=np.int32)).to(dev)
        q = torch.from_numpy(np.ascontiguousarray(strong, dtype=np.int32)).to(dev)
        return self.engine.augment_strong(self.cache, idx, p, q, self.mean, self.std)

    def views(self, sample_idx, generator=None, n_views=2):
        H, W = self.engine.in_h, self.engine.in_w
        return [self.view(sample_idx, draw_params(len(sample_idx), H, W, generator)) for _ in range(n_views)]


class AugmentedDataset:
    """dataset/all_dataset.py:64-91 contract over an HBM-resident uint8 cache: every access to "image" /
    "image_aug_1" / "image_aug_2" of the TRAIN set is a fresh RandomAffine + HFlip draw (two independent
    draws for the two views, :75-76); a test set (train=False) gets the deterministic transform.
    strong=True is the FixMatch transform pair (dataset/dataset.py:63-77): "image_aug_2" of the train set is the
    weak draw followed by RandAugmentMC(n=2, m=10) and the cutout (fm_augment_strong); the other keys stay weak.
    LocalUpdate / globaltest ask for whole batches through device_batch(), so the pixels never leave HBM."""

    def __init__(self, images_u8, targets, train=True, generator=None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 strong=False):
        self.strong = bool(strong)
        self.images_u8 = torch.as_tensor(images_u8, dtype=torch.uint8)
        self.targets = np.asarray(targets, dtype=np.float32)
        self.train, self.generator = train, generator
        self.mean, self.std = mean, std
        self._cav = None

    def __len__(self):
        return len(self.targets)

    def _host_item(self, i):
        """Host-side single item (shape probing, small tests): same arithmetic on the CPU tensor."""
        x = self.images_u8[i].float().div(255.0)
        m = torch.tensor(self.mean).view(3, 1, 1); s = torch.tensor(self.std).view(3, 1, 1)
        return (x - m) / s

    def __getitem__(self, i):
        x = self._host_item(i)
        return {"image": x, "image_aug_1": x, "image_aug_2": x, "target": self.targets[i].copy(), "index": i}

    def device_batch(self, engine, key, sample_idx):
        if self._cav is None or self._cav.engine is not engine:
            self._cav = CachedAugmentedViews(engine, self.images_u8, self.mean, self.std)
        H, W = engine.in_h, engine.in_w
        p = draw_params(len(sample_idx), H, W, self.generator) if self.train else identity_params(len(sample_idx))
        if self.strong and self.train and key == "image_aug_2":
            return self._cav.view_strong(sample_idx, p, draw_strong(len(sample_idx), H, W, self.generator))
        return self._cav.view(sample_idx, p)
