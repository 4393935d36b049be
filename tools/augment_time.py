"""Time of the input-pipeline kernels at bs 128 x 224^2 on a 5 000-image uint8 cache, measured alternately in one process:
  weak          fm_augment (RandomAffine + HFlip + Normalize), the yardstick
  strong        fm_augment_strong with seeded RandAugmentMC(2, 10) draws
  strong_skip   fm_augment_strong with both op slots skipped (weak + cutout: the fixed cost of its five launches)
  fixmatch_weak / fixmatch_strong   two views + one fm_step_fixmatch, the second view weak / strong
The records are uploaded once, so the kernel arms time device work only.  Device events around `--calls` calls after `--warmup`,
repeated `--reps` times alternating the arms; prints one JSON line (median and spread of the repetitions, microseconds per call
for the kernels, milliseconds per step for the two FixMatch arms, and the derived ratios)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fedmlp_amd import spec  # noqa: E402
from fedmlp_amd.augment import draw_params, draw_strong, skip_strong, IMAGENET_MEAN, IMAGENET_STD  # noqa: E402
from fedmlp_amd.engine import Engine  # noqa: E402

COPY_RATE = 6.3e12          # measured copy rate, bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_time: needs a GPU")
    B, C, hw, N = a.batch, a.classes, a.hw, a.images
    eng = Engine("Resnet18", C, hw, hw, 2 * B, device="cuda:0")
    flat, cnt = spec.init_state("Resnet18", C, 1037)
    eng.set_state(flat, cnt)
    eng.adam_reset(3e-5, (0.9, 0.999), 1e-8, 5e-4)
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    # structured pixels (a ramp plus noise), so that the histogram ops do real work
    cache = ((torch.arange(hw, device=dev).view(1, 1, 1, hw) + torch.randint(0, 96, (N, 3, hw, hw), device=dev, generator=g)) % 256
             ).to(torch.uint8).contiguous()
    hg = torch.Generator().manual_seed(1)
    idx = torch.randint(0, N, (B,), generator=hg).to(torch.int32).to(dev)
    params = torch.from_numpy(draw_params(B, hw, hw, hg)).to(dev)
    strong = torch.from_numpy(draw_strong(B, hw, hw, hg)).to(dev)
    skipped = torch.from_numpy(skip_strong(B, (100, 100, 116, 116))).to(dev)
    y = (torch.rand((B, C), device=dev, generator=g) < 0.3).float()
    lo = torch.zeros(1, device=dev)
    act = [1] + [0] * (C - 1)

    def weak():
        return eng.augment(cache, idx, params, IMAGENET_MEAN, IMAGENET_STD)

    def strong_view(rec=strong):
        return eng.augment_strong(cache, idx, params, rec, IMAGENET_MEAN, IMAGENET_STD)

    def fixmatch(second):
        eng.step_fixmatch(weak(), second(), y, [2.0] * C, [1.0] * C, act, 1, B, lo)

    arms = {"weak": (weak, a.calls), "strong": (strong_view, a.calls), "strong_skip": (lambda: strong_view(skipped), a.calls),
            "fixmatch_weak": (lambda: fixmatch(weak), a.steps), "fixmatch_strong": (lambda: fixmatch(strong_view), a.steps)}
    times = {k: [] for k in arms}
    for fn, _ in arms.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, (fn, n) in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(n):
                fn()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / n)
    out = {"batch": B, "hw": hw, "images": N, "calls": a.calls, "steps": a.steps, "reps": a.reps}
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        unit, scale = ("ms", 1.0) if k.startswith("fixmatch") else ("us", 1e3)
        out[f"{k}_{unit}"] = round(med[k] * scale, 3)
        out[f"{k}_spread_{unit}"] = round(float(max(v) - min(v)) * scale, 3)
    px = B * 3 * hw * hw
    # bytes the strong call really moves: cache read, A write, stats reads of A and B (at most), apply read + write, final read, fp32 write
    strong_bytes = px * (1 + 1 + 1 + 1 + 1 + 1 + 1 + 4)
    out["strong_over_weak"] = round(med["strong"] / med["weak"], 3)
    out["strong_floor_us"] = round(strong_bytes / COPY_RATE * 1e6, 2)
    out["strong_bytes_per_s"] = round(strong_bytes / (med["strong"] * 1e-3), 0)
    out["strong_share_of_fixmatch_step"] = round(med["strong"] / med["fixmatch_strong"], 4)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
