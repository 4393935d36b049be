"""Per-step time of the autograd path (train-mode net(x) -> loss.backward() -> fedmlp_amd.optim.Adam.step()) against the
fused fm_step_bce, ResNet-18 at bs 128 x 224^2 by default, measured alternately in one process:
  fused      Engine.step_bce (forward + loss + backward + Adam in one call)
  one_view   one net(x) call, BCE with pos_weight in torch, backward into the accumulator, Adam
  two_views  net(x1), net(x2), one backward over both (the earlier call is recomputed), Adam
  one_view_dx  one_view with x.requires_grad: the backward also forms d loss / d x (the stem's data gradient) into x.grad
  one_view_frozen  one_view after net.freeze_bn(): every BatchNorm applies its running statistics, forward and backward
Device events around `--steps` steps after `--warmup`, repeated `--reps` times alternating the arms; prints one JSON line
(median and spread of the repetitions, ms per step)."""
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
from fedmlp_amd.model import HipNet  # noqa: E402
from fedmlp_amd.optim import Adam  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("autograd_step_time: needs a GPU")
    B, C, hw = a.batch, a.classes, a.hw
    flat, cnt = spec.init_state("Resnet18", C, 1037)
    net = HipNet("Resnet18", C, flat, cnt).train()
    net.default_max_images = B
    eng = net.bind(hw, hw, B)
    g = torch.Generator(device="cuda").manual_seed(0)
    x1 = torch.randn((B, 3, hw, hw), device="cuda", generator=g)
    x2 = torch.randn((B, 3, hw, hw), device="cuda", generator=g)
    y = (torch.rand((B, C), device="cuda", generator=g) < 0.3).float()
    pw = [2.0] * C
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(pw, device="cuda"), reduction="sum")
    opt = Adam(net, lr=3e-5, weight_decay=5e-4)
    lo = torch.zeros(1, device="cuda")

    def fused():
        eng.step_bce(x1, y, pw, B, lo)
        net.mark_trained()

    def one_view():
        _, z = net(x1)
        loss = crit(z, y) / (B * C)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def two_views():
        _, z1 = net(x1)
        _, z2 = net(x2)
        loss = (crit(z1, y) + crit(z2, y)) / (B * C)
        opt.zero_grad()
        loss.backward()
        opt.step()

    xg = x1.clone().requires_grad_(True)

    def one_view_dx():
        xg.grad = None
        _, z = net(xg)
        loss = crit(z, y) / (B * C)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def one_view_frozen():
        net.freeze_bn(True)
        try:
            one_view()
        finally:
            net.freeze_bn(False)

    arms = {"fused": fused, "one_view": one_view, "two_views": two_views, "one_view_dx": one_view_dx,
            "one_view_frozen": one_view_frozen}
    times = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, fn in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                fn()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / a.steps)
    out = {"batch": B, "hw": hw, "steps": a.steps, "reps": a.reps}
    for k, v in times.items():
        out[k + "_ms"] = round(float(np.median(v)), 3)
        out[k + "_spread_ms"] = round(float(max(v) - min(v)), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
