"""Per-step time of the autograd path (train-mode net(x) -> loss.backward() -> fedmlp_amd.optim.Adam.step()) against the
fused fm_step_bce, ResNet-18 at bs 128 x 224^2 by default, measured alternately in one process:
  fused      Engine.step_bce (forward + loss + backward + Adam in one call)
  one_view   one net(x) call, BCE with pos_weight in torch, backward into the accumulator, Adam
  two_views  net(x1), net(x2), one backward over both (the earlier call is recomputed), Adam
  one_view_dx  one_view with x.requires_grad: the backward also forms d loss / d x (the stem's data gradient) into x.grad
  one_view_frozen  one_view after net.freeze_bn(): every BatchNorm applies its running statistics, forward and backward
Device events around `--steps` steps after `--warmup`, repeated `--reps` times alternating the arms; prints one JSON line
(median and spread of the repetitions, ms per step).
--optim adam|adamw|sgd picks the optimizer of the autograd arms (sgd: momentum 0.9, Nesterov, weight decay), --clip X calls
clip_grad_norm_(net, X) before every optimizer step.  The optimizer calls are also timed alone over the gradients the last
backward left: optim_only (opt.step()), adam_only (Engine.adam_step, the yardstick: the same arena, 28 B per parameter),
norm_only (Engine.grad_norm), clip_norm_only, clip_value_only -- ms per call."""
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
from fedmlp_amd.optim import SGD, Adam, AdamW, clip_grad_norm_, clip_grad_value_  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--optim", choices=["adam", "adamw", "sgd"], default="adam")
    ap.add_argument("--clip", type=float, default=None, help="clip_grad_norm_(net, X) before every optimizer step")
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
    if a.optim == "adam":
        opt = Adam(net, lr=3e-5, weight_decay=5e-4)
    elif a.optim == "adamw":
        opt = AdamW(net, lr=3e-5, weight_decay=1e-2)
    else:
        opt = SGD(net, lr=1e-4, momentum=0.9, nesterov=True, weight_decay=5e-4)

    def opt_step():
        if a.clip is not None:
            clip_grad_norm_(net, a.clip)
        opt.step()

    lo = torch.zeros(1, device="cuda")

    def fused():
        eng.step_bce(x1, y, pw, B, lo)
        net.mark_trained()

    def one_view():
        _, z = net(x1)
        loss = crit(z, y) / (B * C)
        opt.zero_grad()
        loss.backward()
        opt_step()

    def two_views():
        _, z1 = net(x1)
        _, z2 = net(x2)
        loss = (crit(z1, y) + crit(z2, y)) / (B * C)
        opt.zero_grad()
        loss.backward()
        opt_step()

    xg = x1.clone().requires_grad_(True)

    def one_view_dx():
        xg.grad = None
        _, z = net(xg)
        loss = crit(z, y) / (B * C)
        opt.zero_grad()
        loss.backward()
        opt_step()

    def one_view_frozen():
        net.freeze_bn(True)
        try:
            one_view()
        finally:
            net.freeze_bn(False)

    # the optimizer calls alone, over whatever the last backward left in the accumulator (a step does not empty it)
    def adam_only():
        eng.adam_step(3e-5, weight_decay=5e-4)
        net.mark_trained()

    arms = {"fused": fused, "one_view": one_view, "two_views": two_views, "one_view_dx": one_view_dx,
            "one_view_frozen": one_view_frozen, "optim_only": opt.step, "adam_only": adam_only, "norm_only": eng.grad_norm,
            "clip_norm_only": lambda: clip_grad_norm_(net, 1e30), "clip_value_only": lambda: clip_grad_value_(net, 1e30)}
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
    out = {"batch": B, "hw": hw, "steps": a.steps, "reps": a.reps, "optim": a.optim, "clip": a.clip}
    for k, v in times.items():
        out[k + "_ms"] = round(float(np.median(v)), 3)
        out[k + "_spread_ms"] = round(float(max(v) - min(v)), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
