"""Per-step time of the autograd path (train-mode net(x) -> loss.backward() -> fedmlp_amd.optim.Adam.step()) against the
fused fm_step_bce, ResNet-18 (--model Efficient_b0: EfficientNet-B0, fp32) at bs 128 x 224^2 by default, measured alternately in
one process:
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
norm_only (Engine.grad_norm), clip_norm_only, clip_value_only -- ms per call.
--trainable all|head|top (a comma list runs several in the same process) adds, per mask T, the arms one_view[T] (one_view with only
that part of the net trainable: head = the classifier, top = layer4 + fc / _blocks.15 + head + _fc) and fwd_bwd[T] (its forward
and backward without the optimizer step: what the truncated backward saves).  The mask an arm runs under is installed once before its timed
loop, not inside a step; the fused arm and the unsuffixed arms run under the default one.
--groups 2 builds the optimizer with two parameter groups (the classifier, and everything else at a tenth of the learning rate):
optim_only is then the grouped step (fm_*_step_groups), single_only the single-group engine call of the same optimizer beside
it."""
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
    ap.add_argument("--model", choices=["Resnet18", "Efficient_b0"], default="Resnet18")
    ap.add_argument("--trainable", default="", help="comma list of all|head|top: per-mask one_view[T] / fwd_bwd[T] arms")
    ap.add_argument("--groups", type=int, choices=[1, 2], default=1, help="2: the optimizer has two parameter groups")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("autograd_step_time: needs a GPU")
    B, C, hw = a.batch, a.classes, a.hw
    flat, cnt = spec.init_state(a.model, C, 1037)
    net = HipNet(a.model, C, flat, cnt).train()
    net.default_max_images = B
    eng = net.bind(hw, hw, B)
    eng.stochastic = False                   # EfficientNet-B0: identity drop-connect / dropout multipliers in every arm
    head = ["fc"] if a.model == "Resnet18" else ["_fc"]
    parts = {"all": None, "head": head, "top": ["layer4", "fc"] if a.model == "Resnet18" else ["_blocks.15", "_conv_head", "_bn1", "_fc"]}
    masks = [t for t in a.trainable.split(",") if t]
    if any(t not in parts for t in masks):
        raise SystemExit("autograd_step_time: --trainable takes all, head, top")
    groups = None
    if a.groups == 2:
        rest = [k for k in net.trainable() if not any(k.startswith(h + ".") for h in head)]
        groups = [{"params": head}, {"params": rest, "lr": 3e-6}]
    g = torch.Generator(device="cuda").manual_seed(0)
    x1 = torch.randn((B, 3, hw, hw), device="cuda", generator=g)
    x2 = torch.randn((B, 3, hw, hw), device="cuda", generator=g)
    y = (torch.rand((B, C), device="cuda", generator=g) < 0.3).float()
    pw = [2.0] * C
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(pw, device="cuda"), reduction="sum")
    if a.optim == "adam":
        opt = Adam(net, lr=3e-5, weight_decay=5e-4, groups=groups)
    elif a.optim == "adamw":
        opt = AdamW(net, lr=3e-5, weight_decay=1e-2, groups=groups)
    else:
        opt = SGD(net, lr=1e-4, momentum=0.9, nesterov=True, weight_decay=5e-4, groups=groups)

    def mask(t):
        """install the mask an arm runs under (host bookkeeping; the engine is told when it changes)"""
        net.requires_grad_(True)
        if parts[t] is not None:
            net.requires_grad_(False).requires_grad_(True, parts[t])

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

    def fwd_bwd():
        _, z = net(x1)
        loss = crit(z, y) / (B * C)
        opt.zero_grad()
        loss.backward()

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

    def single_only():
        if a.optim == "adam":
            eng.adam_step(3e-5, weight_decay=5e-4)
        elif a.optim == "adamw":
            eng.adamw_step(3e-5, weight_decay=1e-2)
        else:
            eng.sgd_step(1e-4, 0.9, 0.0, 5e-4, True)
        net.mark_trained()

    # arm -> the mask it runs under, installed ONCE before its timed loop (and its warm-up), never inside a step
    under = {}
    arms = {"fused": fused, "one_view": one_view, "two_views": two_views, "one_view_dx": one_view_dx,
            "one_view_frozen": one_view_frozen}
    for t in masks:
        arms[f"one_view[{t}]"], arms[f"fwd_bwd[{t}]"] = one_view, fwd_bwd
        under[f"one_view[{t}]"] = under[f"fwd_bwd[{t}]"] = t
    arms.update({"optim_only": opt.step, "single_only": single_only, "adam_only": adam_only, "norm_only": eng.grad_norm,
                 "clip_norm_only": lambda: clip_grad_norm_(net, 1e30), "clip_value_only": lambda: clip_grad_value_(net, 1e30)})
    times = {k: [] for k in arms}
    def install(k):
        mask(under.get(k, "all"))
        net.bind(hw, hw, B)                  # tells the engine when the mask changed (the fused steps refuse a non-default one)

    for k, fn in arms.items():
        install(k)
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, fn in arms.items():
            install(k)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                fn()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / a.steps)
    out = {"model": a.model, "batch": B, "hw": hw, "steps": a.steps, "reps": a.reps, "optim": a.optim, "clip": a.clip,
           "trainable": masks, "groups": a.groups}
    for k, v in times.items():
        out[k + "_ms"] = round(float(np.median(v)), 3)
        out[k + "_spread_ms"] = round(float(max(v) - min(v)), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
