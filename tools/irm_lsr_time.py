"""Per-step time of the FedLSR step and of FedIRM's relation-phase step, each two ways, ResNet-18 at bs 128 x 224^2, stream mode 0
by default, measured alternately in one process:
  lsr_autograd   net(x1), net(x2), train_FedLSR's head in torch (float32, ~40 small launches), loss.backward() -- which
                 recomputes the first forward: three forwards per step -- and fedmlp_amd.optim.Adam.  Runs on any build: the baseline
  lsr_fused      Engine.step_fedlsr (fm_step_fedlsr): two-view forward, the head kernel, backward, Adam in one call
  fixmatch       Engine.step_fixmatch: the fused two-view step that exists already, the floor for a two-view step
  irm_autograd   the EMA model's train-mode forward (teacher slot), net(x1), net(x2), the relation-phase head in torch with its
                 mask.sum().item() host read, loss.backward(), Adam, the EMA blend (teacher_axpby: every state entry)
  irm_split      the same EMA forward, Engine.forward_train(x1, x2), Engine.loss_fedirm_rel, Engine.backward_step,
                 Engine.teacher_ema_params
Device events around `--steps` steps after `--warmup`, repeated `--reps` times alternating the arms; prints one JSON line (median
and spread of the repetitions, ms per step).  --arms a,b runs only those (a kernel trace of one arm).  An arm whose entry point the loaded library lacks is reported as null."""
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


def confuse_matrix(z, lab):
    den = (lab.sum(0) + 1e-8).to(z.dtype)
    return torch.sigmoid(lab.to(z.dtype).t() @ z / den[:, None] / 2.0)


def kd_loss(Q, P):
    F = torch.nn.functional
    return (F.kl_div(Q.log(), P, reduction="batchmean") + F.kl_div(P.log(), Q, reduction="batchmean")) / 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model", choices=["Resnet18", "Efficient_b0"], default="Resnet18")
    ap.add_argument("--arms", default="", help="comma list of arms to run (default: all), e.g. for a kernel trace of one arm")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("irm_lsr_time: needs a GPU")
    B, C, hw = a.batch, a.classes, a.hw
    flat, cnt = spec.init_state(a.model, C, 1037)
    net = HipNet(a.model, C, flat, cnt).train()
    net.default_max_images = 2 * B
    eng = net.bind(hw, hw, 2 * B)
    eng.stochastic = False
    eng.teacher_snapshot()                   # the EMA model starts as a copy of the student
    g = torch.Generator(device="cuda").manual_seed(0)
    x1 = torch.randn((B, 3, hw, hw), device="cuda", generator=g)
    x2 = x1 + 0.1 * torch.randn((B, 3, hw, hw), device="cuda", generator=g)
    y = (torch.rand((B, C), device="cuda", generator=g) < 0.3).float()
    pw, act = [2.0] * C, [1.0] + [0.0] * (C - 1)
    pwt = torch.tensor(pw, device="cuda")
    target = torch.sigmoid(torch.randn((C, C), device="cuda", generator=g))
    opt = Adam(net, lr=3e-5, betas=(0.9, 0.999), weight_decay=5e-4)
    mix1, beta, cw = 0.37, 0.4, 0.6
    lo = torch.zeros(1, device="cuda")
    F = torch.nn.functional

    def lsr_head(z1, z2):
        q1 = torch.clamp(torch.sigmoid(z1 * 3), min=1e-6, max=1.0)
        q2 = torch.clamp(torch.sigmoid(z2 * 3), min=1e-6, max=1.0)
        p = torch.sigmoid(z1) * mix1 + torch.sigmoid(z2) * (1 - mix1)
        pred = torch.sigmoid(torch.log(p / (1 - p)) * 2)
        lm = ((q1 + q2) / 2).log()
        js = (F.kl_div(lm, q1, reduction="mean") + F.kl_div(lm, q2, reduction="mean")) / 2
        return F.binary_cross_entropy_with_logits(pred, y, pos_weight=pwt) + js * beta

    def lsr_autograd():
        _, z1 = net(x1)
        _, z2 = net(x2)
        loss = lsr_head(z1, z2)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def lsr_fused():
        eng.step_fedlsr(x1, x2, y, pw, mix1, beta, lo)
        net.mark_trained()

    def fixmatch():
        eng.step_fixmatch(x1, x2, y, pw, pw, act, 1, B, lo)
        net.mark_trained()

    def ema_forward():
        eng.teacher_swap()
        _, zt = eng.forward_train(x2)
        eng.teacher_swap()
        return zt

    def irm_autograd():
        zt = ema_forward()
        _, z1 = net(x1)
        with torch.no_grad():
            p = torch.sigmoid(z1)
            unc = -1.0 * (torch.sum(p * torch.log(p + 1e-6), dim=1) + torch.sum((1 - p) * torch.log(1 - p + 1e-6), dim=1))
            mask = torch.all((p > 0.7) | (p < 0.3), dim=1) & (unc < 2.0)
        if mask.sum().item() != 0:
            source = confuse_matrix(z1[mask], p[mask] > 0.5)
        else:
            source = 0.5 * torch.ones((C, C), device="cuda")
        loss = cw * torch.sum((torch.sigmoid(z1) - torch.sigmoid(zt)) ** 2) / B + cw * torch.sum(kd_loss(source, target))
        _, z2 = net(x2)
        confuse_matrix(z1.detach(), y)
        sup = F.binary_cross_entropy_with_logits(z1, y, pos_weight=pwt, reduction="none") + \
            F.binary_cross_entropy_with_logits(z2, y, pos_weight=pwt, reduction="none")
        loss = loss + sup[:, :1].sum() / (B * 1)
        opt.zero_grad()
        loss.backward()
        opt.step()
        eng.teacher_axpby(0.99, 0.01)

    rel = torch.zeros((C, C), device="cuda")

    def irm_split():
        zt = ema_forward()
        _, z = eng.forward_train(x1, x2)
        dz, _ = eng.loss_fedirm_rel(z, zt, y, pw, act, 1, B, cw, target, rel)
        eng.backward_step(dz)
        eng.teacher_ema_params(0.99)
        net.mark_trained()

    arms = {"lsr_autograd": lsr_autograd, "fixmatch": fixmatch, "irm_autograd": irm_autograd}
    if hasattr(eng.lib, "fm_step_fedlsr"):
        arms["lsr_fused"] = lsr_fused
    if hasattr(eng.lib, "fm_loss_fedirm_rel"):
        arms["irm_split"] = irm_split
    if a.arms:
        arms = {k: arms[k] for k in a.arms.split(",")}
    times = {k: [] for k in arms}

    def prepare(k):
        eng.adam_reset(3e-5, (0.9, 0.999), 1e-8, 5e-4)      # every arm starts its window from a fresh optimizer

    for k, fn in arms.items():
        prepare(k)
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, fn in arms.items():
            prepare(k)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                fn()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / a.steps)
    out = {"model": a.model, "batch": B, "hw": hw, "classes": C, "steps": a.steps, "reps": a.reps,
           "stream_mode": int(eng.lib.fm_stream_mode(eng.h))}
    for k in ("lsr_autograd", "lsr_fused", "fixmatch", "irm_autograd", "irm_split"):
        v = times.get(k)
        out[k + "_ms"] = round(float(np.median(v)), 3) if v else None
        out[k + "_spread_ms"] = round(float(max(v) - min(v)), 3) if v else None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
