"""Per-step time of the RSCFed, FedNoRo (warm-up) and CBAFed (stage 2) steps, each two ways, ResNet-18 at bs 128 x 224^2, stream
mode 0 by default, measured alternately in one process:
  rscfed_split   Engine.forward_eval(x2, teacher), Engine.forward_train(x1), the head in torch on the [B, C] logits
                 (oracle.steps_ref.loss_rscfed, gradient by torch.autograd.grad), Engine.backward_step, Engine.teacher_axpby:
                 what train_RSCFed did before the fused step
  rscfed_fused   Engine.step_rscfed (fm_step_rscfed): one call
  fednoro_split  forward_eval(x, teacher), forward_train(x), oracle.steps_ref.loss_la_kd in torch, backward_step
  fednoro_fused  Engine.step_fednoro
  cbafed_split   forward_train(x), oracle.steps_ref.cbafed_stage2_targets -- two int(tensor.sum()) host reads per missing class --
                 and loss_cbafed_stage2 in torch, backward_step
  cbafed_fused   Engine.step_cbafed with tao: the decisions on the device, no host read
  bce            Engine.step_bce: the plain one-view fused step, the floor
The split arms form the torch head here, in the tool; the library has no such path any more.  Device events around `--steps` steps
after `--warmup`, repeated `--reps` times alternating the arms; prints one JSON line (median and spread of the repetitions, ms
per step).  --arms a,b runs only those."""
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
from fedmlp_amd.engine import Engine  # noqa: E402
from oracle import steps_ref as R  # noqa: E402

ARMS = ("rscfed_split", "rscfed_fused", "fednoro_split", "fednoro_fused", "cbafed_split", "cbafed_fused", "bce")


def head_grad(z, loss_fn):
    zl = z.detach().requires_grad_(True)
    loss = loss_fn(zl)
    (dz,) = torch.autograd.grad(loss, zl)
    return loss.detach(), dz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, default=0)
    ap.add_argument("--model", choices=["Resnet18", "Efficient_b0"], default="Resnet18")
    ap.add_argument("--arms", default="", help="comma list of arms to run (default: all)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("baseline_heads_time: needs a GPU")
    B, C, hw = a.batch, a.classes, a.hw
    eng = Engine(a.model, C, hw, hw, 2 * B, streams=a.streams)
    eng.stochastic = False
    eng.set_state(*spec.init_state(a.model, C, 1037))
    eng.teacher_snapshot()
    g = torch.Generator(device="cuda").manual_seed(0)
    x1 = torch.randn((B, 3, hw, hw), device="cuda", generator=g)
    x2 = x1 + 0.1 * torch.randn((B, 3, hw, hw), device="cuda", generator=g)
    y = (torch.rand((B, C), device="cuda", generator=g) < 0.3).float()
    pw, am = [2.0] * C, [1.0] + [0.0] * (C - 1)
    act, neg = [0], list(range(1, C))
    # thresholds just above 1/2: the fresh net's probabilities fall on both sides, so pseudo-labels are formed every step
    tao = [0.52] * C
    w_kd = 0.8 * 0.0067
    lo = torch.zeros(1, device="cuda")
    pw_dev = torch.tensor(pw, device="cuda")
    counts = torch.zeros(C + 1, dtype=torch.int64, device="cuda")
    host_w = list(pw)

    def rscfed_split():
        _, zt = eng.forward_eval(x2, teacher=True)
        _, z = eng.forward_train(x1)
        _, dz = head_grad(z, lambda zz: R.loss_rscfed(zz, zt, y, pw, act, neg, B, 1))
        eng.backward_step(dz)
        eng.teacher_axpby(1 - 0.001, 0.001)

    def rscfed_fused():
        eng.step_rscfed(x1, x2, y, pw, am, 1, B, 1 - 0.001, 0.001, lo)

    def fednoro_split():
        _, zt = eng.forward_eval(x1, teacher=True)
        _, z = eng.forward_train(x1)
        _, dz = head_grad(z, lambda zz: R.loss_la_kd(zz, zt, y, act, neg, w_kd))
        eng.backward_step(dz)

    def fednoro_fused():
        eng.step_fednoro(x1, y, am, w_kd, lo)

    def cbafed_split():
        _, z = eng.forward_train(x1)
        labels, idx_neg, w, _ = R.cbafed_stage2_targets(torch.sigmoid(z), y, neg, tao, host_w)
        host_w[:] = w
        _, dz = head_grad(z, lambda zz: R.loss_cbafed_stage2(zz, labels, idx_neg, w, act, neg, B, 1))
        eng.backward_step(dz)

    def cbafed_fused():
        eng.step_cbafed(x1, y, am, 1, B, tao, pw_dev, counts, lo)

    def bce():
        eng.step_bce(x1, y, pw, B, lo)

    fns = {"rscfed_split": rscfed_split, "rscfed_fused": rscfed_fused, "fednoro_split": fednoro_split,
           "fednoro_fused": fednoro_fused, "cbafed_split": cbafed_split, "cbafed_fused": cbafed_fused, "bce": bce}
    arms = {k: fns[k] for k in (a.arms.split(",") if a.arms else ARMS)}
    times = {k: [] for k in arms}

    def prepare():
        eng.adam_reset(3e-5, (0.9, 0.999), 1e-8, 5e-4)      # every arm starts its window from a fresh optimizer

    for fn in arms.values():
        prepare()
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, fn in arms.items():
            prepare()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                fn()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / a.steps)
    out = {"model": a.model, "batch": B, "hw": hw, "classes": C, "steps": a.steps, "reps": a.reps,
           "stream_mode": int(eng.lib.fm_stream_mode(eng.h))}
    for k in ARMS:
        v = times.get(k)
        out[k + "_ms"] = round(float(np.median(v)), 3) if v else None
        out[k + "_spread_ms"] = round(float(max(v) - min(v)), 3) if v else None
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
