"""What the server optimizer's launch costs, alone: fm_server_opt_step (one launch over the parameters plus the one-block norm
stage) against the same update composed of torch elementwise ops on the same tensors, for the four rules on ResNet-18 and
EfficientNet-B0 (the state's size is the model's: the engines are built at 32 x 32, batch 2).  A process that runs only this.
Device events around `--steps` back-to-back calls, after `--warmup` calls, `--reps` times per arm, the two arms alternating; every
window starts from the same aggregate and a fresh install.  Median and spread (max - min) of the repetitions in microseconds per
call, and the bytes per second the launch's 28 B (AVGM 20 B) per parameter make.  Both arms stream four arenas of the model's
size back to back, so whatever part of them the last-level cache holds helps both alike.  Prints one JSON line per model; --out
writes the list to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fedmlp_amd import server_opt, spec  # noqa: E402
from fedmlp_amd.engine import Engine  # noqa: E402

HP = dict(beta1=0.9, beta2=0.99, tau=1e-3)
LR = {"avgm": 1.0, "adagrad": 1e-2, "adam": 1e-2, "yogi": 1e-2}
BYTES = {"avgm": 20, "adagrad": 28, "adam": 28, "yogi": 28}


def composed(rule, a, x, m, v, lr):
    """the update as a user writes it today on eng.state_tensor(): torch ops over the parameter arena, one pass each"""
    b1, b2, tau = HP["beta1"], HP["beta2"], HP["tau"]
    d = a - x
    if rule == "avgm":
        m.mul_(b1).add_(d)
        a.copy_(x + lr * m)
        return
    m.mul_(b1).add_(d, alpha=1 - b1)
    q = d * d
    if rule == "adagrad":
        v.add_(q)
    elif rule == "adam":
        v.mul_(b2).add_(q, alpha=1 - b2)
    else:
        v.sub_((1 - b2) * q * torch.sign(v - q))
    a.copy_(x + lr * m / (v.sqrt() + tau))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--out", default="", help="also write the JSON list to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("server_opt_time: needs a GPU")
    results = []
    for model in ("Resnet18", "Efficient_b0"):
        eng = Engine(model, a.classes, 32, 32, 2)
        x0, cnt = spec.init_state(model, a.classes, 1037)
        eng.set_state(x0, cnt)
        old = eng.state_tensor().clone()
        n_params = int(eng.debug_optim_arena(0).numel())         # the parameter arena, layout padding included
        agg = old + 1e-3 * torch.randn(old.numel(), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        out = {"model": model, "arena_floats": n_params, "state_floats": int(old.numel()), "steps": a.steps, "reps": a.reps}
        for rule in server_opt.RULES:
            m = torch.zeros(n_params, device="cuda")
            v = torch.full((n_params,), HP["tau"] ** 2, device="cuda")

            def launch():
                server_opt.server_step(eng, old)

            def torch_ops():
                composed(rule, eng.state_tensor()[:n_params], old[:n_params], m, v, LR[rule])

            def window(fn):
                eng.state_tensor().copy_(agg)
                if server_opt.server_active(eng):
                    server_opt.server_end(eng)
                server_opt.server_begin(eng, rule, LR[rule], **HP)
                m.zero_(); v.fill_(HP["tau"] ** 2)
                for _ in range(a.warmup):
                    fn()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.steps):
                    fn()
                t1.record()
                t1.synchronize()
                return t0.elapsed_time(t1) / a.steps * 1e3

            times = {"launch": [], "torch": []}
            for _ in range(a.reps):
                times["launch"].append(window(launch))
                times["torch"].append(window(torch_ops))
            for arm, vals in times.items():
                out[f"{rule}_{arm}_us"] = round(float(np.median(vals)), 2)
                out[f"{rule}_{arm}_spread_us"] = round(float(max(vals) - min(vals)), 2)
            out[f"{rule}_launch_GBps"] = round(BYTES[rule] * n_params / (out[f"{rule}_launch_us"] * 1e-6) / 1e9, 1)
            server_opt.server_end(eng)
        print(json.dumps(out), flush=True)
        results.append(out)
        eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
