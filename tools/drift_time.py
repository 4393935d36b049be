"""What a client-drift correction costs a fused step: Engine.step_bce and Engine.step_stage1, ResNet-18 at bs 128 x 224^2 by
default, in one process, with three arms per step measured alternately:
  none       nothing installed (the yardstick: the launches of a handle that never heard of fm_drift_begin)
  fedprox    drift_begin(mu = 0.01): r = g + mu (p - a); 16 B per parameter
  scaffold   drift_begin(shift, track): r = g + s, S += g; 20 B per parameter
Device events around `--steps` back-to-back calls after `--warmup`, `--reps` times per arm; median and spread (max - min) of the
repetitions in ms per step.  Then the correction launch alone: fm_profile_ops' device events around the `drift_correct` launch
during `--steps` further step_bce calls per form (fedprox, scaffold, and both terms with track: 28 B per parameter, the Adam
launch's traffic), ms per launch and the bytes per second that makes.  Prints one JSON line; --out also writes it to a file."""
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
from fedmlp_amd.drift import drift_active, drift_begin, drift_end  # noqa: E402
from fedmlp_amd.engine import Engine  # noqa: E402

ARMS = ("none", "fedprox", "scaffold")
BYTES = {"fedprox": 16, "scaffold": 20, "both": 28}       # per parameter: g, r (+ p, a) (+ s) (+ S read and written)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model", choices=["Resnet18", "Efficient_b0"], default="Resnet18")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("drift_time: needs a GPU")
    B, C, hw = a.batch, a.classes, a.hw
    eng = Engine(a.model, C, hw, hw, 2 * B)
    eng.stochastic = False
    eng.set_state(*spec.init_state(a.model, C, 1037))
    eng.teacher_snapshot()
    g = torch.Generator(device="cuda").manual_seed(0)
    x1 = torch.randn((B, 3, hw, hw), device="cuda", generator=g)
    x2 = torch.randn((B, 3, hw, hw), device="cuda", generator=g)
    y = (torch.rand((B, C), device="cuda", generator=g) < 0.3).float()
    shift = 1e-4 * torch.randn(eng.nf, device="cuda", generator=g)
    pw, act = [2.0] + [5.0] * (C - 1), [1.0] + [0.0] * (C - 1)
    lo = torch.zeros(1, device="cuda")
    n_params = int(eng.debug_optim_arena(0).numel())       # the trainable arena the launch streams, layout padding included

    steps = {"bce": lambda: eng.step_bce(x1, y, pw, B, lo), "stage1": lambda: eng.step_stage1(x1, x2, y, act, 1, B, lo)}

    def install(arm):
        if drift_active(eng):
            drift_end(eng, mean=False)
        eng.adam_reset(3e-5, (0.9, 0.999), 1e-8, 5e-4)      # every window starts from a fresh optimizer
        if arm == "fedprox":
            drift_begin(eng, mu=0.01)
        elif arm == "scaffold":
            drift_begin(eng, shift=shift, track=True)
        elif arm == "both":
            drift_begin(eng, mu=0.01, shift=shift, track=True)

    out = {"model": a.model, "batch": B, "hw": hw, "classes": C, "steps": a.steps, "reps": a.reps, "arena_floats": n_params,
           "stream_mode": int(eng.lib.fm_stream_mode(eng.h))}
    for sname, fn in steps.items():
        times = {k: [] for k in ARMS}
        for arm in ARMS:
            install(arm)
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for arm in ARMS:
                install(arm)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.steps):
                    fn()
                t1.record()
                t1.synchronize()
                times[arm].append(t0.elapsed_time(t1) / a.steps)
        for arm in ARMS:
            v = times[arm]
            out[f"{sname}_{arm}_ms"] = round(float(np.median(v)), 4)
            out[f"{sname}_{arm}_spread_ms"] = round(float(max(v) - min(v)), 4)
    # the launch alone (profiled windows: the per-op events slow the host, so no step time is taken here)
    for form in ("fedprox", "scaffold", "both"):
        install(form)
        eng.profile_ops(True)
        for _ in range(a.steps):
            steps["bce"]()
        rows = [(n, ms) for lab, n, ms in eng.profile_ops(False) if lab.startswith("drift_correct")]
        n, ms = sum(r[0] for r in rows), sum(r[1] for r in rows)
        assert n == a.steps, (form, rows)
        out[f"launch_{form}_ms"] = round(ms / n, 5)
        out[f"launch_{form}_GBps"] = round(BYTES[form] * n_params / (ms / n * 1e-3) / 1e9, 1)
    install("none")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
