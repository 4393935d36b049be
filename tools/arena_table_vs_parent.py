"""Every kernel that walks the state arena's entry / chunk table (csrc/arena_table.h), run once on fixed inputs: one SHA-256 per
output, so two builds of the library (FEDMLP_HIP_LIB selects one, a fresh process per build) can be compared line by line --
tools/arena_table_vs_parent.sh does that.  ResNet-18 and EfficientNet-B0 (fp32) at 64 x 64, batch 4, 5 classes:
  1. forward_train + backward_grads twice under a mask that freezes one block (the masked accumulate: copy, then add);
  2. two steps each of adam / adamw / sgd_step_groups with three groups;
  3. those steps again with a drift correction (mu > 0, a shift, track) under the same mask (the masked drift kernel);
  4. the four server rules, two steps each with the norm, x_old 16-byte aligned and then offset by one float;
  5. state_dist with K = 3, ref offset by one float and ref = None.
Also printed: how many parameter entries begin off a 16-byte boundary, and how many of those have a full first chunk.
--time: device events around --steps back-to-back calls after --warmup calls, --reps times, one JSON line of microseconds per
call for adam_step_groups, the masked drift + AdamW pair, state_dist (K = 3) and the masked forward + backward (the only way to
the masked accumulate)."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fedmlp_amd import drift, server_opt, spec  # noqa: E402
from fedmlp_amd.engine import Engine  # noqa: E402

C_, HW, B = 5, 64, 4
ONE_BLOCK = {"Resnet18": "layer1.0", "Efficient_b0": "_blocks.1"}
ADAM = [(1e-3, (0.9, 0.999), 1e-8, 5e-4), (1e-4, (0.8, 0.99), 1e-8, 0.0), (1e-2, (0.95, 0.9), 1e-6, 5e-3)]
ADAMW = [(1e-3, (0.9, 0.999), 1e-8, 1e-2), (1e-4, (0.8, 0.99), 1e-8, 0.0), (1e-2, (0.95, 0.9), 1e-6, 5e-2)]
SGD = [(1e-2, 0.9, 0.0, 5e-4, True), (1e-3, 0.0, 0.0, 0.0, False), (1e-1, 0.8, 0.1, 1e-3, False)]
SERVER = dict(beta1=0.9, beta2=0.99, tau=1e-3)
SERVER_LR = {"avgm": 1.0, "adagrad": 1e-2, "adam": 1e-2, "yogi": 1e-2}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


class Run:
    def __init__(self, model):
        self.model = model
        self.eng = eng = Engine(model, C_, HW, HW, 2 * B)
        eng.stochastic = False
        ent = spec.entries(model, C_)
        self.params = [i for i, (k, _, dt) in enumerate(ent) if dt == "f32" and spec.is_trainable(k)]
        frozen = {i for i in self.params if ent[i][0].startswith(ONE_BLOCK[model] + ".")}
        assert frozen
        self.flags = [int(i in set(self.params) - frozen) for i in range(len(ent))]
        self.groups = [-1] * len(ent)
        for j, i in enumerate(self.params):
            self.groups[i] = j % 3
        self.state0 = spec.init_state(model, C_, 1037)
        g = torch.Generator().manual_seed(7)
        self.x = torch.randn((B, 3, HW, HW), generator=g).cuda()
        self.dz = torch.randn((B, C_), generator=g).cuda()
        self.shift = (1e-3 * torch.randn(eng.nf, generator=g)).cuda()
        self.noise = torch.randn(eng.state_tensor().numel(), generator=g).cuda()
        self.reset()

    def reset(self):
        eng = self.eng
        eng.set_state(*self.state0)
        eng.adam_reset(1e-3)
        eng.zero_grad()
        eng.set_trainable(self.flags)
        eng.optim_groups(self.groups, 3)

    def backward(self):
        self.eng.forward_train(self.x)
        self.eng.backward_grads(self.dz)

    def step(self, kind):
        if kind == "adam":
            self.eng.adam_step_groups(ADAM)
        elif kind == "adamw":
            self.eng.adamw_step_groups(ADAMW)
        else:
            self.eng.sgd_step_groups(SGD)

    def new_optimizer(self, kind):
        if kind == "sgd":
            self.eng.sgd_reset()
        else:
            self.eng.adam_reset(1e-3)

    def arenas(self, tag):
        eng = self.eng
        for name, t in (("state", eng.state_tensor()), ("m", eng.debug_optim_arena(0)), ("v", eng.debug_optim_arena(1)),
                        ("acc", eng.debug_optim_arena(2))):
            print(f"{self.model} {tag} {name} {sha(t)}")

    # ---- the outputs ----------------------------------------------------------------------------------------------------
    def outputs(self):
        eng, model = self.eng, self.model
        spans = eng.debug_entry_spans()
        off = [(int(o), int(n)) for o, n in spans if o >= 0]
        print(f"{model} parameter entries {len(off)}, beginning off a 16-byte boundary {sum(o % 4 != 0 for o, _ in off)}, "
              f"of those with a full first chunk {sum(o % 4 != 0 and n >= 8192 for o, n in off)}")
        self.backward()
        self.arenas("backward1")
        self.backward()
        self.arenas("backward2")
        for corrected in (False, True):
            if corrected:
                drift.drift_begin(eng, mu=0.01, shift=self.shift, track=True)
            for kind in ("adam", "adamw", "sgd"):
                self.new_optimizer(kind)
                for s in range(2):
                    self.step(kind)
                    tag = f"{'drift_' if corrected else ''}{kind}{s + 1}"
                    self.arenas(tag)
                    if corrected:
                        print(f"{model} {tag} gcorr {sha(drift.drift_last(eng))}")
            if corrected:
                mean, steps = drift.drift_end(eng)
                print(f"{model} drift_end steps {steps} gsum_mean {sha(mean)}")
        old = eng.state_tensor().clone()
        shifted = torch.empty(old.numel() + 1, device="cuda")[1:]
        shifted.copy_(old)
        assert old.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
        agg = old + 1e-3 * self.noise
        for rule in server_opt.RULES:
            eng.state_tensor().copy_(agg)
            server_opt.server_begin(eng, rule, SERVER_LR[rule], **SERVER)
            for s, x_old in enumerate((old, shifted)):
                norm = server_opt.server_step(eng, x_old)
                _, m, v = server_opt.server_get_state(eng)
                print(f"{model} server_{rule}{s + 1} norm {sha(norm)} state {sha(eng.state_tensor())} m {sha(m)} v {sha(v)}")
            server_opt.server_end(eng)
        states = [old + (k + 1) * 1e-3 * self.noise.roll(k) for k in range(3)]
        print(f"{model} state_dist ref_off1 {sha(eng.state_dist(states, ref=shifted))}")
        print(f"{model} state_dist ref_none {sha(eng.state_dist(states))}")

    # ---- the times ------------------------------------------------------------------------------------------------------
    def times(self, a):
        eng = self.eng
        self.backward()
        old = eng.state_tensor().clone()
        states = [old + (k + 1) * 1e-3 * self.noise.roll(k) for k in range(3)]

        def drift_adamw():
            self.step("adamw")

        lines = {"masked_forward_backward": self.backward, "state_dist_k3": lambda: eng.state_dist(states),
                 "adam_step_groups": lambda: self.step("adam"), "masked_drift_adamw_pair": drift_adamw}
        out = {"model": self.model, "lib": os.path.basename(os.environ.get("FEDMLP_HIP_LIB") or "libfedmlp_hip.so"),
               "steps": a.steps, "warmup": a.warmup, "reps": a.reps}
        for name, fn in lines.items():
            if name == "masked_drift_adamw_pair":
                drift.drift_begin(eng, mu=0.01, shift=self.shift, track=True)
            vals = []
            for _ in range(a.reps):
                for _ in range(a.warmup):
                    fn()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.steps):
                    fn()
                t1.record()
                t1.synchronize()
                vals.append(t0.elapsed_time(t1) / a.steps * 1e3)
            if name == "masked_drift_adamw_pair":
                drift.drift_end(eng, mean=False)
            out[name + "_us"] = [round(v, 2) for v in vals]
        print(json.dumps(out), flush=True)


def judge(lines_path, server_paths, out_path):
    """--time lines of both libraries (and tools/server_opt_time.py's files, parent first) -> one record per timed line: the
    medians, the parent's spread (max - min over its repetitions) and whether new median <= parent median + parent spread"""
    pooled = {}
    with open(lines_path) as f:
        for rec in map(json.loads, f):
            side = "parent" if "parent" in rec["lib"] else "new"
            for k, v in rec.items():
                if k.endswith("_us"):
                    pooled.setdefault((rec["model"], k[:-3]), {"parent": [], "new": []})[side] += v
    out = []
    for (model, name), t in pooled.items():
        pm, nm, spread = float(np.median(t["parent"])), float(np.median(t["new"])), max(t["parent"]) - min(t["parent"])
        out.append({"model": model, "line": name, "parent_us": t["parent"], "new_us": t["new"], "parent_median_us": round(pm, 2),
                    "new_median_us": round(nm, 2), "parent_spread_us": round(spread, 2), "holds": bool(nm <= pm + spread)})
    if server_paths:
        par, new = (json.load(open(p)) for p in server_paths)
        for rp, rn in zip(par, new):
            for rule in server_opt.RULES:
                pm, nm, spread = rp[f"{rule}_launch_us"], rn[f"{rule}_launch_us"], rp[f"{rule}_launch_spread_us"]
                out.append({"model": rp["model"], "line": f"server_{rule}", "parent_median_us": pm, "new_median_us": nm,
                            "parent_spread_us": spread, "new_spread_us": rn[f"{rule}_launch_spread_us"], "holds": bool(nm <= pm + spread)})
    for r in out:
        print(f"{r['model']:13s} {r['line']:24s} parent {r['parent_median_us']:9.2f} us (spread {r['parent_spread_us']:7.2f})  new "
              f"{r['new_median_us']:9.2f} us  {'holds' if r['holds'] else 'MISSES'}")
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--judge", nargs="+", metavar="FILE", help="LINES.jsonl [SERVER_PARENT.json SERVER_NEW.json] OUT.json: no GPU")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.judge:
        return judge(a.judge[0], a.judge[1:-1], a.judge[-1])
    if not torch.cuda.is_available():
        raise SystemExit("arena_table_vs_parent: needs a GPU")
    for model in ("Resnet18", "Efficient_b0"):
        run = Run(model)
        if a.time:
            run.times(a)
        else:
            run.outputs()
        torch.cuda.synchronize()
        run.eng.close()


if __name__ == "__main__":
    main()
