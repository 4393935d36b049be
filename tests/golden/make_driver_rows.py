#!/usr/bin/env python3
"""Recorder of tests/golden/driver_rows.json: every --exp row of fedmlp_amd.driver (and fedmlp_amd.driver_rofl) run through its
command-line surface only -- sys.argv, main(), --save_every 1 --save_dir TMP -- so the same file runs on any commit of the driver.
The driver seeds every RNG and the engine's kernels are deterministic: per round the record keeps mean_loss (JSON round-trips a
float exactly), a SHA-1 over the tensors of the saved model_<rnd>.pth in key order, and the `test` metrics where the row
evaluates.  The times (sec, eval_sec, samples_per_sec_per_gpu) are not recorded.

Every row runs TWICE; a row whose two runs differ in a recorded value is not written (and is named on stdout).  The FedMLP rows
are written only if some stage-2 call of LocalUpdate._select_all picked at least one clean and one noise sample (the thresholds
below are sized for 32 local samples).

usage (on a GPU, from the tree whose driver is to be recorded): python tests/golden/make_driver_rows.py [OUT.json [ROW ...]]"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COMMON = ["--model", "Resnet18", "--pretrained", "0", "--hw", "32", "--n_local", "32", "--batch_size", "16"]
SMALL = ["--n_clients", "2", "--n_classes", "4"]
FEDMLP = ["--exp", "FedMLP", "--rounds_FedMLP_stage1", "2", "--rounds_warmup", "4", "--clean_threshold", "0.5",
          "--noise_threshold", "0.5"] + SMALL
# the smallest settings that still cross every phase boundary of the row
ROWS = {
    "FedAVG": ["--exp", "FedAVG", "--rounds_warmup", "2"] + SMALL,
    "FedAVG_scaffold": ["--exp", "FedAVG", "--rounds_warmup", "2", "--scaffold", "1"] + SMALL,
    "FedAVG_eval": ["--exp", "FedAVG", "--rounds_warmup", "2", "--eval_every", "1", "--n_test", "64"] + SMALL,
    "FixMatch": ["--exp", "FedAVG+FixMatch", "--rounds_warmup", "2"] + SMALL,
    "FixMatch_augment2": ["--exp", "FedAVG+FixMatch", "--rounds_warmup", "2", "--augment", "2"] + SMALL,
    # a plain stage-1 round, the prototype round S1 - 1, the first stage-2 round, a stage-2 round with pools
    "FedMLP": FEDMLP,
    "FedMLP_prox": FEDMLP + ["--prox_mu", "0.01"],
    "FedLSR": ["--exp", "FedLSR", "--t_w", "3", "--rounds_warmup", "2"] + SMALL,
    # a supervised round, the first relation matrix at SI - 1, two relation-phase rounds
    # (four clients: a class nobody annotates has a NaN row in FedAvg_rela's matrix, and the relation-phase losses are NaN)
    "FedIRM": ["--exp", "FedIRM", "--rounds_FedIRM_sup", "2", "--rounds_warmup", "4", "--n_clients", "4", "--n_classes", "4"],
    "RSCFed": ["--exp", "RSCFed", "--n_clients", "6", "--n_classes", "4", "--rounds_warmup", "2"],
    "FedNoRo": ["--exp", "FedNoRo", "--rounds_warmup", "2"] + SMALL,
    # stage 2's 0.5 / 0.5 blend at round 7, the warm-up's 0.2 / 0.8 blend at round 5
    "CBAFed_stage2_blend": ["--exp", "CBAFed", "--rounds_CBAFed_warmup", "2", "--rounds_warmup", "8"] + SMALL,
    "CBAFed_warmup_blend": ["--exp", "CBAFed", "--rounds_CBAFed_warmup", "6", "--rounds_warmup", "7"] + SMALL,
    "RoFL": ["--rounds_warmup", "2"] + SMALL,              # through fedmlp_amd.driver_rofl
}


def model_sha1(path):
    import torch
    sd = torch.load(path, map_location="cpu")
    h = hashlib.sha1()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def run_row(name):
    """one run of ROWS[name] -> {"argv": [...], "rounds": [{"mean_loss", "sha1"[, "test"]} per round]}"""
    from fedmlp_amd import driver, driver_rofl
    argv = ROWS[name] + COMMON
    old = sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        sys.argv = [name] + argv + ["--save_every", "1", "--save_dir", tmp]
        try:
            log = (driver_rofl if name == "RoFL" else driver).main()
        finally:
            sys.argv = old
        rounds = []
        for rec in log:
            r = {"mean_loss": rec["mean_loss"], "sha1": model_sha1(os.path.join(tmp, f"model_{rec['round']}.pth"))}
            if "test" in rec:
                r["test"] = rec["test"]
            rounds.append(r)
    return {"argv": argv, "rounds": rounds}


def record(name):
    """the row's record, or None with the reason printed: two runs that differ, or a FedMLP run whose stage 2 selects nothing"""
    from fedmlp_amd.local_training import LocalUpdate
    picks = []
    real = LocalUpdate._select_all

    def spy(self, eng, rnd, classes, *a, **k):
        out = real(self, eng, rnd, classes, *a, **k)
        picks.append((rnd, sum(len(c) for c, _ in out), sum(len(n) for _, n in out)))
        return out
    LocalUpdate._select_all = spy
    try:
        first, second = run_row(name), run_row(name)
    finally:
        LocalUpdate._select_all = real
    if first != second:
        print(f"[make_driver_rows] {name}: NOT REPRODUCIBLE, not written\n  {first['rounds']}\n  {second['rounds']}", flush=True)
        return None
    if name.startswith("FedMLP"):
        print(f"[make_driver_rows] {name}: (round, clean, noise) per _select_all call: {picks}", flush=True)
        if not any(c >= 1 and n >= 1 for _, c, n in picks):
            print(f"[make_driver_rows] {name}: no stage-2 call selected a clean and a noise sample, not written", flush=True)
            return None
    return first


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "driver_rows.json")
    names = sys.argv[2:] or list(ROWS)
    rows = {}
    for name in names:
        rec = record(name)
        if rec is not None:
            rows[name] = rec
        with open(out, "w") as f:                        # after every row: a run that stops early leaves what it has
            json.dump(rows, f, indent=1)
            f.write("\n")
    print(f"[make_driver_rows] wrote {sorted(rows)}; left out {sorted(set(names) - set(rows))}", flush=True)


if __name__ == "__main__":
    main()
