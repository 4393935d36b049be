#!/usr/bin/env python3
"""Time the evaluation metrics on the device against the host path.

  metrics   fm_eval_metrics (Engine.eval_metrics, all three outputs) on seeded [N, C] scores / labels already in HBM: device
            events around back-to-back calls, warm, enough calls for a window of at least --window seconds; beside it
            multilabel_metrics_device (the call plus its one 6 C x 8-byte read) and the host's multilabel_metrics on the same
            arrays (a host clock, --threads threads at most).  Sizes: (32768, 8, prevalence 0.3), the paired mAP study's test
            set, and (131072, 14, prevalence 0.05).  Also printed: the pair pass's compares (P N + 2 P Nn per class, what the
            kernel does) per second.
  globaltest  end to end both ways at N = 4096 images of 3 x 224 x 224, ResNet-18, the two paths alternating in one process (a
            host clock around each call; both end in a device-to-host read).

Prints one JSON line.  usage: python tools/eval_time.py [--window 0.5] [--threads 16] [--skip-globaltest] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fedmlp_amd import evaluations as EV          # noqa: E402
from fedmlp_amd.engine import Engine              # noqa: E402


def problem(N, C, prev, seed):
    rs = np.random.RandomState(seed)
    y = (rs.uniform(size=(N, C)) < prev).astype(np.float32)
    z = (3.0 * rs.standard_normal((N, C)) + 2.0 * (y - prev)).astype(np.float32)     # a scorer with some signal
    p = torch.sigmoid(torch.from_numpy(z)).numpy()
    return y, p


def device_window(fn, window, warm=3):
    """the mean time of a call over one window of back-to-back calls between two device events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    reps, ms = 4, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= window * 1e3 or reps >= 1 << 16:
            return ms / reps, reps, ms
        reps = max(reps * 2, int(reps * window * 1e3 / max(ms, 1e-3)) + 1)


def host_window(fn, window):
    fn()
    ts, t_end = [], time.perf_counter() + window
    while not ts or time.perf_counter() < t_end:
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def time_metrics(eng, N, C, prev, window):
    y, p = problem(N, C, prev, 11)
    yd, pd = torch.from_numpy(y).to(eng.device), torch.from_numpy(p).to(eng.device)
    call_ms, reps, win_ms = device_window(lambda: eng.eval_metrics(pd, yd, 0.5), window)
    cnt_ms, _, _ = device_window(lambda: eng.eval_metrics(pd, yd, 0.5, ap=False, auc=False), window)
    read = host_window(lambda: EV.multilabel_metrics_device(eng, yd, pd), window)
    host = host_window(lambda: EV.multilabel_metrics(y, p), window)
    dev, ref = EV.multilabel_metrics_device(eng, yd, pd), EV.multilabel_metrics(y, p)
    P = y.sum(0).astype(np.float64)
    pairs = float((P * N + 2.0 * P * (N - P)).sum())
    return {"N": N, "C": C, "prevalence": prev, "fm_eval_metrics_ms": call_ms, "calls_in_window": reps, "window_ms": win_ms,
            "counts_only_ms": cnt_ms, "compares": pairs, "compares_per_s": pairs / (call_ms * 1e-3),
            "device_with_read_ms_median": float(np.median(read)), "host_ms_median": float(np.median(host)),
            "host_ms_min": float(np.min(host)), "host_reps": len(host), "host_over_device": float(np.median(host)) / call_ms,
            "mAP_device_minus_host": float(dev["mAP"]) - float(ref["mAP"]), "auc_device_minus_host": dev["auc"] - ref["auc"]}


class _Images:
    """N seeded images kept in HBM behind globaltest's dataset contract"""

    def __init__(self, n, C, hw, device):
        g = torch.Generator(device=device).manual_seed(5)
        self._v = {"image": torch.randn((n, 3, hw, hw), device=device, generator=g)}
        self.targets = (np.random.RandomState(6).uniform(size=(n, C)) < 0.3).astype(np.float32)

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return {"image": self._v["image"][i], "target": self.targets[i].copy(), "index": i}

    def device_views(self, device):
        return self._v


def time_globaltest(N, C, hw, bs, rounds):
    from fedmlp_amd.model import build_model
    args = argparse.Namespace(model="Resnet18", n_classes=C, batch_size=bs, seed=1037, pretrained=0)
    net = build_model(args)
    from fedmlp_amd.launch import default_device
    ds = _Images(N, C, hw, default_device())
    out = {"host": [], "device": []}
    for which in ("host", "device"):                       # warm both
        EV.globaltest(net, ds, args, device_metrics=which == "device")
    for _ in range(rounds):
        for which in ("host", "device"):                   # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            EV.globaltest(net, ds, args, device_metrics=which == "device")
            torch.cuda.synchronize()
            out[which].append((time.perf_counter() - t0) * 1e3)
    return {"N": N, "C": C, "hw": hw, "batch": 4 * bs, "host_path_ms": out["host"], "device_path_ms": out["device"],
            "host_path_ms_median": float(np.median(out["host"])), "device_path_ms_median": float(np.median(out["device"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-globaltest", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_num_threads(min(a.threads, 16))
    eng = Engine("Resnet18", 8, 64, 64, 8)
    res = {"metrics": [time_metrics(eng, 32768, 8, 0.3, a.window), time_metrics(eng, 131072, 14, 0.05, a.window)],
           "host_threads": torch.get_num_threads()}
    eng.close()
    if not a.skip_globaltest:
        res["globaltest"] = time_globaltest(4096, 8, 224, 32, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
