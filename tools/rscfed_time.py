#!/usr/bin/env python3
"""Time one full RSCFed aggregation (utils/FedAvg.py:25-41) of ResNet-18 states: 8 clients, K = 6 per group, M = 10 groups.

Device path: fedavg.rscfed_device (per group one fm_state_dist, one read of the norms, one fm_fed_w; a final fm_fed_w),
timed with device events around the whole call, warm, --reps repetitions; the event pair includes the M device-to-host
reads of the norms and the host arithmetic between the launches, which is what a caller waits for.  The two kernels are
also timed on their own (device events around back-to-back launches).
Comparison: the host drop-in fedavg.RSCFed on CPU state_dicts at --threads threads (the reference's arithmetic; without the
device path it is the only route, after one device-to-host copy per client state, which is not counted here).
Bytes: the aggregation as the reference does it moves (M (2K + 1) + M + 1) states; the device path moves
M (K + K + 1) + (M + 1) states (state_dist reads K, fed_w reads K and writes 1), reported over a copy's measured rate.
Prints one JSON line.  usage: python tools/rscfed_time.py [--reps 20] [--host-reps 2] [--threads 16] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fedmlp_amd import fedavg, spec               # noqa: E402
from fedmlp_amd.engine import Engine              # noqa: E402

N_CLIENTS, K, M, C, HW = 8, 6, 10, 5, 64


def events_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_num_threads(a.threads)
    eng = Engine("Resnet18", C, HW, HW, 8)
    base, _ = spec.init_state("Resnet18", C, 1037)
    rs = np.random.RandomState(3)
    states, flats, cnts = [], [], []
    for _ in range(N_CLIENTS):
        flat = (base * (1.0 + 0.01 * rs.standard_normal(base.size))).astype(np.float32)
        cnt = rs.randint(30, 40, size=eng.ni).astype(np.int64)
        eng.set_state(flat, cnt)
        states.append(eng.state_tensor().clone())
        flats.append(flat)
        cnts.append(cnt)
    dict_len = [5000, 4999, 37, 5000, 1, 2500, 5000, 123]
    dma = [list(rs.choice(N_CLIENTS, K, replace=False)) for _ in range(M)]
    counters = np.stack(cnts)
    ns = states[0].numel()
    state_bytes = ns * 4

    full = events_ms(lambda: fedavg.rscfed_device(eng, states, counters, dma, dict_len), a.reps, 3)
    sel = [states[i] for i in dma[0]]
    out = torch.empty_like(states[0])
    dist = events_ms(lambda: eng.state_dist(sel), a.reps, 3)
    fold = events_ms(lambda: eng.fed_w(sel, [1.0] * K, out), a.reps, 3)
    big = torch.empty(64 * ns, device=eng.device)
    big2 = torch.empty_like(big)
    copy = events_ms(lambda: big2.copy_(big), 10, 3)
    copy_tbs = 2 * big.numel() * 4 / (np.median(copy) * 1e-3) / 1e12
    del big, big2

    sds = [spec.flat_to_state_dict("Resnet18", C, f, c) for f, c in zip(flats, cnts)]
    host = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        fedavg.RSCFed(dma, sds, K, dict_len, M)
        host.append((time.perf_counter() - t0) * 1e3)

    dev_states = M * (2 * K + 1) + (M + 1)
    ref_states = M * (2 * K + 1) + M + 1
    med = float(np.median(full))
    res = {
        "workload": f"RSCFed aggregation, ResNet-18, {N_CLIENTS} clients, K={K}, M={M}",
        "state_mb": state_bytes / 1e6,
        "device_ms_median": med, "device_ms_min": float(np.min(full)), "device_ms_max": float(np.max(full)), "reps": a.reps,
        "device_bytes_gb": dev_states * state_bytes / 1e9, "reference_bytes_gb": ref_states * state_bytes / 1e9,
        "device_tb_per_s": dev_states * state_bytes / (med * 1e-3) / 1e12,
        "copy_tb_per_s": copy_tbs, "fraction_of_copy": dev_states * state_bytes / (med * 1e-3) / 1e12 / copy_tbs,
        "state_dist_ms_median": float(np.median(dist)), "state_dist_tb_per_s": K * state_bytes / (np.median(dist) * 1e-3) / 1e12,
        "fed_w_ms_median": float(np.median(fold)), "fed_w_tb_per_s": (K + 1) * state_bytes / (np.median(fold) * 1e-3) / 1e12,
        "host_ms": host, "host_threads": a.threads, "host_over_device": float(np.min(host)) / med,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
