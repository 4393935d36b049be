#!/usr/bin/env python3
"""Known answers for the RSCFed aggregation, produced by THE REFERENCE'S OWN utils/FedAvg.py (Fed_w, model_dist, RSCFed:
utils/FedAvg.py:16-49) on small CPU state_dicts in the build container.

Eight clients with four entries each (a 4-d weight, an odd-length vector, an int64 num_batches_tracked, a 5-element bias)
drawn from numpy RandomState seeds -- tests/test_rscfed_cpu.py regenerates them with client_state() below, so the fixture
holds the seeds, not the values -- uneven sample counts including 1, and M = 4 groups of K = 3 client ids.  Recorded: per
group the reference's model_dist of every member to the group mean and the weights a*b it derives, the first group's
Fed_w result under those (non-integer) weights, and the full RSCFed output.  fp32 values are written as the doubles they
equal, so json round-trips them exactly.
Writes tests/golden/rscfed_kat.json.
usage: python tests/golden/make_rscfed_golden.py /path/to/reference"""
import importlib.util
import json
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

SHAPES = OrderedDict([("conv.weight", (4, 3, 3, 3)), ("bn.running_mean", (1001,)), ("bn.num_batches_tracked", ()),
                      ("fc.bias", (5,))])
SEEDS = [11, 12, 13, 14, 15, 16, 17, 18]
DICT_LEN = [5000, 4999, 37, 5000, 1, 2500, 5000, 123]
DMA = [[0, 1, 2], [3, 4, 5], [6, 7, 0], [2, 4, 7]]
K, M = 3, 4


def client_state(seed):
    """OrderedDict[str, np.ndarray]: fp32 standard normals per entry in SHAPES order, the counter an int64 below 50."""
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    for key, shape in SHAPES.items():
        if key.endswith("num_batches_tracked"):
            sd[key] = np.array(rs.randint(0, 50), dtype=np.int64)
        else:
            sd[key] = rs.standard_normal(shape).astype(np.float32)
    return sd


def main():
    ref = sys.argv[1]
    spec = importlib.util.spec_from_file_location("ref_fedavg", os.path.join(ref, "utils", "FedAvg.py"))
    F = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(F)
    torch.set_num_threads(1)
    w_locals = [OrderedDict((k, torch.from_numpy(np.asarray(v))) for k, v in client_state(s).items()) for s in SEEDS]

    def dump(sd):
        return {k: np.asarray(v.numpy(), dtype=np.float64).reshape(-1).tolist() for k, v in sd.items()}

    groups = []
    for group in DMA:
        sel = [w_locals[i] for i in group]
        n_total = sum(DICT_LEN[i] for i in group)
        w_avg = F.Fed_w(sel, [1] * K)
        dists = [F.model_dist(w_locals[i], w_avg) for i in group]
        wts = [DICT_LEN[i] / n_total * math.exp((-0.01) * (d / DICT_LEN[i])) for i, d in zip(group, dists)]
        groups.append({"ids": group, "dist": dists, "weight": wts})
    sub0 = F.Fed_w([w_locals[i] for i in DMA[0]], groups[0]["weight"])
    out = F.RSCFed(DMA, w_locals, K, DICT_LEN, M)
    kat = {"shapes": {k: list(v) for k, v in SHAPES.items()}, "seeds": SEEDS, "dict_len": DICT_LEN, "DMA": DMA, "K": K, "M": M,
           "groups": groups, "fed_w_group0": dump(sub0), "out": dump(out),
           "out_dtype": {k: str(v.dtype) for k, v in out.items()}}
    with open(os.path.join(HERE, "rscfed_kat.json"), "w") as f:
        json.dump(kat, f)
    print("wrote rscfed_kat.json:", os.path.getsize(os.path.join(HERE, "rscfed_kat.json")), "bytes")


if __name__ == "__main__":
    main()
