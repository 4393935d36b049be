#!/usr/bin/env python3
"""Record tests/golden/rank_metrics.json: what scikit-learn and the reference's own metric functions give on the seeded
inputs of tests/eval_cases.py.

Runs only in the build container, like make_golden.py (the reference and scikit-learn do not exist on the GPU box), with
the same recipe: stub the absent modules, make `.cuda()` the identity.  Nothing of the reference's source travels: only
the numbers it produced.

Per case: sklearn's per-class average_precision_score and auc(roc_curve), the integer counts {tp, npos, npred, tn}, the
reference's Recall / BACC / Precision / F1Measure / Hamming_Loss over all classes and with classid = 0 and C - 1.  Every
column of these cases has both classes.  The degenerate group (no positives, no negatives, N = 1) records inputs only.
The `valloss` record is the reference's utils/valloss_cal.py on a linear stub net, with the torch seed it was drawn
under and the sample order its SubsetRandomSampler produced.

usage: python tests/golden/make_eval_golden.py
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

for name in ("seaborn", "tensorboardX"):
    sys.modules.setdefault(name, types.ModuleType(name))
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self

import sklearn                                                                    # noqa: E402
from sklearn.metrics import auc, average_precision_score, roc_curve              # noqa: E402
from utils.multilabel_metrixs import BACC, F1Measure, Hamming_Loss, Precision, Recall   # noqa: E402  (reference)
import utils.valloss_cal as VL                                                    # noqa: E402  (reference)

from tests import eval_cases as E                                                 # noqa: E402


def record_case(c):
    y, p = E.make_case(c["n"], c["C"], c["family"], c["prev"], c["seed"])
    pred = p > E.THRESHOLD
    C = c["C"]
    rec = dict(c)
    rec["sha"] = E.checksum(y, p)
    rec["AP"] = [float(average_precision_score(y[:, k], p[:, k])) for k in range(C)]
    rec["AUC"] = [float(auc(*roc_curve(y[:, k], p[:, k], pos_label=1)[:2])) for k in range(C)]
    rec["counts"] = E.counts_of(y, p).tolist()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # the classid branches divide 0 by 0 where nothing is predicted
        rec["all"] = {"BACC": float(BACC(y, pred)), "R": float(Recall(y, pred)), "F1": float(F1Measure(y, pred)),
                      "P": float(Precision(y, pred)), "hamming_loss": float(Hamming_Loss(y, pred))}
        rec["classid"] = {str(k): {"BACC": float(BACC(y, pred, k)), "R": float(Recall(y, pred, k)),
                                   "F1": float(F1Measure(y, pred, k)), "P": float(Precision(y, pred, k))}
                          for k in sorted({0, C - 1})}
    return rec


class _Stub(torch.nn.Module):
    def __init__(self, W):
        super().__init__()
        self.W = torch.from_numpy(W)

    def forward(self, x):
        return None, x @ self.W


class _DS(torch.utils.data.Dataset):
    def __init__(self, x, t):
        self.x, self.targets, self.seen = x, t, []

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        self.seen.append(int(i))
        return {"image": torch.from_numpy(self.x[i]), "target": torch.from_numpy(self.targets[i])}


def record_valloss():
    v = dict(E.VALLOSS)
    x, t, W = E.valloss_problem()
    ds = _DS(x, t)
    args = types.SimpleNamespace(batch_size=v["batch_size"], n_classes=v["C"], device="cpu")
    torch.manual_seed(v["torch_seed"])
    v["loss"] = float(VL.valloss(_Stub(W), ds, args))
    v["order"] = ds.seen               # the rows in the order the reference's sampler drew them
    return v


if __name__ == "__main__":
    out = {"sklearn": sklearn.__version__, "threshold": E.THRESHOLD,
           "cases": [record_case(c) for c in E.case_list()],
           "degenerate": [dict(d, sha=E.checksum(*E.make_degenerate(d["n"], d["family"], d["seed"])))
                          for d in E.degenerate_list()],
           "valloss": record_valloss()}
    path = os.path.join(HERE, "rank_metrics.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes,", len(out["cases"]), "cases")
