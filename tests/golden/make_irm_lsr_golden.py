#!/usr/bin/env python3
"""Known answers for the building blocks of the FedLSR / FedIRM heads, produced by THE REFERENCE'S OWN functions on the CPU:
LocalUpdate.js, anti_sigmoid, get_confuse_matrix, kd_loss, sigmoid_mse_loss, find_rows (utils/local_training.py:57-113,
1258-1269; none of them touches the GPU: the .cuda() calls are in the training loops) and utils/FedAvg.py's FedAvg_rela (:95-103).
Inputs: B = 6, C = 8 (the class count the reference hard-codes in get_confuse_matrix), float64 for the loss functions so that
tests/irm_lsr_ref.py is pinned to float64 rounding, float32 for FedAvg_rela (pinned bit for bit); three clients for
FedAvg_rela, class 7 annotated by client 1 alone.  The methods are called on an instance made without the constructor (they
use no instance state).  A package the reference imports and this machine lacks is replaced by an empty stand-in, as
make_golden.py does for seaborn / tensorboardX.
Writes tests/golden/irm_lsr_kat.npz.
usage: python tests/golden/make_irm_lsr_golden.py /path/to/reference"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
B, C = 6, 8
WEIGHT = [5000, 37, 1234]
CLASS_ACTIVE = [[0, 1, 2], [0, 2], [1, 2], [0], [2, 1], [0, 1], [2, 0], [1]]


class _Stub(types.ModuleType):
    """stands in for an absent package: any attribute is another stand-in, importable as a submodule"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        m = _Stub(self.__name__ + "." + name)
        sys.modules[m.__name__] = m
        setattr(self, name, m)
        return m

    def __call__(self, *a, **k):
        return self


def import_with_stubs(name):
    for _ in range(64):
        try:
            return importlib.import_module(name)
        except ModuleNotFoundError as ex:
            if not ex.name or ex.name.startswith("utils"):
                raise
            parts = ex.name.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), _Stub(".".join(parts[:i])))
    raise RuntimeError("too many missing packages")


def inputs():
    rs = np.random.RandomState(20211)
    z1 = rs.uniform(-4, 4, (B, C))
    z2 = z1 + rs.uniform(-1, 1, (B, C))
    y = (rs.rand(B, C) < 0.4).astype(np.float64)
    y[:, 3] = 0.0                                             # a class without positives: the + 1e-8 denominator
    conf = z1.copy()
    conf[[0, 2, 5]] = np.where(z1[[0, 2, 5]] >= 0, 1.0, -1.0) * rs.uniform(1.0, 5.0, (3, C))      # rows 0, 2, 5 pass find_rows
    mats = [1.0 / (1.0 + np.exp(-rs.standard_normal((C, C)))) for _ in range(3)]
    return z1, z2, y, conf, mats


def main():
    ref = sys.argv[1]
    sys.path.insert(0, ref)
    torch.set_num_threads(1)
    LT = import_with_stubs("utils.local_training")
    spec = importlib.util.spec_from_file_location("ref_fedavg", os.path.join(ref, "utils", "FedAvg.py"))
    FA = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(FA)
    lu = LT.LocalUpdate.__new__(LT.LocalUpdate)
    z1, z2, y, conf, mats = inputs()
    t = torch.from_numpy
    q1 = torch.clamp(torch.sigmoid(t(z1) * 3), min=1e-6, max=1.0)
    q2 = torch.clamp(torch.sigmoid(t(z2) * 3), min=1e-6, max=1.0)
    p = torch.sigmoid(t(z1)) * 0.3 + torch.sigmoid(t(z2)) * 0.7
    rows = lu.find_rows(torch.sigmoid(t(conf)), 0.7, 0.3)
    pseudo = torch.sigmoid(t(conf))[rows] > 0.5
    Q = lu.get_confuse_matrix(t(conf)[rows], pseudo)
    P32 = [t(m.astype(np.float32)) for m in mats]
    out = {
        "z1": z1, "z2": z2, "y": y, "conf": conf, "mats": np.stack(mats),
        "js": lu.js(q1, q2).numpy(),
        "anti_sigmoid": lu.anti_sigmoid(p).numpy(),
        "confuse_y": lu.get_confuse_matrix(t(z1), t(y)).numpy(),
        "find_rows": rows.numpy().astype(np.int64),
        "confuse_pseudo": Q.numpy(),
        "kd": lu.kd_loss(Q, t(mats[0])).numpy(),
        "mse": lu.sigmoid_mse_loss(t(z1), t(z2)).numpy(),
        "rela_weight": np.asarray(WEIGHT, np.int64),
        "rela_active": np.asarray([c + [-1] * (3 - len(c)) for c in CLASS_ACTIVE], np.int64),
        "rela": FA.FedAvg_rela(P32, WEIGHT, CLASS_ACTIVE).numpy(),
    }
    assert out["rela"].dtype == np.float32 and out["js"].dtype == np.float64
    path = os.path.join(HERE, "irm_lsr_kat.npz")
    np.savez(path, **out)
    print("wrote irm_lsr_kat.npz:", os.path.getsize(path), "bytes; find_rows =", out["find_rows"].tolist())


if __name__ == "__main__":
    main()
