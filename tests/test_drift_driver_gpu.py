"""The driver's --prox_mu and --scaffold (fedmlp_amd/drift.py on the FedAVG row) end to end on one GPU, in-process like
tests/test_driver_gpu.py: two rounds of eight clients each, the final global model read from the checkpoint --save_every writes.
The driver seeds every generator from --seed, so two runs with the same flags give the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COMMON = ["--exp", "FedAVG", "--rounds_warmup", "2", "--n_local", "64", "--hw", "64", "--pretrained", "0", "--save_every", "2"]


def _run(argv, out_dir):
    from fedmlp_amd import driver
    os.makedirs(out_dir, exist_ok=True)
    old = sys.argv
    sys.argv = ["driver"] + COMMON + ["--save_dir", str(out_dir)] + argv
    try:
        log = driver.main()
    finally:
        sys.argv = old
    return log, torch.load(os.path.join(str(out_dir), "model_1.pth"), map_location="cpu")


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _run([], tmp_path_factory.mktemp("plain"))


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def _finite(sd):
    return all(bool(torch.isfinite(v).all()) for v in sd.values() if v.dtype == torch.float32)


def test_fedprox_run(plain, tmp_path):
    log, sd = _run(["--prox_mu", "0.01"], tmp_path)
    assert len(log) == 2 and all(np.isfinite(r["mean_loss"]) for r in log)
    assert all(r["prox_mu"] == 0.01 and "scaffold" not in r for r in log)
    assert _finite(sd) and not _same(sd, plain[1])


def test_scaffold_run(plain, tmp_path):
    log, sd = _run(["--scaffold", "1"], tmp_path)
    assert len(log) == 2 and all(np.isfinite(r["mean_loss"]) for r in log)
    assert all("prox_mu" not in r for r in log)
    norms = [r["scaffold"]["c_norm"] for r in log]
    assert all(np.isfinite(n) and n > 0 for n in norms), norms
    # round 0 runs under zero control variates (c = c_i = 0): its clients' models are the plain run's; round 1 is shifted
    assert _finite(sd) and not _same(sd, plain[1])


def test_flags_at_their_defaults_change_nothing(plain, tmp_path):
    log, sd = _run(["--prox_mu", "0", "--scaffold", "0"], tmp_path)
    assert all("prox_mu" not in r and "scaffold" not in r for r in log + plain[0])
    assert [r["mean_loss"] for r in log] == [r["mean_loss"] for r in plain[0]]
    assert _same(sd, plain[1])
