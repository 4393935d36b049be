"""The driver's RSCFed / FedNoRo / CBAFed rows (main.py:114-128, 140-166, 213-215, 269-316) end to end on one GPU, in-process like
tests/test_driver_gpu.py.  RSCFed's global model is also checked against fedavg.RSCFed on the clients' host state_dicts, to the
agreement of tests/test_rscfed_gpu.py (the device norms move the weights by less than an fp32 ulp: rtol 1e-6).  The multi-rank
gather of the client states needs more than one GPU and is not covered here."""
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMMON = ["--n_local", "32", "--hw", "32", "--batch_size", "16", "--pretrained", "0"]


def _run(argv):
    from fedmlp_amd import driver
    old = sys.argv
    sys.argv = ["driver"] + argv + COMMON
    try:
        return driver.main()
    finally:
        sys.argv = old


def test_driver_rscfed(monkeypatch):
    import random
    from fedmlp_amd import driver, fedavg, spec
    seen = []
    real = driver.rscfed_round

    def spy(eng, DMA, states, counters, n_all, rank, world, dist):
        rec = None
        if not seen:                                        # round 0: the clients as host state_dicts
            sds = []
            for c in range(len(n_all)):
                eng.state_tensor().copy_(states[c])
                flat, _ = eng.get_state()
                sds.append(spec.flat_to_state_dict(eng.model, eng.n_classes, flat, counters[c]))
            rec = {"DMA": [list(g) for g in DMA], "sds": sds, "n_all": list(n_all)}
        cnt = real(eng, DMA, states, counters, n_all, rank, world, dist)
        if rec is not None:
            rec["got"], rec["cnt"] = eng.get_state()[0], cnt
        seen.append(rec)
        return cnt
    monkeypatch.setattr(driver, "rscfed_round", spy)
    log = _run(["--exp", "RSCFed", "--n_clients", "6", "--rounds_warmup", "2", "--seed", "1037"])
    assert len(log) == 2 and all(np.isfinite(r["mean_loss"]) for r in log)
    assert len(seen) == 2
    r = seen[0]
    # every rank steps one random.Random(seed) alike: the DMA of round 0 is the first M draws of K from it
    rng = random.Random(1037)
    assert r["DMA"] == [rng.sample(range(6), driver.RSCFED_K) for _ in range(driver.RSCFED_M)]
    want = fedavg.RSCFed(r["DMA"], r["sds"], driver.RSCFED_K, r["n_all"], driver.RSCFED_M)
    names = [k for k, _, dt in spec.entries("Resnet18", 8) if dt == "f32"]
    want_flat = np.concatenate([want[k].numpy().reshape(-1) for k in names])
    want_cnt = np.array([float(v) for k, v in want.items() if k.endswith("num_batches_tracked")])
    np.testing.assert_allclose(r["got"], want_flat, rtol=1e-6, atol=0)
    np.testing.assert_array_equal(r["cnt"], np.trunc(want_cnt + 1e-9).astype(np.int64))      # float counters, truncated on load
    assert (r["cnt"] == 2).all()                            # 32 samples at batch size 16: two train-mode forwards per client


def test_driver_fednoro():
    log = _run(["--exp", "FedNoRo", "--rounds_warmup", "2"])
    assert len(log) == 2 and all(np.isfinite(r["mean_loss"]) for r in log)


def test_driver_cbafed(monkeypatch):
    """warm-up 2, 7 rounds: tao from round 1 on, stage 2 (and the reset of res) from round 2.  Stage 2's first 0.5 / 0.5 blend
    would be round 2 + 5 = 7, one past this run, so the blends themselves are run by test_driver_cbafed_blend_round"""
    from fedmlp_amd import fedavg
    asked = []
    real = fedavg.cbafed_blend
    taos = []
    real_tao = fedavg.cbafed_tao

    def spy(rnd, warmup):
        out = real(rnd, warmup)
        asked.append((rnd, warmup) + out)
        return out

    def spy_tao(class_num_lists, data_nums):
        out = real_tao(class_num_lists, data_nums)
        taos.append((len(class_num_lists), list(data_nums), out[1]))
        return out
    monkeypatch.setattr(fedavg, "cbafed_blend", spy)
    monkeypatch.setattr(fedavg, "cbafed_tao", spy_tao)
    log = _run(["--exp", "CBAFed", "--rounds_CBAFed_warmup", "2", "--rounds_warmup", "7"])
    assert len(log) == 7 and all(np.isfinite(r["mean_loss"]) for r in log)
    assert [a[0] for a in asked] == list(range(7)) and all(a[1] == 2 for a in asked)
    assert [a[4] for a in asked] == [True, False, True, False, False, False, False]          # res set at 0, reset at 2
    assert len(taos) == 6                                    # from round warmup - 1 on
    assert all(n == 8 for n, _, _ in taos)                   # every client's counts reach the aggregation
    assert taos[0][1] == [32] * 8                            # the warm-up's data_num: the local set
    assert all(all(d >= 32 for d in dn) for _, dn, _ in taos[1:])     # stage 2: B annotation_num per step, plus the pseudo rows
    assert all(bool(((t >= 0.55) & (t <= 0.95)).all()) for _, _, t in taos)


@pytest.mark.parametrize("warmup,rounds", [("6", "7"), ("2", "8")], ids=["warmup_blend", "stage2_blend"])
def test_driver_cbafed_blend_round(warmup, rounds):
    """warm-up 6 of 7 rounds: round 5 is the warm-up's 0.2 / 0.8 blend with the model stored at round 0; warm-up 2 of 8 rounds:
    round 7 is stage 2's 0.5 / 0.5 blend with the model stored at round 2, on the data_num-weighted FedAvg"""
    log = _run(["--exp", "CBAFed", "--rounds_CBAFed_warmup", warmup, "--rounds_warmup", rounds, "--n_clients", "2"])
    assert len(log) == int(rounds) and all(np.isfinite(r["mean_loss"]) for r in log)
