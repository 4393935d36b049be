"""The driver's --server_opt end to end on one GPU, in-process like tests/test_drift_driver_gpu.py: two rounds of two clients on the
smallest engine (32 x 32 input, batch 4, 5 classes).  The driver seeds every generator from --seed, so two runs with the same flags
give the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import server_opt_ref as R

pytestmark = pytest.mark.gpu

COMMON = ["--exp", "FedAVG", "--n_clients", "2", "--n_local", "8", "--batch_size", "4", "--hw", "32", "--n_classes", "5",
          "--pretrained", "0"]
F = np.float32


_SEED = []


def _seed():
    """Eight samples per client at the driver's 15 % label rate: the first --seed under which both clients' synthetic labels
    (driver.DeviceDataset draws them first, from the seed + 1000 c) hold a positive of every class, which LocalUpdate's class
    weights n / count need"""
    if not _SEED:
        for seed in range(1, 2000):
            ok = True
            for c in range(2):
                g = torch.Generator(device="cuda").manual_seed(seed + 1000 * c)
                ok = ok and bool((torch.rand((8, 5), device="cuda", generator=g) < 0.15).any(0).all())
            if ok:
                _SEED.append(seed)
                break
    return _SEED[0]


def _run(argv, out_dir, rounds=2):
    from fedmlp_amd import driver
    os.makedirs(out_dir, exist_ok=True)
    old = sys.argv
    sys.argv = (["driver"] + COMMON + ["--seed", str(_seed()), "--rounds_warmup", str(rounds), "--save_every", str(rounds),
                                       "--save_dir", str(out_dir)] + argv)
    try:
        log = driver.main()
    finally:
        sys.argv = old
    return log, torch.load(os.path.join(str(out_dir), f"model_{rounds - 1}.pth"), map_location="cpu")


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def _records(log):
    return [{k: v for k, v in r.items() if k not in ("sec", "samples_per_sec_per_gpu")} for r in log]


def test_the_flag_at_none_changes_nothing(tmp_path):
    log0, sd0 = _run([], tmp_path / "plain")
    log1, sd1 = _run(["--server_opt", "none"], tmp_path / "none")
    assert _records(log0) == _records(log1) and all("server_opt" not in r for r in log0 + log1)
    assert _same(sd0, sd1)
    assert not os.path.exists(os.path.join(str(tmp_path / "none"), "server_opt_1.pth"))


def test_yogi_run_is_the_reference_rule(tmp_path, monkeypatch):
    from fedmlp_amd import server_opt
    seen = []
    real = server_opt.ServerOptimizer.step

    def step(self, eng, old_global):
        rec = {"old": old_global.clone(), "avg": eng.state_tensor().clone(), "spans": eng.debug_entry_spans()}
        out = real(self, eng, old_global)
        rec["new"] = eng.state_tensor().clone()
        seen.append(rec)
        return out
    monkeypatch.setattr(server_opt.ServerOptimizer, "step", step)
    log, sd = _run(["--server_opt", "yogi"], tmp_path / "yogi")
    assert len(seen) == 2
    hp = dict(lr=1e-2, beta1=0.9, beta2=0.99, tau=1e-3)
    # the rule is elementwise, so it is applied in the engine's own layout: over the parameter entries' slots [0, end) -- padding
    # and gaps in between hold zeros in both models and stay zeros under the rule -- while everything behind is the aggregate's
    spans = seen[0]["spans"]
    spans = spans[spans[:, 0] >= 0]
    end = int((spans[:, 0] + spans[:, 1]).max())
    m, v = R.init("yogi", end, hp["tau"])
    for rnd, rec in enumerate(seen):
        old, avg, new = (rec[k].cpu().numpy() for k in ("old", "avg", "new"))
        want, m, v = R.step("yogi", old[:end], avg[:end], m, v, **hp)
        assert np.array_equal(new[:end].view(np.uint32), want.view(np.uint32)), f"round {rnd}: the new global model"
        assert np.array_equal(new[end:].view(np.uint32), avg[end:].view(np.uint32)), f"round {rnd}: the running statistics"
        assert int((new[:end] != avg[:end]).sum()) > 0
        r = log[rnd]["server_opt"]
        d = (avg[:end] - old[:end]).astype(np.float64)
        assert r["rule"] == "yogi" and r["step"] == rnd + 1
        assert abs(r["delta_norm"] - float(np.sqrt((d * d).sum()))) <= 1e-9 * r["delta_norm"] and r["delta_norm"] > 0
    monkeypatch.undo()
    # the saved optimizer resumes through --init_server_opt: its step count goes on from 2
    path = os.path.join(str(tmp_path / "yogi"), "server_opt_1.pth")
    saved = torch.load(path, map_location="cpu")
    assert saved["step"] == 2 and saved["hyper"]["rule"] == "yogi" and bool(saved["m"].any()) and bool((saved["v"] > 0).any())
    seen.clear()
    monkeypatch.setattr(server_opt.ServerOptimizer, "step", step)
    log2, _ = _run(["--server_opt", "yogi", "--init_server_opt", path], tmp_path / "resume", rounds=1)
    monkeypatch.undo()
    assert log2[0]["server_opt"]["step"] == 3 and np.isfinite(log2[0]["mean_loss"]) and len(seen) == 1
    # ... with its moments: the resumed round is the reference stepped from the saved m and v.  They are in state_dict order, so
    # the captured engine-layout operands go through an engine of the driver's shape to be read in that order too
    from fedmlp_amd import spec
    from fedmlp_amd.engine import Engine
    tr = np.concatenate([np.full(int(np.prod(shape)), spec.is_trainable(k)) for k, shape, dt in spec.entries("Resnet18", 5)
                         if dt == "f32"])
    conv = Engine("Resnet18", 5, 32, 32, 16)
    try:
        flat = {}
        for k in ("old", "avg", "new"):
            conv.state_tensor().copy_(seen[0][k])
            flat[k] = conv.get_state()[0]
    finally:
        conv.close()
    sm, sv = saved["m"].numpy(), saved["v"].numpy()
    want, _, _ = R.step("yogi", flat["old"][tr], flat["avg"][tr], sm[tr], sv[tr], **hp)
    assert np.array_equal(flat["new"][tr].view(np.uint32), want.view(np.uint32)), "the resumed step did not start from the saved moments"
    fresh, _, _ = R.step("yogi", flat["old"][tr], flat["avg"][tr], *R.init("yogi", int(tr.sum()), hp["tau"]), **hp)
    assert int((fresh != want).sum()) > 0.3 * want.size, "the saved moments make no difference: the check above shows nothing"
    assert np.array_equal(flat["new"][~tr].view(np.uint32), flat["avg"][~tr].view(np.uint32))
    # a flag that contradicts the file is refused; one that repeats it is not
    with pytest.raises(SystemExit, match="contradicts"):
        _run(["--server_opt", "yogi", "--init_server_opt", path, "--server_lr", "0.5"], tmp_path / "clash", rounds=1)
    _run(["--server_opt", "yogi", "--init_server_opt", path, "--server_lr", "0.01"], tmp_path / "same", rounds=1)
