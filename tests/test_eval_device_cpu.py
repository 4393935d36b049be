"""The host half of the on-device evaluation: the factored count helper and class_metrics against the reference's
multilabel_metrixs, the pure valloss arithmetic against the reference's valloss_cal, the host AP / ROC-AUC against
scikit-learn (tests/golden/rank_metrics.json, recorded by tests/golden/make_eval_golden.py), the rank-sharded
probabilities on gloo, and the driver's defaults."""
import datetime
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import eval_cases as E
from tests.helpers import load_golden


@pytest.fixture(scope="module")
def golden():
    return load_golden("rank_metrics.json")


def _case(c):
    y, p = E.make_case(c["n"], c["C"], c["family"], c["prev"], c["seed"])
    assert E.checksum(y, p) == c["sha"], f"{c['name']}: the generator no longer makes the arrays the fixture was recorded on"
    return y, p


def _same(got, want, tol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    assert np.array_equal(np.isinf(got), np.isinf(want)), (what, got, want)
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= tol), (what, got, want)


def test_fixture_covers_the_cases(golden):
    assert [c["name"] for c in golden["cases"]] == [c["name"] for c in E.case_list()]
    assert [d["name"] for d in golden["degenerate"]] == [d["name"] for d in E.degenerate_list()]
    for c in golden["cases"]:                       # every column is two-class: no test leaves a column out
        cnt = np.array(c["counts"])
        assert np.all(cnt[:, 1] > 0) and np.all(cnt[:, 1] < c["n"])


def test_count_helper_and_class_metrics_equal_the_reference(golden):
    from fedmlp_amd.evaluations import class_count_metrics, class_metrics, count_metrics, multilabel_metrics
    for c in golden["cases"]:
        y, p = _case(c)
        cnt = E.counts_of(y, p)
        assert np.array_equal(cnt, np.array(c["counts"], np.int64)), c["name"]
        m = count_metrics(cnt[:, 0], cnt[:, 1], cnt[:, 2], cnt[:, 3], c["n"])
        full = multilabel_metrics(y, p)
        for k, want in c["all"].items():
            _same(m[k], want, 1e-12, (c["name"], k))
            assert full[k] == m[k], (c["name"], k)          # multilabel_metrics evaluates the helper's expression
        for cid, want in c["classid"].items():
            got = class_metrics(y, p > E.THRESHOLD, int(cid))
            got2 = class_count_metrics(*cnt[int(cid)], c["n"])
            for k in ("BACC", "R", "F1", "P"):
                _same(got[k], want[k], 1e-12, (c["name"], cid, k))
                _same(got2[k], want[k], 1e-12, (c["name"], cid, k, "counts"))


def test_host_ap_auc_equal_sklearn(golden):
    from fedmlp_amd.evaluations import average_precision, roc_auc
    for c in golden["cases"]:
        y, p = _case(c)
        tol = c["n"] * 2.0 ** -51
        for k in range(c["C"]):
            assert abs(average_precision(y[:, k], p[:, k]) - c["AP"][k]) <= tol, (c["name"], k)
            assert abs(roc_auc(y[:, k], p[:, k]) - c["AUC"][k]) <= tol, (c["name"], k)


def test_valloss_arithmetic_equals_the_reference(golden):
    from fedmlp_amd.evaluations import valloss_from_logits
    v = golden["valloss"]
    assert {k: v[k] for k in E.VALLOSS} == E.VALLOSS
    x, t, W = E.valloss_problem()
    n = int(v["N"] * 0.1)
    assert sorted(v["order"]) == list(range(n))
    logits = torch.from_numpy(x[:n]) @ torch.from_numpy(W)
    got = valloss_from_logits(logits, t, v["order"], 4 * v["batch_size"])
    assert abs(got - v["loss"]) <= 1e-6 * abs(v["loss"]), (got, v["loss"])


def test_valloss_draws_one_randperm_of_the_split():
    """valloss(net, ds, args): the first int(0.1 N) samples in the order of one torch.randperm from the global generator"""
    from fedmlp_amd import evaluations as EV
    x, t, W = E.valloss_problem()

    class Net:
        default_max_images = 8

        def eval(self):
            return self

        def __call__(self, xb):
            return None, xb.reshape(xb.shape[0], -1) @ torch.from_numpy(W)

    class DS:
        targets = t

        def __len__(self):
            return len(t)

        def __getitem__(self, i):
            return {"image": torch.from_numpy(x[i])}

    args = type("A", (), {"batch_size": 2, "n_classes": 3})()
    torch.manual_seed(77)
    got = EV.valloss(Net(), DS(), args)
    torch.manual_seed(77)
    order = torch.randperm(23).tolist()
    want = EV.valloss_from_logits(torch.from_numpy(x[:23]) @ torch.from_numpy(W), t, order, 8)
    assert got == want


# ---- sharded_probs: world 2 on gloo is bit-identical to world 1 ----------------------------------------------------
N_ROWS, BS, NC = 1000, 128, 5          # 8 blocks, the last of 104 rows; ranks 0 / 1 get 4 blocks each, 512 and 488 rows


def _fake_forward(rows):
    r = torch.tensor(rows, dtype=torch.float32)[:, None]
    return torch.sin(r * 0.37 + torch.arange(NC, dtype=torch.float32)[None, :]) * 9.0


def _worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2, timeout=datetime.timedelta(seconds=180))
    from fedmlp_amd.evaluations import sharded_probs
    seen = []

    def fwd(rows):
        seen.append((rows[0], len(rows)))
        return _fake_forward(rows)

    probs = sharded_probs(fwd, N_ROWS, NC, rank, 2, BS, "cpu")
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), probs=probs.numpy(), seen=np.array(seen))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_probs_world2_is_bit_identical_to_world1(tmp_path):
    from fedmlp_amd.evaluations import sharded_probs
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(port, str(tmp_path)), nprocs=2, join=True)
    one = sharded_probs(_fake_forward, N_ROWS, NC, 0, 1, BS, "cpu").numpy()
    assert np.array_equal(one, torch.sigmoid(_fake_forward(list(range(N_ROWS)))).numpy())
    rows = 0
    for r in range(2):
        got = np.load(os.path.join(str(tmp_path), f"r{r}.npz"))
        assert got["probs"].tobytes() == one.tobytes(), r
        assert [int(a) // BS % 2 for a, _ in got["seen"]] == [r] * 4      # its own blocks only
        rows += int(got["seen"][:, 1].sum())
    assert rows == N_ROWS


def test_driver_defaults_leave_evaluation_off(monkeypatch):
    from fedmlp_amd import driver
    monkeypatch.setattr(sys, "argv", ["driver"])
    a = driver.args_parser()
    assert a.eval_every == 0 and a.n_test == 1024
    monkeypatch.setattr(sys, "argv", ["driver", "--eval_every", "10", "--n_test", "96"])
    a = driver.args_parser()
    assert (a.eval_every, a.n_test) == (10, 96)
