"""fm_eval_metrics (csrc/metrics.hip) and the device paths of globaltest / classtest / the driver's --eval_every on the GPU,
against scikit-learn and the reference's metric functions (tests/golden/rank_metrics.json), the host functions and the
reference's globaltest (tests/golden/eval_metrics.json).

Bound on AP / AUC: N 2^-51 absolute.  The counts are exact integers and each ratio is one correctly rounded fp64 division;
a sum of P <= N terms of at most 1, in any order, is off by less than N 2^-53 P before the division by P; both sides carry
that error, so doubling gives the bound."""
import argparse
import json
import sys

import numpy as np
import pytest
import torch

from tests import eval_cases as E
from tests.helpers import load_golden, make_args

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from fedmlp_amd.engine import Engine
    e = Engine("Resnet18", 4, 32, 32, 8)
    yield e
    e.close()


def _run(eng, y, p, **kw):
    dev = eng.device
    ap, auc, cnt = eng.eval_metrics(torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev), E.THRESHOLD, **kw)
    return tuple(None if t is None else t.cpu().numpy() for t in (ap, auc, cnt))


def test_every_fixture_case(eng):
    g = load_golden("rank_metrics.json")
    assert [c["name"] for c in g["cases"]] == [c["name"] for c in E.case_list()]
    bad, worst = [], 0.0
    for c in g["cases"]:
        y, p = E.make_case(c["n"], c["C"], c["family"], c["prev"], c["seed"])
        assert E.checksum(y, p) == c["sha"], c["name"]
        ap, auc, cnt = _run(eng, y, p)
        tol = c["n"] * 2.0 ** -51
        d_ap, d_auc = np.abs(ap - np.array(c["AP"])), np.abs(auc - np.array(c["AUC"]))
        worst = max(worst, float(np.nanmax(d_ap / tol)), float(np.nanmax(d_auc / tol)))
        if not (np.array_equal(cnt, np.array(c["counts"], np.int64)) and np.all(d_ap <= tol) and np.all(d_auc <= tol)):
            bad.append((c["name"], float(d_ap.max()), float(d_auc.max()), tol))
    print(f"fm_eval_metrics: {len(g['cases'])} cases, worst |difference| / (N 2^-51) = {worst:.3f}")
    assert not bad, bad[:10]


def test_degenerate_columns_follow_the_host_functions(eng):
    from fedmlp_amd.evaluations import average_precision, roc_auc
    g = load_golden("rank_metrics.json")
    for d in g["degenerate"]:
        y, p = E.make_degenerate(d["n"], d["family"], d["seed"])
        assert E.checksum(y, p) == d["sha"], d["name"]
        ap, auc, cnt = _run(eng, y, p)
        assert np.array_equal(cnt, E.counts_of(y, p)), d["name"]
        with np.errstate(invalid="ignore", divide="ignore"):
            w_ap = np.array([average_precision(y[:, k], p[:, k]) for k in range(4)])
            w_auc = np.array([roc_auc(y[:, k], p[:, k]) for k in range(4)])
        assert np.isnan(w_ap[0]) and np.isnan(w_auc[0]) and np.isnan(w_auc[1]) and w_ap[1] == 1.0
        for got, want in ((ap, w_ap), (auc, w_auc)):
            assert np.array_equal(np.isnan(got), np.isnan(want)), (d["name"], got, want)
            fin = np.isfinite(want)
            assert np.all(np.abs(got[fin] - want[fin]) <= d["n"] * 2.0 ** -51), (d["name"], got, want)


def test_null_outputs_and_repeatability(eng):
    y, p = E.make_case(5000, 5, "five_level", 0.3, 42)
    full = _run(eng, y, p)
    again = _run(eng, y, p)
    for a, b in zip(full, again):
        assert a.tobytes() == b.tobytes()                   # NaN-proof bit comparison
    only_ap = _run(eng, y, p, auc=False, counts=False)
    only_auc = _run(eng, y, p, ap=False, counts=False)
    only_cnt = _run(eng, y, p, ap=False, auc=False)
    assert only_ap[1] is None and only_ap[2] is None and only_ap[0].tobytes() == full[0].tobytes()
    assert only_auc[0] is None and only_auc[2] is None and only_auc[1].tobytes() == full[1].tobytes()
    assert only_cnt[0] is None and only_cnt[1] is None and only_cnt[2].tobytes() == full[2].tobytes()


def test_argument_checks(eng):
    dev = eng.device
    s = torch.zeros((8, 3), device=dev)
    with pytest.raises(ValueError):
        eng.eval_metrics(s, torch.zeros((8, 4), device=dev))
    with pytest.raises(ValueError):
        eng.eval_metrics(s.double(), s.double())
    with pytest.raises(ValueError):
        eng.eval_metrics(torch.zeros((8, 6), device=dev)[:, ::2], s)
    with pytest.raises(ValueError):
        eng.eval_metrics(s.cpu(), s.cpu())
    with pytest.raises(ValueError):
        eng.eval_metrics(torch.zeros((8, 33), device=dev), torch.zeros((8, 33), device=dev))


def test_large_tie_groups_match_the_host_metrics(eng):
    """N = 20000, C = 8, prevalence 0.1, five-level scores: tie groups of thousands across every tile boundary"""
    from fedmlp_amd.evaluations import multilabel_metrics, multilabel_metrics_device
    N = 20000
    y, p = E.make_case(N, 8, "five_level", 0.1, 4321)
    want = multilabel_metrics(y, p)
    dev = eng.device
    got = multilabel_metrics_device(eng, torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev))
    assert set(got) == set(want)
    for k in ("BACC", "R", "F1", "P", "hamming_loss"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert abs(float(got["mAP"]) - float(want["mAP"])) <= N * 2.0 ** -51
    assert abs(got["auc"] - want["auc"]) <= N * 2.0 ** -51
    ap, auc, _ = _run(eng, y, p)
    from fedmlp_amd.evaluations import average_precision, roc_auc
    for k in range(8):
        assert abs(ap[k] - average_precision(y[:, k], p[:, k])) <= N * 2.0 ** -51
        assert abs(auc[k] - roc_auc(y[:, k], p[:, k])) <= N * 2.0 ** -51


def _eval_problem():
    from fedmlp_amd.model import build_model
    from tests.test_local_training_gpu import SynthDataset
    g = load_golden("eval_metrics.json")
    args = make_args(n_classes=g["C"], batch_size=g["bs"], seed=g["init_seed"])
    return g, args, build_model(args), SynthDataset(g["N"], g["C"], g["hw"], g["data_seed"], False)


def test_globaltest_device_metrics_match_the_reference_and_the_host_path():
    from fedmlp_amd.evaluations import globaltest
    g, args, net, ds = _eval_problem()
    dev = globaltest(net, ds, args, device_metrics=True)
    host = globaltest(net, ds, args)
    assert set(dev) == set(host) == set(g["metrics"])
    for k, want in g["metrics"].items():
        assert abs(float(dev[k]) - want) <= 1e-4 * abs(want) + 1e-6, (k, float(dev[k]), want)
        assert abs(float(dev[k]) - float(host[k])) <= 1e-4 * abs(float(host[k])) + 1e-6, (k, float(dev[k]), float(host[k]))


def test_classtest_device_metrics_equal_the_host_path():
    from fedmlp_amd.evaluations import classtest
    g, args, net, ds = _eval_problem()
    for classid in (1, 4):
        host = classtest(net, ds, args, classid)
        dev = classtest(net, ds, args, classid, device_metrics=True)
        assert set(host) == set(dev) == {"BACC", "R", "F1", "P"}
        assert np.array([host[k] for k in sorted(host)]).tobytes() == np.array([dev[k] for k in sorted(host)]).tobytes(), \
            (classid, host, dev)


def _driver(argv):
    from fedmlp_amd import driver
    old = sys.argv
    sys.argv = ["driver"] + argv
    try:
        return driver.main()
    finally:
        sys.argv = old


def test_driver_eval_every(tmp_path, capsys):
    """FedAVG, 2 rounds, --eval_every 1 on 96 test rows: two blocks of 4 * 16, the second one short"""
    from fedmlp_amd import driver
    from fedmlp_amd.engine import Engine
    from fedmlp_amd.evaluations import globaltest
    from fedmlp_amd.model import ResidentNet, build_model
    base = ["--exp", "FedAVG", "--n_clients", "2", "--n_classes", "4", "--rounds_warmup", "2", "--batch_size", "16",
            "--n_local", "96", "--hw", "64", "--pretrained", "0"]
    log = _driver(base + ["--eval_every", "1", "--n_test", "96", "--save_every", "2", "--save_dir", str(tmp_path)])
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(log) == 2 and printed == log
    keys = {"mAP", "BACC", "R", "F1", "auc", "P", "hamming_loss"}
    for rec in log:
        assert set(rec["test"]) == keys and all(np.isfinite(v) for v in rec["test"].values()), rec
        assert 0 < rec["eval_sec"] <= rec["sec"]
    # round 2's numbers are globaltest(device_metrics=True) of the model it saved, on the same test set
    args = argparse.Namespace(model="Resnet18", n_classes=4, batch_size=16, seed=1037, pretrained=0, pretrained_path=None)
    host = build_model(args)
    host.load_state_dict(torch.load(str(tmp_path / "model_1.pth"), map_location="cpu"))
    host._pull()
    e = Engine("Resnet18", 4, 64, 64, 64)
    try:
        e.set_state(host.flat, host.counters)
        ds = driver.ShardedTestSet(96, 4, 64, 1037 + 500, 64, 0, 1, e.device)
        assert sorted(ds.blocks) == [0, 1] and ds.blocks[1].shape[0] == 32
        want = globaltest(ResidentNet(e), ds, args, device_metrics=True)
    finally:
        e.close()
    for k in keys:
        assert log[1]["test"][k] == float(want[k]), (k, log[1]["test"][k], float(want[k]))
    # without --eval_every the records are today's
    log0 = _driver(base)
    assert all(set(r) == {"round", "sec", "mean_loss", "samples_per_sec_per_gpu"} for r in log0) and len(log0) == 2
