"""driver.run_rounds and the rows of fedmlp_amd/rows.py without a GPU: a CPU stand-in for the engine (tests/test_fedavg_gloo's
FakeEngine), stand-in clients whose train_* note their arguments, move the engine's state like a training would and return
canned tuples of the trainers' lengths; world size 1, dist = None.

What is asserted is what the reference's main.py (:106-319) and the driver before the rows were objects do, written out here by
hand: which trainer a row calls with what in which round, what a row carries from one round to the next, the weights and the
scale of its FedAvg, CBAFed's blend in exact fp32 arithmetic, and that every client starts from the global model.  (FedIRM with
rounds_FedIRM_sup = 2: main.py:170 hands the class lists over from round SI - 1 = 1 on; the matrix first reaches a client in
round 2.)  fedavg.gather_dicts runs under gloo at world size 2."""
import datetime
import json
import os
import random
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedmlp_amd import driver, driver_rofl, fedavg, rows
from tests.test_fedavg_gloo import FakeEngine

C, D, NSTATE = 4, 8, 64
RESULT = 6                       # LocalUpdate._result: (state_dict, mean loss, None, None, negative list, active list)


class Engine(FakeEngine):
    device, nf = "cpu", NSTATE

    def __init__(self):
        g = torch.Generator().manual_seed(7)
        super().__init__(torch.randn(NSTATE, generator=g), np.array([3, 5], np.int64))


class Net:
    def __init__(self, eng):
        self.eng = eng

    def state_dict(self):
        return {"w": self.eng.state.clone()}


class Client:
    """every train_* of LocalUpdate: notes (name, round, client, args, kwargs), what the engine held when it was called and
    what it held afterwards; the canned return depends on the client and the round only"""

    def __init__(self, c, eng, calls):
        self.c, self.eng, self.calls = c, eng, calls
        self.active_class_list = [c % C]
        self.negative_class_list = [k for k in range(C) if k != c % C]
        self.n_calls = 0

    def _trained(self, name, a, k):
        rnd = self.n_calls
        self.n_calls += 1
        g = torch.Generator().manual_seed(1000 * rnd + self.c)
        call = {"name": name, "rnd": rnd, "c": self.c, "a": a, "k": k,
                "seen": (self.eng.state.clone(), self.eng.cnt.copy()), "gen": g}
        self.eng.state.add_(torch.randn(NSTATE, generator=g))
        self.eng.cnt = self.eng.cnt + np.array([self.c + 1 + rnd, 2], np.int64)
        call["after"] = (self.eng.state.clone(), self.eng.cnt.copy())
        call["ret"] = (None, 1.0 + self.c + 10 * rnd, None, None, self.negative_class_list, self.active_class_list)
        self.calls.append(call)
        return call

    def _plain(name):
        def train(self, *a, **k):
            return self._trained(name, a, k)["ret"]
        return train
    train = _plain("train")
    train_FixMatch = _plain("train_FixMatch")
    train_FedLSR = _plain("train_FedLSR")
    train_RSCFed = _plain("train_RSCFed")
    train_FedNoRo = _plain("train_FedNoRo")

    def train_FedMLP(self, rnd, tao, Prototype, writer1, neg, act, net):
        call = self._trained("train_FedMLP", (rnd, tao, Prototype, writer1, neg, act), {"net": net})
        if neg is not None:                                  # a prototype pass: (..., t, proto)
            g = call["gen"]
            call["ret"] += (torch.rand(C, generator=g).double().numpy(), torch.randn((2 * C, D), generator=g))
        return call["ret"]

    def train_FedIRM(self, rnd, target_matrix, writer1, neg, act, net):
        call = self._trained("train_FedIRM", (rnd, target_matrix, writer1, neg, act), {"net": net})
        if neg is not None:
            call["ret"] += (torch.rand((C, C), generator=call["gen"]),)
        return call["ret"]

    def train_CBAFed(self, rnd, net, **k):
        call = self._trained("train_CBAFed", (rnd, net), k)
        call["ret"] += (torch.rand(C, generator=call["gen"]) * 10, 20 + 3 * self.c + rnd)      # class_num_list, data_num
        return call["ret"]

    def train_RoFL(self, net, f_G, epoch):
        call = self._trained("train_RoFL", (net, f_G, epoch), {})
        call["ret"] = (None, call["ret"][1], torch.randn((2 * C, D), generator=call["gen"]))
        return call["ret"]


class Run:
    """one run_rounds of `argv` on stand-ins; notes every RoundAccumulator.add / reduce and the engine after every aggregation"""

    def __init__(self, monkeypatch, argv, n_clients, scaffold=None):
        parse = driver_rofl.args_parser if "--exp" not in argv else driver.args_parser
        args = parse(argv + ["--n_clients", str(n_clients), "--n_classes", str(C), "--feature_dim", str(D)])
        self.args, self.eng, self.calls, self.adds, self.reduces, self.globs = args, Engine(), [], [], [], []
        self.n_all = [30 + 10 * c for c in range(n_clients)]
        self.init = (self.eng.state.clone(), self.eng.cnt.copy())
        real_add, real_reduce = driver.RoundAccumulator.add, driver.RoundAccumulator.reduce
        run = self

        def add(acc, n_c, state, counters, active, t=None, proto=None):
            run.adds.append({"n_c": n_c, "n_total": acc.n_total, "state": state.clone(), "cnt": np.array(counters),
                             "active": active, "t": t, "proto": proto})
            return real_add(acc, n_c, state, counters, active, t, proto)

        def reduce(acc, eng, dev, with_tao_proto, scale=1.0):
            out = real_reduce(acc, eng, dev, with_tao_proto, scale)
            run.reduces.append({"with_tao_proto": with_tao_proto, "scale": scale, "out": out, "state": eng.state.clone(),
                                "cnt_float": acc.cnt_float.copy()})
            return out
        monkeypatch.setattr(driver.RoundAccumulator, "add", add)
        monkeypatch.setattr(driver.RoundAccumulator, "reduce", reduce)
        self.row = rows.ROWS[args.exp](args, self.eng, self.n_all, 0, 1, None, "cpu")
        real_aggregate = self.row.aggregate

        def aggregate(rnd, acc):
            cnt = real_aggregate(rnd, acc)
            run.globs.append((self.eng.state.clone(), np.array(cnt), self.eng.cnt.copy()))
            return cnt
        self.row.aggregate = aggregate
        self.net = Net(self.eng)
        clients = {c: Client(c, self.eng, self.calls) for c in range(n_clients)}
        self.log = driver.run_rounds(args, self.row, self.eng, self.net, clients, 0, 1, "cpu", scaffold=scaffold)
        self.n = n_clients

    def round(self, rnd):
        return self.calls[rnd * self.n:(rnd + 1) * self.n]


def _fedavg(calls, weights, total, scale=1.0):
    """RoundAccumulator's arithmetic by hand: fp32 acc += (n_c / total) * state in client order, then * scale; the counters in
    float64"""
    acc, cnt = torch.zeros(NSTATE), np.zeros(2)
    for call, n_c in zip(calls, weights):
        w = n_c / float(total)
        acc.add_(call["after"][0], alpha=w)
        cnt += w * call["after"][1].astype(np.float64)
    return acc.mul_(scale), cnt * scale


def _trunc(x):
    return np.trunc(x + 1e-9).astype(np.int64)


# ---- the table ---------------------------------------------------------------------------------------------------------
def test_the_table_names_every_row():
    choices = driver.build_parser()._option_string_actions["--exp"].choices
    assert sorted(choices) == sorted(["FedMLP", "FedAVG", "FedAVG+FixMatch", "FedLSR", "FedIRM", "RSCFed", "FedNoRo", "CBAFed"])
    assert sorted(rows.ROWS) == sorted(list(choices) + ["RoFL"])
    assert driver.DRIFT_EXPS == ("FedAVG", "FedAVG+FixMatch", "FedMLP")
    assert sorted(e for e, r in rows.ROWS.items() if r.client_ema) == ["FedIRM", "RSCFed"]
    assert (driver.RSCFED_M, driver.RSCFED_K) == (10, 6)
    with pytest.raises(SystemExit):
        driver.args_parser(["--exp", "RoFL"])
    assert driver_rofl.args_parser([]).exp == "RoFL"


# ---- every row that adds to the accumulator ------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,trainer", [
    (["--exp", "FedAVG"], "train"), (["--exp", "FedAVG+FixMatch"], "train_FixMatch"), (["--exp", "FedLSR"], "train_FedLSR"),
    (["--exp", "FedNoRo"], "train_FedNoRo"), (["--exp", "FedMLP", "--rounds_FedMLP_stage1", "2"], "train_FedMLP"),
    (["--exp", "FedIRM", "--rounds_FedIRM_sup", "2"], "train_FedIRM"), (["--exp", "CBAFed", "--rounds_CBAFed_warmup", "9"], "train_CBAFed"),
    ([], "train_RoFL")], ids=lambda v: v if isinstance(v, str) else None)
def test_clients_start_from_the_global_model_and_fedavg_by_n_all(monkeypatch, argv, trainer, capsys):
    r = Run(monkeypatch, argv + ["--rounds_warmup", "3"], 3)
    assert [c["name"] for c in r.calls] == [trainer] * 9 and [c["c"] for c in r.calls] == [0, 1, 2] * 3
    glob = r.init
    for rnd in range(3):
        for call in r.round(rnd):                            # net = deepcopy(netglob) before each client (main.py:181-184)
            assert torch.equal(call["seen"][0], glob[0]) and np.array_equal(call["seen"][1], glob[1])
        want, want_cnt = _fedavg(r.round(rnd), r.n_all, sum(r.n_all))
        state, cnt, eng_cnt = r.globs[rnd]
        assert torch.equal(state, want)
        assert np.array_equal(cnt, _trunc(want_cnt)) and np.array_equal(eng_cnt, cnt)
        glob = (state, cnt)
    assert torch.equal(r.eng.state, glob[0])
    # the records: the keys, the mean of the clients' losses, rank 0 prints them
    assert [set(rec) for rec in r.log] == [{"round", "sec", "mean_loss", "samples_per_sec_per_gpu"}] * 3
    assert [rec["mean_loss"] for rec in r.log] == [float(np.mean([1.0 + c + 10 * rnd for c in range(3)])) for rnd in range(3)]
    assert [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")] == r.log


def test_record_extras_and_the_order_behind_fedavg(monkeypatch, tmp_path):
    """--prox_mu and a SCAFFOLD object in the record; server_update after the global model is taken over, before the row's
    end_round; --save_every through net.state_dict()"""
    r = Run(monkeypatch, ["--exp", "FedAVG", "--rounds_warmup", "2", "--prox_mu", "0.5", "--save_every", "2", "--save_dir", str(tmp_path)], 2)
    assert [rec["prox_mu"] for rec in r.log] == [0.5, 0.5]
    assert sorted(os.listdir(tmp_path)) == ["model_1.pth"]
    assert torch.equal(torch.load(os.path.join(tmp_path, "model_1.pth"))["w"], r.globs[1][0])
    order = []

    class Scaffold:
        c_global = torch.tensor([3.0, 4.0])

        def server_update(self):
            order.append("server_update")
    monkeypatch.setattr(rows.FedAVG, "end_round", lambda self, rnd: order.append("end_round"))
    monkeypatch.setattr(rows.FedAVG, "begin_round", lambda self, rnd: order.append("begin_round"))
    r = Run(monkeypatch, ["--exp", "FedAVG", "--rounds_warmup", "1", "--scaffold", "1"], 2, scaffold=Scaffold())
    assert order == ["begin_round", "server_update", "end_round"]
    assert r.log[0]["scaffold"] == {"c_norm": 5.0} and "prox_mu" not in r.log[0]


# ---- FedMLP (main.py:140-160, 216-234) ---------------------------------------------------------------------------------
def test_fedmlp_row(monkeypatch):
    r = Run(monkeypatch, ["--exp", "FedMLP", "--rounds_FedMLP_stage1", "2", "--rounds_warmup", "4"], 2)
    for rnd in range(4):
        for call in r.round(rnd):
            got_rnd, tao, proto, writer, neg, act = call["a"]
            assert got_rnd == rnd and writer is None and call["k"] == {"net": r.net}
            if rnd == 0:
                assert neg is None and act is None
            else:
                assert neg == [k for k in range(C) if k != call["c"]] and act == [call["c"]]
            if rnd <= 1:                                     # until round S1 - 1 = 1 has been aggregated
                assert tao == [0] * C and proto is None
            else:                                            # exactly what the previous round's reduce returned
                assert tao is r.reduces[rnd - 1]["out"][1] and proto is r.reduces[rnd - 1]["out"][2]
        for call, add in zip(r.round(rnd), r.adds[2 * rnd:2 * rnd + 2]):
            assert add["n_c"] == r.n_all[call["c"]] and add["active"] == [call["c"]]
            if rnd == 0:
                assert add["t"] is None and add["proto"] is None
            else:
                assert add["t"] is call["ret"][6] and add["proto"] is call["ret"][7] and len(call["ret"]) == RESULT + 2
        assert r.reduces[rnd]["with_tao_proto"] == (rnd >= 1) and r.reduces[rnd]["scale"] == 1.0
    assert r.reduces[0]["out"][1] is None and r.reduces[1]["out"][1] is not None
    assert r.row.tao is r.reduces[3]["out"][1] and r.row.Prototype is r.reduces[3]["out"][2]


# ---- FedIRM (main.py:169-177, 192-193, 238-251) ------------------------------------------------------------------------
def test_fedirm_row(monkeypatch):
    folds = []
    real = fedavg.FedAvg_rela

    def spy(protos, weight, class_active_client_list):
        out = real(protos, weight, class_active_client_list)
        folds.append({"protos": protos, "weight": weight, "cls": class_active_client_list, "out": out})
        return out
    monkeypatch.setattr(fedavg, "FedAvg_rela", spy)
    r = Run(monkeypatch, ["--exp", "FedIRM", "--rounds_FedIRM_sup", "2", "--rounds_warmup", "4"], 5)
    assert len(folds) == 3                                   # rounds 1, 2, 3
    P1 = folds[0]["out"]                                     # round SI - 1: Prototype = FedAvg_rela(...)
    lam = 1.0
    P2 = (1 - lam) * P1 + lam * folds[1]["out"]              # afterwards: the fold with lam = 1
    P3 = (1 - lam) * P2 + lam * folds[2]["out"]
    want_P = [None, None, P1, P2]
    for rnd in range(4):
        for call in r.round(rnd):
            got_rnd, P, writer, neg, act = call["a"]
            assert got_rnd == rnd and writer is None and call["k"] == {"net": r.net}
            assert (P is None) if want_P[rnd] is None else torch.equal(P, want_P[rnd])
            if rnd == 0:                                     # rnd < SI - 1: the supervised call, six values back
                assert neg is None and act is None and len(call["ret"]) == RESULT
            else:
                assert neg == [k for k in range(C) if k != call["c"] % C] and act == [call["c"] % C]
        if rnd >= 1:
            f = folds[rnd - 1]
            assert all(torch.equal(p, call["ret"][6]) for p, call in zip(f["protos"], r.round(rnd))) and len(f["protos"]) == 5
            assert f["weight"] == r.n_all and f["cls"] == [[0, 4], [1], [2], [3]]     # client c annotates class c mod C
    assert r.row.Prototype is not None and torch.equal(r.row.Prototype, P3)
    assert all(a["t"] is None and a["proto"] is None for a in r.adds) and len(r.adds) == 20


# ---- RSCFed (main.py:114-121, 164-166, 213-215) ------------------------------------------------------------------------
def test_rscfed_row(monkeypatch):
    seen = []

    def rscfed_round(eng, DMA, states, counters, n_all, rank, world, dist_):
        seen.append({"DMA": DMA, "states": dict(states), "counters": dict(counters), "n_all": n_all,
                     "rest": (rank, world, dist_)})
        eng.state_tensor().fill_(float(len(seen)))
        cnt = np.array([10 * len(seen), 7], np.int64)
        eng.counters(cnt)
        return cnt
    monkeypatch.setattr(driver, "rscfed_round", rscfed_round)
    r = Run(monkeypatch, ["--exp", "RSCFed", "--rounds_warmup", "3", "--seed", "11"], 7)
    assert r.adds == [] and r.reduces == []                  # RSCFed is not a FedAvg by n_all
    rng = random.Random(11)                                  # ONE generator, continued over the rounds
    glob = r.init
    for rnd in range(3):
        s = seen[rnd]
        assert s["DMA"] == [rng.sample(range(7), 6) for _ in range(10)]
        assert s["n_all"] == r.n_all and s["rest"] == (0, 1, None) and sorted(s["states"]) == list(range(7))
        for call in r.round(rnd):
            assert call["name"] == "train_RSCFed" and call["a"] == (rnd, r.net) and call["k"] == {}
            assert torch.equal(call["seen"][0], glob[0]) and np.array_equal(call["seen"][1], glob[1])
            assert torch.equal(s["states"][call["c"]], call["after"][0])
            assert np.array_equal(s["counters"][call["c"]], call["after"][1])
        glob = (torch.full((NSTATE,), float(rnd + 1)), np.array([10 * (rnd + 1), 7]))
        assert torch.equal(r.globs[rnd][0], glob[0]) and np.array_equal(r.globs[rnd][1], glob[1])


# ---- FedNoRo (main.py:127-128, 140-144) --------------------------------------------------------------------------------
def test_fednoro_row(monkeypatch):
    r = Run(monkeypatch, ["--exp", "FedNoRo", "--rounds_warmup", "4", "--begin", "1", "--end", "3", "--a", "0.75"], 2)
    kds = []
    for rnd in range(4):
        for call in r.round(rnd):
            assert call["a"] == (call["c"], rnd, r.net, None)
            assert call["k"] == {"weight_kd": fedavg.consistency_weight(rnd, 1, 3) * 0.75}
        kds.append(r.round(rnd)[0]["k"]["weight_kd"])
    assert kds[0] == kds[1] < kds[2] < kds[3] == 0.75        # the ramp between --begin and --end, times --a


# ---- CBAFed (main.py:149-157, 269-316) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [8, 13])
def test_cbafed_row(monkeypatch, rounds):
    """WC = 2.  8 rounds: the stores at rounds 0 and 2 and stage 2's first 0.5 / 0.5 blend at round 7; 13 rounds: the blend of
    round 12 mixes in what round 7 left, the blended model"""
    WC = 2
    taos, blends = [], []
    real_tao, real_blend = fedavg.cbafed_tao, fedavg.cbafed_blend

    def spy_tao(class_num_lists, data_nums):
        out = real_tao(class_num_lists, data_nums)
        taos.append({"cn": class_num_lists, "dn": data_nums, "out": out})
        return out

    def spy_blend(rnd, warmup):
        blends.append((rnd, warmup))
        return real_blend(rnd, warmup)
    monkeypatch.setattr(fedavg, "cbafed_tao", spy_tao)
    monkeypatch.setattr(fedavg, "cbafed_blend", spy_blend)
    r = Run(monkeypatch, ["--exp", "CBAFed", "--rounds_CBAFed_warmup", str(WC), "--rounds_warmup", str(rounds)], 2)
    assert blends == [(rnd, WC) for rnd in range(rounds)]
    assert len(taos) == rounds - (WC - 1)                    # from round WC - 1 on
    # main.py:274-288, 303-316 for WC = 2: round 0 stores; round 2 (the first of stage 2) stores; rounds 7, 12 blend 0.5 / 0.5
    blend_at = {7: 2, 12: 7}                                 # round -> the round whose model it mixes in
    kept_cnt = {}                                            # round -> the float counters of the model it left
    glob = r.init
    for rnd in range(rounds):
        calls = r.round(rnd)
        for call in calls:
            assert call["a"] == (rnd, r.net)
            if rnd < WC:
                assert call["k"] == {}                       # the warm-up call has no pt / tao
            else:
                prev = taos[rnd - 1 - (WC - 1)]["out"]       # the previous round's cbafed_tao
                assert set(call["k"]) == {"pt", "tao"} and call["k"]["pt"] is prev[0] and call["k"]["tao"] is prev[1]
            assert torch.equal(call["seen"][0], glob[0]) and np.array_equal(call["seen"][1], glob[1])
        data_num = [20 + 3 * c + rnd for c in range(2)]      # what the stand-ins return
        weights, total = (r.n_all, sum(r.n_all)) if rnd < WC else (data_num, 1.0)
        scale = 1.0 if rnd < WC else 1.0 / float(sum(data_num))
        adds = r.adds[2 * rnd:2 * rnd + 2]
        assert [a["n_c"] for a in adds] == weights and all(a["n_total"] == total for a in adds)
        assert all(a["t"] is None and a["proto"] is None for a in adds)
        assert r.reduces[rnd]["scale"] == scale and not r.reduces[rnd]["with_tao_proto"]
        want, want_cnt = _fedavg(calls, weights, total, scale)
        assert torch.equal(r.reduces[rnd]["state"], want)
        np.testing.assert_array_equal(r.reduces[rnd]["cnt_float"], want_cnt)
        if rnd in blend_at:
            res, res_cnt = r.globs[blend_at[rnd]][0], kept_cnt[blend_at[rnd]]
            # two rounded fp32 products, then their sum
            want = want * torch.tensor(0.5) + res * torch.tensor(0.5)
            want_cnt = 0.5 * want_cnt + 0.5 * res_cnt
        kept_cnt[rnd] = want_cnt
        state, cnt, eng_cnt = r.globs[rnd]
        assert torch.equal(state, want)
        assert np.array_equal(cnt, _trunc(want_cnt)) and np.array_equal(eng_cnt, cnt)
        glob = (state, cnt)
        if rnd >= WC - 1:
            t = taos[rnd - (WC - 1)]
            assert t["dn"] == data_num and all(torch.equal(a, call["ret"][6]) for a, call in zip(t["cn"], calls))
    assert r.row.pt is taos[-1]["out"][0] and r.row.tao is taos[-1]["out"][1]


def test_cbafed_warmup_blend(monkeypatch):
    """WC = 6 of 7 rounds: round 5 is the warm-up's 0.2 / 0.8 blend with the model stored at round 0, FedAvg by n_all"""
    r = Run(monkeypatch, ["--exp", "CBAFed", "--rounds_CBAFed_warmup", "6", "--rounds_warmup", "7"], 2)
    fed5, cnt5 = _fedavg(r.round(5), r.n_all, sum(r.n_all))
    fed0, cnt0 = _fedavg(r.round(0), r.n_all, sum(r.n_all))
    assert torch.equal(r.globs[0][0], fed0)
    assert torch.equal(r.globs[5][0], fed5 * torch.tensor(0.2) + fed0 * torch.tensor(0.8))
    assert np.array_equal(r.globs[5][1], _trunc(0.2 * cnt5 + (1.0 - 0.2) * cnt0))
    assert [a["n_c"] for a in r.adds[:12]] == r.n_all * 6 and [a["n_c"] for a in r.adds[12:]] == [26, 29]
    assert r.reduces[6]["scale"] == 1.0 / 55.0


# ---- RoFL (main.py:98-99, 167-168, 253-268) ----------------------------------------------------------------------------
def test_rofl_row(monkeypatch):
    folds = []
    real = fedavg.rofl_centroids

    def spy(f_G, f_locals):
        out = real(f_G, f_locals)
        folds.append({"f_G": f_G, "f_locals": f_locals, "out": out})
        return out
    monkeypatch.setattr(fedavg, "rofl_centroids", spy)
    r = Run(monkeypatch, ["--rounds_warmup", "3", "--seed", "5"], 3)
    f_G = torch.randn((2 * C, D), generator=torch.Generator().manual_seed(5))
    for rnd in range(3):
        for call in r.round(rnd):
            net, got, epoch = call["a"]
            assert net is r.net and epoch == rnd and torch.equal(got, f_G)
        assert torch.equal(folds[rnd]["f_G"], f_G) and len(folds[rnd]["f_locals"]) == 3
        assert all(a is call["ret"][2] for a, call in zip(folds[rnd]["f_locals"], r.round(rnd)))     # clients 0 .. n-1 in order
        f_G = folds[rnd]["out"]
    assert r.row.f_G is f_G and len(folds) == 3


# ---- fedavg.gather_dicts under gloo ------------------------------------------------------------------------------------
def _gather_worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2, timeout=datetime.timedelta(seconds=180))
    mine = {0: torch.tensor([1.0, 2.0]), 2: ("c", 3)} if rank == 0 else {1: np.array([4, 5])}
    got = fedavg.gather_dicts(dist, mine)
    torch.save(got, os.path.join(out_dir, f"g{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_dicts_merges_the_ranks(tmp_path):
    mine = {3: "x"}
    assert fedavg.gather_dicts(None, mine) is mine           # one rank: the identity
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_gather_worker, args=(port, str(tmp_path)), nprocs=2, join=True)
    for rank in range(2):
        got = torch.load(os.path.join(str(tmp_path), f"g{rank}.pt"), weights_only=False)
        assert sorted(got) == [0, 1, 2]
        assert torch.equal(got[0], torch.tensor([1.0, 2.0])) and np.array_equal(got[1], np.array([4, 5])) and got[2] == ("c", 3)
