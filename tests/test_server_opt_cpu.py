"""Server optimizers (FedAvgM, FedAdagrad, FedAdam, FedYogi) without a GPU: the C ABI's bookkeeping (include/fedmlp_hip_server.h =
_lib.SERVER_SYMBOLS = the library's exports), the reference rule tests/server_opt_ref.py against float64 closed forms, the host
drop-in fedmlp_amd.server_opt.apply against that reference bit for bit, the optimizer's state_dict, the driver's flags, and where
driver.run_rounds calls the step."""
import ctypes as C
import datetime
import os
import re
import socket
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedmlp_amd import _lib, server_opt
from tests import server_opt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fm_server_opt_begin": 2, "fm_server_opt_step": 3, "fm_server_opt_get_state": 4, "fm_server_opt_set_state": 4,
         "fm_server_opt_end": 1, "fm_server_opt_active": 1}
F = np.float32
HP = {"avgm": dict(lr=1.0, beta1=0.9), "adagrad": dict(lr=1e-2, beta1=0.9, tau=1e-3),
      "adam": dict(lr=1e-2, beta1=0.9, beta2=0.99, tau=1e-3), "yogi": dict(lr=1e-2, beta1=0.9, beta2=0.99, tau=1e-3)}


def _declared(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m: a for m, a in re.findall(r"^int\s+(fm_\w+)\s*\(([^;]*)\);", text, flags=re.M | re.S)}


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_header_table_and_exports_agree():
    decl = _declared("fedmlp_hip_server.h")
    assert set(decl) == set(_lib.SERVER_SYMBOLS) == set(NAMES)
    others = set(_declared("fedmlp_hip.h")) | set(_declared("fedmlp_hip_rofl.h")) | set(_declared("fedmlp_hip_drift.h"))
    assert not set(decl) & others
    assert not set(_lib.SERVER_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.ROFL_SYMBOLS) | set(_lib.DRIFT_SYMBOLS))
    for name, args in decl.items():
        res, argtypes = _lib.SERVER_SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == len(args.split(",")) == NAMES[name], name
    assert [f for f, _ in _lib.FmServerOpt._fields_] == ["rule", "lr", "beta1", "beta2", "tau"] and C.sizeof(_lib.FmServerOpt) == 20
    with open(os.path.join(ROOT, "Makefile")) as f:
        assert "include/fedmlp_hip_server.h" in f.read()
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfedmlp_hip.so not built (run `make`)")
    lib = _lib.load()
    for name, (res, argtypes) in _lib.SERVER_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == argtypes, name


def test_the_wrappers_live_outside_engine():
    """Engine's method list is closed: the wrappers are functions of fedmlp_amd/server_opt.py that go through the engine's stream
    check; the step counts as a weight move, the others as plain work"""
    import ast
    with open(os.path.join(ROOT, "fedmlp_amd", "server_opt.py")) as f:
        tree = ast.parse(f.read())
    fns = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    for name, fm in (("server_begin", "fm_server_opt_begin"), ("server_step", "fm_server_opt_step"),
                     ("server_get_state", "fm_server_opt_get_state"), ("server_set_state", "fm_server_opt_set_state"),
                     ("server_end", "fm_server_opt_end")):
        calls = [n for n in ast.walk(fns[name]) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)]
        attrs = [c.func.attr for c in calls]
        assert "_check_stream" in attrs and fm in attrs, name
        enq = [c for c in calls if c.func.attr == "_enqueue"]
        assert len(enq) == 1, name
        kw = {k.arg: ast.literal_eval(k.value) for k in enq[0].keywords}
        assert kw == ({"weights": True} if name == "server_step" else {}) and not enq[0].args, name
    with open(os.path.join(ROOT, "fedmlp_amd", "engine.py")) as f:
        assert "fm_server_opt" not in f.read()


# ---- the reference rule against float64 closed forms ------------------------------------------------------------------------
# rounded fp32 operations on the way to x' / m / v of the FIRST step, counted off the header's statement of the rule (the sign of
# Yogi is a decision, not a rounding).  The test allows one fp32 ulp (2^-23 relative) per operation.
OPS_X = {"avgm": 5, "adagrad": 11, "adam": 13, "yogi": 13}
OPS_M = {"avgm": 3, "adagrad": 4, "adam": 4, "yogi": 4}
OPS_V = {"adagrad": 3, "adam": 5, "yogi": 5}
ULP = 2.0 ** -23


def _first_step_data(tau):
    """x, a: both signs, |d| from 1e-6 to 1, d*d above and below tau^2, exact zeros of d, and d == tau (Yogi: v == q)"""
    rs = np.random.RandomState(3)
    n = 4096
    x = rs.standard_normal(n).astype(F)
    mag = (10.0 ** rs.uniform(-6, 0, n)).astype(F)
    d = mag * rs.choice([-1.0, 1.0], n).astype(F)
    a = (x + d).astype(F)
    a[:64] = x[:64]                                  # d == 0
    x[64:96] = 0.0
    a[64:96] = F(tau)                                # d == tau exactly: q = fl(tau * tau) = v
    return x, a


@pytest.mark.parametrize("rule", R.RULES)
def test_first_step_closed_form(rule):
    hp = HP[rule]
    lr, b1 = float(F(hp["lr"])), float(F(hp["beta1"]))
    b2, tau = float(F(hp.get("beta2", 0.0))), float(F(hp.get("tau", 0.0)))
    x, a = _first_step_data(hp.get("tau", 1e-3))
    m0, v0 = R.init(rule, x.size, hp.get("tau", 0.0))
    assert not m0.any() and (v0 is None or np.all(v0 == F(tau) * F(tau)))
    x1, m1, v1 = R.step(rule, x, a, m0, v0, **hp)
    assert x1.dtype == F and m1.dtype == F
    x64, d64 = x.astype(np.float64), a.astype(np.float64) - x.astype(np.float64)
    if rule == "avgm":
        m64 = d64
        t64 = lr * m64
    else:
        omb1, omb2 = float(F(1.0) - F(b1)), float(F(1.0) - F(b2))
        m64 = omb1 * d64
        q64, v064 = d64 * d64, float(F(tau) * F(tau))
        if rule == "adagrad":
            v64 = v064 + q64
        elif rule == "adam":
            v64 = b2 * v064 + omb2 * q64
        else:
            d32 = a - x
            s = np.sign(v0 - d32 * d32).astype(np.float64)       # the rule's own decision, from its fp32 operands
            assert (s > 0).any() and (s < 0).any() and (s[64:96] == 0).all(), "Yogi's sign is not exercised all three ways"
            v64 = v064 - omb2 * q64 * s
            assert np.array_equal(v1[64:96].view(np.int32), v0[64:96].view(np.int32)), "v moved where v == q"
        t64 = lr * m64 / (np.sqrt(v64) + tau)
        assert np.all(np.abs(v1 - v64) <= OPS_V[rule] * ULP * np.abs(v64)), rule
        assert (d64 * d64 > v064).any() and (d64 * d64 < v064).any()
    want = x64 + t64
    scale = np.maximum(np.maximum(np.abs(x64), np.abs(want)), np.abs(t64))
    err_x = np.abs(x1 - want)
    print(f"\n[server_opt] {rule}: first step, max error / bound {float((err_x / (OPS_X[rule] * ULP * scale + 1e-300)).max()):.3f}")
    assert np.all(err_x <= OPS_X[rule] * ULP * scale), rule
    assert np.all(np.abs(m1 - m64) <= OPS_M[rule] * ULP * np.abs(m64)), rule
    # a zero pseudo-gradient leaves x bit-identical (and its moments where they started)
    assert np.array_equal(x1[:64].view(np.int32), x[:64].view(np.int32)) and not m1[:64].any()
    assert int((x1[96:] != x[96:]).sum()) > 0.5 * (x.size - 96), "the step moved nothing"


def test_rule_rounds_every_operation_on_its_own():
    """the fp32 rule differs somewhere from the same expressions evaluated in float64 and rounded once"""
    x, a = _first_step_data(1e-3)
    hp = HP["adam"]
    m, v = R.init("adam", x.size, hp["tau"])
    for _ in range(2):
        x1, m, v = R.step("adam", x, a, m, v, **hp)
    b1, omb1 = float(F(hp["beta1"])), float(F(1.0) - F(hp["beta1"]))
    d = a.astype(np.float64) - x
    m64 = b1 * (omb1 * d) + omb1 * d
    assert int((m64.astype(F) != m).sum()) > 0
    assert np.allclose(m, m64, rtol=1e-6, atol=0)


# ---- the host drop-in ------------------------------------------------------------------------------------------------------
KEYS = [("conv.weight", (6, 3, 3, 3), "f"), ("bn.weight", (6,), "f"), ("bn.bias", (6,), "f"), ("bn.running_mean", (6,), "f"),
        ("bn.running_var", (6,), "f"), ("bn.num_batches_tracked", (), "i"), ("fc.weight", (5, 6), "f"), ("fc.bias", (5,), "f")]
PARAMS = [k for k, _, dt in KEYS if dt == "f" and "running" not in k]


def _sd(seed, scale=1.0):
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    for k, shape, dt in KEYS:
        if dt == "i":
            sd[k] = torch.tensor(seed * 10, dtype=torch.int64)
        else:
            v = rs.standard_normal(shape).astype(F) * F(scale)
            sd[k] = torch.from_numpy(np.abs(v) + F(0.5) if k.endswith("running_var") else v)
    return sd


def _avg(x, seed):
    """an aggregate near x: parameters moved by 1e-6 .. 1, a few left where they are"""
    rs = np.random.RandomState(seed)
    out = _sd(seed + 100)
    for k in PARAMS:
        xn = x[k].numpy()
        p = (10.0 ** rs.uniform(-6, 0, xn.shape)).astype(F) * rs.choice([-1.0, 1.0], xn.shape).astype(F)
        p.reshape(-1)[::7] = 0
        out[k] = torch.from_numpy((xn + p).astype(F))
    return out


def _ref_rounds(rule, x, avgs):
    """the reference over consecutive rounds -> [(x' per key, m per key, v per key)]"""
    hp = HP[rule]
    st = {k: R.init(rule, x[k].numel(), hp.get("tau", 0.0)) for k in PARAMS}
    cur, out = {k: x[k].numpy().reshape(-1) for k in PARAMS}, []
    for w_avg in avgs:
        res = {}
        for k in PARAMS:
            x1, m, v = R.step(rule, cur[k], w_avg[k].numpy().reshape(-1), st[k][0], st[k][1], **hp)
            st[k] = (m, v)
            res[k] = x1
        cur = res
        out.append((res, {k: st[k][0] for k in PARAMS}, {k: st[k][1] for k in PARAMS}))
    return out


def _make(rule):
    return server_opt.make(rule, **HP[rule])


def _bits(t):
    return np.asarray(t, dtype=F).reshape(-1).view(np.int32)


def _run_apply(opt, x, seeds):
    outs, avgs = [], []
    for s in seeds:
        w_avg = _avg(x, s)
        avgs.append(w_avg)
        x = server_opt.apply(opt, x, w_avg)
        outs.append(x)
    return outs, avgs


@pytest.mark.parametrize("rule", R.RULES)
def test_apply_equals_the_reference_bit_for_bit(rule):
    x0 = _sd(1)
    opt = _make(rule)
    outs, avgs = _run_apply(opt, x0, (11, 12, 13))
    ref = _ref_rounds(rule, x0, avgs)
    assert opt.steps == 3
    for rnd, (out, w_avg) in enumerate(zip(outs, avgs)):
        assert list(out) == [k for k, _, _ in KEYS]
        for k, shape, dt in KEYS:
            if k in PARAMS:
                assert out[k].dtype == torch.float32 and tuple(out[k].shape) == shape
                assert np.array_equal(_bits(out[k]), ref[rnd][0][k].view(np.int32)), (rule, rnd, k)
            else:                                    # buffers and counters: exactly w_avg's, and no alias of them
                assert out[k].dtype == w_avg[k].dtype and torch.equal(out[k], w_avg[k]), k
                assert out[k].data_ptr() != w_avg[k].data_ptr()
    # the moments, flat in state_dict order with zeros at the buffers' slots
    sd = opt.state_dict()
    assert sd["step"] == 3 and sd["hyper"]["rule"] == rule
    off = 0
    for k, shape, dt in KEYS:
        if dt == "i":
            continue
        n = int(np.prod(shape))
        if k in PARAMS:
            assert np.array_equal(_bits(sd["m"][off:off + n]), ref[2][1][k].view(np.int32)), k
            if rule != "avgm":
                assert np.array_equal(_bits(sd["v"][off:off + n]), ref[2][2][k].view(np.int32)), k
        else:
            assert not sd["m"][off:off + n].any() and not sd["v"][off:off + n].any(), k
        off += n
    assert off == sd["m"].numel() == sd["v"].numel()


@pytest.mark.parametrize("rule", R.RULES)
def test_state_dict_round_trip(rule):
    x0 = _sd(2)
    straight, _ = _run_apply(_make(rule), x0, (21, 22, 23))
    first = _make(rule)
    two, _ = _run_apply(first, x0, (21, 22))
    sd = first.state_dict()
    sd = {"hyper": dict(sd["hyper"]), "step": sd["step"], "m": sd["m"].clone(), "v": sd["v"].clone()}
    again = server_opt.CLASSES[rule]()
    again.load_state_dict(sd)
    assert again.steps == 2 and again.hyper() == first.hyper()
    third = server_opt.apply(again, two[1], _avg(two[1], 23))
    for k in PARAMS:
        assert np.array_equal(_bits(third[k]), _bits(straight[2][k])), (rule, k)
    assert again.steps == 3
    # ... and the optimizer that was asked for its state goes on unchanged
    third = server_opt.apply(first, two[1], _avg(two[1], 23))
    for k in PARAMS:
        assert np.array_equal(_bits(third[k]), _bits(straight[2][k])), (rule, k)
    with pytest.raises(ValueError):
        server_opt.CLASSES["avgm" if rule != "avgm" else "adam"]().load_state_dict(sd)


def test_load_state_dict_checks_what_it_takes():
    """the file's hyper-parameters replace the object's, after the constructor's checks; a refused state changes nothing"""
    opt = server_opt.FedYogi(lr=0.5)
    good = {"hyper": {"rule": "yogi", "lr": 0.25, "beta1": 0.5, "beta2": 0.75, "tau": 0.125}, "step": 4, "m": None, "v": None}
    opt.load_state_dict(good)
    assert opt.hyper() == good["hyper"] and opt.steps == 4
    for key, val, text in (("lr", -1.0, "lr must be finite"), ("lr", float("nan"), "lr must be finite"), ("beta1", 1.0, "beta1 must lie"),
                           ("beta2", -0.5, "beta2 must lie"), ("tau", 0.0, "tau must be finite and > 0"),
                           ("tau", float("inf"), "tau must be finite and > 0")):
        bad = dict(good, hyper=dict(good["hyper"], **{key: val}), step=9)
        with pytest.raises(ValueError, match=text):
            opt.load_state_dict(bad)
        assert opt.hyper() == good["hyper"] and opt.steps == 4
    with pytest.raises(ValueError, match="step must be >= 0"):
        opt.load_state_dict(dict(good, step=-1))
    with pytest.raises(ValueError, match="differ in size"):
        opt.load_state_dict(dict(good, m=torch.zeros(4), v=torch.zeros(5)))
    assert opt.hyper() == good["hyper"] and opt.steps == 4
    # what a rule does not read is not checked, as in the constructor
    server_opt.FedAvgM().load_state_dict({"hyper": {"rule": "avgm", "lr": 1.0, "beta1": 0.5, "beta2": 7.0, "tau": -1.0},
                                          "step": 0, "m": None, "v": None})


def test_classes_and_their_defaults():
    assert server_opt.FedAvgM().hyper() == {"rule": "avgm", "lr": 1.0, "beta1": 0.9, "beta2": 0.0, "tau": 0.0}
    assert server_opt.FedAdagrad().hyper() == {"rule": "adagrad", "lr": 1e-2, "beta1": 0.9, "beta2": 0.0, "tau": 1e-3}
    assert server_opt.FedAdam().hyper() == {"rule": "adam", "lr": 1e-2, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}
    assert server_opt.FedYogi().hyper() == {"rule": "yogi", "lr": 1e-2, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}
    assert server_opt.FedAvgM(lr=0.5, momentum=0.7).beta1 == 0.7
    for cls in server_opt.CLASSES.values():
        for m in ("begin", "step", "end", "state_dict", "load_state_dict"):
            assert callable(getattr(cls, m))
    for bad in (dict(lr=-1.0), dict(lr=float("nan")), dict(lr=float("inf")), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0),
                dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan"))):
        with pytest.raises(ValueError):
            server_opt.FedYogi(**bad)
    server_opt.FedAdagrad(lr=0.0)


# ---- two ranks over gloo: the host path, no communication of its own ---------------------------------------------------------
WORLD = 2


def _gloo_worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=180))
    x0 = _sd(5)
    for rule in R.RULES:
        outs, _ = _run_apply(_make(rule), x0, (31, 32))
        np.save(os.path.join(out_dir, f"{rule}{rank}.npy"), np.concatenate([_bits(outs[1][k]) for k, _, _ in KEYS]))
    dist.barrier()
    dist.destroy_process_group()


def test_world_2_gloo_same_bits(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_gloo_worker, args=(port, str(tmp_path)), nprocs=WORLD, join=True)
    for rule in R.RULES:
        a, b = (np.load(os.path.join(str(tmp_path), f"{rule}{r}.npy")) for r in range(WORLD))
        assert a.size > 0 and np.array_equal(a, b), rule


# ---- the driver's flags ---------------------------------------------------------------------------------------------------
def _refused(capsys, parse, argv):
    with pytest.raises(SystemExit):
        parse(argv)
    return capsys.readouterr().err


def test_driver_flags(capsys):
    from fedmlp_amd import driver, driver_rofl
    base = vars(driver.args_parser([]))
    assert base["server_opt"] == "none" and base["init_server_opt"] is None
    assert all(base[k] is None for k in ("server_lr", "server_beta1", "server_beta2", "server_tau"))
    assert vars(driver.args_parser(["--server_opt", "none"])) == base
    for exp in ("FedMLP", "FedAVG", "FedAVG+FixMatch", "FedLSR", "FedIRM", "FedNoRo"):
        for rule in ("avgm", "adagrad", "adam", "yogi"):
            assert driver.args_parser(["--exp", exp, "--server_opt", rule]).server_opt == rule
    a = driver.args_parser(["--exp", "FedAVG", "--server_opt", "yogi", "--server_lr", "0.1", "--server_beta1", "0.5",
                            "--server_beta2", "0.9", "--server_tau", "0.01", "--prox_mu", "0.01"])
    assert (a.server_lr, a.server_beta1, a.server_beta2, a.server_tau, a.prox_mu) == (0.1, 0.5, 0.9, 0.01, 0.01)
    assert driver.args_parser(["--exp", "FedAVG", "--server_opt", "adam", "--scaffold", "1"]).scaffold == 1
    assert driver_rofl.args_parser(["--server_opt", "adam"]).server_opt == "adam"
    for exp in ("RSCFed", "CBAFed"):
        assert driver.args_parser(["--exp", exp]).exp == exp
        err = _refused(capsys, driver.args_parser, ["--exp", exp, "--server_opt", "adam"])
        assert "server arithmetic of its own" in err and "RSCFed" in err and "CBAFed" in err
    assert "invalid choice" in _refused(capsys, driver.args_parser, ["--server_opt", "sgd"])
    for flag, val, text in (("--server_lr", "-1", "lr must be finite and >= 0"), ("--server_lr", "nan", "lr must be finite and >= 0"),
                            ("--server_lr", "inf", "lr must be finite and >= 0"), ("--server_beta1", "1", "beta1 must lie in [0, 1)"),
                            ("--server_beta1", "-0.5", "beta1 must lie in [0, 1)"), ("--server_beta2", "1.5", "beta2 must lie in [0, 1)"),
                            ("--server_tau", "0", "tau must be finite and > 0"), ("--server_tau", "inf", "tau must be finite and > 0")):
        assert text in _refused(capsys, driver.args_parser, ["--exp", "FedAVG", "--server_opt", "yogi", flag, val]), (flag, val)
        assert text in _refused(capsys, driver_rofl.args_parser, ["--server_opt", "yogi", flag, val]), (flag, val)
    for flag in ("--server_lr", "--server_beta1", "--server_beta2", "--server_tau"):
        assert f"{flag} needs --server_opt" in _refused(capsys, driver.args_parser, [flag, "0.5"])
    assert "--init_server_opt needs --server_opt" in _refused(capsys, driver.args_parser, ["--init_server_opt", "x.pth"])


# ---- run_rounds ------------------------------------------------------------------------------------------------------------
class _Server:
    rule = "yogi"

    def __init__(self, events):
        self.events, self.steps, self.seen = events, 0, []

    def step(self, eng, old_global):
        self.events.append("step")
        self.seen.append((old_global.clone(), eng.state.clone()))
        eng.state.mul_(0.5)                          # the new global model is neither the aggregate nor the old one
        self.steps += 1
        return torch.tensor(float(self.steps), dtype=torch.float64)

    def state_dict(self):
        return {"step": self.steps}


def _run_rounds(server, tmp_path=None, rounds=3):
    from fedmlp_amd import driver, rows
    from tests.test_driver_rows_cpu import C as NC, D, Client, Engine, Net
    argv = ["--exp", "FedAVG", "--rounds_warmup", str(rounds), "--n_clients", "2", "--n_classes", str(NC), "--feature_dim", str(D)]
    if tmp_path is not None:
        argv += ["--save_every", "2", "--save_dir", str(tmp_path)]
    args = driver.args_parser(argv)
    for k in ("server_opt", "server_lr", "server_beta1", "server_beta2", "server_tau", "init_server_opt"):
        delattr(args, k)                             # run_rounds reads none of them
    eng, calls, events = Engine(), [], []
    if server is not None:
        server.events = events
    row = rows.ROWS[args.exp](args, eng, [30, 40], 0, 1, None, "cpu")
    real_aggregate, real_end = row.aggregate, row.end_round
    aggs = []

    def aggregate(rnd, acc):
        cnt = real_aggregate(rnd, acc)
        events.append("aggregate")
        aggs.append(eng.state.clone())
        return cnt

    def end_round(rnd):
        events.append("end_round")
        return real_end(rnd)
    row.aggregate, row.end_round = aggregate, end_round
    clients = {c: Client(c, eng, calls) for c in range(2)}
    start = eng.state.clone()
    kw = {} if server is None else {"server": server}
    log = driver.run_rounds(args, row, eng, Net(eng), clients, 0, 1, "cpu", **kw)
    return log, events, aggs, calls, start


def test_run_rounds_calls_the_step_once_per_round(tmp_path):
    srv = _Server(None)
    log, events, aggs, calls, start = _run_rounds(srv, tmp_path)
    assert events == ["aggregate", "step", "end_round"] * 3 and srv.steps == 3
    glob = start
    for rnd in range(3):
        old, agg = srv.seen[rnd]
        assert torch.equal(old, glob), "the step did not get the round's starting global model"
        assert torch.equal(agg, aggs[rnd]), "the step did not see the aggregate in the engine"
        glob = agg * 0.5
        for call in calls[2 * rnd:2 * rnd + 2]:
            assert torch.equal(call["seen"][0], old), "a client did not start from the server's new global model"
        assert log[rnd]["server_opt"] == {"rule": "yogi", "step": rnd + 1, "delta_norm": float(rnd + 1)}
    assert torch.load(os.path.join(str(tmp_path), "server_opt_1.pth")) == {"step": 2}
    assert not os.path.exists(os.path.join(str(tmp_path), "server_opt_0.pth"))


def test_run_rounds_without_a_server(tmp_path):
    log, events, aggs, calls, start = _run_rounds(None, tmp_path)
    assert events == ["aggregate", "end_round"] * 3
    assert all("server_opt" not in rec for rec in log)
    assert os.path.exists(os.path.join(str(tmp_path), "model_1.pth"))
    assert not os.path.exists(os.path.join(str(tmp_path), "server_opt_1.pth"))
    for call in calls[2:4]:
        assert torch.equal(call["seen"][0], aggs[0])
