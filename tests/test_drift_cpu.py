"""Client-drift correction (FedProx, SCAFFOLD) without a GPU: the C ABI's bookkeeping (include/fedmlp_hip_drift.h = _lib.DRIFT_SYMBOLS
= the library's exports), the properties of the reference rule tests/drift_ref.py restates, Scaffold's server update against hand
arithmetic (one process, and a world of two over gloo), and the driver's two flags."""
import ctypes as C
import datetime
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedmlp_amd import _lib
from tests import drift_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fm_drift_begin": 4, "fm_drift_last": 2, "fm_drift_end": 3, "fm_drift_active": 1}


def _declared(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m: a for m, a in re.findall(r"^int\s+(fm_\w+)\s*\(([^;]*)\);", text, flags=re.M | re.S)}


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_header_table_and_exports_agree():
    decl = _declared("fedmlp_hip_drift.h")
    assert set(decl) == set(_lib.DRIFT_SYMBOLS) == set(NAMES)
    others = set(_declared("fedmlp_hip.h")) | set(_declared("fedmlp_hip_rofl.h"))
    assert not set(decl) & others
    assert not set(_lib.DRIFT_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.ROFL_SYMBOLS))
    for name, args in decl.items():
        res, argtypes = _lib.DRIFT_SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == len(args.split(",")) == NAMES[name], name
    assert _lib.DRIFT_SYMBOLS["fm_drift_begin"][1][1] is C.c_float and _lib.DRIFT_SYMBOLS["fm_drift_begin"][1][3] is C.c_int32
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfedmlp_hip.so not built (run `make`)")
    lib = _lib.load()
    for name, (res, argtypes) in _lib.DRIFT_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == argtypes, name


def test_the_wrappers_enqueue_plain_work_outside_engine():
    """Engine's method list is closed (tests/test_rofl_abi_cpu.py): the wrappers are functions of fedmlp_amd/drift.py that go through
    the engine's stream check and count as plain work, never as a weight move"""
    import ast
    with open(os.path.join(ROOT, "fedmlp_amd", "drift.py")) as f:
        tree = ast.parse(f.read())
    fns = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    for name, fm in (("drift_begin", "fm_drift_begin"), ("drift_last", "fm_drift_last"), ("drift_end", "fm_drift_end")):
        calls = [n for n in ast.walk(fns[name]) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)]
        attrs = [c.func.attr for c in calls]
        assert "_check_stream" in attrs and fm in attrs, name
        enq = [c for c in calls if c.func.attr == "_enqueue"]
        assert len(enq) == 1 and not enq[0].args and not enq[0].keywords, name
    with open(os.path.join(ROOT, "fedmlp_amd", "engine.py")) as f:
        assert "fm_drift" not in f.read()


# ---- the rule ------------------------------------------------------------------------------------------------------------
def _rand(n, seed, dtype=np.float32):
    return np.random.RandomState(seed).standard_normal(n).astype(dtype)


def test_rule_is_the_identity_without_terms():
    g = _rand(1000, 1)
    g[:4] = [0.0, -0.0, np.float32(1e-45), -3.0]
    r = R.correct(g, p=_rand(1000, 2), a=_rand(1000, 3), mu=0.0, s=None)
    assert r.dtype == np.float32 and np.array_equal(r.view(np.int32), g.view(np.int32))
    assert r is not g


def test_rule_rounds_every_operation_on_its_own():
    """the fp32 rule differs from the same expression with a fused multiply-add (one rounding for mu * d + g) somewhere, and is
    what separate fp32 operations give everywhere"""
    g, p, a, s = _rand(4096, 4), _rand(4096, 5), _rand(4096, 6), _rand(4096, 7)
    mu = 0.1
    r = R.correct(g, p, a, mu, s)
    want = np.empty_like(g)
    for i in range(g.size):
        d = np.float32(p[i] - a[i])
        m = np.float32(np.float32(mu) * d)
        want[i] = np.float32(np.float32(g[i] + m) + s[i])
    assert np.array_equal(r, want)
    fused = (np.float64(np.float32(mu)) * (p - a).astype(np.float64) + g.astype(np.float64)).astype(np.float32) + s
    assert int((fused != r).sum()) > 0
    S = R.track(R.track(np.zeros_like(g), g), p)
    assert np.array_equal(S, (g + p).astype(np.float32)) and np.array_equal(R.mean(S, 2), S / np.float32(2))
    assert not R.mean(S, 0).any()


def test_mean_raw_gradient_is_option_ii_for_sgd():
    """float64, random data: K SGD steps y <- y - eta (g_k + c - c_i) from x; then c_i - c + (x - y) / (K eta) is the mean of the
    raw gradients g_k, whatever the shift"""
    rs = np.random.RandomState(11)
    n, K, eta = 257, 5, 0.05
    x = rs.standard_normal(n)
    c, c_i = rs.standard_normal(n), rs.standard_normal(n)
    y, S = x.copy(), np.zeros(n)
    for _ in range(K):
        g = rs.standard_normal(n) + 0.3 * y              # a gradient that depends on the iterate
        y = y - eta * R.correct(g, s=c - c_i)
        S = R.track(S, g)
    want = R.option_ii(c_i, c, x, y, K, eta)
    np.testing.assert_allclose(R.mean(S, K), want, rtol=0, atol=1e-12 * float(np.abs(S).max()) / eta)


# ---- Scaffold.server_update ------------------------------------------------------------------------------------------------
def test_server_update_by_hand():
    from fedmlp_amd.drift import Scaffold
    sc = Scaffold(3, 4, "cpu")
    assert sc.c_global.dtype == torch.float32 and not sc.c_global.any()
    d0, d1 = torch.tensor([1.0, 2.0, -4.0]), torch.tensor([3.0, -2.0, 0.5])
    out = sc.server_update([d0, d1])
    assert torch.equal(out, torch.tensor([1.0, 0.0, -0.875])) and out is sc.c_global        # (d0 + d1) / 4
    sc.deltas = [torch.tensor([4.0, 4.0, 4.0])]
    sc.server_update()                                                                        # the noted deltas, then forgotten
    assert torch.equal(sc.c_global, torch.tensor([2.0, 1.0, 0.125])) and sc.deltas == []
    sc.server_update()
    assert torch.equal(sc.c_global, torch.tensor([2.0, 1.0, 0.125]))
    # against the numpy bookkeeping, fp32 op for op
    ref = R.ScaffoldRef(5, 3)
    sc = Scaffold(5, 3, "cpu")
    for rnd in range(2):
        deltas_t, deltas_r = [], []
        for i in range(3):
            m = _rand(5, 20 + 3 * rnd + i)
            assert np.array_equal((sc.c_global - sc._local(i)).numpy(), ref.shift(i))
            new = torch.from_numpy(m)
            dt = new - sc._local(i)
            sc.c_local[i] = new
            deltas_t.append(dt)
            deltas_r.append(ref.end(i, m))
        assert np.array_equal(sc.server_update(deltas_t).numpy(), ref.server_update(deltas_r))


WORLD = 2


def _gloo_worker(rank, port, out_dir):
    from fedmlp_amd.drift import Scaffold
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=180))
    sc = Scaffold(6, 3, "cpu")                      # three clients: rank 0 trains clients 0 and 2, rank 1 client 1
    sc.c_global += 1.0
    mine = [c for c in range(3) if c % WORLD == rank]
    out = sc.server_update([torch.from_numpy(_rand(6, 40 + c)) for c in mine])
    np.save(os.path.join(out_dir, f"s{rank}.npy"), out.numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_server_update_world_2_gloo(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_gloo_worker, args=(port, str(tmp_path)), nprocs=WORLD, join=True)
    d = [_rand(6, 40 + c) for c in range(3)]
    want = np.ones(6, np.float32) + ((d[0] + d[2]) + d[1]) / np.float32(3)      # each rank's own sum, then the ranks' sum
    for r in range(WORLD):
        assert np.array_equal(np.load(os.path.join(str(tmp_path), f"s{r}.npy")), want)


# ---- the driver's flags ---------------------------------------------------------------------------------------------------
def test_driver_flags():
    from fedmlp_amd import driver, driver_rofl
    base = vars(driver.args_parser([]))
    assert base["prox_mu"] == 0.0 and base["scaffold"] == 0
    # the defaults leave every other field as it is without the flags
    explicit = vars(driver.args_parser(["--prox_mu", "0", "--scaffold", "0"]))
    assert explicit == base
    for exp in driver.DRIFT_EXPS:
        assert driver.args_parser(["--exp", exp, "--prox_mu", "0.01"]).prox_mu == 0.01
        assert driver.args_parser(["--exp", exp, "--scaffold", "1"]).scaffold == 1
    assert driver.DRIFT_EXPS == ("FedAVG", "FedAVG+FixMatch", "FedMLP")
    for exp in ("FedLSR", "FedIRM", "FedNoRo", "CBAFed"):
        assert driver.args_parser(["--exp", exp]).exp == exp                        # without the flags: as ever
        for flag in (["--prox_mu", "0.01"], ["--scaffold", "1"]):
            with pytest.raises(SystemExit):
                driver.args_parser(["--exp", exp] + flag)
    for bad in (["--prox_mu", "0.01", "--scaffold", "1"], ["--prox_mu", "-1"], ["--prox_mu", "nan"], ["--prox_mu", "inf"],
                ["--scaffold", "2"]):
        with pytest.raises(SystemExit):
            driver.args_parser(["--exp", "FedAVG"] + bad)
    with pytest.raises(SystemExit):
        driver_rofl.args_parser(["--scaffold", "1"])
    assert driver_rofl.args_parser([]).exp == "RoFL"


def test_refusal_names_the_three_rows(capsys):
    from fedmlp_amd import driver
    with pytest.raises(SystemExit):
        driver.args_parser(["--exp", "FedLSR", "--prox_mu", "0.01"])
    err = capsys.readouterr().err
    assert all(name in err for name in ("FedAVG", "FedAVG+FixMatch", "FedMLP"))


def test_local_update_has_no_drift_by_default():
    import ast
    with open(os.path.join(ROOT, "fedmlp_amd", "local_training.py")) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "LocalUpdate")
    fns = {fn.name: fn for fn in cls.body if isinstance(fn, ast.FunctionDef)}

    def calls(fn):
        return [n.func.attr for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)]
    assert calls(fns["train"]).count("_drift_begin") == 1 and calls(fns["train"]).count("_drift_end") == 1
    assert calls(fns["train_FixMatch"]).count("_drift_begin") == 1 and calls(fns["train_FixMatch"]).count("_drift_end") == 1
    assert calls(fns["train_FedMLP"]).count("_drift_begin") == 2 and calls(fns["train_FedMLP"]).count("_drift_end") == 2
    init = ast.unparse(fns["__init__"])
    assert "self.drift = None" in init
