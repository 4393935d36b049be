"""The host drop-ins of the RSCFed aggregation (fedmlp_amd.fedavg.Fed_w / model_dist / RSCFed) against the reference's own
utils/FedAvg.py:16-49, recorded in tests/golden/rscfed_kat.json by tests/golden/make_rscfed_golden.py: Fed_w and RSCFed
bit for bit on every entry (the float-valued num_batches_tracked included), model_dist to rtol 1e-6 (torch.norm's own
summation order may differ between CPUs).  Plus the C ABI's declarations."""
import importlib.util
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from fedmlp_amd.fedavg import Fed_w, RSCFed, model_dist
from tests.helpers import GOLDEN, load_golden


@pytest.fixture(scope="module")
def kat():
    return load_golden("rscfed_kat.json")


@pytest.fixture(scope="module")
def w_locals(kat):
    spec = importlib.util.spec_from_file_location("make_rscfed_golden", os.path.join(GOLDEN, "make_rscfed_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert {k: list(v) for k, v in mod.SHAPES.items()} == kat["shapes"]
    return [OrderedDict((k, torch.from_numpy(np.asarray(v))) for k, v in mod.client_state(s).items()) for s in kat["seeds"]]


def _assert_same(got, want, dtypes=None):
    assert list(got.keys()) == list(want.keys())
    for k, v in want.items():
        g = got[k].numpy()
        assert g.dtype == np.float32, (k, g.dtype)
        if dtypes is not None:
            assert str(got[k].dtype) == dtypes[k]
        np.testing.assert_array_equal(g.reshape(-1), np.array(v, dtype=np.float32), err_msg=k)


def test_fixture_has_the_cases_it_is_for(kat, w_locals):
    assert kat["K"] == 3 and kat["M"] == 4 and 1 in kat["dict_len"] and len(set(kat["dict_len"])) > 4
    sd = w_locals[0]
    assert len(sd) == 4 and any(v.numel() % 2 == 1 and v.numel() > 1000 for v in sd.values())
    assert sum(v.dtype == torch.int64 for v in sd.values()) == 1


def test_fed_w_reproduces_the_reference_bit_for_bit(kat, w_locals):
    """Non-integer double weights (the first group's a*b): float entries and the counter, which is fp32 from the first product."""
    g = kat["groups"][0]
    got = Fed_w([w_locals[i] for i in g["ids"]], g["weight"])
    _assert_same(got, kat["fed_w_group0"])
    assert float(got["bn.num_batches_tracked"]) != int(float(got["bn.num_batches_tracked"]))     # a float counter, e.g. 13.19


def test_model_dist_matches_the_reference(kat, w_locals):
    for g in kat["groups"]:
        w_avg = Fed_w([w_locals[i] for i in g["ids"]], [1] * kat["K"])
        assert w_avg["bn.num_batches_tracked"].dtype == torch.float32
        for i, want in zip(g["ids"], g["dist"]):
            np.testing.assert_allclose(model_dist(w_locals[i], w_avg), want, rtol=1e-6)


def test_rscfed_reproduces_the_reference_bit_for_bit(kat, w_locals):
    got = RSCFed(kat["DMA"], w_locals, kat["K"], kat["dict_len"], kat["M"])
    _assert_same(got, kat["out"], kat["out_dtype"])


def test_fed_w_divides_by_the_rounded_double_sum():
    """Weights whose fp32 roundings sum to another fp32 than their double sum: the divisor is float32(sum(weight)), not the
    sum of the rounded weights fm_fedavg_fold forms."""
    wts = [0.2604923103919594, 0.8050278270130223, 0.5486993038355893, 0.014041700164018955]
    d_double = np.float32(sum(wts))
    d_rounded = np.float32(sum(float(np.float32(x)) for x in wts))
    assert d_double != d_rounded                                             # the case is really exercised
    rs = np.random.RandomState(3)
    vs = [rs.standard_normal(257).astype(np.float32) for _ in wts]
    got = Fed_w([{"v": torch.from_numpy(v)} for v in vs], wts)["v"].numpy()
    acc = vs[0] * np.float32(wts[0])
    for v, x in zip(vs[1:], wts[1:]):
        acc = acc + v * np.float32(x)
    np.testing.assert_array_equal(got, acc / d_double)
    assert (got != acc / d_rounded).any()
    ref = torch.from_numpy(vs[0]) * wts[0]                                   # torch itself, the reference's expression
    for v, x in zip(vs[1:], wts[1:]):
        ref += torch.from_numpy(v) * x
    np.testing.assert_array_equal(got, (ref / sum(wts)).numpy())


def test_row_sums_are_the_left_to_right_fp32_chain():
    """rscfed_device sums a group's rows of terms at once: the same bits as model_dist's one-by-one accumulation."""
    from fedmlp_amd.fedavg import _dist_rows, _dist_sum
    rs = np.random.RandomState(9)
    t = (rs.standard_normal((6, 122)) ** 2 * rs.choice([1e-3, 1.0, 30.0], size=(6, 122))).astype(np.float32)
    assert _dist_rows(t) == [_dist_sum(r) for r in t]
    assert _dist_rows(t) != [float(np.float32(r.astype(np.float64).sum())) for r in t]      # not a wider or pairwise sum


def test_cabi_declares_the_aggregation():
    from fedmlp_amd import _lib
    assert len(_lib.SYMBOLS["fm_fed_w"][1]) == 5 and len(_lib.SYMBOLS["fm_state_dist"][1]) == 6
