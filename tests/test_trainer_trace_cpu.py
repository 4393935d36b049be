"""LocalUpdate's trainers against a recorded trace, without a GPU: what each train_* asks of the engine and in which order, what it
draws from the global RNGs, what it returns and what it leaves on the client.

A LocalUpdate subclass binds a recording stand-in for the engine (device "cpu"): every method call is noted with its scalars and
the shape and a checksum of each tensor; the stand-in answers with deterministic tensors of the right shapes.  The dataset's
device_batch draws from torch's global RNG, so a fetch moved to another place changes the data of every later one.  Every branch of
every trainer runs under fixed torch / numpy / random seeds and is compared, exactly, with tests/golden/trainer_traces.json.

The fixture was recorded with this module's recorder from the local_training.py of the commit BEFORE the epoch loop, the teacher
slot and the return head were stated once (`python tests/test_trainer_trace_cpu.py OUT.json`, with that commit's tree on
PYTHONPATH), so it pins the refactored file to the behaviour of the eleven hand-written loops it replaced."""
import hashlib
import json
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "trainer_traces.json")
N, C, D, BS, EP = 7, 4, 6, 3, 2


def _sum(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _enc(v):
    """JSON form: tensors and arrays by value, with their type"""
    if isinstance(v, torch.Tensor):
        return {"tensor": str(v.dtype), "shape": list(v.shape), "v": v.detach().double().flatten().tolist()}
    if isinstance(v, np.ndarray):
        return {"array": str(v.dtype), "shape": list(v.shape), "v": v.astype(np.float64).flatten().tolist()}
    if isinstance(v, (np.floating, np.integer)):
        return {"scalar": type(v).__name__, "v": float(v)}
    if isinstance(v, dict):
        return {str(k): _enc(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_enc(x) for x in v]
    return v


def _arg(v):
    """trace form: scalars as they are, tensors and arrays as (shape, checksum)"""
    if isinstance(v, torch.Tensor):
        return ["tensor", str(v.dtype), list(v.shape), _sum(v.detach().contiguous().numpy())]
    if isinstance(v, np.ndarray):
        return ["array", str(v.dtype), list(v.shape), _sum(v)]
    if isinstance(v, (np.floating, np.integer)):
        return float(v)
    if isinstance(v, (list, tuple)):
        return [_arg(x) for x in v]
    return v


class RecordingEngine:
    """every Engine method LocalUpdate calls, recorded; answers depend only on the arguments and on how many calls came before"""
    device = "cpu"
    feature_dim = D
    n_classes = C

    def __init__(self, trace):
        self.trace = trace

    def _val(self):
        return 0.125 * (len(self.trace) % 17 + 1)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*a, **k):
            self.trace.append([name, [_arg(x) for x in a], {kk: _arg(x) for kk, x in sorted(k.items())}])
            answer = getattr(type(self), "_" + name, None)
            return answer(self, *a, **k) if answer else None
        return call

    def _step(self, *a):
        a[-1].fill_(self._val())
    _step_bce = _step_stage1 = _step_stage2 = _step_fixmatch = _step_fedlsr = _step_rscfed = _step_fednoro = _step_cbafed = _step

    def _forward_train(self, x1, x2=None):
        rows = x1.shape[0] * (1 if x2 is None else 2)
        x = x1 if x2 is None else torch.cat([x1, x2])
        f = x.reshape(rows, -1)
        return f[:, :D] * self._val(), f[:, D:D + C] - self._val()

    def _forward_eval(self, x, teacher=False):
        f = x.reshape(x.shape[0], -1)
        return f[:, :D] - 0.5, f[:, D:D + C] - 0.5

    def _loss(self, z, *a):
        rel = a[-1]
        if isinstance(rel, torch.Tensor) and tuple(rel.shape) == (C, C):
            rel += torch.arange(C * C, dtype=torch.float32).reshape(C, C) * self._val()
        return z * 0.5, torch.full((1,), self._val())
    _loss_fedirm_sup = _loss_fedirm_rel = _loss

    def _get_state(self):
        return np.full(5, self._val(), np.float32), np.full(2, len(self.trace), np.int64)

    def _proto_finalize(self, zero_guard, n_local, active_mask):
        return np.full(C, self._val(), np.float64), np.full((2 * C, D), self._val(), np.float32) * np.arange(1, D + 1, dtype=np.float32)

    def _cos_tag(self, feat, proto, classes):
        return torch.stack([feat[:, c % D] - feat.mean(dim=1) for c in classes])

    def _select_topk_rows(self, sims, pools, clean_thr, noise_thr):
        out = []
        for k in range(sims.shape[0]):
            s = sims[k].numpy() if pools[k] is None else sims[k].numpy()[list(pools[k])]
            order = np.argsort(-s, kind="stable")
            kt, kb = int(clean_thr * (s >= 0).sum()), int(noise_thr * (s < 0).sum())
            out.append((order[:kt].tolist(), order[::-1][:kb].tolist()))
        return out


def _net_class():
    from fedmlp_amd.model import HipNet

    class Net(HipNet):
        """the part of HipNet LocalUpdate touches"""
        def __init__(self, trace, tag):
            self.trace, self.tag = trace, tag
            self.flat, self.counters, self._version = np.arange(5, dtype=np.float32), np.zeros(2, np.int64), 0

        def mark_trained(self):
            self.trace.append([self.tag + ".mark_trained", [], {}])

        def _pull(self):
            self.trace.append([self.tag + "._pull", [], {}])

        def state_dict(self):
            return {"w": torch.arange(3.0) + len(self.trace)}
    return Net


class Dataset:
    def __init__(self):
        g = torch.Generator().manual_seed(5)
        self.base = {k: torch.randn((N + 3, 3, 4, 4), generator=g) for k in ("image", "image_aug_1", "image_aug_2")}
        y = (torch.rand((N + 3, C), generator=g) < 0.5).float()
        y[:C] = torch.eye(C)                                   # every class has a positive among the local samples
        self.targets = y.numpy()

    def device_batch(self, eng, key, ds_idx):
        """a fresh augmentation draw per fetch, from the global RNG"""
        return self.base[key][list(ds_idx)] + 0.1 * torch.rand((len(ds_idx), 3, 4, 4))


def _args():
    return types.SimpleNamespace(n_classes=C, batch_size=BS, local_ep=EP, base_lr=3e-5, annotation_num=2, t_w=5,
                                 rounds_FedIRM_sup=2, rounds_FedNoRo_warmup=2, rounds_CBAFed_warmup=2, rounds_FedMLP_stage1=2,
                                 consistency=1.0, consistency_rampup=30, ema_decay=0.99, L=0.3, U=0.7, clean_threshold=0.5,
                                 noise_threshold=0.5)


def _client():
    from fedmlp_amd.local_training import LocalUpdate

    trace = []

    class Traced(LocalUpdate):
        def _bind(self, net, key):
            trace.append(["_bind", [key], {}])
            return RecordingEngine(trace)

    Net = _net_class()
    neg_idx = {c: [c, c + 1, 8] for c in range(C)}
    lu = Traced(_args(), 1, Dataset(), list(range(N)), None, neg_idx, active_class_list=[1, 3], teacher_neg=Net(trace, "teacher"))
    return lu, Net(trace, "net"), trace


def _rng_hash():
    st = np.random.get_state()
    return [_sum(torch.get_rng_state().numpy()), _sum(st[1]) + ":" + str(st[2])]


def _run(lu, trace, seed, fn):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    del trace[:]
    try:
        ret = _enc(fn())
    except NotImplementedError as ex:
        ret = {"raises": "NotImplementedError", "text": str(ex)}
    fields = {k: _enc(getattr(lu, k)) for k in ("iter_num", "epoch", "loss_w", "class_num_list", "traindata_idx", "idxss", "flag")}
    return {"trace": json.loads(json.dumps(trace)), "return": ret, "fields": fields, "rng": _rng_hash()}


def record():
    """every branch of every trainer -> {case: {trace, return, fields, rng}}; the cases of one list share a client, in order"""
    target = np.arange(C * C, dtype=np.float32).reshape(C, C) / 10.0
    proto = np.linspace(-1.0, 1.0, 2 * C * D, dtype=np.float32).reshape(2 * C, D)
    neg, act = [0, 2], [1, 3]
    groups = [
        [("train", lambda lu, net: lu.train(0, net))],
        [("fixmatch", lambda lu, net: lu.train_FixMatch(0, net))],
        [("fedlsr_ramp", lambda lu, net: lu.train_FedLSR(2, net)), ("fedlsr_full", lambda lu, net: lu.train_FedLSR(5, net))],
        [("rscfed", lambda lu, net: lu.train_RSCFed(0, net))],
        [("fednoro_warm", lambda lu, net: lu.train_FedNoRo(1, 0, net, weight_kd=0.8)),
         ("fednoro_after", lambda lu, net: lu.train_FedNoRo(1, 2, net, weight_kd=0.8))],
        [("cbafed_warm", lambda lu, net: lu.train_CBAFed(0, net)),
         ("cbafed_stage2", lambda lu, net: lu.train_CBAFed(2, net, tao=[0.5, 0.6, 0.7, 0.8]))],
        [("fedirm_sup", lambda lu, net: lu.train_FedIRM(0, target, None, neg, act, net)),
         ("fedirm_sup_last", lambda lu, net: lu.train_FedIRM(1, target, None, neg, act, net)),
         ("fedirm_rel_first", lambda lu, net: lu.train_FedIRM(2, target, None, neg, act, net)),
         ("fedirm_rel_second", lambda lu, net: lu.train_FedIRM(3, target, None, neg, act, net))],
        [("fedmlp_stage1", lambda lu, net: lu.train_FedMLP(0, None, None, None, neg, act, net)),
         ("fedmlp_stage1_last", lambda lu, net: lu.train_FedMLP(1, None, None, None, neg, act, net)),
         ("fedmlp_stage2_first", lambda lu, net: lu.train_FedMLP(2, None, proto, None, neg, act, net)),
         ("fedmlp_stage2_later", lambda lu, net: lu.train_FedMLP(3, None, proto, None, neg, act, net))],
    ]
    out = {}
    for group in groups:
        random.seed(11)
        lu, net, trace = _client()
        for i, (name, fn) in enumerate(group):
            out[name] = _run(lu, trace, 100 + i, lambda: fn(lu, net))
    return out


def test_every_trainer_branch_matches_the_recorded_trace():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = json.loads(json.dumps(record()))
    assert sorted(got) == sorted(want) and len(want) == 17
    for case in want:
        for part in ("trace", "return", "fields", "rng"):
            if part == "trace":
                assert len(got[case][part]) == len(want[case][part]), (case, len(got[case][part]), len(want[case][part]))
                for i, (g, w) in enumerate(zip(got[case][part], want[case][part])):
                    assert g == w, f"{case}: call {i} is {g}, recorded {w}"
            assert got[case][part] == want[case][part], (case, part)
    # the trace has teeth: both views are fetched, the relation matrix accumulates, the teacher slot is used on both paths
    calls = lambda case: [c[0] for c in want[case]["trace"]]    # noqa: E731
    assert calls("fedirm_rel_first").count("teacher_snapshot") == 1 and calls("fedirm_rel_second").count("set_state") == 1
    assert calls("rscfed").count("teacher_swap") == 4 and want["fedirm_sup"]["fields"]["iter_num"] == 0
    assert want["fedirm_rel_first"]["fields"]["iter_num"] == EP * 3 and want["fednoro_after"]["return"]["raises"]


if __name__ == "__main__":
    sys.path.append(ROOT)                                      # behind PYTHONPATH: the tree whose trainers are recorded
    with open(sys.argv[1], "w") as f:
        json.dump(record(), f, separators=(",", ":"))
