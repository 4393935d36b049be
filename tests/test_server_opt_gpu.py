"""Server optimizers on a real MI355X (include/fedmlp_hip_server.h, fedmlp_amd/csrc/server_opt.hip, fedmlp_amd/server_opt.py): the one
launch of fm_server_opt_step against tests/server_opt_ref.py, element for element, over the engines' full states at the smallest
engines the models allow (32 x 32 input, batch 2): ResNet-18 and EfficientNet-B0 with 5 classes (fc.bias, 5 floats, and fc.weight
sit at odd element offsets) and ResNet-18 with 14.

A round is played the way the driver plays it: the engine holds x_k, `old` is a clone of its device state, the aggregate
a_k = x_k + p_k is loaded with fm_set_state, the step turns it into x_{k+1}.  p_k mixes exact zeros, both signs and magnitudes from
1e-6 to 1, so that d*d lies above tau^2 = 1e-6 on one stretch and below it on another and no intermediate is subnormal.
Everything is compared in state_dict order (fm_get_state's floats, the moments in net.grads() layout)."""
import ctypes as C

import numpy as np
import pytest
import torch

from fedmlp_amd import _lib, server_opt, spec
from fedmlp_amd.engine import Engine
from tests import server_opt_ref as R

pytestmark = pytest.mark.gpu

HW, B = 32, 2
CONFIGS = [("Resnet18", 5), ("Efficient_b0", 5), ("Resnet18", 14)]
IDS = [f"{m}-C{c}" for m, c in CONFIGS]
HP = {"avgm": dict(lr=1.0, beta1=0.9), "adagrad": dict(lr=1e-2, beta1=0.9, tau=1e-3),
      "adam": dict(lr=1e-2, beta1=0.9, beta2=0.99, tau=1e-3), "yogi": dict(lr=1e-2, beta1=0.9, beta2=0.99, tau=1e-3)}
F = np.float32


# ---- engines and data, made once ---------------------------------------------------------------------------------------------
class _Engines:
    def __init__(self):
        self.engines = {}

    def get(self, model, n_classes, slot=0, precision="fp32", streams=0):
        key = (model, n_classes, slot, precision, streams)
        eng = self.engines.get(key)
        if eng is None:
            eng = self.engines[key] = Engine(model, n_classes, HW, HW, B, precision=precision, streams=streams)
            eng.stochastic = False
        if server_opt.server_active(eng):
            server_opt.server_end(eng)
        return eng

    def close(self):
        for eng in self.engines.values():
            eng.close()
        self.engines.clear()


@pytest.fixture(scope="module")
def engines():
    e = _Engines()
    yield e
    e.close()


_DATA = {}


def _trainable(model, n_classes):
    m, off = np.zeros(spec.sizes(model, n_classes)[0], bool), 0
    for k, shape, dt in spec.entries(model, n_classes):
        if dt != "f32":
            continue
        n = int(np.prod(shape))
        m[off:off + n] = spec.is_trainable(k)
        off += n
    return m


def _data(model, n_classes):
    """x0 (the model's initial state), its counters, the trainable mask and three perturbations p_k, shared and never written"""
    key = (model, n_classes)
    if key not in _DATA:
        x0, cnt = spec.init_state(model, n_classes, 1037)
        rs = np.random.RandomState(77)
        ps = []
        for _ in range(3):
            p = (10.0 ** rs.uniform(-6, 0, x0.size)).astype(F)
            p *= rs.choice(np.array([-1.0, 1.0], F), x0.size)
            p[rs.randint(0, 8, x0.size) == 0] = 0                 # exact zeros: d == 0 there
            ps.append(p)
        for a in [x0] + ps:
            a.setflags(write=False)
        _DATA[key] = (x0, cnt, _trainable(model, n_classes), ps)
    return _DATA[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _begin(eng, rule):
    hp = HP[rule]
    server_opt.server_begin(eng, rule, hp["lr"], hp["beta1"], hp.get("beta2", 0.0), hp.get("tau", 0.0))


def _round(eng, a, cnt, norm=True):
    """one round as the driver plays it: old = the engine's state, the aggregate loaded, the step -> (old, its copy, the norm)"""
    old = eng.state_tensor().clone()
    keep = old.clone()
    eng.set_state(a, cnt)
    return old, keep, server_opt.server_step(eng, old, norm=norm)


# ---- bits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", R.RULES)
@pytest.mark.parametrize("model,n_classes", CONFIGS, ids=IDS)
def test_three_steps_bit_for_bit(engines, model, n_classes, rule):
    x0, cnt0, tr, ps = _data(model, n_classes)
    eng = engines.get(model, n_classes)
    eng.set_state(x0, cnt0)
    _begin(eng, rule)
    assert server_opt.server_active(eng)
    hp = HP[rule]
    x = np.array(x0)
    m, v = R.init(rule, int(tr.sum()), hp.get("tau", 0.0))
    for k in range(3):
        a = (x + ps[k]).astype(F)
        cnt = cnt0 + 3 * (k + 1)
        old, keep, _ = _round(eng, a, cnt)
        got, got_cnt = eng.get_state()
        steps, gm, gv = server_opt.server_get_state(eng)
        want, m, v = R.step(rule, x[tr], a[tr], m, v, **hp)
        bad = int((_bits(got[tr]) != _bits(want)).sum())
        assert bad == 0, f"step {k}: {bad} of {want.size} parameters differ from the reference rule"
        assert np.array_equal(_bits(got[~tr]), _bits(a[~tr])), "a running statistic is not the aggregate's"
        assert np.array_equal(got_cnt, cnt), "the counters moved"
        assert torch.equal(old.view(torch.int32), keep.view(torch.int32)), "x_old was written"
        gm, gv = gm.cpu().numpy(), gv.cpu().numpy()
        assert steps == k + 1
        assert np.array_equal(_bits(gm[tr]), _bits(m)) and not gm[~tr].any(), "first moment"
        if rule == "avgm":
            assert not gv.any()
        else:
            assert np.array_equal(_bits(gv[tr]), _bits(v)) and not gv[~tr].any(), "second moment"
        assert int((got[tr] != x[tr]).sum()) > 0.3 * want.size, "the step left the model where the round started"
        x = got
    server_opt.server_end(eng)
    assert not server_opt.server_active(eng)


@pytest.mark.parametrize("rule", ["avgm", "yogi"])
def test_x_old_off_a_16_byte_boundary(engines, rule):
    """x_old_dev one float into a buffer: the kernel reads it lane by lane, and the step and its norm carry the aligned call's bits"""
    model, n_classes = "Efficient_b0", 5
    x0, cnt0, tr, ps = _data(model, n_classes)
    eng = engines.get(model, n_classes)
    a = (x0 + ps[0]).astype(F)
    res = []
    for shift in (0, 1):
        eng.set_state(x0, cnt0)
        _begin(eng, rule)
        st = eng.state_tensor()
        buf = torch.full((st.numel() + 4,), float("nan"), device="cuda")
        old = buf[shift:shift + st.numel()]
        old.copy_(st)
        assert old.data_ptr() % 16 == 4 * shift
        eng.set_state(a, cnt0)
        norm = server_opt.server_step(eng, old)
        steps, m, v = server_opt.server_get_state(eng)
        res.append((eng.state_tensor().clone(), m, v, norm.cpu().numpy().tobytes()))
        server_opt.server_end(eng)
    (w0, m0, v0, n0), (w1, m1, v1, n1) = res
    for g, w in ((w1, w0), (m1, m0), (v1, v0)):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    assert n0 == n1 and bool(torch.isfinite(w1).all())
    want, _, _ = R.step(rule, x0[tr], a[tr], *R.init(rule, int(tr.sum()), HP[rule].get("tau", 0.0)), **HP[rule])
    assert np.array_equal(_bits(eng.get_state()[0][tr]), _bits(want))


# ---- padding -----------------------------------------------------------------------------------------------------------------
def _real_slots(eng, model, n_classes, which):
    """bool over the engine layout: the slots fm_set_state fills from the given state_dict positions (loaded as ones into a state
    of zeros: everything else -- padding inside the matrices, gaps between the entries -- stays zero)"""
    nf, ni = spec.sizes(model, n_classes)
    eng.state_tensor().zero_()
    eng.set_state(which.astype(F), np.zeros(ni, np.int64))
    return eng.state_tensor() != 0


@pytest.mark.parametrize("model,n_classes", CONFIGS, ids=IDS)
def test_padding_stays_zero(engines, model, n_classes):
    x0, cnt0, tr, ps = _data(model, n_classes)
    eng = engines.get(model, n_classes)
    entry = _real_slots(eng, model, n_classes, np.ones(x0.size, bool))
    eng.set_state(x0, cnt0)
    _begin(eng, "yogi")
    x = np.array(x0)
    for k in range(3):
        _round(eng, (x + ps[k]).astype(F), cnt0, norm=False)
        x = eng.get_state()[0]
    st = eng.state_tensor()
    assert int(entry.sum()) == x0.size and not st[~entry].any(), "a non-entry slot of the state is not an exact zero"
    assert bool(torch.isfinite(st).all())
    server_opt.server_end(eng)


# ---- the norm ----------------------------------------------------------------------------------------------------------------
def _norm_want(x, a, tr):
    """the float64 norm of the fp32 differences over the trainable entries, summed in extended precision -> (norm, n)"""
    d = (a[tr] - x[tr]).astype(np.longdouble)
    return float(np.sqrt(np.sum(d * d))), int(tr.sum())


@pytest.mark.parametrize("model,n_classes", CONFIGS, ids=IDS)
def test_delta_norm(engines, model, n_classes):
    """|d|_2 within n 2^-53 (the fp64 sum of n squares, whatever its order: agg.hip's bound) + 2^-53 (the square root's rounding),
    relative; the same operands give the same 8 bytes; AVGM's launch gives the adaptive ones' norm"""
    x0, cnt0, tr, ps = _data(model, n_classes)
    eng = engines.get(model, n_classes)
    a = (x0 + ps[0]).astype(F)
    want, n = _norm_want(x0, a, tr)
    seen = []
    for rule in ("adam", "adam", "avgm"):
        eng.set_state(x0, cnt0)
        _begin(eng, rule)
        _, _, norm = _round(eng, a, cnt0)
        server_opt.server_end(eng)
        assert norm.dtype == torch.float64 and norm.dim() == 0
        seen.append(norm.cpu().numpy().tobytes())
    got = float(np.frombuffer(seen[0], np.float64)[0])
    bound = n * 2.0 ** -53 + 2.0 ** -53
    print(f"\n[server_opt] {model} C={n_classes}: |d| {got:.17g}, relative error {abs(got - want) / want:.3e}, bound {bound:.3e}")
    assert want > 0 and abs(got - want) <= bound * want
    assert seen[0] == seen[1] == seen[2]


@pytest.mark.parametrize("model,n_classes", CONFIGS[:2], ids=IDS[:2])
def test_delta_norm_ignores_non_entry_slots(model, n_classes):
    """a large finite value planted in non-entry slots of the aggregate (padding inside a matrix, a gap between entries: whichever
    the layout has inside the parameter arena) does not move the norm.  An engine of its own: no forward follows."""
    x0, cnt0, tr, ps = _data(model, n_classes)
    eng = Engine(model, n_classes, HW, HW, B)
    try:
        entry = _real_slots(eng, model, n_classes, np.ones(x0.size, bool))
        spans = eng.debug_entry_spans()
        spans = spans[spans[:, 0] >= 0]
        np_end = int((spans[:, 0] + spans[:, 1]).max())          # the parameter entries end here
        in_span = torch.zeros_like(entry)
        for off, ln in spans:
            in_span[off:off + ln] = True
        free = (~entry[:np_end]).nonzero().flatten()
        pad = free[in_span[free]][:3].tolist()
        gap = free[~in_span[free]][:3].tolist()
        if model == "Efficient_b0":
            assert pad, "EfficientNet-B0's padded channels are gone: this test needs another non-entry slot"
        a = (x0 + ps[1]).astype(F)
        norms = []
        for plant in (False, True):
            eng.set_state(x0, cnt0)
            _begin(eng, "adagrad")
            old = eng.state_tensor().clone()
            eng.set_state(a, cnt0)
            if plant:
                st = eng.state_tensor()
                for i in pad + gap:
                    st[i] = 1e30
            norms.append(server_opt.server_step(eng, old).cpu().numpy().tobytes())
            server_opt.server_end(eng)
        print(f"\n[server_opt] {model}: planted {len(pad)} padding and {len(gap)} gap slots")
        assert pad or gap, "this layout has no non-entry slot inside the parameter arena: the test checks nothing"
        assert norms[0] == norms[1], "a non-entry slot entered the norm"
    finally:
        eng.close()


# ---- coherence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [0, 1])
@pytest.mark.parametrize("model,precision", [("Resnet18", "fp32"), ("Efficient_b0", "fp32"), ("Efficient_b0", "bf16")])
def test_forward_after_the_step_sees_the_new_weights(engines, model, precision, streams):
    """Every copy the engine derives from the weights is built for the aggregate (an eval forward), then the step moves the weights:
    the next eval forward must equal, bit for bit, that of a fresh engine handed the stepped state through fm_set_state."""
    n_classes = 5
    x0, cnt0, tr, ps = _data(model, n_classes)
    eng = engines.get(model, n_classes, precision=precision, streams=streams)
    xb = torch.randn((B, 3, HW, HW), generator=torch.Generator().manual_seed(5)).cuda()
    eng.set_state(x0, cnt0)
    _begin(eng, "yogi")
    old = eng.state_tensor().clone()
    eng.set_state((x0 + ps[0]).astype(F), cnt0)
    before = [t.clone() for t in eng.forward_eval(xb)]
    server_opt.server_step(eng, old)
    after = [t.clone() for t in eng.forward_eval(xb)]
    stepped = eng.get_state()
    server_opt.server_end(eng)
    twin = Engine(model, n_classes, HW, HW, B, precision=precision, streams=streams)
    try:
        twin.stochastic = False
        twin.set_state(*stepped)
        want = [t.clone() for t in twin.forward_eval(xb)]
    finally:
        twin.close()
    for g, w, b in zip(after, want, before):
        assert bool(torch.isfinite(g).all())
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), "the forward after the step read a stale copy of the weights"
        assert not torch.equal(g, b), "the step did not move the forward's output"


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(engines):
    """Every FM_ERR_ARG of the header, with nothing enqueued and nothing moved: the state, and while an optimizer is installed (the
    moments cannot be read otherwise) both moments and the step count, carry the same bits afterwards."""
    model, n_classes = "Resnet18", 5
    x0, cnt0, tr, ps = _data(model, n_classes)
    eng = engines.get(model, n_classes)
    eng.set_state(x0, cnt0)
    lib, h = eng.lib, eng.h
    buf = torch.zeros(eng.nf, device="cuda")
    ptr = C.c_void_p(buf.data_ptr())
    steps_out = C.c_int64()

    def snap():
        s = {"w": eng.state_tensor().clone(), "cnt": eng.counters().copy(), "active": server_opt.server_active(eng)}
        if s["active"]:
            s["steps"], s["m"], s["v"] = server_opt.server_get_state(eng)
        return s

    def refused(fn, *args, text):
        before = snap()
        rc = fn(h, *args)
        msg = lib.fm_last_error().decode()
        assert rc == -1 and text in msg, (rc, msg)              # FM_ERR_ARG
        with pytest.raises(_lib.FmError):
            _lib.check(rc)
        eng.sync()
        after = snap()
        assert after["active"] == before["active"] and np.array_equal(after["cnt"], before["cnt"])
        assert torch.equal(after["w"].view(torch.int32), before["w"].view(torch.int32))
        if before["active"]:
            assert after["steps"] == before["steps"]
            for k in ("m", "v"):
                assert torch.equal(after[k].view(torch.int32), before[k].view(torch.int32)), k

    def hp(rule=2, lr=1e-2, beta1=0.9, beta2=0.99, tau=1e-3):
        return C.byref(_lib.FmServerOpt(rule, lr, beta1, beta2, tau))

    old = eng.state_tensor().clone()
    oldp = C.c_void_p(old.data_ptr())
    nothing = "no server optimizer is installed"
    refused(lib.fm_server_opt_step, oldp, None, text=nothing)
    refused(lib.fm_server_opt_get_state, ptr, ptr, C.byref(steps_out), text=nothing)
    refused(lib.fm_server_opt_set_state, ptr, ptr, 1, text=nothing)
    refused(lib.fm_server_opt_end, text=nothing)
    for rule in (-1, 4):
        refused(lib.fm_server_opt_begin, hp(rule=rule), text="unknown rule")
    for lr in (-0.1, float("nan"), float("inf")):
        refused(lib.fm_server_opt_begin, hp(lr=lr), text="lr must be finite and >= 0")
    for rule in range(4):
        for b in (1.0, -0.1, float("nan")):
            refused(lib.fm_server_opt_begin, hp(rule=rule, beta1=b), text="beta1 must lie in [0, 1)")
    for rule in (2, 3):
        for b in (1.0, -0.1, float("nan")):
            refused(lib.fm_server_opt_begin, hp(rule=rule, beta2=b), text="beta2 must lie in [0, 1)")
    for rule in (1, 2, 3):
        for tau in (0.0, -1e-3, float("inf"), float("nan")):
            refused(lib.fm_server_opt_begin, hp(rule=rule, tau=tau), text="tau must be finite and > 0")
    assert not server_opt.server_active(eng)
    # what a rule does not read is not checked
    _lib.check(lib.fm_server_opt_begin(h, hp(rule=0, beta2=5.0, tau=-1.0)))
    server_opt.server_end(eng)
    _lib.check(lib.fm_server_opt_begin(h, hp(rule=1, beta2=5.0)))
    server_opt.server_end(eng)
    # installed, one step behind it: non-zero moments
    _begin(eng, "adam")
    _round(eng, (x0 + ps[0]).astype(F), cnt0)
    refused(lib.fm_server_opt_begin, hp(), text="already installed")
    refused(lib.fm_server_opt_step, None, None, text="null x_old_dev")
    own = eng.state_tensor()
    for p in (own.data_ptr(), own.data_ptr() + 4 * (own.numel() - 1), own.data_ptr() - 4 * (own.numel() - 1)):
        refused(lib.fm_server_opt_step, C.c_void_p(p), None, text="engine's own state buffer")
    refused(lib.fm_server_opt_set_state, None, ptr, 1, text="null moment")
    refused(lib.fm_server_opt_set_state, ptr, None, 1, text="null moment")
    refused(lib.fm_server_opt_set_state, ptr, ptr, -1, text="steps must be >= 0")
    with pytest.raises(ValueError):
        server_opt.server_step(eng, old[:-4])
    with pytest.raises(ValueError):
        server_opt.server_step(eng, old.cpu())
    # fm_set_state, the optimizer resets and the drift correction leave the install alone
    from fedmlp_amd.drift import drift_begin, drift_end
    before = snap()
    eng.adam_reset(1e-3)
    eng.sgd_reset()
    drift_begin(eng, mu=0.1)
    drift_end(eng, mean=False)
    eng.set_state(*eng.get_state())
    after = snap()
    assert after["active"] and after["steps"] == before["steps"] == 1
    assert torch.equal(after["m"], before["m"]) and torch.equal(after["v"], before["v"]) and bool(before["m"].any())
    server_opt.server_end(eng)


# ---- resume ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["avgm", "yogi"])
def test_resume(engines, rule):
    """two steps, the optimizer's state_dict(); a second engine installs it (begin + fm_server_opt_set_state); the third step gives
    the same bits on both"""
    model, n_classes = "Efficient_b0", 5
    x0, cnt0, tr, ps = _data(model, n_classes)
    e1, e2 = engines.get(model, n_classes), engines.get(model, n_classes, slot=1)
    opt1 = server_opt.make(rule, **HP[rule])
    e1.set_state(x0, cnt0)
    opt1.begin(e1)
    x = np.array(x0)
    for k in range(2):
        old = e1.state_tensor().clone()
        e1.set_state((x + ps[k]).astype(F), cnt0)
        opt1.step(e1, old)
        x = e1.get_state()[0]
    sd = opt1.state_dict()
    assert sd["step"] == 2 and sd["hyper"]["rule"] == rule and bool(sd["m"].any())
    opt2 = server_opt.CLASSES[rule]()
    opt2.load_state_dict({k: (t.cpu() if torch.is_tensor(t) else t) for k, t in sd.items()})
    e2.set_state(x, cnt0)
    opt2.begin(e2)
    a = (x + ps[2]).astype(F)
    res = []
    for eng, opt in ((e1, opt1), (e2, opt2)):
        eng.set_state(x, cnt0)
        old = eng.state_tensor().clone()
        eng.set_state(a, cnt0)
        norm = opt.step(eng, old)
        res.append((eng.state_tensor().clone(), opt.state_dict(), norm.cpu().numpy().tobytes()))
    (w1, s1, n1), (w2, s2, n2) = res
    assert torch.equal(w1.view(torch.int32), w2.view(torch.int32)) and n1 == n2
    assert s1["step"] == s2["step"] == 3 and s1["hyper"] == s2["hyper"]
    for k in ("m", "v"):
        assert torch.equal(s1[k].view(torch.int32), s2[k].view(torch.int32)), k
    # end() hands the state back to the object: state_dict() keeps working, and the handle is free for another install
    opt1.end(e1)
    opt2.end(e2)
    s3 = opt1.state_dict()
    assert s3["step"] == 3 and torch.equal(s3["m"], s1["m"]) and not server_opt.server_active(e1)


# ---- only while installed ----------------------------------------------------------------------------------------------------
def test_launch_only_from_the_step(engines):
    """tests/test_drift_gpu.py::test_launch_only_while_installed's method: the engine's own list of the ops it enqueued.  A training
    step and an aggregation enqueue no server launch, installed or not, and as many ops as ever; each fm_server_opt_step is one."""
    model, n_classes = "Efficient_b0", 5
    x0, cnt0, tr, ps = _data(model, n_classes)
    eng = engines.get(model, n_classes)
    eng.set_state(x0, cnt0)
    eng.adam_reset(1e-3)
    g = torch.Generator().manual_seed(9)
    xb = torch.randn((B, 3, HW, HW), generator=g).cuda()
    yb = (torch.rand((B, n_classes), generator=g) < 0.3).float().cuda()
    loss = torch.zeros(1, device="cuda")
    old = eng.state_tensor().clone()

    def count(fn):
        eng.profile_ops(True, read=True)
        fn()
        rows = eng.profile_ops(False, read=True)
        return sum(n for lab, n, _ in rows if lab.startswith("server_opt")), sum(n for _, n, _ in rows)

    def train_and_aggregate():
        eng.step_bce(xb, yb, [1.0] * n_classes, B, loss)
        eng.state_scale(1.0)
        eng.fedavg_allreduce(1.0)

    mine, total = count(train_and_aggregate)
    assert mine == 0 and total > 0
    _begin(eng, "yogi")
    assert count(train_and_aggregate) == (0, total)
    assert count(lambda: [server_opt.server_step(eng, old) for _ in range(2)]) == (2, 2)
    server_opt.server_end(eng)
    assert count(train_and_aggregate) == (0, total)
