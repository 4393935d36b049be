"""Coherence matrix: every call that changes the resident state (tests/coherence_cases.MUTATORS) against every first consumer of a
copy the engine derives from it (READERS), on five handles, to the bit.

A cell: warm(E) builds every derived copy of handle E for the states (S0, T0); cold(T) only loads them into the twin T; the
mutator runs on both; the reader is the next call on each.  Every tensor the reader returns, and afterwards both states of both
handles, must carry the same bits: a flag that a mutator forgot leaves E on a copy built for S0 and shows here.  Two guards keep a
cell from passing vacuously: where the mutator moves what the reader reads (coherence_cases.affects) E's output must differ from
its output at (S0, T0), elsewhere it must equal it.  The positive control shows that readers a, b, c do see a stale copy: a torch
write through a view taken BEFORE the copies were rebuilt (the documented misuse of state_tensor()) makes each differ from a twin
that was handed the same state, and re-obtaining the view repairs it.

The Python layer on top (Engine.serial / weights_version, HipNet._dirty / _owner / _version) gets the same mutators: after one
that moves the weights a pending backward raises, after any other it gives the undisturbed gradients; a bound HipNet's
state_dict() is the engine's state.  Counts go to coherence_matrix.json beside the other parity reports."""
import numpy as np
import pytest
import torch

from fedmlp_amd import spec
from tests import coherence_cases as CC
from tests.test_local_training_gpu import _dump as _dump_report

pytestmark = pytest.mark.gpu

REPORT = {}
_PAIRS = {}        # handle -> (E, T, ctx)
_BASE = {}         # (handle, reader) -> the reader's output at (S0, T0), on the host
_STOCHASTIC = {}   # id -> (cached engine a HipNet was bound to, its `stochastic` before this module switched it off)


def _dump():
    _dump_report(REPORT, "coherence_matrix.json")


def _rep(handle):
    return REPORT.setdefault(handle, {"cells": 0, "must_differ": 0, "must_be_unchanged": 0, "positive_control": []})


def _bits(t):
    return t.detach().contiguous().cpu().reshape(-1).view(torch.uint8)


def _same(a, b):
    """the same bits (NaN-proof), tensor by tensor"""
    assert len(a) == len(b)
    return [x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b)]


def _host(out):
    return tuple(t.detach().cpu().clone() for t in out)


def _state_eq(got, want):
    return np.array_equal(got[0].view(np.int32), np.asarray(want[0]).view(np.int32)) and np.array_equal(got[1], want[1])


def _teacher_state(e):
    e.teacher_swap()
    st = e.get_state()
    e.teacher_swap()
    return st


def cold(e, ctx):
    e.set_state(*ctx.T0)
    e.teacher_snapshot()
    e.set_state(*ctx.S0)


def warm(e, ctx):
    """(S0, T0) loaded and every derived copy built for them, the state where it was"""
    cold(e, ctx)
    CC.r_eval(e, ctx)
    CC.r_eval_teacher(e, ctx)
    CC.r_train_grads_frozen(e, ctx)
    if ctx.precision == "fp32":
        CC.r_hooks(e, ctx)
    e.zero_grad()
    assert _state_eq(e.get_state(), ctx.S0), "warm moved the student's state"
    # (a swap pair leaves each net's own copies valid and the student-only ones stale: the readers below rebuild those)
    assert _state_eq(_teacher_state(e), ctx.T0), "warm moved the teacher's state"
    CC.r_eval(e, ctx)
    CC.r_eval_teacher(e, ctx)
    CC.r_train_grads_frozen(e, ctx)
    e.zero_grad()
    assert getattr(e, "_grad_owner", None) is None


def _pair(handle):
    if handle not in _PAIRS:
        for h in list(_PAIRS):                 # one pair alive at a time (the cells are grouped by handle)
            _close(h)
        E, T = CC.make_engine(handle), CC.make_engine(handle)
        _PAIRS[handle] = (E, T, CC.make_ctx(handle, E))
    return _PAIRS[handle]


def _close(handle):
    E, T, _ = _PAIRS.pop(handle)
    E.close()
    T.close()
    for k in [k for k in _BASE if k[0] == handle]:
        del _BASE[k]


@pytest.fixture(scope="module", autouse=True)
def _handles():
    yield
    for h in list(_PAIRS):
        _close(h)
    for eng, was in _STOCHASTIC.values():
        eng.stochastic = was
    _STOCHASTIC.clear()
    _dump()


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a failed comparison is a finding and the matrix goes on; a device error is sticky, and nothing more is launched after it"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as err:                   # noqa: BLE001
        pytest.exit(f"device error, the module stops here: {err}", returncode=3)


def _baseline(handle, reader, E, ctx):
    if (handle, reader) not in _BASE:
        warm(E, ctx)
        _BASE[handle, reader] = _host(CC.READERS[reader][0](E, ctx))
    return _BASE[handle, reader]


def _run_cell(handle, mutator, reader, E, T, ctx, base):
    mut, rd = CC.MUTATORS[mutator][0], CC.READERS[reader][0]
    warm(E, ctx)
    cold(T, ctx)
    mut(E, ctx)
    mut(T, ctx)
    got, want = _host(rd(E, ctx)), _host(rd(T, ctx))
    same = _same(got, want)
    assert all(same), f"{handle}: after {mutator}, reader {reader} on the warm handle differs from the cold twin in outputs " \
                      f"{[i for i, s in enumerate(same) if not s]}: a derived copy is stale"
    assert _state_eq(E.get_state(), T.get_state()), f"{handle}: {mutator}, {reader}: the students' states differ afterwards"
    assert _state_eq(_teacher_state(E), _teacher_state(T)), f"{handle}: {mutator}, {reader}: the teachers' states differ"
    rep = _rep(handle)
    rep["cells"] += 1
    moves = CC.MUTATORS[mutator][1]
    for i, unchanged in enumerate(_same(got, base)):
        dep = CC.reads(reader, i)
        if dep is None:
            continue
        if moves & dep:
            assert not unchanged, f"{handle}: {mutator} left output {i} of reader {reader} at its (S0, T0) bits: it was not seen"
        else:
            assert unchanged, f"{handle}: {mutator} must not move output {i} of reader {reader}"
    rep["must_differ" if CC.affects(mutator, reader) else "must_be_unchanged"] += 1


ALL_CELLS = [(h, m, r) for h in CC.HANDLES for m, r in CC.cells(h)]


@pytest.mark.parametrize("handle,mutator,reader", ALL_CELLS, ids=["-".join(c) for c in ALL_CELLS])
def test_cell(handle, mutator, reader):
    E, T, ctx = _pair(handle)
    base = _baseline(handle, reader, E, ctx)
    _run_cell(handle, mutator, reader, E, T, ctx, base)
    _dump()


# The twin of test_cell has lived through the earlier cells: a copy it built lazily then (the stem's data-gradient matrix, remade
# at its first consumer only) is rebuilt only if its flag was raised, so a flag broken everywhere would leave both handles
# stale alike.  A twin created inside the test has built nothing: the identity cells the matrix asks for, and three weight
# changes against the two readers of that matrix (c: dx, e: the stem's data gradient).
FRESH = [(h, "identity", r) for h in ("r18_64", "eff_64_bf16") for r in CC.READERS] + \
        [("r18_64", m, r) for m in ("set_state", "adam_step", "teacher_swap") for r in ("c", "e")]


@pytest.mark.parametrize("handle,mutator,reader", FRESH, ids=["-".join(c) for c in FRESH])
def test_fresh_pair(handle, mutator, reader):
    """a cell on two handles created here: the cold side rests on nothing an earlier cell left behind"""
    for h in list(_PAIRS):
        _close(h)
    E, T = CC.make_engine(handle), CC.make_engine(handle)
    try:
        ctx = CC.make_ctx(handle, E)
        warm(E, ctx)
        base = _host(CC.READERS[reader][0](E, ctx))
        _run_cell(handle + "/fresh", mutator, reader, E, T, ctx, base)
    finally:
        E.close()
        T.close()
    _dump()


@pytest.mark.parametrize("handle", list(CC.HANDLES))
def test_positive_control(handle):
    """A write through a state view taken before the derived copies were (re)built is NOT seen: readers a, b, c then differ from
    a twin that was handed the same state -- so each of them does depend on a derived copy, and the matrix can see staleness
    there.  (c) runs under frozen BatchNorm here, so that the stale pass leaves the state alone; it reads the same copies.
    The teacher's view is taken while the teacher sits in the student's slot.
    Every reader differed on every handle, so none is dropped from `affects`.  Which of a reader's tensors went stale is
    recorded in the report: on the two handles whose forward GEMMs read fp32 weights from the state itself (r18_64_fp32pipe,
    eff_64) the feature and logits of (c) stay right and only its gradients and dx -- the transposed data-gradient packs --
    go stale; (a) and (b) go stale there at least through the folded eval affine."""
    E, T, ctx = _pair(handle)
    readers = {"a": CC.r_eval, "b": CC.r_eval_teacher, "c": CC.r_train_grads_frozen}
    warm(E, ctx)
    E.teacher_swap()
    vt = E.state_tensor()
    E.teacher_swap()
    vs = E.state_tensor()
    for rd in readers.values():              # every copy rebuilt and every flag cleared, the views still in hand
        rd(E, ctx)
    vs.mul_(1.25)
    vt.mul_(1.25)
    k = np.float32(1.25)
    T.set_state(ctx.T0[0] * k, ctx.T0[1])
    T.teacher_snapshot()
    T.set_state(ctx.S0[0] * k, ctx.S0[1])
    want = {n: _host(rd(T, ctx)) for n, rd in readers.items()}
    rep = _rep(handle)
    for n, rd in readers.items():
        stale = _host(rd(E, ctx))
        differs = [not s for s in _same(stale, want[n])]
        assert any(differs), f"{handle}: reader {n} saw a write it was not told about: it reads no derived copy here"
        rep["positive_control"].append({"reader": n, "stale_outputs_that_differ": differs})
    E.state_tensor()                          # the contract: re-obtain the view, and the flags are raised
    E.teacher_swap()
    E.state_tensor()
    E.teacher_swap()
    for n, rd in readers.items():
        assert all(_same(_host(rd(E, ctx)), want[n])), f"{handle}: reader {n} is still stale after state_tensor() was re-obtained"
    assert _state_eq(E.get_state(), T.get_state()) and _state_eq(_teacher_state(E), _teacher_state(T))
    _dump()


# ---- the Python layer: serial / weights_version, the host copy of a bound net ---------------------------------------------------
PY_HANDLES = ["r18_64", "eff_64"]


def _moves_weights(mutator):
    return "w" in CC.MUTATORS[mutator][1]


def _forward(net, ctx):
    x = ctx.x1.clone().requires_grad_(True)
    _, z = net(x)
    return x, (z * ctx.dz).sum()


def _grads_of(net, x):
    return tuple(g.clone() for g in net.grads().values()) + (x.grad.clone(),)


def _drop_grads(eng):
    eng.zero_grad()
    eng._grad_owner = None


def _resident(handle):
    from fedmlp_amd.model import ResidentNet
    E, _, ctx = _pair(handle)
    warm(E, ctx)
    return E, ResidentNet(E).train(), ctx


def _bound(handle):
    from fedmlp_amd.model import HipNet
    _, _, ctx = _pair(handle)
    net = HipNet(ctx.model, CC.C_, ctx.S0[0].copy(), ctx.S0[1].copy()).train()
    net.default_max_images = ctx.imgs
    eng = net.bind(ctx.side, ctx.side, ctx.imgs)
    _STOCHASTIC.setdefault(id(eng), (eng, eng.stochastic))     # the process-wide engine: handed back as it was found
    eng.stochastic = False
    eng.teacher_snapshot()                                     # a known teacher, whatever the cached engine held
    return eng, net, ctx


_UNDISTURBED = {}


def _undisturbed(kind, handle):
    """gradients and x.grad of one forward + backward with nothing in between"""
    if (kind, handle) not in _UNDISTURBED:
        eng, net, ctx = (_resident if kind == "resident" else _bound)(handle)
        try:
            x, loss = _forward(net, ctx)
            loss.backward()
            _UNDISTURBED[kind, handle] = _host(_grads_of(net, x))
        finally:
            _drop_grads(eng)
    return _UNDISTURBED[kind, handle]


@pytest.mark.parametrize("mutator", list(CC.MUTATORS))
@pytest.mark.parametrize("handle", PY_HANDLES)
@pytest.mark.parametrize("kind", ["resident", "bound"])
def test_pending_backward(kind, handle, mutator):
    """net(x) in train mode, the mutator, loss.backward(): a mutator that moves the weights makes the backward raise (what
    test_backward_after_step_raises expects of an optimizer step), any other leaves it the undisturbed gradients through the
    recompute path.  The split is by the weights, not by the class: a batch-statistics backward reads no running statistics
    (coherence_cases.STATS_ONLY).  A bound HipNet is told of the change the way local_training.py / optim.py tell it
    (mark_trained); its state_dict() must then be the engine's state."""
    want = None if _moves_weights(mutator) else _undisturbed(kind, handle)
    eng, net, ctx = (_resident if kind == "resident" else _bound)(handle)
    try:
        x, loss = _forward(net, ctx)
        CC.MUTATORS[mutator][0](eng, ctx)
        if _moves_weights(mutator):
            if kind == "bound":
                net.mark_trained()
            with pytest.raises(RuntimeError, match="weights changed"):
                loss.backward()
            assert x.grad is None
        else:
            loss.backward()
            assert all(_same(_host(_grads_of(net, x)), want)), f"{kind} {handle}: {mutator} disturbed a pending backward"
        if kind == "bound" and CC.MUTATORS[mutator][1] & {"w", "stats"}:
            if not _moves_weights(mutator):
                net.mark_trained()
            _assert_state_dict_is_the_engines(net, eng, ctx)
    finally:
        _drop_grads(eng)


def _assert_state_dict_is_the_engines(net, eng, ctx):
    flat, cnt = eng.get_state()
    want = spec.flat_to_state_dict(ctx.model, CC.C_, flat, cnt)
    got = net.state_dict()
    assert list(got) == list(want)
    for k, v in want.items():
        g = got[k].numpy()
        assert g.dtype == v.dtype and np.array_equal(g.reshape(-1).view(np.uint8), np.ascontiguousarray(v).reshape(-1).view(np.uint8)), k


@pytest.mark.parametrize("handle", PY_HANDLES)
def test_bound_net_sees_moved_running_statistics(handle):
    """a train-mode net(x) alone: state_dict() holds the moved running statistics and counters, not the host copy"""
    eng, net, ctx = _bound(handle)
    before = net.state_dict()
    with torch.no_grad():
        net(ctx.x1)
    _assert_state_dict_is_the_engines(net, eng, ctx)
    after = net.state_dict()
    moved = [k for k in after if ("running_" in k or "num_batches" in k) and not torch.equal(after[k], before[k])]
    assert len(moved) == sum("running_" in k or "num_batches" in k for k in after)
    assert all(torch.equal(after[k], before[k]) for k in after if spec.is_trainable(k))
