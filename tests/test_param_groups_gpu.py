"""Frozen layers (net.requires_grad_ / fm_set_trainable) and optimizer parameter groups (fm_optim_groups, fm_*_step_groups) on a
real MI355X: ResNet-18 and EfficientNet-B0 (fp32) at 64 x 64, batch 4, 5 classes -- the chunking of the entry table, the entry
boundaries, the padded 24 -> 32 / 40 -> 48 channels and the packed stem do not depend on the image size.

Bit comparisons run over the raw engine-layout arenas (weights: Engine.state_tensor(); moments and accumulator:
Engine.debug_optim_arena), layout padding included.  The optimizer tests fill the accumulator with ONE backward at the initial
weights under the default mask and then step twice from it (the second step is the later-step form), so every line of a
comparison steps from the same (p, g, m, v) whatever its mask or groups: the updates are element-wise.

Float64 reference and bound of the per-group arithmetic: tests/test_optim_gpu.py's (torch's formulas with the fp32-rounded
hyper-parameters, 4 ulp(p) + 1e-5 |dp|)."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fedmlp_amd import _lib, spec
from fedmlp_amd.engine import Engine
from fedmlp_amd.model import ResidentNet
from fedmlp_amd.optim import AdamW, clip_grad_norm_
from tests.test_optim_gpu import NORM_RTOL, _adamw_ref, _excess, _sgd_ref

pytestmark = pytest.mark.gpu

C_, HW, B = 5, 64, 4
MODELS = ["Resnet18", "Efficient_b0"]
TOP = {"Resnet18": ["layer4", "fc"], "Efficient_b0": ["_blocks.15", "_conv_head", "_bn1", "_fc"]}
HEAD = {"Resnet18": ["fc"], "Efficient_b0": ["_fc"]}
ONE_BLOCK = {"Resnet18": ["layer1.0"], "Efficient_b0": ["_blocks.1"]}
STEM = {"Resnet18": ["conv1", "bn1"], "Efficient_b0": ["_conv_stem", "_bn0"]}


# ---- the entry table, host side -------------------------------------------------------------------------------------
def _entries(model):
    return spec.entries(model, C_)


def _params(model):
    """indices (state entry order) of the parameters"""
    return [i for i, (k, _, dt) in enumerate(_entries(model)) if dt == "f32" and spec.is_trainable(k)]


def _flags(model, on):
    on = set(on)
    return [int(i in on) for i in range(len(_entries(model)))]


def _flat_ranges(model):
    """state entry index -> (start, stop) in the flat fp32 state_dict layout (grads() / optim_state() / get_state())"""
    out, off = {}, 0
    for i, (k, shape, dt) in enumerate(_entries(model)):
        if dt != "f32":
            continue
        n = int(np.prod(shape))
        out[i] = (off, off + n)
        off += n
    return out


def _flat_mask(model, idx):
    r = _flat_ranges(model)
    m = torch.zeros(spec.sizes(model, C_)[0], dtype=torch.bool)
    for i in idx:
        m[r[i][0]:r[i][1]] = True
    return m


def _arena_mask(eng, idx):
    """bool [NP] on the device: the arena floats of the given state entries' spans"""
    spans = eng.debug_entry_spans()
    m = torch.zeros(eng.debug_optim_arena(0).numel(), dtype=torch.bool, device="cuda")
    for i in idx:
        off, n = int(spans[i, 0]), int(spans[i, 1])
        assert off >= 0 and n > 0, i
        m[off:off + n] = True
    return m


# ---- engines ----------------------------------------------------------------------------------------------------------
class _Lines:
    """Engines by (model, slot), reset to the model's initial state on every get().  A `pristine` slot never has a mask or group
    call made on it by the reset."""

    def __init__(self):
        self.engines = {}

    def get(self, model, slot=0, pristine=False):
        eng = self.engines.get((model, slot))
        if eng is None:
            eng = self.engines[(model, slot)] = Engine(model, C_, HW, HW, 2 * B)
            eng.stochastic = False           # EfficientNet-B0: no drop-connect / dropout draws (identity multipliers)
        flat, cnt = spec.init_state(model, C_, 1037)
        eng.set_state(flat, cnt)
        eng.adam_reset(1e-3)
        eng.zero_grad()
        eng.bn_freeze(False)
        eng._grad_owner = None
        if not pristine:
            eng.set_trainable(_flags(model, _params(model)))
            eng.optim_groups(None, 0)
        eng._frozen_keys, eng._groups_key = frozenset(), None
        return eng, ResidentNet(eng).train()

    def close(self):
        for eng in self.engines.values():
            eng.close()
        self.engines.clear()


@pytest.fixture(scope="module")
def lines():
    ln = _Lines()
    yield ln
    ln.close()


def _batch(seed, grad=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 3, HW, HW), generator=g).cuda()
    y = (torch.rand((B, C_), generator=g) < 0.4).float().cuda()
    return x.requires_grad_(grad), y


def _loss(net, x, y):
    f, z = net(x)
    return F.binary_cross_entropy_with_logits(z, y) + 1e-3 * f.pow(2).mean()


def _fill(net, seed=100):
    net.zero_grad()
    _loss(net, *_batch(seed)).backward()


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _snap(eng):
    return {"w": _bits(eng.state_tensor()), "m": _bits(eng.debug_optim_arena(0)), "v": _bits(eng.debug_optim_arena(1)),
            "step": eng.optim_state()[0]}


# ---- the optimizer cases ------------------------------------------------------------------------------------------------
ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
CASES = {
    "adam": ("adam", ADAM),
    "adamw": ("adamw", dict(ADAM, weight_decay=1e-2)),
    "sgd_nesterov": ("sgd", dict(lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=True)),
    "sgd_plain": ("sgd", dict(lr=1e-2, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)),
}


def _row(kind, hp):
    if kind == "sgd":
        return (hp["lr"], hp["momentum"], hp["dampening"], hp["weight_decay"], hp["nesterov"])
    return (hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])


def _step_single(eng, kind, hp):
    {"adam": eng.adam_step, "adamw": eng.adamw_step, "sgd": eng.sgd_step}[kind](*_row(kind, hp))


def _step_groups(eng, kind, hps):
    {"adam": eng.adam_step_groups, "adamw": eng.adamw_step_groups, "sgd": eng.sgd_step_groups}[kind]([_row(kind, h) for h in hps])


_REF = {}


def _reference(lines, model, kind, hp):
    """[snapshot after step 1, after step 2] of the EXISTING single-group entry points; computed once per (model, hp), shared."""
    key = (model, kind, tuple(sorted((k, str(v)) for k, v in hp.items())))
    if key not in _REF:
        eng, net = lines.get(model, 0)
        _fill(net)
        snaps = []
        for _ in range(2):
            _step_single(eng, kind, hp)
            snaps.append(_snap(eng))
        _REF[key] = snaps
    return _REF[key]


def _same(a, b, what):
    assert a["step"] == b["step"], what
    for k in ("w", "m", "v"):
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs in {int((a[k] != b[k]).sum())} of {a[k].numel()} arena words"


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", list(CASES))
def test_one_group_is_the_existing_step_bit_for_bit(lines, model, case):
    kind, hp = CASES[case]
    ref = _reference(lines, model, kind, hp)
    eng, net = lines.get(model, 1)
    _fill(net)
    p = _params(model)
    eng.optim_groups([0 if i in set(p) else -1 for i in range(len(_entries(model)))], 1)
    for s in range(2):
        _step_groups(eng, kind, [hp])
        _same(_snap(eng), ref[s], f"{model} {case} step {s + 1}")
    assert ref[1]["step"] == 2 and not torch.equal(ref[0]["w"], ref[1]["w"])


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", list(CASES))
def test_three_groups_with_identical_hyper_parameters(lines, model, case):
    """entries round-robin over three groups: every adjacent pair of entries sits in different groups"""
    kind, hp = CASES[case]
    ref = _reference(lines, model, kind, hp)
    eng, net = lines.get(model, 1)
    _fill(net)
    of = [-1] * len(_entries(model))
    for j, i in enumerate(_params(model)):
        of[i] = j % 3
    eng.optim_groups(of, 3)
    for s in range(2):
        _step_groups(eng, kind, [hp, hp, hp])
        _same(_snap(eng), ref[s], f"{model} {case} step {s + 1}")


# 3 ---------------------------------------------------------------------------------------------------------------------
GROUP_HPS = {
    "adamw": [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
              dict(lr=1e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.0),
              dict(lr=1e-2, betas=(0.95, 0.9), eps=1e-6, weight_decay=5e-2)],
    "adam": [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4),
             dict(lr=1e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.0),
             dict(lr=1e-2, betas=(0.95, 0.9), eps=1e-6, weight_decay=5e-3)],
    "sgd": [dict(lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=True),
            dict(lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False),      # another MODE in the same launch
            dict(lr=1e-1, momentum=0.8, dampening=0.1, weight_decay=1e-3, nesterov=False)],
}


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", ["adamw", "sgd", "adam"])
def test_different_hyper_parameters_per_group(lines, model, kind):
    """lr x1, x0.1, x10, different weight decay and betas / momenta.  Each group's entries (a) within 4 ulp(p) + 1e-5 |dp| of torch's
    formula in float64 with that group's fp32-rounded hyper-parameters (AdamW, SGD: the optimizers tests/test_optim_gpu.py holds to
    that bound), and (b) the same bits as the existing single-group step taken with that group's hyper-parameters."""
    hps = GROUP_HPS[kind]
    eng, net = lines.get(model, 1)
    _fill(net)
    params = _params(model)
    of = [-1] * len(_entries(model))
    for j, i in enumerate(params):
        of[i] = j % 3
    members = [[i for j, i in enumerate(params) if j % 3 == g] for g in range(3)]
    fmask = [_flat_mask(model, m) for m in members]
    eng.optim_groups(of, 3)
    g64 = eng.grads().cpu().double()
    snaps, worst = [], {}
    for s in range(2):
        p0 = torch.from_numpy(eng.get_state()[0]).double()
        step, m0, v0 = eng.optim_state()
        m0, v0 = m0.cpu().double(), v0.cpu().double()
        assert step == s
        _step_groups(eng, kind, hps)
        snaps.append(_snap(eng))
        p1 = torch.from_numpy(eng.get_state()[0])
        _, m1, v1 = eng.optim_state()
        m1, v1 = m1.cpu(), v1.cpu()
        if kind == "adam":
            # no float64 leg: coupled Adam keeps adam_kernel's all-fp32 lerp (the fused steps' code), which does not meet the
            # 4 ulp(p) + 1e-5 |dp| bound where beta1 m and (1 - beta1) g cancel (tests/test_optim_gpu.py holds only SGD and
            # AdamW to it); Adam's groups are held to the single-group step's bits below
            continue
        for g, hp in enumerate(hps):
            sel = fmask[g]
            if kind == "adamw":
                want_p, want_m, want_v = _adamw_ref(p0[sel], g64[sel], m0[sel], v0[sel], s, hp)
                state = {"exp_avg": (m1[sel], want_m, m0[sel]), "exp_avg_sq": (v1[sel], want_v, v0[sel])}
            else:
                want_p, want_b = _sgd_ref(p0[sel], g64[sel], m0[sel], s, hp)
                state = {"momentum_buffer": (m1[sel], want_b, m0[sel])}
                if not hp["momentum"]:
                    assert torch.equal(m1[sel].double(), m0[sel]), "momentum 0 wrote the buffer"
            assert float((p1[sel].double() - p0[sel]).abs().max()) > 0, "the step changed nothing"
            worst[f"g{g} p"] = max(worst.get(f"g{g} p", 0.0), _excess(p1[sel], want_p, p0[sel]))
            for k, (got, want, old) in state.items():
                nz = (want != 0) | (old != 0) | (got != 0)
                if bool(nz.any()):
                    worst[f"g{g} {k}"] = max(worst.get(f"g{g} {k}", 0.0), _excess(got[nz], want[nz], old[nz]))
    print(f"\n[param groups] {model} {kind}: max error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    amask = [_arena_mask(eng, m) for m in members]
    for g, hp in enumerate(hps):
        ref = _reference(lines, model, kind, hp)
        for s in range(2):
            for k in ("w", "m", "v"):
                got, want = snaps[s][k][:amask[g].numel()][amask[g]], ref[s][k][:amask[g].numel()][amask[g]]
                assert torch.equal(got, want), f"{model} {kind} group {g} step {s + 1}: {k} is not the single-group step's"


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", list(CASES))
def test_nobody_writes_a_neighbours_floats(lines, model, case):
    """Every other parameter frozen, every third in no group: the skipped entries' weights and moments keep their bits, the
    stepped ones are the single-group step's, the floats outside every entry are still exact zeros."""
    kind, hp = CASES[case]
    ref = _reference(lines, model, kind, hp)
    eng, net = lines.get(model, 1)
    _fill(net)                                   # under the default mask: the accumulator holds every gradient
    params = _params(model)
    spans = eng.debug_entry_spans()
    if model == "Efficient_b0":
        edges = [int(spans[i, 0]) for i in params] + [int(spans[i, 0] + spans[i, 1]) for i in params]
        assert any(e % 4 for e in edges), "no entry boundary off a 16-byte boundary: the boundary case has disappeared"
    frozen = [i for j, i in enumerate(params) if j % 2 == 1]
    nogroup = [i for j, i in enumerate(params) if j % 3 == 2]
    stepped = [i for i in params if i not in set(frozen) | set(nogroup)]
    skipped = [i for i in params if i not in set(stepped)]
    assert stepped and set(frozen) - set(nogroup) and set(nogroup) - set(frozen)
    before = _snap(eng)
    eng.set_trainable(_flags(model, [i for i in params if i not in set(frozen)]))
    eng.optim_groups([(-1 if i in set(nogroup) else 0) if i in set(params) else -1 for i in range(len(_entries(model)))], 1)
    NP = eng.debug_optim_arena(0).numel()
    on, off = _arena_mask(eng, stepped), _arena_mask(eng, skipped)
    gaps = ~_arena_mask(eng, params)
    assert int(gaps.sum()) > 0 and not bool((on & off).any())
    for s in range(2):
        _step_groups(eng, kind, [hp])
        got = _snap(eng)
        assert got["step"] == s + 1
        for k in ("w", "m", "v"):
            a, r, b = got[k][:NP], ref[s][k][:NP], before[k][:NP]
            assert torch.equal(a[off], b[off]), f"{model} {case} step {s + 1}: a skipped entry's {k} moved"
            assert torch.equal(a[on], r[on]), f"{model} {case} step {s + 1}: a stepped entry's {k} is not the single-group step's"
            assert not bool(a[gaps].any()), f"{model} {case} step {s + 1}: {k} is not zero outside the entries"
        assert torch.equal(got["w"][NP:], before["w"][NP:]), "the running statistics moved"
    assert not torch.equal(got["w"][:NP][on], before["w"][:NP][on])


# 5, 6 ------------------------------------------------------------------------------------------------------------------
def _scenario(eng, net, form, want_dx=False):
    """the accumulator (state_dict layout and raw arena) after: `copy` one forward + backward; `add` two of them into the same
    accumulator; `recompute` two forwards sharing one backward (the earlier node recomputes its forward)"""
    net.zero_grad()
    x1, y1 = _batch(200, want_dx)
    if form == "recompute":
        x2, y2 = _batch(201)
        (_loss(net, x1, y1) + _loss(net, x2, y2)).backward()
    else:
        for _ in range(2 if form == "add" else 1):
            _loss(net, x1, y1).backward()
    return eng.grads().clone(), eng.debug_optim_arena(2).clone(), (x1.grad.clone() if want_dx else None)


_CONTROL = {}


def _control(lines, model, form, want_dx=False):
    key = (model, form, want_dx)
    if key not in _CONTROL:
        eng, net = lines.get(model, 2)
        _CONTROL[key] = _scenario(eng, net, form, want_dx)
    return _CONTROL[key]


def _mask_names(model, mask):
    if mask == "head":
        return HEAD[model]
    if mask == "top":
        return TOP[model]
    if mask == "one_block":
        return ONE_BLOCK[model]
    return None


def _apply_mask(net, model, mask):
    if mask == "all":
        return net.requires_grad_(True)
    if mask == "no_stem":
        return net.requires_grad_(True).requires_grad_(False, STEM[model])
    return net.requires_grad_(False).requires_grad_(True, _mask_names(model, mask))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("form", ["copy", "add", "recompute"])
@pytest.mark.parametrize("mask", ["head", "top", "one_block", "no_stem", "all"])
def test_masked_gradients(lines, model, form, mask):
    want, want_raw, _ = _control(lines, model, form)
    eng, net = lines.get(model, 2)
    _apply_mask(net, model, mask)
    got, raw, _ = _scenario(eng, net, form)
    live = net.trainable()
    keys = [k for k, _, _ in _entries(model)]
    on = [i for i in _params(model) if live[keys[i]]]
    off = [i for i in _params(model) if not live[keys[i]]]
    assert on and (off or mask == "all")
    f_on, f_off = _flat_mask(model, on).cuda(), _flat_mask(model, off).cuda()
    assert not bool(got[f_off].any()), f"{model} {mask} {form}: a frozen entry of net.grads() is not zero"
    assert torch.equal(_bits(got[f_on]), _bits(want[f_on])), f"{model} {mask} {form}: a trainable entry differs from the control"
    assert bool(want[f_on].any())
    a_on, a_off = _arena_mask(eng, on), _arena_mask(eng, off)
    assert not bool(raw[a_off].any()) and not bool(raw[~(a_on | a_off)].any())
    assert torch.equal(_bits(raw[a_on]), _bits(want_raw[a_on]))
    g = net.grads()
    assert all(not bool(g[k].any()) for k in g if not live[k])


@pytest.mark.parametrize("model", MODELS)
def test_input_gradient_with_everything_frozen(lines, model):
    _, _, want_dx = _control(lines, model, "copy", True)
    eng, net = lines.get(model, 2)
    net.requires_grad_(False)
    got, raw, dx = _scenario(eng, net, "copy", True)
    assert bool(want_dx.any()) and torch.equal(_bits(dx), _bits(want_dx))
    assert not bool(got.any()) and not bool(raw.any())


# 7 ---------------------------------------------------------------------------------------------------------------------
def _ops(eng, fn):
    eng.profile_ops(1)                           # enable, and drop what was recorded so far
    fn()
    return collections.Counter({lab: n for lab, n, _ in eng.profile_ops(1)})


def _gemms(eng, fn):
    eng.profile_enable(1)
    for f in range(9):
        eng.profile_read(f)
    fn()
    return [eng.profile_read(f)[0] for f in range(9)]


@pytest.mark.parametrize("model", MODELS)
def test_truncation_really_happens(lines, model):
    """The engine's own launch profile: ops recorded by forward + backward minus those of the forward alone."""
    eng, net = lines.get(model, 3, pristine=True)
    x, y = _batch(300)

    def fwd():
        with torch.no_grad():
            net(x)

    def fwd_bwd():
        net.zero_grad()
        _loss(net, x, y).backward()

    def backward_ops():
        return _ops(eng, fwd_bwd) - _ops(eng, fwd)

    def ctx(label):
        return int(label.rsplit("@", 1)[1])

    expected = backward_ops()                    # the mask was never touched on this engine: the list as it always was
    assert len(expected) > 20 and any(ctx(k) == 399 for k in expected)
    resnet = model == "Resnet18"                 # its conv GEMMs are counted per kernel family as well (fm_profile_read)
    if resnet:
        gemm_fwd = _gemms(eng, fwd)
        gemm_all = _gemms(eng, fwd_bwd)
        eng.profile_enable(0)
        assert sum(gemm_all) > sum(gemm_fwd) > 0

    net.requires_grad_(False).requires_grad_(True, HEAD[model])
    head = backward_ops()
    assert dict(head) == {"k_fc_bwd@500": 1}, head
    if resnet:
        assert _gemms(eng, fwd_bwd) == gemm_fwd, "a convolution GEMM ran in a head-only backward"
        eng.profile_enable(0)

    net.requires_grad_(False).requires_grad_(True, TOP[model])
    top = backward_ops()
    first = {"Resnet18": 406, "Efficient_b0": 415}[model]          # layer4.0 / _blocks.15 (the head's ops carry 500)
    assert top and all(ctx(k) >= first for k in top), sorted(top)
    assert any(ctx(k) == first for k in top) and all(top[k] == expected[k] for k in top)
    assert set(top) < set(expected)

    net.requires_grad_(True)
    assert backward_ops() == expected
    eng.profile_ops(0)


# 8 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_clipping_under_a_mask(lines, model):
    eng, net = lines.get(model, 2)
    net.requires_grad_(False).requires_grad_(True, TOP[model])
    _fill(net, 11)
    live = net.trainable()
    g = net.grads()
    want = float(torch.cat([g[k].reshape(-1) for k in g if live[k]]).double().pow(2).sum().sqrt())
    n = clip_grad_norm_(net, 1e30)
    rel = abs(float(n) - want) / want
    print(f"\n[param groups] {model} masked grad norm {float(n):.9g}, float64 over the trainable entries {want:.9g}, "
          f"relative error {rel:.3e} (bound {NORM_RTOL:.3e})")
    assert want > 0 and rel <= NORM_RTOL


# 9 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_fused_steps_refuse_a_mask(lines, model):
    eng, _ = lines.get(model, 4)
    ref, _ = lines.get(model, 5, pristine=True)  # an engine whose mask is never touched
    x, y = _batch(400)
    pw = [1.0] * C_
    params = _params(model)
    eng.set_trainable(_flags(model, params[len(params) // 2:]))
    assert list(eng.get_trainable()) == _flags(model, params[len(params) // 2:])
    before = _snap(eng)
    lo = torch.zeros(1, device="cuda")
    with pytest.raises(_lib.FmError, match="autograd path"):
        eng.step_bce(x, y, pw, B, lo)
    _same(_snap(eng), before, "a refused fused step")
    eng.set_trainable(_flags(model, params))          # requires_grad_(True): the default mask again
    lo_ref = torch.zeros(1, device="cuda")
    eng.step_bce(x, y, pw, B, lo)
    ref.step_bce(x, y, pw, B, lo_ref)
    assert torch.equal(_bits(lo), _bits(lo_ref))
    _same(_snap(eng), _snap(ref), f"{model}: fm_step_bce after the mask was cleared")


# 10 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_fine_tuning_recipe(lines, model):
    """freeze_bn() + layer4 / fc trainable + AdamW in two groups, two steps."""
    eng, net = lines.get(model, 2)
    net.freeze_bn().requires_grad_(False).requires_grad_(True, TOP[model])
    opt = AdamW(net, lr=1e-2, groups=[{"params": HEAD[model]}, {"params": [n for n in TOP[model] if n not in HEAD[model]], "lr": 1e-3}])
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    x, y = _batch(500)
    losses = []
    for _ in range(2):
        opt.zero_grad()
        loss = _loss(net, x, y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    sd1 = net.state_dict()
    live = net.trainable()
    for k, v in sd1.items():
        if k not in live or not live[k]:
            assert torch.equal(v, sd0[k]), f"{k} (running statistic, counter or frozen weight) moved"
        elif k.endswith(".weight"):
            assert not torch.equal(v, sd0[k]), f"{k} is trainable and did not move"
    assert opt.state_dict()["state"]["step"] == 2
    assert losses[1] != losses[0] and all(np.isfinite(losses))
    net.freeze_bn(False)
