"""The tables of the coherence tests (tests/test_coherence_cpu.py, tests/test_coherence_gpu.py): which entry point of
include/fedmlp_hip.h may change what, the calls that change the resident state (MUTATORS) and the first consumers of every copy the
engine derives from it (READERS).  Importing this module needs no GPU and no library; the callables touch the device only when run.

The derived copies and the flag that guards each are listed in DESIGN.md ("Coherence of the derived copies").  Everything here is
compared to the bit: the engine is run-to-run deterministic, so a handle whose copies were all built for another state (warm) and a
handle that only ever loaded the states (cold) must agree exactly after the same calls."""
import ast
import os
import re
import types

import numpy as np
import torch

from fedmlp_amd import spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_ = 5
LR = 1e-2          # large enough that one optimizer step moves every fp32 weight it touches

# ---- 1. every fm_* entry point of include/fedmlp_hip.h -------------------------------------------------------------------------
# student: may change the student's weights or running statistics (fm_state_device: the caller may write through the pointer;
#          fm_counters: the num_batches_tracked counters are part of the state)
# teacher: may change the teacher's;  both: either;  work: enqueues work (and may overwrite the activations a train forward
# saved) but changes no state;  pure: host-only
_STUDENT = """fm_set_state fm_state_device fm_counters fm_state_scale fm_fedavg_fold fm_fed_w fm_fedavg_allreduce fm_step_bce
fm_step_stage1 fm_step_stage2 fm_step_fixmatch fm_step_fedlsr fm_step_fednoro fm_step_cbafed fm_forward_train fm_backward_step
fm_adam_step fm_sgd_step fm_adamw_step fm_adam_step_groups fm_adamw_step_groups fm_sgd_step_groups"""
_TEACHER = "fm_teacher_snapshot fm_teacher_axpby fm_teacher_ema_params"
_BOTH = "fm_teacher_swap fm_step_rscfed"
_WORK = """fm_state_dist fm_adam_reset fm_forward_eval fm_loss_fedlsr fm_loss_fedirm_sup fm_loss_fedirm_rel fm_loss_rscfed fm_loss_lakd
fm_loss_cbafed fm_proto_reset fm_proto_accumulate fm_proto_finalize fm_cos_tag fm_select_topk fm_select_topk_rows fm_augment
fm_augment_strong fm_eval_metrics fm_backward_grads fm_backward_grads_x fm_forward_recompute fm_get_grads fm_sgd_reset fm_grad_norm
fm_clip_grad_norm fm_clip_grad_value fm_optim_get_state fm_optim_set_state"""
_PURE = """fm_last_error fm_version fm_create fm_destroy fm_sync fm_state_sizes fm_get_state fm_comm_preflight fm_comm_unique_id
fm_comm_init fm_comm_destroy fm_comm_size fm_fedavg_tao fm_fedavg_proto fm_bn_freeze fm_bn_frozen fm_zero_grad fm_set_trainable
fm_get_trainable fm_optim_groups fm_set_stochastic fm_feature_dim fm_stream_mode fm_mfma_products fm_products fm_planes_mode
fm_profile_enable fm_profile_read fm_profile_ops"""
FM_CLASS = {}
for _cls, _names in (("student", _STUDENT), ("teacher", _TEACHER), ("both", _BOTH), ("work", _WORK), ("pure", _PURE)):
    for _n in _names.split():
        assert _n not in FM_CLASS, _n
        FM_CLASS[_n] = _cls

# student-class entry points whose wrapper bumps Engine.serial but not Engine.weights_version, with the reason
STATS_ONLY = {
    "fm_forward_train": "moves the BatchNorm running statistics only; weights_version gates a batch-statistics backward, which "
                        "reads none of them (two net(x) and one backward of their summed loss must work); a frozen-BatchNorm "
                        "forward is guarded by HipNet._stats_ver instead",
}
# student / teacher / both entry points reachable from Engine that no MUTATORS entry calls, with the reason
NOT_IN_MATRIX = {
    "fm_fedavg_allreduce": "needs a communicator: tests/test_rccl_gpu.py",
    "fm_counters": "the counters feed no kernel; checked through the state read-back of every cell",
    "fm_step_stage2": "fm_step_bce's tail (net_backward_and_step -> adam_step -> weights_stepped) with another loss head",
    "fm_step_fixmatch": "fm_step_bce's tail with a two-view forward, as fm_step_stage1 has",
    "fm_step_fedlsr": "fm_step_bce's tail with a two-view forward, as fm_step_stage1 has",
    "fm_step_fednoro": "fm_step_stage1's teacher forward and fm_step_bce's tail",
    "fm_step_cbafed": "fm_step_bce's tail with another loss head",
}


def header_entry_points():
    """the fm_* functions include/fedmlp_hip.h declares"""
    with open(os.path.join(ROOT, "include", "fedmlp_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return re.findall(r"^(?:int|const char\*)\s+(fm_\w+)\s*\(", text, flags=re.M)


def _enqueue_kind(call):
    """'weights' for self._enqueue(weights=True), 'plain' for self._enqueue()"""
    for kw in call.keywords:
        if kw.arg == "weights" and isinstance(kw.value, ast.Constant) and kw.value.value is True:
            return "weights"
    return "plain"


def engine_ledger():
    """Engine method -> {"fm": the self.lib.fm_* names in its body, "enqueue": the kinds of its own self._enqueue calls, "calls":
    the other Engine methods it calls}, read from fedmlp_amd/engine.py with ast; closed() adds what the called methods do."""
    with open(os.path.join(ROOT, "fedmlp_amd", "engine.py")) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Engine")
    out = {}
    for fn in cls.body:
        if not isinstance(fn, ast.FunctionDef):
            continue
        rec = {"fm": set(), "enqueue": set(), "calls": set()}
        for n in ast.walk(fn):
            if isinstance(n, ast.Attribute) and n.attr.startswith("fm_") and isinstance(n.value, ast.Attribute) \
                    and n.value.attr == "lib":
                rec["fm"].add(n.attr)
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and isinstance(n.func.value, ast.Name) \
                    and n.func.value.id == "self":
                if n.func.attr == "_enqueue":
                    rec["enqueue"].add(_enqueue_kind(n))
                else:
                    rec["calls"].add(n.func.attr)
        out[fn.name] = rec
    return out


def closed(ledger, name, through_wrappers=True, seen=None):
    """(fm names, enqueue kinds) of an Engine method together with the Engine methods it calls.  through_wrappers False: only
    helpers that call no entry point themselves are followed (_step_groups), so that a wrapper is not excused by another
    wrapper it happens to call (fedavg_fold calls state_tensor() only when it is given no destination)."""
    seen = set() if seen is None else seen
    if name in seen or name not in ledger:
        return set(), set()
    seen.add(name)
    fm, enq = set(ledger[name]["fm"]), set(ledger[name]["enqueue"])
    for c in ledger[name]["calls"]:
        if not through_wrappers and ledger.get(c, {}).get("fm"):
            continue
        f2, e2 = closed(ledger, c, through_wrappers, seen)
        fm |= f2
        enq |= e2
    return fm, enq


def _calls_on(fn_node, var, funcs, seen):
    """method names called on the variable `var` in a function of this module, following its calls of other module functions"""
    names = set()
    for n in ast.walk(fn_node):
        if not isinstance(n, ast.Call):
            continue
        if isinstance(n.func, ast.Attribute) and isinstance(n.func.value, ast.Name) and n.func.value.id == var:
            names.add(n.func.attr)
        elif isinstance(n.func, ast.Name) and n.func.id in funcs and n.func.id not in seen:
            seen.add(n.func.id)
            names |= _calls_on(funcs[n.func.id], funcs[n.func.id].args.args[0].arg, funcs, seen)
    return names


def engine_methods_of(fn):
    """the Engine methods a MUTATORS / READERS callable of this module calls on its first argument (read from the source)"""
    with open(__file__.replace(".pyc", ".py")) as f:
        tree = ast.parse(f.read())
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    node = funcs[fn.__name__]
    return _calls_on(node, node.args.args[0].arg, funcs, {fn.__name__})


# ---- 2. fixed inputs -------------------------------------------------------------------------------------------------------------
def perturbed_state(model, seed):
    """spec.init_state with the BatchNorm affine, running statistics and biases moved off 0 / 1 the way
    tests/test_effnet_gpu.py::_oracle moves them, so that the folded eval affine is not trivial.  -> (flat, counters)"""
    flat, cnt = spec.init_state(model, C_, seed)
    g = torch.Generator().manual_seed(seed + 1)
    out, off = flat.copy(), 0
    for key, shape, dt in spec.entries(model, C_):
        if dt != "f32":
            continue
        n = int(np.prod(shape))
        t = torch.from_numpy(out[off:off + n])
        if key.endswith("running_var"):
            t.mul_(0.5 + torch.rand(n, generator=g))
        elif key.endswith("running_mean") or key.endswith(".bias"):
            t.add_(0.1 * torch.randn(n, generator=g))
        elif len(shape) == 1:
            t.mul_(1.0 + 0.1 * torch.randn(n, generator=g))
        off += n
    cnt = cnt + 3                                   # a counter that is not 0 either
    return out, cnt


# handle -> (model, precision, side, images, products)
HANDLES = {
    "r18_64": ("Resnet18", "fp32", 64, 4, None),
    "r18_64_fp32pipe": ("Resnet18", "fp32", 64, 4, 0),
    "r18_224": ("Resnet18", "fp32", 224, 2, None),
    "eff_64": ("Efficient_b0", "fp32", 64, 4, None),
    "eff_64_bf16": ("Efficient_b0", "bf16", 64, 4, None),
}
_STATES = {}


def states(model):
    """(S0, T0, S1, S2): the student's and the teacher's state, the state set_state moves to, and a second one for the folds"""
    if model not in _STATES:
        _STATES[model] = tuple(perturbed_state(model, s) for s in (1037, 2041, 3001, 3002))
        for flat, cnt in _STATES[model]:
            flat.setflags(write=False)
            cnt.setflags(write=False)
    return _STATES[model]


def make_engine(handle):
    from fedmlp_amd.engine import Engine
    model, precision, side, imgs, products = HANDLES[handle]
    e = Engine(model, C_, side, side, imgs, precision=precision, products=products)
    e.stochastic = False
    return e


def host_inputs(handle):
    """the batches, labels and gradient seeds of a handle, from one seeded CPU generator"""
    model, precision, side, imgs, _ = HANDLES[handle]
    g = torch.Generator().manual_seed(77)
    D = spec.FEATURE_DIM[model]
    nf = spec.sizes(model, C_)[0]
    y = (torch.rand((imgs, C_), generator=g) < 0.4).float()
    y[0, 1] = 1.0
    return dict(x1=torch.randn((imgs, 3, side, side), generator=g), x2=torch.randn((imgs, 3, side, side), generator=g), y=y,
                dz=torch.randn((imgs, C_), generator=g), dfeat=0.01 * torch.randn((imgs, D), generator=g),
                m=1e-3 * torch.randn(nf, generator=g), v=1e-6 * torch.rand(nf, generator=g),
                scores=torch.rand((16, C_), generator=g), labels=(torch.rand((16, C_), generator=g) < 0.5).float())


def make_ctx(handle, e):
    """the fixed inputs of a handle on e's device; the two arena tensors of the folds are laid out by e itself (set_state of S1 /
    S2, then a clone of the state view), so e holds S2 afterwards"""
    model, precision, side, imgs, _ = HANDLES[handle]
    S0, T0, S1, S2 = states(model)
    ctx = types.SimpleNamespace(handle=handle, model=model, precision=precision, side=side, imgs=imgs, S0=S0, T0=T0, S1=S1,
                                device=e.device)
    for k, t in host_inputs(handle).items():
        setattr(ctx, k, t.to(e.device))
    arenas = []
    for st in (S1, S2):
        e.set_state(*st)
        arenas.append(e.state_tensor().clone())
    ctx.A1, ctx.A2 = arenas
    ctx.pos_weight = [1.0, 2.0, 0.5, 1.5, 1.0]
    ctx.active = [0.0, 1.0, 0.0, 0.0, 0.0]
    ctx.groups = [i % 2 for i in range(len(spec.entries(model, C_)))]
    ctx.loss = torch.zeros(1, device=e.device)
    ctx.hooks = hook_inputs(ctx, e)
    return ctx


# ---- 3. MUTATORS: (engine, ctx) -> None ----------------------------------------------------------------------------------------
# `moves`: what the call may leave different from (S0, T0): "w" the student's weights, "stats" its running statistics (and
# counters), "tw" / "tstats" the teacher's.  Every fused step is preceded by adam_reset (a control of its own below): the step
# reads the handle's hyper-parameters and moments, which must not depend on the cells that ran before.
def m_identity(e, ctx):
    pass


def m_set_state(e, ctx):
    e.set_state(*ctx.S1)


def m_view_copy(e, ctx):
    e.state_tensor().copy_(ctx.A1)


def m_view_mul(e, ctx):
    e.state_tensor().mul_(1.25)


def m_state_scale(e, ctx):
    e.state_scale(0.75)


def m_fedavg_fold(e, ctx):
    e.fedavg_fold([ctx.A1, ctx.A2], [3, 5])


def m_fed_w(e, ctx):
    e.fed_w([ctx.A1, ctx.A2], [0.3, 1.7])


def m_step_bce(e, ctx):
    e.adam_reset(LR)
    e.step_bce(ctx.x1, ctx.y, ctx.pos_weight, ctx.imgs, ctx.loss)


def m_step_stage1(e, ctx):
    B = ctx.imgs // 2
    e.adam_reset(LR)
    e.step_stage1(ctx.x1[:B], ctx.x2[:B], ctx.y[:B], ctx.active, 1, B, ctx.loss)


def m_step_rscfed(e, ctx):
    B = ctx.imgs // 2
    e.adam_reset(LR)
    e.step_rscfed(ctx.x1[:B], ctx.x2[:B], ctx.y[:B], ctx.pos_weight, ctx.active, 1, B, 0.9, 0.1, ctx.loss)


def m_fwd_backward_step(e, ctx):
    e.adam_reset(LR)
    e.forward_train(ctx.x1)
    e.backward_step(ctx.dz)


def _fwd_grads(e, ctx):
    e.zero_grad()
    e.forward_train(ctx.x1)
    e.backward_grads(ctx.dz)


def m_adam_step(e, ctx):
    e.adam_reset(LR)
    _fwd_grads(e, ctx)
    e.adam_step(LR)


def m_adamw_step(e, ctx):
    e.adam_reset(LR)
    _fwd_grads(e, ctx)
    e.adamw_step(LR)


def m_sgd_step(e, ctx):
    e.sgd_reset(LR, 0.9)
    _fwd_grads(e, ctx)
    e.sgd_step(LR, 0.9)


def m_adam_step_groups(e, ctx):
    e.adam_reset(LR)
    _fwd_grads(e, ctx)
    e.optim_groups(ctx.groups, 2)
    e.adam_step_groups([(LR, (0.9, 0.999), 1e-8, 0.0), (2 * LR, (0.8, 0.99), 1e-8, 1e-3)])
    e.optim_groups(None, 0)


def m_adamw_step_groups(e, ctx):
    e.adam_reset(LR)
    _fwd_grads(e, ctx)
    e.optim_groups(ctx.groups, 2)
    e.adamw_step_groups([(LR, (0.9, 0.999), 1e-8, 1e-2), (2 * LR, (0.8, 0.99), 1e-8, 0.0)])
    e.optim_groups(None, 0)


def m_sgd_step_groups(e, ctx):
    e.sgd_reset(LR, 0.9)
    _fwd_grads(e, ctx)
    e.optim_groups(ctx.groups, 2)
    e.sgd_step_groups([(LR, 0.9, 0.0, 0.0, False), (2 * LR, 0.0, 0.0, 1e-3, False)])
    e.optim_groups(None, 0)


def m_forward_train(e, ctx):
    e.forward_train(ctx.x1)


def m_forward_train_frozen(e, ctx):
    e.bn_freeze(True)
    e.forward_train(ctx.x1)
    e.bn_freeze(False)


def m_teacher_snapshot(e, ctx):
    e.teacher_snapshot()


def m_teacher_axpby(e, ctx):
    e.teacher_axpby(0.9, 0.1)


def m_teacher_ema_params(e, ctx):
    e.teacher_ema_params(0.9)


def m_teacher_swap(e, ctx):
    e.teacher_swap()


def m_adam_reset(e, ctx):
    e.adam_reset(LR)


def m_sgd_reset(e, ctx):
    e.sgd_reset(LR, 0.9)


def m_set_optim_state(e, ctx):
    e.set_optim_state(3, ctx.m, ctx.v)


def m_forward_eval(e, ctx):
    e.forward_eval(ctx.x1)


def m_eval_metrics(e, ctx):
    e.eval_metrics(ctx.scores, ctx.labels)


_ALL = frozenset({"w", "stats"})
_T = frozenset({"tw", "tstats"})
# name -> (callable, moves)
MUTATORS = {
    "identity": (m_identity, frozenset()),
    "set_state": (m_set_state, _ALL),
    "view_copy": (m_view_copy, _ALL),
    "view_mul": (m_view_mul, _ALL),
    "state_scale": (m_state_scale, _ALL),
    "fedavg_fold": (m_fedavg_fold, _ALL),
    "fed_w": (m_fed_w, _ALL),
    "step_bce": (m_step_bce, _ALL),
    "step_stage1": (m_step_stage1, _ALL),
    "step_rscfed": (m_step_rscfed, _ALL | _T),
    "fwd_backward_step": (m_fwd_backward_step, _ALL),
    "adam_step": (m_adam_step, _ALL),
    "adamw_step": (m_adamw_step, _ALL),
    "sgd_step": (m_sgd_step, _ALL),
    "adam_step_groups": (m_adam_step_groups, _ALL),
    "adamw_step_groups": (m_adamw_step_groups, _ALL),
    "sgd_step_groups": (m_sgd_step_groups, _ALL),
    "forward_train": (m_forward_train, frozenset({"stats"})),
    "forward_train_frozen": (m_forward_train_frozen, frozenset()),
    "teacher_snapshot": (m_teacher_snapshot, _T),
    "teacher_axpby": (m_teacher_axpby, _T),
    "teacher_ema_params": (m_teacher_ema_params, frozenset({"tw"})),
    "teacher_swap": (m_teacher_swap, _ALL | _T),
    "adam_reset": (m_adam_reset, frozenset()),
    "sgd_reset": (m_sgd_reset, frozenset()),
    "set_optim_state": (m_set_optim_state, frozenset()),
    "forward_eval": (m_forward_eval, frozenset()),
    "eval_metrics": (m_eval_metrics, frozenset()),
}
# mutators whose callable calls a student-class entry point although nothing may move (the ledger test pins this set)
MOVES_NOTHING_BY_DESIGN = {"forward_train_frozen"}
SUBSET_224 = (("set_state", "view_mul", "adam_step", "step_bce", "teacher_snapshot", "teacher_swap"), ("a", "b", "c"))


# ---- 4. READERS: (engine, ctx) -> tuple of tensors -----------------------------------------------------------------------------
def r_eval(e, ctx):
    """(a) eval affine, forward planes or shadows, the stem_rows weight planes"""
    return tuple(t.clone() for t in e.forward_eval(ctx.x2))


def r_eval_teacher(e, ctx):
    """(b) the teacher's affine and shadows"""
    return tuple(t.clone() for t in e.forward_eval(ctx.x2, teacher=True))


def r_train_grads(e, ctx):
    """(c) forward copies, the data-gradient packs and their planes, the stem's data-gradient matrix.  zero_grad is a host flag."""
    e.zero_grad()
    f, z = e.forward_train(ctx.x1)
    dx = torch.full_like(ctx.x1, float("nan"))
    e.backward_grads(ctx.dz, ctx.dfeat, dx=dx)
    return f, z, e.grads(), dx


def r_train_grads_frozen(e, ctx):
    """(c) under frozen BatchNorm: reads the same copies and leaves the state where it is (warm, positive control)"""
    e.bn_freeze(True)
    try:
        return r_train_grads(e, ctx)
    finally:
        e.bn_freeze(False)


def r_step_stage1(e, ctx):
    """(d) the teacher forward on the side lane beside the student's; adam_reset fixes the moments and reads no derived copy"""
    B = ctx.imgs // 2
    loss = torch.zeros(1, device=ctx.device)
    e.adam_reset(LR)
    e.step_stage1(ctx.x1[:B], ctx.x2[:B], ctx.y[:B], ctx.active, 1, B, loss)
    flat, cnt = e.get_state()
    return loss, torch.from_numpy(flat), torch.from_numpy(cnt)


def hook_inputs(ctx, e):
    """operands of reader (e): per chosen conv a buffer that holds any operand or result of it (the larger map x the wider padded
    channel count: the hooks read and write at most that)"""
    n = e.debug_num_convs()
    info = [e.debug_conv_info(i) for i in range(n)]
    pick = {"stem": next(i for i, c in enumerate(info) if c["cin"] == 3)}
    if ctx.model == "Resnet18":
        pick["s1"] = next(i for i, c in enumerate(info) if c["k"] == 3 and c["stride"] == 1)
        pick["s2"] = next(i for i, c in enumerate(info) if c["k"] == 3 and c["stride"] == 2)
    else:               # EfficientNet-B0's dense convs are 1x1: one that widens (expand), one that narrows (project)
        pick["expand"] = next(i for i, c in enumerate(info) if c["k"] == 1 and c["cout"] > c["cin"] and c["cin"] != 3)
        pick["project"] = next(i for i, c in enumerate(info) if c["k"] == 1 and c["cout"] < c["cin"])
    g = torch.Generator().manual_seed(99)
    bf = ctx.precision == "bf16"
    out = {}
    for name, ci in pick.items():
        c = info[ci]
        numel = ctx.imgs * max(c["hin"] * c["win"], c["hout"] * c["wout"]) * max(c["cin_p"], c["cout_p"], 4)
        x, dy = torch.randn(numel, generator=g), torch.randn(numel, generator=g)
        if bf and name != "stem":
            x, dy = x.to(torch.bfloat16), dy.to(torch.bfloat16)
        out[name] = (ci, numel, x.to(e.device), dy.to(e.device))
    return out


def r_hooks(e, ctx):
    """(e) single kernels on the student's copies: raw forward and data gradient of the stem and two more convs"""
    outs = []
    dev = ctx.device
    if ctx.precision == "bf16":
        ci, numel, _, _ = ctx.hooks["stem"]
        o = torch.zeros(numel, device=dev, dtype=torch.bfloat16)
        e.debug_pw_fwd(ci, ctx.x1, o, ctx.imgs)
        outs.append(o)
        for name in ("expand", "project"):
            ci, numel, x, dy = ctx.hooks[name]
            for op in (0, 1):
                o = torch.zeros(numel, device=dev, dtype=torch.bfloat16)
                e.debug_pw(op, ci, x if op == 0 else None, dy if op == 1 else None, o, ctx.imgs)
                outs.append(o)
        return tuple(outs)
    for name, (ci, numel, x, dy) in ctx.hooks.items():
        for op in (0, 1):
            o = torch.zeros(numel, device=dev)
            e.debug_conv(op, ci, x if op == 0 else None, dy if op == 1 else None, o, ctx.imgs)
            outs.append(o)
    if ctx.model == "Resnet18":
        ci, numel, x, dy = ctx.hooks["s2"]
        o = torch.zeros(numel, device=dev)
        e.debug_block_dgrad(2, dy, x, o, ctx.imgs)
        outs.append(o)
    return tuple(outs)


def r_state(e, ctx):
    """(f) the state itself, through both read paths"""
    flat, cnt = e.get_state()
    return torch.from_numpy(flat), torch.from_numpy(cnt), e.state_tensor().clone()


_W = frozenset({"w"})
# name -> (callable, what each returned tensor depends on: one set per tensor, a single set for all of them, None for a tensor that
# is compared between the handles only -- the counters, which a step bumps whatever the weights are)
READERS = {
    "a": (r_eval, (_ALL,)),
    "b": (r_eval_teacher, (_T,)),
    "c": (r_train_grads, (_W,)),                              # a batch-statistics forward reads no running statistics
    # the loss of a step reads the student's weights and the whole teacher; the state it leaves holds the running statistics too
    "d": (r_step_stage1, (_W | _T, _ALL | _T, None)),
    "e": (r_hooks, (_W,)),
    "f": (r_state, (_ALL, None, _ALL)),
}


def reads(reader, i):
    """what output i of a reader depends on (None: nothing is claimed)"""
    outs = READERS[reader][1]
    return outs[0] if len(outs) == 1 else outs[i]


def affects(mutator, reader):
    """True: the mutator moves something the reader reads.  Per returned tensor: where the mutator moves what the tensor depends
    on, it must differ from the reader's output at (S0, T0); where not, it must be the same bits."""
    return any(o is not None and MUTATORS[mutator][1] & o for o in READERS[reader][1])


def cells(handle):
    """the (mutator, reader) cells of a handle"""
    if handle == "r18_224":
        return [(m, r) for m in SUBSET_224[0] for r in SUBSET_224[1]]
    return [(m, r) for m in MUTATORS for r in READERS]
