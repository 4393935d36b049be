"""The order between the engine's two lanes under schedule perturbation, on a real MI355X.

The main lane (the caller's stream) and the side lane (teacher forward, weight gradients) are ordered by hand-placed events
only ("Lane protocol").  Here one lane is held back by a delay kernel (fm_debug_lane_delay) in front of ONE of its
launches, for longer than the whole two-step sequence takes, so that the other lane runs as far ahead as its event waits allow:
a missing wait then reads stale data or overwrites early, inside buffers the step owns, and the bits leave those of a one-stream
handle.  Every delay point of both lanes is visited, for every sequence that crosses the lanes.  The mutants (fm_debug_drop_wait)
switch one kind of wait off and show that the same sweep sees it.

Cases are cut by sequence, lane and position range so that each takes a few seconds; lane_delay.json (beside the other parity
reports, a copy under profiles/) records points, step time, delay, positions, seconds and detecting positions."""
import time

import numpy as np
import pytest
import torch

from fedmlp_amd import spec

pytestmark = pytest.mark.gpu

C_, HW, B = 5, 64, 6
LR = 3e-5
MASK = [0.0, 1.0, 0.0, 0.0, 0.0]
PW = [3.0, 1.5, 4.0, 2.0, 2.5]
MAX_DELAY_US = 20000                   # FM_LANE_DELAY_MAX_US
KINDS = ("side_begin", "side_guard", "side_join", "ev_in", "ev_t")
# the lane to hold back so that the OTHER lane runs past the missing wait: the lane whose event the wait is for
MUTANT_LANE = {"side_begin": 0, "side_guard": 1, "side_join": 1, "ev_in": 0, "ev_t": 1}
W3 = ("side_begin", "side_guard", "side_join")          # weight gradients on the side lane
W5 = KINDS                                              # ... and a teacher forward


# ---- the sequences: two consecutive steps each, different data per step (a stale read must not find the right values) ----
def _steps_stage1(e, d, out):
    lo = torch.zeros(2, device="cuda")
    for s in range(2):
        e.step_stage1(d["x1"][s], d["x2"][s], d["y"][s], MASK, 1, 8, lo[s:s + 1])
    out["loss"] = lo


def _steps_bce(e, d, out):
    lo = torch.zeros(2, device="cuda")
    for s in range(2):
        e.step_bce(d["x1"][s], d["y"][s], PW, 8, lo[s:s + 1])
    out["loss"] = lo


def _steps_rscfed(e, d, out):
    lo = torch.zeros(2, device="cuda")
    for s in range(2):
        e.step_rscfed(d["x1"][s], d["x2"][s], d["y"][s], PW, MASK, 1, 8, 0.9, 0.1, lo[s:s + 1])
    out["loss"] = lo


def _steps_split(e, d, out):
    """the split path of test_autograd_path_equals_across_stream_modes, twice"""
    for s in range(2):
        x1, x2 = d["x1"][s], d["x2"][s]
        e.zero_grad()
        feat, logits = e.forward_train(x1, x2)
        dx1, dx2 = torch.empty_like(x1), torch.empty_like(x2)
        e.backward_grads(d["dlogits"][s], d["dfeat"][s], dx=(dx1, dx2))
        e.forward_recompute(x1, x2)
        e.backward_grads(d["dlogits"][s])
        out[f"accumulated_grads{s}"] = e.grads()
        e.adam_step(LR)
        out[f"feat{s}"], out[f"logits{s}"], out[f"dx1_{s}"], out[f"dx2_{s}"] = feat, logits, dx1, dx2


class Seq:
    def __init__(self, name, model, steps, kinds, streams=0, precision="fp32", freeze=False, teacher_moves=False,
                 chunks=(2, 1)):
        self.name, self.model, self.steps, self.kinds = name, model, steps, kinds
        self.streams, self.precision, self.freeze, self.teacher_moves = streams, precision, freeze, teacher_moves
        self.chunks = chunks           # cases per lane (main, side): narrower ranges, never sparser ones
        self.max_images = 16 if model == "Resnet18" else 4 * B


R, E = "Resnet18", "Efficient_b0"
SEQS = [
    Seq("r18_stage1", R, _steps_stage1, W5),
    Seq("r18_bce", R, _steps_bce, W3),
    Seq("r18_rscfed", R, _steps_rscfed, W5, teacher_moves=True),
    Seq("r18_split", R, _steps_split, W3, chunks=(3, 1)),
    Seq("r18_split_bn_freeze", R, _steps_split, W3, freeze=True, chunks=(3, 1)),
    Seq("eff_f32_stage1", E, _steps_stage1, W5, chunks=(6, 2)),
    Seq("eff_f32_bce", E, _steps_bce, W3, chunks=(4, 1)),
    Seq("eff_bf16_stage1", E, _steps_stage1, W5, precision="bf16", chunks=(6, 2)),
    Seq("eff_bf16_bce", E, _steps_bce, W3, precision="bf16", chunks=(4, 1)),
    Seq("r18_stage1_teacher_only", R, _steps_stage1, ("ev_in", "ev_t"), streams=2),
]
SEQ = {s.name: s for s in SEQS}


def _data(model):
    g = torch.Generator().manual_seed(4400 + len(model))
    D = spec.FEATURE_DIM[model]
    d = {"x1": [], "x2": [], "y": [], "dlogits": [], "dfeat": []}
    for _ in range(2):
        d["x1"].append(torch.randn((B, 3, HW, HW), generator=g).cuda())
        d["x2"].append(torch.randn((B, 3, HW, HW), generator=g).cuda())
        d["y"].append((torch.rand((B, C_), generator=g) < 0.3).float().cuda())
        d["dlogits"].append(torch.randn((2 * B, C_), generator=g).cuda())
        d["dfeat"].append(torch.randn((2 * B, D), generator=g).cuda())
    return d


BN_MOMENTUM = {R: 0.1, E: 0.01}        # torchvision's / efficientnet-pytorch's, as the engine applies them


def _initial_state(e, x):
    """spec.init_state with every BatchNorm's running statistics set to the statistics of batch x.  With the initial 0 / 1 an
    eval-mode forward of the untrained EfficientNet-B0 loses its signal below fp32 resolution of the classifier's bias: the
    teacher's logits would be the same bits for every input, and a teacher forward that read a stale input or came too late for
    the loss head could not be told from a correct one."""
    flat, cnt = spec.init_state(e.model, C_, 1037)
    m = BN_MOMENTUM[e.model]
    e.stochastic = False
    e.bn_freeze(False)
    e.set_state(flat, cnt)
    e.forward_train(x)                 # one view: running <- (1 - m) running + m batch
    moved, _ = e.get_state()
    sd, sd1 = spec.flat_to_state_dict(e.model, C_, flat, cnt), spec.flat_to_state_dict(e.model, C_, moved, cnt)
    for k in sd:
        if k.endswith("running_mean") or k.endswith("running_var"):
            batch = (sd1[k].astype(np.float64) - (1.0 - m) * sd[k]) / m
            sd[k] = (np.maximum(batch, 0.0) if k.endswith("running_var") else batch).astype(np.float32)
    return spec.state_dict_to_flat(e.model, C_, sd)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _first_diff(got, want, describe=True):
    """None, or a text naming the first compared tensor that differs and (describe) its first differing entry, read back only now"""
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            if not np.array_equal(g, w):
                return f"{k}: {g.tolist()} != {w.tolist()}"
            continue
        if torch.equal(_bits(g), _bits(w)):
            continue
        if not describe:
            return k
        gh, wh = g.detach().cpu().numpy().ravel(), w.detach().cpu().numpy().ravel()
        bad = np.flatnonzero(gh.view(np.uint32) != wh.view(np.uint32))
        return f"{k}: {bad.size} of {gh.size} differ, first at {int(bad[0])}: {gh[bad[0]]!r} != {wh[bad[0]]!r}"
    return None


class Ctx:
    """One sequence's engine, reference, point counts and delay.  One at a time: the cases below come in sequence order."""

    def __init__(self, seq):
        from fedmlp_amd.engine import Engine
        self.seq, self.data = seq, _data(seq.model)
        # reference: the same sequence on a one-stream handle, once
        ref = Engine(seq.model, C_, HW, HW, seq.max_images, streams=1, precision=seq.precision)
        try:
            assert ref.stream_mode == 1
            flat, cnt = _initial_state(ref, self.data["x1"][0])
            self._prepare(ref)
            ref.set_state(flat, cnt)
            self.w0 = ref.state_tensor().clone()
            self.ref = self.run(ref)
            for k, v in self.ref.items():
                if not isinstance(v, np.ndarray) and v.dtype == torch.float32:
                    assert bool(torch.isfinite(v).all()), k
            assert not torch.equal(self.ref["state"], self.w0)
            # the undelayed two-step time, with events; the second run is the one-stream handle's own repeat
            self.reset(ref)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            again = {}
            seq.steps(ref, self.data, again)
            b.record()
            b.synchronize()
            self.step_ms = a.elapsed_time(b)
            key = "loss" if "loss" in again else "logits1"
            assert torch.equal(_bits(again[key]), _bits(self.ref[key])), "the one-stream handle does not repeat itself"
        finally:
            ref.close()
        self.delay_us = int(min(MAX_DELAY_US, 1.5 * self.step_ms * 1000.0))
        self.e = Engine(seq.model, C_, HW, HW, seq.max_images, streams=seq.streams, precision=seq.precision)
        # a handle that fell back to one stream would pass everything below vacuously
        assert self.e.stream_mode == seq.streams, f"asked for stream mode {seq.streams}, got {self.e.stream_mode}"
        self._prepare(self.e)
        self.e.set_state(flat, cnt)
        # count the delay points and the waits: one run with micros = 0
        self.e.debug_lane_delay(0, 0, 0)
        got = self.run(self.e)
        info = self.e.debug_lane_points(disarm=True)
        self.points, self.waits = info["points"], info["waits"]
        assert not info["fired"] and not any(info["skipped"].values())
        why = _first_diff(got, self.ref)
        assert why is None, f"{seq.name}, undelayed: {why}"
        assert {k for k in KINDS if self.waits[k]} == set(seq.kinds), (seq.name, self.waits)
        assert self.points[0] > 0 and self.points[1] > 0, self.points
        self.rec = REPORT.setdefault(seq.name, {})
        self.rec.update({"points": {"main": self.points[0], "side": self.points[1]}, "step_ms": round(self.step_ms, 3),
                         "delay_us": self.delay_us, "waits_per_run": {k: v for k, v in self.waits.items() if v}})
        self.rec.setdefault("positions_run", {"main": [], "side": []})
        self.rec.setdefault("seconds_per_case", {})
        self.rec.setdefault("detecting_positions", {})
        self.detected = {}             # kind -> {chunk: detecting positions}
        self.ran = {"main": set(), "side": set()}

    def _prepare(self, e):
        e.stochastic = False
        e.bn_freeze(self.seq.freeze)

    def reset(self, e):
        e.state_tensor().copy_(self.w0)
        e.counters(new=np.zeros(e.ni, np.int64))
        e.adam_reset(LR)
        e.teacher_snapshot()           # in every run: the teacher's shadows are stale, so the ev_in fork has something to protect

    def run(self, e):
        """reset, the two steps, everything compared (device tensors; counters on the host)"""
        self.reset(e)
        out = {}
        self.seq.steps(e, self.data, out)
        torch.cuda.synchronize()       # both lanes, whatever a mutant left unjoined
        out["state"] = e.state_tensor().clone()
        out["grads"] = e.debug_optim_arena(3).clone()
        out["counters"] = np.asarray(e.counters()).copy()
        if self.seq.teacher_moves:
            e.teacher_swap()
            out["teacher_state"] = e.state_tensor().clone()
            e.teacher_swap()
        return out

    def sweep(self, lane, positions, must_match):
        """The sequence with the delay at each of `positions` of `lane`: the positions whose bits differ from the reference"""
        e, differ = self.e, {}
        for p in positions:
            e.debug_lane_delay(lane, p, self.delay_us)
            t0 = time.perf_counter()
            got = self.run(e)          # reset (no delay point in it), the steps, a device synchronisation
            dt = time.perf_counter() - t0
            info = e.debug_lane_points(disarm=True)
            assert info["fired"], f"{self.seq.name}: lane {lane} never reached point {p} ({info['points']})"
            assert info["points"] == self.points, (info["points"], self.points)
            if must_match:
                assert dt * 1e6 >= self.delay_us, f"{self.seq.name} lane {lane} point {p}: {dt * 1e6:.0f} us < the delay {self.delay_us}"
            why = _first_diff(got, self.ref, describe=must_match)
            if why is not None:
                differ[p] = why
        return differ

    def close(self):
        torch.cuda.synchronize()
        self.e.close()


REPORT = {}
_CTX = []


def _ctx(name):
    if _CTX and _CTX[0].seq.name != name:
        _CTX.pop().close()
    if not _CTX:
        _CTX.append(Ctx(SEQ[name]))
    return _CTX[0]


@pytest.fixture(scope="module", autouse=True)
def _close_last():
    yield
    while _CTX:
        _CTX.pop().close()


def _chunk(points, k, n):
    return range(points * k // n, points * (k + 1) // n)


def _ranges(positions):
    """[[first, last], ..] of a set of positions"""
    out = []
    for p in sorted(positions):
        if out and p == out[-1][1] + 1:
            out[-1][1] = p
        else:
            out.append([p, p])
    return out


def _dump():
    import json
    import os
    from tests.test_local_training_gpu import _dump as dump_report
    dump_report(REPORT, "lane_delay.json")             # beside the other parity reports
    try:                               # the committed copy: best effort, a read-only tree is not a failure
        with open(os.path.join("profiles", "lane_delay.json"), "w") as f:
            json.dump(REPORT, f, indent=1)
    except OSError:
        pass


def _cases():
    out = []
    for s in SEQS:
        for lane in (0, 1):
            for k in range(s.chunks[lane]):
                out.append(pytest.param(("sweep", s.name, lane, k), id=f"{s.name}-{'main' if lane == 0 else 'side'}-{k}"))
        for kind in s.kinds:
            for k in range(s.chunks[MUTANT_LANE[kind]]):
                out.append(pytest.param(("mutant", s.name, kind, k), id=f"{s.name}-drop_{kind}-{k}"))
        out.append(pytest.param(("verdict", s.name, None, None), id=f"{s.name}-verdict"))
    return out


@pytest.mark.parametrize("case", _cases())
def test_lane_delay(case):
    """sweep:   the delay at every point of one lane's range; the reference's bits everywhere, and each delayed run lasts at
                least the delay (the kernel ran where it was asked to).
    mutant:  the same sweep, over the lane the wait orders against, with that one kind of wait switched off.
    verdict: the ranges that ran are the whole of 0 .. points - 1 on both lanes, and every wait kind the sequence executes was
             detected at one position at least -- else the sweep is blind there or the wait is redundant."""
    what, name, arg, k = case
    c = _ctx(name)
    seq, t0 = c.seq, time.perf_counter()
    if what == "sweep":
        lane = arg
        lname = "main" if lane == 0 else "side"
        rng = _chunk(c.points[lane], k, seq.chunks[lane])
        differ = c.sweep(lane, rng, must_match=True)
        c.ran[lname] |= set(rng)
        c.rec["positions_run"][lname] = _ranges(c.ran[lname])
        c.rec["seconds_per_case"][f"{lname}-{k}"] = round(time.perf_counter() - t0, 2)
        _dump()
        assert not differ, (f"{name}: holding the {lname} lane back changes the bits at {len(differ)} of {len(rng)} points: "
                            + "; ".join(f"point {p}: {w}" for p, w in list(differ.items())[:4]))
    elif what == "mutant":
        kind, lane = arg, MUTANT_LANE[arg]
        rng = _chunk(c.points[lane], k, seq.chunks[lane])
        c.e.debug_drop_wait(kind, True)
        try:
            differ = c.sweep(lane, rng, must_match=False)
            skipped = c.e.debug_lane_points()["skipped"]
        finally:
            c.e.debug_drop_wait(kind, False)
        assert skipped[kind] == c.waits[kind] and sum(skipped.values()) == skipped[kind], (skipped, c.waits)
        c.detected.setdefault(kind, {})[k] = sorted(differ)
        c.rec["detecting_positions"][kind] = sum(len(v) for v in c.detected[kind].values())
        c.rec["seconds_per_case"][f"drop_{kind}-{k}"] = round(time.perf_counter() - t0, 2)
        _dump()
    else:
        for lane, lname in ((0, "main"), (1, "side")):
            n = seq.chunks[lane]
            planned = sorted(p for j in range(n) for p in _chunk(c.points[lane], j, n))
            assert planned == list(range(c.points[lane])), f"{name}: the {lname} cases do not cover 0 .. {c.points[lane] - 1}"
            assert sorted(c.ran[lname]) == planned, f"{name}: not every {lname} point was run (run this sequence's cases together)"
        blind = []
        for kind in seq.kinds:
            got = c.detected.get(kind, {})
            assert len(got) == seq.chunks[MUTANT_LANE[kind]], f"{name}: not every drop_{kind} case was run"
            if not any(got.values()):
                blind.append(kind)
        if blind and len(blind) == len(seq.kinds):
            plain, held = _overlap_probe()
            assert held < plain + 0.5 * MAX_DELAY_US / 1000.0, \
                f"{name}: no mutant is seen because the lanes do not overlap on this machine: main lane {held:.2f} ms with the side lane held, {plain:.2f} ms without"
        assert not blind, f"{name}: no delay position detects the dropped wait(s) {blind}: the sweep is blind there, or the wait is redundant"


def _overlap_probe():
    """Do the lanes overlap on this machine at all?  A teacher-only handle with the ev_t wait dropped has nothing on the main
    lane that waits for the side lane: with the side lane held at its first point for the longest delay, a stage-1 step's main
    lane must end about when it does unheld.  -> (unheld ms, held ms) of the main lane, by events."""
    from fedmlp_amd.engine import Engine
    d = _data(R)
    e = Engine(R, C_, HW, HW, 16, streams=2)
    try:
        assert e.stream_mode == 2
        e.set_state(*spec.init_state(R, C_, 1037))
        e.adam_reset(LR)
        e.teacher_snapshot()
        lo = torch.zeros(1, device="cuda")

        def main_ms():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            e.step_stage1(d["x1"][0], d["x2"][0], d["y"][0], MASK, 1, 8, lo)
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        main_ms()
        plain = main_ms()
        e.debug_drop_wait("ev_t", True)
        try:
            e.debug_lane_delay(1, 0, MAX_DELAY_US)
            held = main_ms()
            assert e.debug_lane_points(disarm=True)["fired"]
        finally:
            e.debug_drop_wait("ev_t", False)
            torch.cuda.synchronize()
    finally:
        e.close()
    REPORT["overlap_probe"] = {"main_lane_ms": round(plain, 3), "main_lane_ms_side_held": round(held, 3),
                               "side_held_us": MAX_DELAY_US}
    _dump()
    return plain, held


def test_the_lanes_overlap():
    """The stimulus works on this machine: holding the side lane does not hold a main lane that does not wait for it."""
    plain, held = _overlap_probe()
    assert held < plain + 0.5 * MAX_DELAY_US / 1000.0, \
        f"the lanes do not overlap: the main lane took {held:.2f} ms with the side lane held for {MAX_DELAY_US / 1000} ms, {plain:.2f} ms without"


def test_hook_contract():
    """Bad arguments are refused with FM_ERR_ARG and a text, arm nothing and enqueue nothing; a plain step afterwards gives the
    one-stream handle's bits."""
    from fedmlp_amd.engine import Engine
    from fedmlp_amd._lib import FmError
    d = _data(R)
    flat, cnt = spec.init_state(R, C_, 1037)
    outs = []
    for streams in (1, 0):
        e = Engine(R, C_, HW, HW, 16, streams=streams)
        try:
            assert e.stream_mode == streams
            e.set_state(flat, cnt)
            e.adam_reset(LR)
            e.teacher_snapshot()
            bad = [lambda: e.debug_lane_delay(2, 0, 100), lambda: e.debug_lane_delay(-1, 0, 100),
                   lambda: e.debug_lane_delay(0, -1, 100), lambda: e.debug_lane_delay(0, 0, MAX_DELAY_US + 1),
                   lambda: e.debug_lane_delay(0, 0, -1), lambda: e.debug_drop_wait(len(KINDS)), lambda: e.debug_drop_wait(-1)]
            if streams == 1:
                bad.append(lambda: e.debug_lane_delay(1, 0, 100))
            for call in bad:
                with pytest.raises(FmError, match="error -1: bad argument: fm_debug_"):
                    call()
            lo = torch.zeros(1, device="cuda")
            t0 = time.perf_counter()
            e.step_stage1(d["x1"][0], d["x2"][0], d["y"][0], MASK, 1, 8, lo)
            torch.cuda.synchronize()
            info = e.debug_lane_points()
            assert info["points"] == (0, 0) and not info["fired"] and not any(info["skipped"].values()), info
            outs.append((lo.clone(), e.state_tensor().clone(), e.debug_optim_arena(3).clone(), time.perf_counter() - t0))
        finally:
            e.close()
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(_bits(a), _bits(b))


def test_stage1_at_the_benchmarked_shape_equals_across_stream_modes():
    """ResNet-18 at 224 x 224, two views of 16: three stage-1 steps in stream modes 0, 1 and 2 leave the same bits.  This is
    where the stem's row kernel, the ring weight gradient and weight gradients longer than the data-gradient chain are live;
    undelayed, with the timing the machine gives."""
    from fedmlp_amd.engine import Engine
    hw, Bb = 224, 16
    g = torch.Generator().manual_seed(4501)
    xs = [(torch.randn((Bb, 3, hw, hw), generator=g).cuda(), torch.randn((Bb, 3, hw, hw), generator=g).cuda(),
           (torch.rand((Bb, C_), generator=g) < 0.3).float().cuda()) for _ in range(3)]
    flat, cnt = spec.init_state(R, C_, 1037)
    outs = []
    for streams in (0, 1, 2):
        e = Engine(R, C_, hw, hw, 2 * Bb, streams=streams)
        try:
            assert e.stream_mode == streams, f"asked for stream mode {streams}, got {e.stream_mode}"
            e.set_state(flat, cnt)
            e.adam_reset(LR)
            e.teacher_snapshot()
            lo = torch.zeros(3, device="cuda")
            for s, (x1, x2, y) in enumerate(xs):
                e.step_stage1(x1, x2, y, MASK, 1, Bb, lo[s:s + 1])
            torch.cuda.synchronize()
            outs.append({"loss": lo, "state": e.state_tensor().clone(), "grads": e.debug_optim_arena(3).clone(),
                         "counters": np.asarray(e.counters()).copy()})
        finally:
            e.close()
    assert bool(torch.isfinite(outs[0]["loss"]).all())
    for k in (1, 2):
        why = _first_diff(outs[k], outs[0])
        assert why is None, f"stream mode {(0, 1, 2)[k]} against mode 0: {why}"
