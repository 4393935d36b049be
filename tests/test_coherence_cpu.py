"""The ledger behind tests/test_coherence_gpu.py, checked without a GPU: every fm_* entry point of include/fedmlp_hip.h has a class
(tests/coherence_cases.FM_CLASS), every Engine wrapper bumps the version counters its class demands, every state-changing entry
point is in the matrix or excused by name, and every caller of a state-changing Engine method in local_training.py / optim.py
tells the net (mark_trained), and csrc/engine.hip assigns its staleness flags only in the helpers and remake functions made for it.
Sources are read with ast (engine.hip with re); nothing is imported from the library."""
import ast
import os
import re

from tests import coherence_cases as CC

LEDGER = CC.engine_ledger()
MOVING = ("student", "both")


def _wrappers():
    """(Engine method, fm name, class) for every header entry point a wrapper calls directly"""
    return [(m, fm, CC.FM_CLASS[fm]) for m, rec in LEDGER.items() for fm in sorted(rec["fm"]) if fm in CC.FM_CLASS]


def test_every_entry_point_has_exactly_one_class():
    declared = CC.header_entry_points()
    assert len(declared) == len(set(declared)) and len(declared) >= 80, len(declared)
    assert set(CC.FM_CLASS) == set(declared), (sorted(set(declared) - set(CC.FM_CLASS)), sorted(set(CC.FM_CLASS) - set(declared)))
    assert set(CC.FM_CLASS.values()) == {"student", "teacher", "both", "work", "pure"}
    assert CC.FM_CLASS["fm_state_device"] == "student" and CC.FM_CLASS["fm_teacher_swap"] == CC.FM_CLASS["fm_step_rscfed"] == "both"


def test_engine_calls_nothing_the_headers_do_not_declare():
    for m, rec in LEDGER.items():
        for fm in rec["fm"]:
            assert fm in CC.FM_CLASS or fm.startswith("fm_debug_"), (m, fm)
    reached = {fm for _, fm, _ in _wrappers()}
    # not wrapped by Engine: fm_last_error (read by _lib.check), fm_version (the build's import check) and two host-only queries
    assert set(CC.FM_CLASS) - reached == {"fm_last_error", "fm_version", "fm_feature_dim", "fm_mfma_products"}, \
        sorted(set(CC.FM_CLASS) - reached)
    assert all(CC.FM_CLASS[f] == "pure" for f in set(CC.FM_CLASS) - reached)


def test_wrappers_bump_what_their_class_demands():
    assert set(CC.STATS_ONLY) == {"fm_forward_train"}
    seen = {"weights": 0, "plain": 0, "none": 0}
    for m, fm, cls in _wrappers():
        _, enq = CC.closed(LEDGER, m, through_wrappers=False)
        if cls in MOVING and fm not in CC.STATS_ONLY:
            assert "weights" in enq, f"Engine.{m} calls {fm} ({cls}) without self._enqueue(weights=True)"
            seen["weights"] += 1
        elif cls in ("teacher", "work") or fm in CC.STATS_ONLY:
            assert enq, f"Engine.{m} calls {fm} ({cls}) without self._enqueue()"
            if fm in CC.STATS_ONLY:
                assert LEDGER[m]["enqueue"] == {"plain"}, (m, fm)
            seen["plain"] += 1
    for m, rec in LEDGER.items():
        classes = {CC.FM_CLASS[fm] for fm in rec["fm"] if fm in CC.FM_CLASS}
        if classes == {"pure"}:
            assert not rec["enqueue"], f"Engine.{m} is a host-only query and calls self._enqueue"
            seen["none"] += 1
    assert seen["weights"] >= 20 and seen["plain"] >= 25 and seen["none"] >= 15, seen


def _class_of_methods(methods):
    fm = set()
    for m in methods:
        fm |= CC.closed(LEDGER, m)[0]
    return fm, {CC.FM_CLASS[f] for f in fm if f in CC.FM_CLASS}


def test_every_state_changing_entry_point_is_in_the_matrix():
    assert set(CC.NOT_IN_MATRIX) == {"fm_fedavg_allreduce", "fm_counters", "fm_step_stage2", "fm_step_fixmatch", "fm_step_fedlsr",
                                     "fm_step_fednoro", "fm_step_cbafed"}
    assert all(isinstance(r, str) and len(r) > 10 for r in CC.NOT_IN_MATRIX.values())
    covered = set()
    for name, (fn, moves) in CC.MUTATORS.items():
        methods = CC.engine_methods_of(fn)
        assert methods <= set(LEDGER), (name, methods - set(LEDGER))
        fm, classes = _class_of_methods(methods)
        covered |= fm
        student = bool(classes & {"student", "both"})
        teacher = bool(classes & {"teacher", "both"})
        if name in CC.MOVES_NOTHING_BY_DESIGN:
            assert not moves and student, name
            continue
        # a mutator moves the student's (teacher's) state exactly when it calls a student- (teacher-) class entry point
        assert bool(moves & {"w", "stats"}) == student, (name, moves, classes)
        assert bool(moves & {"tw", "tstats"}) == teacher, (name, moves, classes)
    assert CC.MOVES_NOTHING_BY_DESIGN == {"forward_train_frozen"}
    reachable = {fm for _, fm, cls in _wrappers() if cls in ("student", "teacher", "both")}
    missing = reachable - covered - set(CC.NOT_IN_MATRIX)
    assert not missing, f"state-changing entry points in neither MUTATORS nor NOT_IN_MATRIX: {sorted(missing)}"
    assert not (covered & set(CC.NOT_IN_MATRIX)), covered & set(CC.NOT_IN_MATRIX)


def test_readers_change_nothing_they_should_not():
    for name, (fn, reads) in CC.READERS.items():
        _, classes = _class_of_methods(CC.engine_methods_of(fn))
        # (c) runs a train forward, (d) a whole step, (f) takes the state view: the only readers that call a student-class function
        assert bool(classes & {"student", "both", "teacher"}) == (name in ("c", "d", "f")), (name, classes)


def test_affects_table():
    assert CC.affects("set_state", "a") and CC.affects("teacher_swap", "b") and CC.affects("step_rscfed", "b")
    assert CC.affects("teacher_ema_params", "d") and CC.affects("forward_train", "f") and CC.affects("forward_train", "a")
    assert not CC.affects("forward_train", "c") and not CC.affects("forward_train", "e")      # running statistics only
    assert not CC.affects("teacher_axpby", "a") and not CC.affects("teacher_snapshot", "f")
    for r in CC.READERS:
        for m in ("identity", "forward_train_frozen", "adam_reset", "sgd_reset", "set_optim_state", "forward_eval", "eval_metrics"):
            assert not CC.affects(m, r)
    n = sum(CC.affects(m, r) for m in CC.MUTATORS for r in CC.READERS)
    assert 0 < n < len(CC.MUTATORS) * len(CC.READERS)
    assert len(CC.cells("r18_224")) == 18 and len(CC.cells("r18_64")) == len(CC.MUTATORS) * len(CC.READERS)


# ---- the staleness flags of csrc/engine.hip ----------------------------------------------------------------------
FLAGS = ("ev_dirty", "fwd_dirty", "dgrad_dirty", "stem_dpack_stale")
RAISED_IN = {"net_changed": {"ev_dirty", "fwd_dirty"}, "student_copies_stale": {"dgrad_dirty", "stem_dpack_stale"}}
CLEARED_IN = {"ensure_eval_affine": {"ev_dirty"}, "ensure_fwd_shadows": {"fwd_dirty"}, "ensure_packed": {"dgrad_dirty"},
              "ensure_stem_dpack": {"stem_dpack_stale"}}
# who says "a state changed": the entry points and graph functions of the issue's list, and the helper that calls the other
SAYS_SO = {"net_changed": {"weights_stepped", "fold_states", "fm_set_state", "fm_state_device", "fm_state_scale", "fm_fedavg_allreduce",
                           "forward_train", "eff_forward_train", "fm_teacher_snapshot", "fm_teacher_axpby", "fm_teacher_ema_params"},
           "student_copies_stale": {"net_changed", "fm_teacher_swap"}}


def _engine_functions(text):
    """(name, body) of every function of a source whose definitions open with a `{` alone in column 0 and close with a `}` there"""
    out, head, name, body = [], None, None, None
    for line in text.splitlines():
        if name is None:
            if line == "{" and head:
                name, body = re.match(r"[^(]*?(\w+)\s*\(", head).group(1), []
            elif line[:1] not in ("", " ", "\t", "/", "#", "}"):
                head = line
        elif line == "}":
            out.append((name, "\n".join(body)))
            head = name = None
        else:
            body.append(line)
    return out


_ASSIGNS = re.compile(r"(?:\.|->)\s*(%s)\s*[|&^]?=(?!=)\s*([^;]*);" % "|".join(FLAGS))


def flag_assignments(text):
    """[(function, flag, right-hand side)] of every assignment to a staleness flag through an object (`x.flag =`, `x->flag =`)"""
    return [(fn, m.group(1), m.group(2).strip()) for fn, body in _engine_functions(text) for m in _ASSIGNS.finditer(body)]


def check_flag_sites(text):
    sites = flag_assignments(text)
    assert len(sites) == len(_ASSIGNS.findall(text)), "a staleness flag is assigned outside every function _engine_functions sees"
    raised, cleared = {}, {}
    for fn, flag, rhs in sites:
        assert rhs in ("true", "false"), f"{fn}: {flag} = {rhs}: a staleness flag takes a literal, in its helper or its remake function"
        (raised if rhs == "true" else cleared).setdefault(fn, set()).add(flag)
    assert raised == RAISED_IN, f"staleness flags are raised outside the helpers (or a helper lost one): {raised}"
    assert cleared == CLEARED_IN, f"staleness flags are cleared outside the functions that remake the copies: {cleared}"


def _engine_source():
    with open(os.path.join(CC.ROOT, "fedmlp_amd", "csrc", "engine.hip")) as f:
        return f.read()


def test_staleness_flags_are_raised_by_the_helpers_and_cleared_by_the_remakes():
    """What the GPU matrix cannot reach (fm_fedavg_allreduce needs a communicator) is held against the source: a flag is assigned
    `true` only inside net_changed / student_copies_stale, `false` only inside the function that remakes the copy it guards, and
    the helpers are called by exactly the functions that move a state.  The check itself is shown to see a hand-set flag."""
    text = _engine_source()
    for flag in FLAGS:                           # each is a member with a default, and each is assigned somewhere
        assert len(re.findall(r"\bbool %s = true;" % flag, text)) == 1, flag
    for gone in ("wpack_dirty", "twb_dirty", "ensure_teacher_shadow", "SplitJobBM", "sp_off", "bm_off"):
        assert gone not in text, gone
    check_flag_sites(text)
    fns = dict(_engine_functions(text))
    assert len(fns) > 150 and set(RAISED_IN) | set(CLEARED_IN) | set().union(*SAYS_SO.values()) <= set(fns)
    for helper, callers in SAYS_SO.items():
        got = {fn for fn, body in fns.items() if re.search(r"\b%s\(" % helper, body)}
        assert got == callers, (helper, sorted(got ^ callers))
    # the negative control: one entry point setting a flag by hand, as fm_fedavg_allreduce did, must be seen
    by_hand = text.replace("    net_changed(e, e->student);\n    if (!e->comm) return FM_OK;",
                           "    e->student.ev_dirty = true; e->student.fwd_dirty = true;\n    if (!e->comm) return FM_OK;")
    assert by_hand != text
    try:
        check_flag_sites(by_hand)
    except AssertionError as err:
        assert "fm_fedavg_allreduce" in str(err)
    else:
        raise AssertionError("a flag set by hand in fm_fedavg_allreduce went unnoticed")


# ---- callers of mark_trained ---------------------------------------------------------------------------------------------------
def _moving_methods():
    """Engine methods through which a student / both entry point is reached, minus the statistics-only forward"""
    out = set()
    for m in LEDGER:
        fm, _ = CC.closed(LEDGER, m)
        if any(CC.FM_CLASS.get(f) in MOVING and f not in CC.STATS_ONLY for f in fm):
            out.add(m)
    return out


def _functions(path):
    with open(path) as f:
        tree = ast.parse(f.read())
    return [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]


def _method_calls(fn):
    return {n.func.attr for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}


def test_callers_of_state_changing_methods_mark_the_net_trained():
    moving = _moving_methods() - {"state_tensor", "_state_ptrs", "state_dist"}     # (reading the view changes nothing)
    assert {"step_bce", "step_stage1", "backward_step", "adam_step", "sgd_step_groups", "teacher_swap", "set_state"} <= moving
    checked = 0
    for rel in ("local_training.py", "optim.py"):
        fns = _functions(os.path.join(CC.ROOT, "fedmlp_amd", rel))
        for fn in fns:
            hits = _method_calls(fn) & moving
            if not hits:
                continue
            checked += 1
            if "mark_trained" in _method_calls(fn):
                continue
            # a one-line hook (optim.py's _engine_step*): every function of the module that calls it must mark instead
            callers = [g for g in fns if g is not fn and fn.name in _method_calls(g)]
            assert callers and all("mark_trained" in _method_calls(g) for g in callers), \
                f"{rel}: {fn.name} calls Engine.{sorted(hits)} and neither it nor its callers call mark_trained()"
    assert checked >= 12, checked
