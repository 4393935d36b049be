"""The RoFL client's two entry points live in include/fedmlp_hip_rofl.h, with a ctypes table (_lib.ROFL_SYMBOLS) and wrappers
(engine.RoflHeads, a base of Engine) of their own: include/fedmlp_hip.h's list is closed (tests/test_host_cpu.py,
tests/test_coherence_cpu.py and tests/test_step_refusals_gpu.py enumerate it by name).  The rules those tests hold for the main
header are held for the two here: header = table = exports, argument counts, a class for each (the step moves the student: its
wrapper must bump weights_version; the head only enqueues work), and the trainer that calls the step tells the net."""
import ast
import ctypes as C
import os
import re

import pytest

from fedmlp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS = {"fm_step_rofl": "student", "fm_loss_rofl": "work"}


def _declared(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m: a for m, a in re.findall(r"^int\s+(fm_\w+)\s*\(([^;]*)\);", text, flags=re.M | re.S)}


def test_header_table_and_exports_agree():
    decl = _declared("fedmlp_hip_rofl.h")
    assert set(decl) == set(_lib.ROFL_SYMBOLS) == set(CLASS)
    assert not set(decl) & set(_declared("fedmlp_hip.h")) and not set(_lib.ROFL_SYMBOLS) & set(_lib.SYMBOLS)
    for name, args in decl.items():
        res, argtypes = _lib.ROFL_SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == len(args.split(",")), name       # one ctypes entry per C argument
    assert len(_lib.ROFL_SYMBOLS["fm_loss_rofl"][1]) == 17 and len(_lib.ROFL_SYMBOLS["fm_step_rofl"][1]) == 14
    assert _lib.ROFL_SYMBOLS["fm_loss_rofl"][1][13] is C.c_int64 and _lib.ROFL_SYMBOLS["fm_step_rofl"][1][12] is C.c_int64    # N
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfedmlp_hip.so not built (run `make`)")
    lib = _lib.load()
    for name, (res, argtypes) in _lib.ROFL_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == argtypes, name


def _methods(cls_name):
    with open(os.path.join(ROOT, "fedmlp_amd", "engine.py")) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    return cls, {fn.name: fn for fn in cls.body if isinstance(fn, ast.FunctionDef)}


def _self_calls(fn):
    return {n.func.attr for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)
            and isinstance(n.func.value, ast.Name) and n.func.value.id == "self"}


def _fm_names(fn):
    return {n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute) and n.attr.startswith("fm_")}


def _enqueue_kinds(fn):
    out = set()
    for n in ast.walk(fn):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "_enqueue":
            out.add("weights" if any(k.arg == "weights" and getattr(k.value, "value", None) is True for k in n.keywords) else "plain")
    return out


def test_wrappers_bump_what_their_class_demands():
    """RoflHeads is a base of Engine; step_rofl reaches fm_step_rofl through Engine._step (self._enqueue(weights=True)) and
    loss_rofl reaches fm_loss_rofl through Engine._head (self._enqueue()), and neither enqueues on its own"""
    engine_cls, engine = _methods("Engine")
    assert [b.id for b in engine_cls.bases] == ["RoflHeads"]
    _, rofl = _methods("RoflHeads")
    assert {m for m, fn in rofl.items() if _fm_names(fn)} == {"step_rofl", "loss_rofl"}
    assert _fm_names(rofl["step_rofl"]) == {"fm_step_rofl"} and _fm_names(rofl["loss_rofl"]) == {"fm_loss_rofl"}
    assert "_step" in _self_calls(rofl["step_rofl"]) and "_head" in _self_calls(rofl["loss_rofl"])
    assert _enqueue_kinds(engine["_step"]) == {"weights"} and _enqueue_kinds(engine["_head"]) == {"plain"}
    assert "_check_stream" in _self_calls(engine["_step"]) and "_check_stream" in _self_calls(engine["_head"])
    assert CLASS["fm_step_rofl"] == "student" and CLASS["fm_loss_rofl"] == "work"
    # no other Engine method names a RoFL entry point
    assert not any(_fm_names(fn) & set(CLASS) for fn in engine.values())


def test_the_trainer_marks_the_net_trained():
    with open(os.path.join(ROOT, "fedmlp_amd", "local_training.py")) as f:
        tree = ast.parse(f.read())
    fns = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]
    callers = [fn for fn in fns if "step_rofl" in {n.func.attr for n in ast.walk(fn) if isinstance(n, ast.Call)
                                                     and isinstance(n.func, ast.Attribute)}]
    assert [fn.name for fn in callers] == ["train_RoFL"]
    assert "mark_trained" in {n.func.attr for n in ast.walk(callers[0]) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}


def test_the_step_is_built_on_the_shared_skeleton():
    """fm_step_rofl goes through fused_step with the student-alone forward, so it raises no staleness flag of its own and its
    launch list around the head is fm_step_bce's"""
    with open(os.path.join(ROOT, "fedmlp_amd", "csrc", "engine.hip")) as f:
        text = f.read()
    body = text[text.index("int fm_step_rofl("):]
    body = body[:body.index("\n}\n")]
    assert "fused_step(e, StepFwd::Student" in body and "rofl_bad(" in body and "e->feat" in body
    assert "dirty" not in body and "net_changed" not in body
