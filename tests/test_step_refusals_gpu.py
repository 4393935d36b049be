"""What every fused step (fm_step_*) and every loss head on caller tensors (fm_loss_*) answers to ONE bad argument: FM_ERR_ARG and
the fm_last_error() text below, copied from the entry points as they were written out one by one, before the steps shared a
skeleton and the heads their validators.  A refusal comes before anything is enqueued: after each refused fm_step_* the engine's
state and counters are the bits they were.  Nothing here launches a kernel; the entry points are called through ctypes, as
tests/test_tag_kernels_gpu.py does, on one ResNet-18 engine at 64 x 64 with max_images = 4 and C = 5."""
import ctypes as C

import numpy as np
import pytest
import torch

from fedmlp_amd import _lib, spec

pytestmark = pytest.mark.gpu

NC, HW, MAXB = 5, 64, 4
NULL = "null"
B1 = "B exceeds max_images"
B2 = "2*B exceeds max_images"
BGE1 = "B >= 1"
NORM = "B, annotation_num, bs_norm >= 1; bs_norm * annotation_num < 2^24"
CLASSES = "the head needs at least one active and one missing class"
MASK = ("a requires_grad mask is installed and the fused steps train every layer: use the autograd path (fm_forward_train, "
        "fm_backward_grads, fm_adam_step_groups / fm_adamw_step_groups / fm_sgd_step_groups), or restore the default mask with "
        "fm_set_trainable")
PW, AM = [1.0, 2.0, 1.5, 1.0, 3.0], [0.0, 1.0, 0.0, 1.0, 0.0]
ALL, NONE = [1.0] * NC, [0.0] * NC
TAO = [0.5] * NC
P = "ptr"                                # a required device pointer (never read: every call here is refused)

# entry point -> its arguments after the engine, in order; (views the batch bound counts, or None for a head alone)
SIGS = {
    "fm_step_bce": (1, dict(x=P, y=P, B=2, pw=PW, bs=2, loss=P)),
    "fm_step_stage1": (2, dict(x1=P, x2=P, y=P, B=2, am=AM, ann=2, bs=2, loss=P)),
    "fm_step_stage2": (1, dict(x=P, y=P, distill=P, B=2, loss=P)),
    "fm_step_fixmatch": (2, dict(xw=P, xs=P, y=P, B=2, pw=PW, pwu=PW, am=AM, ann=2, bs=2, loss=P)),
    "fm_step_fedlsr": (2, dict(x1=P, x2=P, y=P, B=2, pw=PW, mix1=C.c_float(0.25), beta=C.c_float(0.4), loss=P)),
    "fm_step_rscfed": (1, dict(x1=P, x2=P, y=P, B=2, pw=PW, am=AM, ann=2, bs=2, wt=C.c_float(0.999), ws=C.c_float(0.001), loss=P)),
    "fm_step_fednoro": (1, dict(x=P, y=P, B=2, am=AM, w_kd=C.c_float(0.8), loss=P)),
    "fm_step_cbafed": (1, dict(x=P, y=P, B=2, am=AM, ann=2, bs=2, tao=None, pw_dev=P, counts=None, loss=P)),
    "fm_loss_fedlsr": (None, dict(z=P, y=P, pw=PW, mix1=C.c_float(0.25), beta=C.c_float(0.4), B=2, dz=P, loss=P)),
    "fm_loss_fedirm_sup": (None, dict(z=P, y=P, pw=PW, am=AM, ann=2, bs=2, B=2, rel=None, dz=P, loss=P)),
    "fm_loss_fedirm_rel": (None, dict(z=P, zt=P, y=P, pw=PW, am=AM, ann=2, bs=2, cw=C.c_float(0.5), target=P, B=2, rel=None, dz=P,
                                      loss=P)),
    "fm_loss_rscfed": (None, dict(z=P, zt=P, y=P, pw=PW, am=AM, ann=2, bs=2, B=2, dz=P, loss=P)),
    "fm_loss_lakd": (None, dict(z=P, zt=P, y=P, am=AM, w_kd=C.c_float(0.8), B=2, dz=P, loss=P)),
    "fm_loss_cbafed": (None, dict(z=P, y=P, am=AM, ann=2, bs=2, tao=None, B=2, pw_dev=P, counts=None, dz=P, loss=P)),
}


def _rows():
    """(entry point, what is wrong, {argument: bad value}, text).  "engine" / "mask" are not arguments: see _refused"""
    rows = []
    for fm, (views, good) in SIGS.items():
        rows.append((fm, "null engine", {"engine": None}, NULL))
        for name, v in good.items():
            if v is P or isinstance(v, list):
                rows.append((fm, f"null {name}", {name: None}, NULL))
        if views:
            rows.append((fm, "B = 0", {"B": 0}, B2 if views == 2 else B1))
            rows.append((fm, "B over max_images", {"B": MAXB // views + 1}, B2 if views == 2 else B1))
            rows.append((fm, "mask", {"mask": True}, MASK))
        else:
            rows.append((fm, "B = 0", {"B": 0}, BGE1 if fm in ("fm_loss_fedlsr", "fm_loss_lakd") else NORM))
        if "mix1" in good:
            rows.append((fm, "mix1 = 1.5", {"mix1": C.c_float(1.5)}, f"{fm}: mix1 in [0, 1]"))
        if fm.split("_")[2] in ("rscfed", "fednoro", "lakd", "cbafed"):
            rows.append((fm, "every class active", {"am": ALL}, CLASSES))
            rows.append((fm, "every class missing", {"am": NONE}, CLASSES))
        if fm.split("_")[2] in ("rscfed", "cbafed", "fedirm"):
            rows.append((fm, "annotation_num = 0", {"ann": 0}, NORM))
        if "tao" in good:
            rows.append((fm, "tao without counts", {"tao": TAO}, f"{fm}: stage 2 (tao given) needs counts_dev"))
    rows.append(("fm_loss_fedirm_rel", "B = 2049", {"B": 2049}, "fm_loss_fedirm_rel: B <= 2048 (the selected-row table)"))
    return rows


ROWS = _rows()


@pytest.fixture(scope="module")
def ctx():
    """the engine, one device buffer behind every pointer argument, and the state and counters no refusal may move"""
    import types
    from fedmlp_amd.engine import Engine
    e = Engine("Resnet18", NC, HW, HW, MAXB)
    flat, cnt = spec.init_state("Resnet18", NC, 3)
    e.set_state(flat, cnt + 3)
    e.teacher_snapshot()
    e.adam_reset(3e-5)
    # every pointer argument: room for the largest batch a row names (B = 5 images; 2 x 2049 rows of logits), should a refusal fail
    buf = torch.zeros(max(5 * 3 * HW * HW, 2 * 2049 * NC), device=e.device)
    e.sync()
    yield types.SimpleNamespace(eng=e, buf=buf, state=e.get_state(), counters=np.array(e.counters()))
    e.close()


def test_the_table_covers_every_fused_step_and_head():
    from tests import coherence_cases as CC
    declared = {f for f in CC.header_entry_points() if f.startswith(("fm_step_", "fm_loss_"))}
    assert declared == set(SIGS)
    assert {fm for fm, *_ in ROWS} == set(SIGS)
    for fm, (views, good) in SIGS.items():
        assert len(good) == len(_lib.SYMBOLS[fm][1]) - 1, fm                  # one value per C argument after the engine
    kinds = {what.split(" ")[0] for _, what, _, _ in ROWS}
    assert {"null", "B", "mask", "mix1", "every", "annotation_num", "tao"} <= kinds


def _refused(ctx, fm, bad):
    eng = ctx.eng
    _, good = SIGS[fm]
    vals = dict(good, **{k: v for k, v in bad.items() if k in good})
    ptr = C.c_void_p(ctx.buf.data_ptr())
    args = [ptr if v is P else _lib.fvec(v, NC) if isinstance(v, list) else v for v in vals.values()]
    if bad.get("mask"):
        flags = np.ones(len(spec.entries("Resnet18", NC)), np.int32)
        flags[0] = 0
        eng.set_trainable(flags)
    try:
        rc = getattr(eng.lib, fm)(None if "engine" in bad else eng.h, *args)
        return rc, eng.lib.fm_last_error().decode()
    finally:
        if bad.get("mask"):
            eng.set_trainable(np.ones(len(spec.entries("Resnet18", NC)), np.int32))


@pytest.mark.parametrize("fm,what,bad,text", ROWS, ids=[f"{fm}-{what.replace(' ', '_')}" for fm, what, _, _ in ROWS])
def test_one_bad_argument_is_refused_with_its_text(ctx, fm, what, bad, text):
    rc, err = _refused(ctx, fm, bad)
    assert rc == -1, (fm, what, rc, err)                                      # FM_ERR_ARG
    assert err == "bad argument: " + text, (fm, what, err)
    if fm.startswith("fm_step_"):
        flat, cnt = ctx.eng.get_state()
        assert flat.tobytes() == ctx.state[0].tobytes() and cnt.tobytes() == ctx.state[1].tobytes(), (fm, what)
        assert np.array(ctx.eng.counters()).tobytes() == ctx.counters.tobytes(), (fm, what)
