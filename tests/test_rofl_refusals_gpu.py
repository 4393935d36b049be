"""What fm_step_rofl and fm_loss_rofl (include/fedmlp_hip_rofl.h) answer to ONE bad argument, in the manner of
tests/test_step_refusals_gpu.py, whose table is closed over include/fedmlp_hip.h: FM_ERR_ARG and the fm_last_error() text, the
shared texts where the refusal is a shared one (null, the batch bounds, the requires_grad mask).  A refusal comes before anything
is enqueued: after each refused fm_step_rofl the engine's state and counters are the bits they were.  Nothing here launches a
kernel; the entry points are called through ctypes on one ResNet-18 engine at 64 x 64 with max_images = 4 and C = 5."""
import ctypes as C

import numpy as np
import pytest

from fedmlp_amd import _lib, spec
from tests.test_step_refusals_gpu import B1, BGE1, MASK, MAXB, NC, NULL, PW, P, ctx      # noqa: F401  (ctx: the fixture)

pytestmark = pytest.mark.gpu

N_BAD = "rofl: 1 <= N, N * n_classes < 2^31"
ALIGN = "rofl: feature and centroid rows must be 16-byte aligned"
P4 = "ptr + 4"                           # a device pointer 4 bytes past a 16-byte boundary
N_KEEP_0 = "rofl: n_keep < 1 (int((1 - forget_rate) * B) of a batch this small keeps no row)"
SIGS = {
    "fm_step_rofl": (1, dict(x=P, y=P, item=P, B=2, n_keep=1, pw=PW, lam_cen=C.c_float(0.5), lam_e=C.c_float(0.8), wl=1, centroids=P,
                             pseudo=P, N=C.c_int64(8), loss=P)),
    "fm_loss_rofl": (None, dict(z=P, feat=P, y=P, item=P, B=2, n_keep=1, pw=PW, lam_cen=C.c_float(0.5), lam_e=C.c_float(0.8), wl=1,
                                centroids=P, pseudo=P, N=C.c_int64(8), dz=P, loss=P, keep=None)),
}


def _rows():
    rows = []
    for fm, (views, good) in SIGS.items():
        rows.append((fm, "null engine", {"engine": None}, NULL))
        for name, v in good.items():
            if v is P or isinstance(v, list):
                rows.append((fm, f"null {name}", {name: None}, NULL))
        if views:
            rows.append((fm, "B = 0", {"B": 0}, B1))
            rows.append((fm, "B over max_images", {"B": MAXB + 1}, B1))
            rows.append((fm, "mask", {"mask": True}, MASK))
        else:
            rows.append((fm, "B = 0", {"B": 0}, BGE1))
            rows.append((fm, "B over max_images", {"B": MAXB + 1, "n_keep": 1}, B1))
        rows.append((fm, "n_keep = 0", {"n_keep": 0}, N_KEEP_0))
        rows.append((fm, "n_keep over B", {"n_keep": 3}, "rofl: n_keep > B"))
        rows.append((fm, "N = 0", {"N": C.c_int64(0)}, N_BAD))
        rows.append((fm, "N C over 2^31", {"N": C.c_int64(2 ** 31 // NC + 1)}, N_BAD))
        rows.append((fm, "centroids off 16 bytes", {"centroids": P4}, ALIGN))
        if "feat" in good:               # (the step reads the engine's own feature buffer)
            rows.append((fm, "feat off 16 bytes", {"feat": P4}, ALIGN))
    return rows


ROWS = _rows()


def test_the_table_covers_both_entry_points():
    assert set(SIGS) == set(_lib.ROFL_SYMBOLS) == {fm for fm, *_ in ROWS}
    for fm, (views, good) in SIGS.items():
        assert len(good) == len(_lib.ROFL_SYMBOLS[fm][1]) - 1, fm                 # one value per C argument after the engine


def _refused(ctx, fm, bad):
    eng = ctx.eng
    _, good = SIGS[fm]
    vals = dict(good, **{k: v for k, v in bad.items() if k in good})
    ptr = C.c_void_p(ctx.buf.data_ptr())
    assert ctx.buf.data_ptr() % 16 == 0
    off = C.c_void_p(ctx.buf.data_ptr() + 4)
    args = [ptr if v is P else off if v is P4 else _lib.fvec(v, NC) if isinstance(v, list) else v for v in vals.values()]
    n_entries = len(spec.entries("Resnet18", NC))
    if bad.get("mask"):
        flags = np.ones(n_entries, np.int32)
        flags[0] = 0
        eng.set_trainable(flags)
    try:
        rc = getattr(eng.lib, fm)(None if "engine" in bad else eng.h, *args)
        return rc, eng.lib.fm_last_error().decode()
    finally:
        if bad.get("mask"):
            eng.set_trainable(np.ones(n_entries, np.int32))


@pytest.mark.parametrize("fm,what,bad,text", ROWS, ids=[f"{fm}-{what.replace(' ', '_')}" for fm, what, _, _ in ROWS])
def test_one_bad_argument_is_refused_with_its_text(ctx, fm, what, bad, text):
    rc, err = _refused(ctx, fm, bad)
    assert rc == -1, (fm, what, rc, err)                                      # FM_ERR_ARG
    assert err == "bad argument: " + text, (fm, what, err)
    if fm.startswith("fm_step_"):
        flat, cnt = ctx.eng.get_state()
        assert flat.tobytes() == ctx.state[0].tobytes() and cnt.tobytes() == ctx.state[1].tobytes(), (fm, what)
        assert np.array(ctx.eng.counters()).tobytes() == ctx.counters.tobytes(), (fm, what)
