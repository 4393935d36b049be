"""step_rofl in the coherence matrix of tests/test_coherence_gpu.py (whose table of state-changing calls is closed over
include/fedmlp_hip.h): the fused RoFL step moves the student's weights and running statistics like step_bce, so after it every
first consumer of a derived copy (tests/coherence_cases.READERS) must answer on a handle whose copies were all built for another
state exactly as on a cold twin, and whatever depends on the weights or statistics must have moved."""
import pytest
import torch

from tests import coherence_cases as CC
from tests import test_coherence_gpu as M

pytestmark = pytest.mark.gpu

MOVES = frozenset({"w", "stats"})
HANDLES = ("r18_64", "eff_64", "eff_64_bf16")
CELLS = [(h, r) for h in HANDLES for r in CC.READERS]
_PAIRS = {}


def m_step_rofl(e, ctx):
    """the client's centroids and label table are the call's own: nothing of them outlives the cell"""
    g = torch.Generator().manual_seed(5)
    f_k = torch.randn((2 * CC.C_, e.feature_dim), generator=g).to(e.device)
    pseudo = torch.zeros((ctx.imgs, CC.C_), dtype=torch.uint8, device=e.device)
    item = torch.arange(ctx.imgs, dtype=torch.int32, device=e.device)
    e.adam_reset(CC.LR)
    e.step_rofl(ctx.x1, ctx.y, item, ctx.imgs - 1, ctx.pos_weight, 0.5, 0.8, True, f_k, pseudo, ctx.loss)


@pytest.fixture(scope="module")
def pairs():
    def get(handle):
        if handle not in _PAIRS:
            for h in list(_PAIRS):                 # one pair alive at a time
                for e in _PAIRS.pop(h)[:2]:
                    e.close()
            E, T = CC.make_engine(handle), CC.make_engine(handle)
            _PAIRS[handle] = (E, T, CC.make_ctx(handle, E))
        return _PAIRS[handle]
    yield get
    for h in list(_PAIRS):
        for e in _PAIRS.pop(h)[:2]:
            e.close()


@pytest.mark.parametrize("handle,reader", CELLS, ids=["-".join(c) for c in CELLS])
def test_cell(pairs, handle, reader):
    E, T, ctx = pairs(handle)
    rd = CC.READERS[reader][0]
    M.warm(E, ctx)
    base = M._host(rd(E, ctx))
    M.warm(E, ctx)
    M.cold(T, ctx)
    m_step_rofl(E, ctx)
    m_step_rofl(T, ctx)
    got, want = M._host(rd(E, ctx)), M._host(rd(T, ctx))
    same = M._same(got, want)
    assert all(same), f"{handle}: after step_rofl, reader {reader} on the warm handle differs from the cold twin in outputs " \
                      f"{[i for i, s in enumerate(same) if not s]}: a derived copy is stale"
    assert M._state_eq(E.get_state(), T.get_state()), f"{handle}: {reader}: the students' states differ afterwards"
    assert M._state_eq(M._teacher_state(E), M._teacher_state(T)), f"{handle}: {reader}: the teachers' states differ"
    for i, unchanged in enumerate(M._same(got, base)):
        dep = CC.reads(reader, i)
        if dep is None:
            continue
        if MOVES & dep:
            assert not unchanged, f"{handle}: step_rofl left output {i} of reader {reader} at its (S0, T0) bits: it was not seen"
        else:
            assert unchanged, f"{handle}: step_rofl must not move output {i} of reader {reader}"
    torch.cuda.synchronize()
