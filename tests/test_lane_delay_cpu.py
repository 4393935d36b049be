"""The host side of tests/test_lane_delay_gpu.py without a GPU: the position ranges of the cases leave no delay point out,
and the wait kinds have one order in the header, the wrapper and the test."""
import os
import re

from tests import test_lane_delay_gpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_case_ranges_partition_every_point_count():
    for n in range(1, 9):
        for points in list(range(0, 40)) + [198, 402, 528, 1001]:
            got = [p for k in range(n) for p in T._chunk(points, k, n)]
            assert got == list(range(points)), (points, n)


def test_ranges_of_positions():
    assert T._ranges(set()) == []
    assert T._ranges({3, 0, 1, 2, 7, 9, 8}) == [[0, 3], [7, 9]]


def test_wait_kinds_have_one_order():
    from fedmlp_amd.engine import Engine
    hdr = open(os.path.join(ROOT, "include", "fedmlp_hip_debug.h")).read()
    enum = re.search(r"enum \{ (FM_WAIT_SIDE_BEGIN[^}]*)\}", hdr).group(1)
    names = tuple(n.split("=")[0].strip()[len("FM_WAIT_"):].lower() for n in enum.split(","))
    assert names == Engine.WAIT_KINDS == T.KINDS
    assert int(re.search(r"#define FM_WAIT_KINDS (\d+)", hdr).group(1)) == len(names)
    assert int(re.search(r"#define FM_LANE_DELAY_MAX_US (\d+)", hdr).group(1)) == T.MAX_DELAY_US
    assert set(T.MUTANT_LANE) == set(T.KINDS)


def test_every_sequence_has_its_sweep_mutant_and_verdict_cases():
    ids = [c.id for c in T._cases()]
    assert len(ids) == len(set(ids))
    for s in T.SEQS:
        assert set(s.kinds) <= set(T.KINDS) and s.chunks[0] >= 1 and s.chunks[1] >= 1
        for lane, lname in ((0, "main"), (1, "side")):
            assert [i for i in ids if i.startswith(f"{s.name}-{lname}-")] == [f"{s.name}-{lname}-{k}" for k in range(s.chunks[lane])]
        for kind in s.kinds:
            n = s.chunks[T.MUTANT_LANE[kind]]
            assert [i for i in ids if i.startswith(f"{s.name}-drop_{kind}-")] == [f"{s.name}-drop_{kind}-{k}" for k in range(n)]
        assert f"{s.name}-verdict" in ids
