"""The host builder of the state arena's entry / chunk table (fedmlp_amd/csrc/arena_table.h), without a GPU: a stand-alone
program (tests/host/arena_table_check.cpp) is compiled with the ROCm toolchain's clang++ under AddressSanitizer and UBSan, run as
a child process on synthetic entry lists, and its tables are held against an independent statement of the header's invariants 1
(chunk geometry) and 2 (chunk order).  A missing compiler fails the test."""
import collections
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANGXX = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
CHUNK, MAX_ENT = 8192, 512

# kind 0: weight rows of [..][Wpad][Ipad] with W x I real, 1: float vector, 2: int64 counter
Desc = collections.namedtuple("Desc", "kind off dense row len Ipad I Wpad W param")


def vec(off, n, param=True):
    return Desc(1, off, n, n, n, 0, 0, 0, 0, param)


def conv(off, O, I, KH, KW, Wpad, Ipad, Ostride=0, param=True):
    dense = KH * Wpad * Ipad
    row = Ostride or dense
    return Desc(0, off, dense, row, (O - 1) * row + dense, Ipad, I, Wpad, KW, param)


COUNTER = Desc(2, 0, 1, 1, 1, 0, 0, 0, 0, False)
NP, NS = 16564, 16564 + 8300
MIXED = [
    vec(3, 5),                                            # shorter than a quad, off a 16-byte boundary
    conv(8, O=2, I=3, KH=1, KW=1, Wpad=2, Ipad=4, Ostride=12),    # len 20, row stride beyond the dense row, mostly padding
    COUNTER,                                              # between parameters in state order: no entry
    vec(NP + 1, 7, param=False),                          # a buffer between parameters in state order
    vec(29, 8192),                                        # exactly one chunk, offset = 1 (mod 4)
    vec(8224, 8193),                                      # second chunk of length 1
    conv(16420, O=4, I=4, KH=3, KW=3, Wpad=3, Ipad=4),      # a dense weight: every element real
    vec(NP + 16, 8200, param=False),                      # a buffer of two chunks
]
CASES = {
    "mixed": (NP, NS, MIXED),
    "param_crosses_NP": (64, 128, [vec(0, 8), vec(60, 5)]),
    "buffer_crosses_NS": (64, 128, [vec(0, 8), vec(120, 9, param=False)]),
    "513_entries": (4 * 513, 4 * 513, [vec(4 * i, 3) for i in range(513)]),
    "512_entries": (4 * 512, 4 * 512 + 8, [vec(4 * i, 3) for i in range(511)] + [vec(4 * 512, 8, param=False)]),
}
REFUSED = {"param_crosses_NP": "a parameter entry lies outside the trainable arena",
           "buffer_crosses_NS": "state entry outside the arena",
           "513_entries": "more parameter entries than the optimizer table holds"}


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    assert os.path.exists(CLANGXX), f"the ROCm toolchain's clang++ is missing: {CLANGXX}"
    exe = str(tmp_path_factory.mktemp("arena_table") / "arena_table_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "arena_table_check.cpp"), "-o", exe], check=True)
    text = "".join(f"case {np_} {ns} {len(descs)}\n" + "".join(" ".join(str(int(x)) for x in d) + "\n" for d in descs)
                   for np_, ns, descs in CASES.values())
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(CASES)
    return dict(zip(CASES, map(json.loads, lines)))


def expected_chunks(descs):
    """invariants 1 and 2: every fp32 entry's span cut at multiples of CHUNK from its offset; the parameters' chunks first, then
    the buffers', each class in state order with ascending start; `ent` counts the fp32 entries in state order"""
    fp32 = [d for d in descs if d.kind != 2]
    chunks = []
    for param in (True, False):
        for e, d in enumerate(fp32):
            if d.param == param:
                chunks += [[d.off + st, min(CHUNK, d.len - st), e] for st in range(0, d.len, CHUNK)]
    return chunks, sum(-(-d.len // CHUNK) for d in fp32 if d.param)


@pytest.mark.parametrize("name", [n for n in CASES if n not in REFUSED])
def test_tables_hold_the_invariants(tables, name):
    _, _, descs = CASES[name]
    t = tables[name]
    assert t["error"] is None
    chunks, n_param = expected_chunks(descs)
    assert t["chunks"] == chunks and t["n_param_chunks"] == n_param
    fp32 = [d for d in descs if d.kind != 2]
    assert len(t["ent"]) == len(fp32) <= MAX_ENT
    it = iter(range(len(fp32)))
    assert t["ent_of"] == [-1 if d.kind == 2 else next(it) for d in descs]
    for e, (d, a) in enumerate(zip(fp32, t["ent"])):
        assert (a["off"], a["len"], a["row"], a["dense"]) == (d.off, d.len, d.row, d.dense)
        geom = (d.Ipad, d.I, d.Wpad, d.W) if d.kind == 0 else (1, 1, 1, 1)
        assert (a["Ipad"], a["I"], a["Wpad"], a["W"]) == geom
        assert bool(a["all_real"]) == (d.row == d.dense and geom[0] == geom[1] and geom[2] == geom[3])
        own = chunks[a["chunk0"]:a["chunk0"] + a["nchunks"]]
        assert own == [c for c in chunks if c[2] == e]              # its chunks are consecutive and all of them
        assert own[0][0] == d.off and sum(c[1] for c in own) == d.len
        assert all(p[0] + p[1] == q[0] for p, q in zip(own, own[1:]))
        assert (a["chunk0"] < n_param) == d.param


def test_the_synthetic_list_reaches_the_edges(tables):
    """the cases the walker's edge paths need: a span shorter than a quad off a boundary, a full chunk off a boundary, a chunk of
    length 1, an entry that is mostly padding, and the parameters as the chunk prefix although a buffer precedes some in state order"""
    t = tables["mixed"]
    spans = [(c[0], c[1]) for c in t["chunks"]]
    assert (3, 5) in spans and (29, 8192) in spans and (8224 + 8192, 1) in spans
    assert [a["all_real"] for a in t["ent"]] == [1, 0, 1, 1, 1, 1, 1] and t["ent"][1]["len"] == 20
    ents = [c[2] for c in t["chunks"]]
    assert ents == [0, 1, 3, 4, 4, 5, 2, 6, 6] and t["n_param_chunks"] == 6


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_keep_their_texts(tables, name):
    assert tables[name] == {"error": REFUSED[name]}
