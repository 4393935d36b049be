"""Every --exp row of the driver, bit for bit against tests/golden/driver_rows.json: per round the mean loss, a SHA-1 over the
tensors of the saved global model and, where the row evaluates, the test metrics.  The driver seeds every RNG and the engine's
kernels are deterministic, so a row run twice gives the same bits.

The fixture was recorded on an MI355X with tests/golden/make_driver_rows.py (`python tests/golden/make_driver_rows.py`) from the
tree of the commit BEFORE the rows became objects (fedmlp_amd/rows.py) and the round loop left main(): that driver.py tested
args.exp at 24 places of one function.  The recorder uses the command line only, so it ran there unchanged; it ran every row twice
and kept the rows whose two runs agreed in every value -- all fourteen.  The two FedMLP rows select clean and noise samples in
their first stage-2 round (per client 16 + 0 and 14 + 1 at --clean_threshold 0.5 --noise_threshold 0.5 on 32 samples).  A row
that has to be recorded again is recorded from that parent commit, never from the tree under test."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "driver_rows.json")) as f:
    FIXTURE = json.load(f)


def _recorder():
    spec = importlib.util.spec_from_file_location("make_driver_rows", os.path.join(GOLDEN, "make_driver_rows.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_row_is_recorded():
    assert sorted(FIXTURE) == sorted(_recorder().ROWS)


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_driver_row_equals_the_parent_commit(name):
    rec = _recorder()
    want = FIXTURE[name]
    assert rec.ROWS[name] + rec.COMMON == want["argv"]
    got = rec.run_row(name)
    assert len(got["rounds"]) == len(want["rounds"])
    for rnd, (g, w) in enumerate(zip(got["rounds"], want["rounds"])):
        print(f"{name} round {rnd}: mean_loss {g['mean_loss']!r} (recorded {w['mean_loss']!r}), sha1 {g['sha1']} ({w['sha1']})")
        assert g == w, (name, rnd)
