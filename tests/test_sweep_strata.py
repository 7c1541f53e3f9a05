"""The committed sweep fixtures (tests/golden/sweep_NN.npz, make_golden.py --sweep) cover every
row of the strata table in tests/strata.py, so a regeneration cannot silently drop one.  CPU only."""
import glob
import os

import numpy as np
import pytest

import replay
import strata


def _sweep_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(replay.GOLDEN_DIR, "sweep_*.npz")))


def test_sweep_covers_every_stratum():
    names = _sweep_names()
    assert 24 <= len(names) <= 32, names
    gaps = strata.missing([replay.load(n) for n in names])
    assert not gaps, f"strata rows no sweep trace covers: {gaps}"


@pytest.mark.parametrize("name", _sweep_names())
def test_sweep_fixture_is_a_replayable_trace(name):
    """Each sweep fixture is a batched trace of the generator's format, within the size budget,
    and its recorded strata are the ones its data actually has."""
    g = replay.load(name)
    assert name in replay.golden_names()
    assert os.path.getsize(os.path.join(replay.GOLDEN_DIR, name + ".npz")) <= 200 * 1024
    K, E = g["op"].shape
    assert (g["op"][0] == 0).all()
    W = g["cfg"]["windows"]
    Fobs = strata.facts(g)["Fobs"]
    assert g["obs"].shape == ((K, E, W, Fobs) if W else (K, E, Fobs))
    note = str(g["note"])
    assert note.split("strata: ")[1].split(", ") == strata.rows_of(g)
    # datasets are identified by their length
    assert len({len(ds[1]) for ds in g["datasets"]}) == len(g["datasets"])
    assert g["obs"].dtype == np.float32 and g["reward"].dtype == np.float64


def test_sweep_budget():
    total = sum(os.path.getsize(os.path.join(replay.GOLDEN_DIR, n + ".npz")) for n in _sweep_names())
    assert total <= 3 * 1024 * 1024
