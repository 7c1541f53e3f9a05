"""The committed slide fixtures (tests/golden/slide_NN.npz, make_golden.py --slide) cover every row of
SLIDE_STRATA in tests/strata.py at shapes that are granted a sliding observation buffer, and a replay
of each of them with the slacks tests/test_gpu_sliding_reference.py uses cannot be vacuous: resets (or,
without auto-reset, steps after the end) land on slide calls.  CPU only."""
import glob
import os

import numpy as np
import pytest

import replay
import special_words
import strata


def _slide_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(replay.GOLDEN_DIR, "slide_*.npz")))


def test_slide_family_covers_every_stratum():
    names = _slide_names()
    assert 8 <= len(names) <= 10, names
    gaps = strata.slide_missing([replay.load(n) for n in names])
    assert not gaps, f"slide strata rows no trace covers: {gaps}"


@pytest.mark.parametrize("name", _slide_names())
def test_slide_fixture_is_a_replayable_trace_that_slides(name):
    """Each slide fixture is a batched trace of the generator's format within the size and shape
    budget, its shape is granted a slack, and its recorded strata are the ones its data has."""
    g = replay.load(name)
    f = strata.facts(g)
    assert name in replay.golden_names()
    assert os.path.getsize(os.path.join(replay.GOLDEN_DIR, name + ".npz")) <= 200 * 1024
    K, E = g["op"].shape
    assert E <= 4 and K <= 200 and all(len(ds[1]) <= 400 for ds in g["datasets"])
    assert (g["op"][0] == 0).all()
    assert strata.slides(f)
    assert g["obs"].shape == (K, E, f["W"], f["Fobs"])
    recorded = str(g["note"]).split("strata: ")[1]
    assert (recorded.split(", ") if recorded else []) == strata.slide_rows_of(g) != []
    assert len({len(ds[1]) for ds in g["datasets"]}) == len(g["datasets"])  # identified by length
    assert g["obs"].dtype == np.float32 and g["reward"].dtype == np.float64
    for ds in g["datasets"]:
        assert ds[0].dtype == np.float32 and ds[1].dtype == np.float64
        assert not special_words.is_signalling_nan(ds[0]).any()  # the reference quiets those
        assert not np.isnan(ds[1]).any()
    for k in replay.STATE_F64:
        assert g[k].dtype == np.float64 and g[k].shape == (K, E)
    # without dyn_persist: no episode starts inside dynamic values an earlier one left in the table
    assert not g["obs"][g["op"] == 0][:, :-1, f["Fs"]:].any()


@pytest.mark.parametrize("name", _slide_names())
def test_slide_fixture_is_not_vacuous_at_any_tested_slack(name):
    """From the trace alone: the head at call k is k % (M + 1).  At every slack the GPU test uses, at
    least three per-env resets land on slide calls, so a row of the previous episode or dataset that
    survived a reset would be compared; the trace without auto-reset has three env-steps after the
    end on slide calls instead; every replay wraps."""
    g = replay.load(name)
    f = strata.facts(g)
    assert strata.slacks_tested(f)[0] == 1 and strata.auto_slack(f["W"]) in strata.slacks_tested(f)
    assert not strata.slide_vacuous(g)
    for M in strata.slacks_tested(f):
        c = strata.slide_counts(g, M)
        assert c["slide_calls"] + c["wraps"] == f["K"] - 1 and c["wraps"] >= 1
        assert (c["resets_on_slide"] if f["autoreset"] else c["after_end_on_slide"]) >= strata.SLIDE_MIN_EVENTS


def test_slide_counts_on_a_hand_made_trace():
    op = np.ones((7, 2), np.uint8)
    op[0] = 0
    op[3, 0] = op[4, 1] = 0          # env 0 resets at call 3 (head 1 of M = 1), env 1 at call 4 (head 0)
    z = np.zeros((7, 2), np.uint8)
    g = dict(op=op, done=z, truncated=z)
    assert strata.slide_counts(g, 1) == dict(slide_calls=3, wraps=3, resets_on_slide=1, after_end_on_slide=0)
    assert strata.slide_counts(g, 3) == dict(slide_calls=5, wraps=1, resets_on_slide=1, after_end_on_slide=0)
    op = np.ones((6, 1), np.uint8)
    op[0] = 0
    done = np.zeros((6, 1), np.uint8)
    done[2:] = 1                     # ended at call 2, stepped on at calls 3, 4, 5 (heads 1, 0, 1)
    assert strata.slide_counts(dict(op=op, done=done, truncated=0 * done), 1)["after_end_on_slide"] == 2


def test_slide_budget():
    total = sum(os.path.getsize(os.path.join(replay.GOLDEN_DIR, n + ".npz")) for n in _slide_names())
    assert total <= 1536 * 1024


def test_which_fixtures_of_the_other_families_slide():
    """The grant restated by strata.slides picks out six traces of the older families; the GPU test
    asserts that the library grants each of them (and every slide trace) a slack."""
    others = [n for n in replay.golden_names() if not n.startswith("slide_")]
    assert [n for n in others if strata.slides(strata.facts(replay.load(n)))] == [
        "c3_window20", "numeric_04", "sweep_00", "sweep_01", "sweep_02", "sweep_03"]
    assert not any(strata.slide_rows_of(replay.load(n)) for n in others if n.startswith("sweep_1"))


def test_interleaved_plans_are_not_vacuous():
    """The seeded step / rollout plans of test_gpu_sliding_reference.test_steps_interleaved_with_rollouts,
    from the traces alone: rollouts of both kinds, a full step after a rollout that kept its
    observations, slide steps, and at least three per-env resets on slide steps."""
    import test_gpu_sliding_reference as t
    for key in t.INTERLEAVED:
        g = replay.load(t.interleaved_trace(key))
        plan = t.interleave_plan(g)
        assert [c[1] for c in plan] == [1] + [c[2] for c in plan[:-1]] and plan[-1][2] == g["op"].shape[0]
        c = t.plan_counts(g, plan)
        assert c["keep"] >= 2 and c["drop"] >= 2 and c["full_step_after_keep"] >= 1, (key, c)
        assert c["slide_steps"] >= 10 and c["resets_on_slide"] >= strata.SLIDE_MIN_EVENTS, (key, c)
