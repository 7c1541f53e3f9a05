"""examples/backtest_stop_sweep.py at a reduced size: the maps it builds, the leaders against the
NumPy models of the strategy fold and the ranking, and exits that really fired."""
import os
import sys

import numpy as np
import pytest

import strategy_model as sm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stop_sweep_example(capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import backtest_stop_sweep
    rows, stops, targets, replicas = 2, 3, 2, 5
    index, score, records, state, (strategy, rule_of_env, exits) = backtest_stop_sweep.main(
        rows=rows, stops=stops, targets=targets, replicas=replicas, K=400, top=4, details=True)
    R, n_pairs = stops * targets, rows * stops * targets
    N = n_pairs * replicas
    assert len(exits) == R and records.shape == state.shape == (N,)
    pair = np.arange(N) % n_pairs
    np.testing.assert_array_equal(strategy, pair // R)
    np.testing.assert_array_equal(rule_of_env, pair % R)
    assert (exits["exit_position"] == 1).all() and len(set(zip(exits["stop_loss"], exits["take_profit"]))) == R
    # every pair has `replicas` envs; the leaders are those of the models over the env records
    board = sm.reduce_vector(records, sm.map_groups(pair, n_pairs))
    assert (board["envs"] == replicas).all()
    want_i, want_s = sm.rank_vector(board, sm.scores_vector(board, "mean_episode_return"), 4, 4)
    assert index.tolist() == want_i.tolist() and sm.same_f64(score, want_s)
    # stops and targets fired, nothing else was asked for
    fired = state["exits"].sum(axis=0)
    assert fired[0] > 0 and fired[2] > 0 and fired[1] == 0 and fired[3] == 0
    out = capsys.readouterr().out
    assert f"= {n_pairs} pairs over {N} envs" in out and "stop" in out and "mean episode return" in out
