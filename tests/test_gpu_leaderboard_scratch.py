"""The three leaderboard analyses share one rule for their scratch (gte_api.hip: a block each, which only grows) and
keep a block each: the reality check, CSCV and the decorrelated leaderboard interleaved on one env while S goes up
across a tile of 256 strategies and down again, every output of every call against its model bit for bit."""
import numpy as np
import pytest

import bootstrap_model as bm
import cscv_model as cm
import diversify_model as dm
import test_gpu_bootstrap as boot
import test_gpu_cscv as cscv
import test_gpu_diversify as div
from gym_trading_env_amd import periods
from leaderboard_gpu import make_env

pytestmark = pytest.mark.gpu

B, R, G, K = 6, 17, 2, 3


@pytest.fixture(scope="module")
def env():
    e = make_env()      # a fresh env: none of the three has any scratch yet
    yield e
    e.close()


def test_interleaved_analyses_across_regrown_scratch(env):
    """S = 64, 257, 64: the first round allocates the three blocks, the second outgrows every one of them while the
    other two hold theirs, the third runs in the larger blocks"""
    mask = np.arange(B) != 3
    ids = [int(b) for b in np.flatnonzero(mask)]
    groups = periods.cscv_groups(range(B), G)
    is_g, oos_g = periods.cscv_splits(G)
    weights = bm.weights(len(ids), R, 2.0, boot.SEED)
    benchmark = np.random.default_rng(1).normal(0, 1e-3, B)
    for turn, S in enumerate((64, 257, 64)):
        tag = f"turn {turn} S={S}"
        stats = boot.craft(S, B, 10 + turn, mask, False)
        got = boot.run_check(env, stats, mask, benchmark, weights)
        boot.assert_same(got, bm.reality_check(stats, mask, benchmark, weights), f"reality check, {tag}")
        assert got["stats_after"] == stats.tobytes()

        stats = cscv.craft(S, B, 20 + turn, groups)
        got = cscv.run_cscv(env, stats, groups, is_g, oos_g, cm.SHARPE)
        cscv.assert_same(got, cm.cscv(stats, groups, is_g, oos_g, cm.SHARPE), f"cscv, {tag}")
        assert got["stats_after"] == stats.tobytes()

        stats, scores = div.craft(S, B, ids, 30 + turn)
        got = div.run_div(env, stats, ids, scores, 0.7, K)
        div.assert_same(got, dm.diversify(stats, ids, scores, 0.7, K), f"diversify, {tag}")
