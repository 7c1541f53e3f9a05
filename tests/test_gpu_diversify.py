"""The decorrelated leaderboard on the device (gte_diversify, include/gte.h) against its model
(tests/diversify_model.py), bit for bit on every output, NaN as NaN: S x (B, mask) over the lane, wave and workgroup
edges with k below, at and beyond the candidates and thresholds from -inf to above one; planted families; crafted
rows (duplicates of the leader, a mirror, constant and all-zero rows, NaN / inf / no step inside and outside the mask,
NaN, +-inf and +-0.0 scores, nobody eligible); twelve decades of row scale; determinism and isolation across a
regrown scratch; the existing ranking kernel; every refusal, with the outputs untouched; the Python pipeline end to
end; the example."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import diversify_model as dm
from gym_trading_env_amd import _abi
from leaderboard_gpu import (GUARD, assert_arrays_same, board as _board, device_records, guarded, id_words as words,
                             make_env)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
KS = (1, 3, 256)
MAX_CORRS = (-INF, -0.5, 0.0, 0.9, 1.0, 2.0)
MASKS = {"B3_all": (3, list(range(3))), "B70_60to69": (70, list(range(60, 70))), "B128_all": (128, list(range(128))),
         "B40_scattered7": (40, [1, 4, 9, 17, 22, 30, 39])}
FLOATS = ("pick_score", "owner_corr", "pick_corr")


@pytest.fixture(scope="module")
def env():
    e = make_env()
    yield e
    e.close()


def craft(S, B, ids, seed, dead=False):
    """([S, B] strategy period records, scores f64 [S]): a few factor rows plus noise, every strategy at a scale of its
    own over twelve decades; a leader and exact duplicates of it (equal scores: the lowest index leads, the others land
    in its cluster); its mirror; a constant row and an all-zero row (q == 0: ineligible); NaN, +inf, -inf in a selected
    period and a selected period without steps (ineligible); the same poisons in periods OUTSIDE the selection, which
    must not matter; a NaN score on an eligible row; +-inf scores; -0.0 against 0.0 scores"""
    rng = np.random.default_rng(seed)
    ids = list(ids)
    factors = rng.normal(0, 1, (5, B))
    x = (factors[rng.integers(0, 5, S)] + 0.2 * rng.normal(0, 1, (S, B))) * 10.0 ** rng.integers(-6, 7, (S, 1))
    steps = rng.integers(1, 50, (S, B))
    scores = np.round(rng.normal(0, 1, S), 2)
    outside = np.setdiff1d(np.arange(B), ids)

    def put(k, row=None, score=None):
        if k < S:
            if row is not None:
                x[k] = row
            if score is not None:
                scores[k] = score
        return k < S
    lead = rng.normal(0, 1, B) * 3e-4
    for k in (3, 17, 40):                                   # 17 and 40 duplicate 3, which leads before them
        put(k, lead, 50.0)
    put(4, -lead, 49.0)                                     # the mirror: the next pick, never in the leader's cluster
    put(5, np.full(B, 0.375))                               # constant
    put(6, np.zeros(B))                                     # all zero
    put(7, np.where(np.arange(B) % 2 == 0, -0.0, 0.0))      # zeros of either sign
    for k, bad in ((11, np.nan), (12, np.inf), (13, -np.inf)):
        if k < S:
            x[k, ids[k % len(ids)]] = bad
    if 14 < S:
        steps[14, ids[-1]] = 0                              # a selected period without steps
    put(20, score=np.nan)                                   # eligible, no candidate
    put(21, score=np.inf)
    put(22, score=-np.inf)
    put(23, score=0.0), put(24, score=-0.0), put(25, score=0.0)
    put(1, score=-np.inf)                                   # (S = 5: the edge scores are there as well)
    put(2, score=-0.0), put(0, score=0.0)
    if len(outside):
        x[:, outside[0]] = np.nan
        x[::2, outside[-1]] = np.inf
        steps[:, outside[-1]] = 0
    if dead:
        steps[:, ids[0]] = 0
    return dm.records(x, steps), scores


def run_div(env, stats, ids, scores, max_corr, k):
    """gte_diversify over host-made records and scores -> dict of host arrays, like the model's; every output stands
    between guard words, which must come back untouched, and the inputs must be what they were"""
    import torch
    dev = env._t["obs"].device
    S, B = stats.shape
    d_stats = device_records(env, stats)
    d_scores = torch.from_numpy(np.ascontiguousarray(scores, np.float64).copy()).to(dev)
    whole, out = {}, {}
    for name, n, dt in (("pick", k, torch.int32), ("pick_score", k, torch.float64), ("cluster_size", k, torch.int32),
                        ("owner", S, torch.int32), ("owner_corr", S, torch.float64),
                        ("pick_corr", k * k, torch.float64)):
        whole[name], out[name] = guarded(torch, dev, n, dt, -7)
    whole["summary"], out["summary"] = guarded(torch, dev, 20, torch.uint8, 0xAB)    # (8 bytes on either side)
    ptrs = _abi.GteDiversifyOut(**{name: v.data_ptr() for name, v in out.items()})
    torch.cuda.synchronize()
    _abi.check(env._lib, env._lib.gte_diversify(env._h, C.c_void_p(d_stats.data_ptr()), S, B, words(ids),
                                                C.c_void_p(d_scores.data_ptr()), float(max_corr), k, C.byref(ptrs)))
    env.synchronize()
    got = {name: v.cpu().numpy() for name, v in out.items()}
    got["summary"] = got["summary"].view(dm.SUMMARY)
    got["pick_corr"] = got["pick_corr"].reshape(k, k)
    for name, v in whole.items():
        edge = torch.cat((v[:GUARD], v[-GUARD:])).cpu().numpy()
        assert (edge == (0xAB if name == "summary" else -7)).all(), f"guard words of {name} were written"
    assert d_stats.cpu().numpy().tobytes() == stats.tobytes(), "the records were written"
    assert d_scores.cpu().numpy().tobytes() == np.ascontiguousarray(scores, np.float64).tobytes(), "the scores were written"
    return got


def assert_same(got, want, tag):
    assert_arrays_same(got, want, ("pick", "pick_score", "cluster_size", "owner", "owner_corr", "pick_corr"), FLOATS, tag)
    assert got["summary"].tobytes() == want["summary"].tobytes(), (tag, got["summary"], want["summary"])


def check(env, stats, ids, scores, max_corr, k, tag):
    got = run_div(env, stats, ids, scores, max_corr, k)
    want = dm.diversify(stats, ids, scores, max_corr, k)
    assert_same(got, want, tag)
    return got, want


# ---- shapes over the edges -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("S", [1, 5, 64, 65, 257, 1000])
def test_every_output_equals_the_model(env, S, mask):
    """Per (S, mask): every threshold, with k = 1, 3 and 256 in turn (over the grid every pair of the two occurs);
    S a single lane, a wave's tail, one wave, a wave and a lane, workgroups with a tail; the mask within one word,
    across the word boundary, both words full, scattered."""
    B, ids = MASKS[mask]
    turn = [1, 5, 64, 65, 257, 1000].index(S) + list(MASKS).index(mask)
    stats, scores = craft(S, B, ids, S * 131 + B)
    seen = set()
    for j, max_corr in enumerate(MAX_CORRS):
        k = KS[(j + turn) % 3]
        seen.add(k)
        got, want = check(env, stats, ids, scores, max_corr, k, f"S={S} {mask} k={k} max_corr={max_corr}")
        if max_corr == -INF and want["summary"][0]["candidates"]:
            assert got["cluster_size"][0] == want["summary"][0]["candidates"] and got["summary"][0]["remaining"] == 0
        if max_corr == 2.0:
            assert set(got["cluster_size"][got["pick"] >= 0].tolist()) <= {1}
    assert seen == set(KS)


def test_one_strategy_that_is_a_candidate(env):
    """S = 1 with a row of its own (craft's row 0 at S = 1 is a plain one too; this one states it): it is picked, its
    cluster is itself, its correlation with itself is the formula's value"""
    x = np.array([[0.1, -0.2, 0.4, 0.05]])
    got, want = check(env, dm.records(x), range(4), np.array([1.5]), 0.7, 3, "S=1")
    assert got["pick"].tolist() == [0, -1, -1] and got["cluster_size"].tolist() == [1, 0, 0]
    assert tuple(got["summary"][0]) == (1, 1, 1, 0, 0) and abs(got["owner_corr"][0] - 1.0) < 1e-15


# ---- planted families ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 3])
def test_planted_families(env, seed):
    x, family = dm.planted(seed)
    got, _ = check(env, dm.records(x), range(24), x.sum(axis=1), 0.9, 16, f"planted {seed}")
    assert tuple(got["summary"][0]) == (6, 257, 257, 0, 0)
    assert sorted(family[got["pick"][:6]].tolist()) == list(range(6)) and (got["pick"][6:] == -1).all()
    for r in range(6):
        assert np.array_equal(np.flatnonzero(got["owner"] == r), np.flatnonzero(family == family[got["pick"][r]]))
    assert int(got["cluster_size"].sum()) == 257


# ---- crafted rows ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_corr", [0.7, -INF, INF])
def test_crafted_rows(env, max_corr):
    """S = 300, B = 24 with periods 5 and 20 outside the selection: what each crafted row is there for is seen"""
    S, B = 300, 24
    ids = [b for b in range(B) if b not in (5, 20)]
    stats, scores = craft(S, B, ids, 77)
    got, want = check(env, stats, ids, scores, max_corr, 40, f"crafted max_corr={max_corr}")
    assert not want["eligible"][[5, 6, 7, 11, 12, 13, 14]].any() and want["eligible"][[3, 4, 17, 20, 21, 22, 40]].all()
    assert (got["owner"][[5, 6, 7, 11, 12, 13, 14, 20]] == -2).all() and np.isnan(got["owner_corr"][20])
    assert got["summary"][0]["eligible"] == S - 7 and got["summary"][0]["candidates"] == S - 8
    assert got["pick"][0] == 21 and got["pick_score"][0] == INF                   # +inf is a score like any other
    if max_corr == 0.7:
        assert got["pick"][1] == 3 and (got["owner"][[3, 17, 40]] == 1).all()     # the duplicates tie: 3 leads, takes them
        assert got["owner_corr"][17].tobytes() == got["owner_corr"][3].tobytes() == got["owner_corr"][40].tobytes()
        assert got["pick"][2] == 4 and got["owner"][4] == 2                       # the mirror hedges the leader and stays
        assert got["pick_corr"][1, 2] == -got["pick_corr"][1, 1]
    elif max_corr == -INF:
        assert got["cluster_size"][0] == S - 8 and (got["pick"][1:] == -1).all() and (got["owner"][want["candidate"]] == 0).all()
    else:
        order = sorted(np.flatnonzero(want["candidate"]).tolist(), key=lambda s: (-scores[s], s))
        assert got["pick"].tolist() == order[:40] and (got["cluster_size"] == 1).all()
        assert order[1:5] == [3, 17, 40, 4]
        zeros = [s for s in order if scores[s] == 0.0]
        assert zeros == sorted(zeros) and {0, 2, 23, 24, 25} <= set(zeros)         # -0.0 == 0.0: by index among them
        assert order[-2:] == [1, 22]                                               # -inf scores come last, by index


def test_nobody_eligible(env):
    S, B = 300, 7
    stats, scores = craft(S, B, range(B), 1, dead=True)
    got, _ = check(env, stats, range(B), scores, 0.7, 5, "dead")
    assert (got["pick"] == -1).all() and np.isnan(got["pick_score"]).all() and not got["cluster_size"].any()
    assert (got["owner"] == -2).all() and np.isnan(got["owner_corr"]).all() and np.isnan(got["pick_corr"]).all()
    assert tuple(got["summary"][0]) == (0, 0, 0, 0, 0)
    scores[:] = np.nan                                      # eligible rows, no candidate among them
    stats, _ = craft(S, B, range(B), 1)
    got, want = check(env, stats, range(B), scores, 0.7, 5, "no candidate")
    assert tuple(got["summary"][0]) == (0, 0, int(want["eligible"].sum()), 0, 0) and want["eligible"].sum() > 250


def test_twelve_decades_of_row_scale(env):
    """one set of shapes, every strategy at its own scale from 1e-6 to 1e6: the clusters are those of the unscaled
    rows (a power-of-ten scale moves a correlation by rounding alone), and the device holds to the model bit for bit"""
    rng = np.random.default_rng(5)
    S, n = 400, 16
    factors = rng.normal(0, 1, (8, n))
    family = rng.integers(0, 8, S)
    base = factors[family] + 0.05 * rng.normal(0, 1, (S, n))
    decade = rng.integers(-6, 7, (S, 1))
    assert decade.min() == -6 and decade.max() == 6
    scale = 10.0 ** decade
    scores = rng.normal(0, 1, S)
    got, _ = check(env, dm.records(base * scale), range(n), scores, 0.9, 20, "scaled")
    plain = dm.diversify(dm.records(base), range(n), scores, 0.9, 20)
    assert np.array_equal(got["pick"], plain["pick"]) and np.array_equal(got["owner"], plain["owner"])
    assert np.nanmax(np.abs(got["owner_corr"] - plain["owner_corr"])) < 1e-14
    assert got["summary"][0]["picked"] == 8 and got["summary"][0]["remaining"] == 0


# ---- determinism and isolation ---------------------------------------------------------------------------------

def test_determinism_and_isolation(env):
    S, B = 700, 70
    ids = [b for b in range(B) if b % 3]
    stats, scores = craft(S, B, ids, 5)
    keys = ("pick", "pick_score", "cluster_size", "owner", "owner_corr", "pick_corr", "summary")
    first = run_div(env, stats, ids, scores, 0.8, 30)
    again = run_div(env, stats, ids, scores, 0.8, 30)
    for name in keys:
        assert first[name].tobytes() == again[name].tobytes(), name
    assert_same(first, dm.diversify(stats, ids, scores, 0.8, 30), "first")
    # a larger call that makes the library take new scratch, a smaller one, and back
    big, big_scores = craft(5000, 128, range(128), 6)
    check(env, big, range(128), big_scores, 0.9, 256, "regrown scratch")
    small, small_scores = craft(5, 3, range(3), 7)
    check(env, small, range(3), small_scores, 0.0, 2, "small after large")
    third = run_div(env, stats, ids, scores, 0.8, 30)
    for name in keys:
        assert first[name].tobytes() == third[name].tobytes(), name


# ---- the existing ranking kernel says the same -----------------------------------------------------------------

@pytest.mark.parametrize("metric", ["sharpe", "mean_reward", "worst_period"])
def test_a_threshold_that_drops_nothing_is_the_ranking(env, metric):
    """max_corr = +inf and the scores of gte_rank_period_stats: the picks and their scores are its top(k) over the
    eligible strategies"""
    S, B, k = 200, 12, 25
    rng = np.random.default_rng(9)
    x = rng.normal(0, 1, (S, B))
    steps = rng.integers(5, 60, (S, B))
    stats = dm.records(x, steps)
    stats["reward_sq_sum"] = x * x / steps * rng.uniform(1.5, 4.0, (S, B))
    stats["reward_sum"][[7, 30]] = 0.25                       # ranked by the score, but constant: no correlation
    stats["steps"][11, 3] = 0                                 # ranked, but not stepped in a correlation period
    board = _board(env, stats)
    sel = [0, 1, 2, 3, 5, 8, 9, 11]
    index, top = (t.cpu().numpy() for t in board.top(256, metric, periods=sel))
    keep = ~np.isin(index, [7, 30, 11])
    assert keep.sum() == S - 3
    pick = board.diversified(k, metric, periods=sel, max_corr=INF)
    assert np.array_equal(pick.picks.cpu().numpy(), index[keep][:k])
    assert pick.scores.cpu().numpy().tobytes() == top[keep][:k].tobytes()
    assert (pick.cluster_size.cpu().numpy() == 1).all()
    assert (pick.num_picked, pick.num_candidates, pick.num_eligible, pick.remaining) == (k, S - 3, S - 3, S - 3 - k)
    assert pick.effective_trials is None and not pick.exhausted
    assert (pick.owner.cpu().numpy()[[7, 30, 11]] == -2).all()


# ---- refusals -------------------------------------------------------------------------------------------------

def test_refusals_leave_every_output_untouched(env):
    import torch
    lib, h = env._lib, env._h
    dev = env._t["obs"].device
    err = lambda: lib.gte_last_error().decode()
    S, B, k = 10, 6, 4
    ids = [0, 1, 3, 4, 5]
    stats, scores = craft(S, B, ids, 1)
    d_stats = device_records(env, stats)
    d_scores = torch.from_numpy(scores.copy()).to(dev)
    sizes = dict(pick=4 * k, pick_score=8 * k, cluster_size=4 * k, owner=4 * S, owner_corr=8 * S, pick_corr=8 * k * k,
                 summary=20)
    out = {name: torch.full((n + 8,), 0x5A, dtype=torch.uint8, device=dev) for name, n in sizes.items()}
    torch.cuda.synchronize()
    ptrs = lambda **over: _abi.GteDiversifyOut(**{**{name: v.data_ptr() for name, v in out.items()}, **over})
    st, sc = C.c_void_p(d_stats.data_ptr()), C.c_void_p(d_scores.data_ptr())
    good, mask = ptrs(), words(ids)
    INVALID = _abi.GTE_ERR_INVALID

    def refused(what, *args):
        assert lib.gte_diversify(*args) == INVALID, what
        assert what in err(), (what, err())
    refused("env is NULL", None, st, S, B, mask, sc, 0.7, k, C.byref(good))
    refused("n_strategies must be >= 1", h, st, 0, B, mask, sc, 0.7, k, C.byref(good))
    refused("n_strategies must be >= 1", h, st, -4, B, mask, sc, 0.7, k, C.byref(good))
    for bad_B in (0, -1, 129):
        refused("n_periods", h, st, S, bad_B, mask, sc, 0.7, k, C.byref(good))
    for bad_k in (0, -1, 257):
        refused("k must lie in [1, 256]", h, st, S, B, mask, sc, 0.7, bad_k, C.byref(good))
    refused("period_mask is NULL", h, st, S, B, None, sc, 0.7, k, C.byref(good))
    for sel in ([], [2], [0, 5]):
        refused("at least three", h, st, S, B, words(sel), sc, 0.7, k, C.byref(good))
    for sel, bit in (([0, 1, 2, 6], 6), ([0, 1, 2, 63], 63), ([0, 1, 2, 64], 64), ([0, 1, 2, 127], 127)):
        refused(f"period_mask selects period {bit}, at or above n_periods 6", h, st, S, B, words(sel), sc, 0.7, k,
                C.byref(good))
    refused("max_corr is NaN", h, st, S, B, mask, sc, float("nan"), k, C.byref(good))
    refused("stats_device", h, None, S, B, mask, sc, 0.7, k, C.byref(good))
    refused("stats_device must be a 16-byte aligned", h, C.c_void_p(d_stats.data_ptr() + 8), S, B, mask, sc, 0.7, k,
            C.byref(good))
    refused("scores_device", h, st, S, B, mask, None, 0.7, k, C.byref(good))
    refused("scores_device must be an 8-byte aligned", h, st, S, B, mask, C.c_void_p(d_scores.data_ptr() + 4), 0.7, k,
            C.byref(good))
    refused("out is NULL", h, st, S, B, mask, sc, 0.7, k, None)
    for name in out:
        refused("out:", h, st, S, B, mask, sc, 0.7, k, C.byref(ptrs(**{name: None})))
    for name in ("pick_score", "owner_corr", "pick_corr"):
        refused("8-byte aligned device pointers", h, st, S, B, mask, sc, 0.7, k,
                C.byref(ptrs(**{name: out[name].data_ptr() + 4})))
    for name in ("pick", "cluster_size", "owner", "summary"):
        refused("4-byte aligned device pointers", h, st, S, B, mask, sc, 0.7, k,
                C.byref(ptrs(**{name: out[name].data_ptr() + 2})))
    # wrong in several ways: the check that stands first reports
    refused("n_strategies must be >= 1", h, None, 0, 0, None, None, float("nan"), 0, None)
    refused("n_periods 0 outside [1, 128]", h, None, S, 0, None, None, float("nan"), 0, None)
    refused("k must lie in", h, None, S, B, None, None, float("nan"), 0, None)
    env.synchronize()
    torch.cuda.synchronize()
    for name, v in out.items():
        assert bool((v == 0x5A).all()), f"{name} was written by a refused call"
    assert d_stats.cpu().numpy().tobytes() == stats.tobytes()
    # any max_corr that is a number goes through
    for fine in (-INF, INF, -3.0, 1e300):
        assert lib.gte_diversify(h, st, S, B, mask, sc, fine, k, C.byref(good)) == _abi.GTE_OK, err()
    env.synchronize()
    # the Python side: what it refuses before any call is made
    board = _board(env, stats)
    for bad_k in (0, 257, 2.5, True):
        with pytest.raises(ValueError, match="k must lie"):
            board.diversified(bad_k)
    with pytest.raises(ValueError, match="NaN"):
        board.diversified(3, max_corr=float("nan"))
    with pytest.raises(ValueError, match="at least three"):
        board.diversified(3, periods=[0, 1])
    with pytest.raises(ValueError, match="at least three"):
        board.diversified(3, corr_periods=[4])
    with pytest.raises(ValueError, match="unknown metric"):
        board.diversified(3, metric="calmar")
    with pytest.raises(ValueError, match="shape"):
        board.diversified(3, scores=np.zeros(S + 1))
    with pytest.raises(IndexError):
        board.diversified(3, corr_periods=[0, 1, 6])
    with pytest.raises(IndexError):
        board.diversified(3).members(3)
    # inside a stream capture: refused, nothing launched
    seen = []
    ready = torch.from_numpy(scores.copy()).to(dev)       # (made before the capture: only the call itself is inside)

    def body(i):
        try:
            board.diversified(3, scores=ready)
        except _abi.GteError as e:
            seen.append(e)
            raise
    env.reset()
    with pytest.raises(Exception):
        env.capture_steps(body, 2)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].status == _abi.GTE_ERR_STATE and "stream capture" in str(seen[0])


# ---- end to end -----------------------------------------------------------------------------------------------

def test_pipeline_backtest_to_diversified():
    """64 envs, 8 strategies, 60 rows in 6 periods: track_periods -> backtest_signals -> by_strategy().diversified(...)
    equals the model applied to .numpy() of the same fold, with the scores the ranking gives; the scores= and
    corr_periods= overrides; effective_trials; members()."""
    import gym_trading_env_amd as gte
    import torch
    from gym_trading_env_amd import periods
    N, S, T = 64, 8, 60
    rng = np.random.default_rng(11)
    close = 100.0 * np.exp(np.cumsum(rng.normal(0, 1e-2, T)))
    feat = rng.normal(0, 1, (T, 3)).astype(np.float32)
    env = gte.BatchedTradingEnv((feat, close), num_envs=N, positions=[-1, 0, 1], windows=None, trading_fees=1e-4,
                                autoreset="next_step", seed=4)
    table = np.repeat(rng.integers(0, 3, (S, T // 4)), 4, axis=1).astype(np.int8)
    table[5] = table[2]                                # strategy 5 is strategy 2 again
    env.bind_signals(table)
    env.reset()
    env.track_periods(periods.blocks(T, 6))
    by = env.backtest_signals(55).period_stats.by_strategy()
    host = by.numpy()
    stepped = np.flatnonzero((host["steps"] > 0).all(axis=0)).tolist()
    assert len(stepped) >= 4, host["steps"]
    sel, corr_sel = stepped, stepped[1:]

    def same(result, want, k):
        got = result.numpy()
        for a, b in (("picks", "pick"), ("scores", "pick_score"), ("cluster_size", "cluster_size"), ("owner", "owner"),
                     ("owner_corr", "owner_corr"), ("corr", "pick_corr")):
            assert got[a].shape == want[b].shape, (a, got[a].shape)
            assert (dm.same_f64(got[a], want[b]) if b in FLOATS else np.array_equal(got[a], want[b])), (a, got[a], want[b])
        s = want["summary"][0]
        assert (got["num_picked"], got["num_candidates"], got["num_eligible"], got["remaining"]) == \
            (int(s["picked"]), int(s["candidates"]), int(s["eligible"]), int(s["remaining"]))
        assert result.exhausted == (s["remaining"] == 0)
        assert result.effective_trials == (int(s["picked"]) if s["remaining"] == 0 else None)
        assert got["k"] == k and result.corr.shape == (k, k)
    sharpe = by.score("sharpe", sel).cpu().numpy()
    res = by.diversified(3, periods=sel)                                     # sharpe, 0.7
    assert isinstance(res, gte.Diversified) and res.picks.is_cuda and res.owner.is_cuda and res.corr.is_cuda
    assert res.max_corr == 0.7 and res.corr_periods == sel
    want = dm.diversify(host, sel, sharpe, 0.7, 3)
    same(res, want, 3)
    assert want["summary"][0]["candidates"] >= 2
    for r in range(3):
        assert res.members(r).cpu().numpy().tolist() == np.flatnonzero(want["owner"] == r).tolist()
    # all of them, at a threshold that drops nothing: exhausted, one cluster per candidate
    every = by.diversified(256, periods=sel, max_corr=1.5)
    same(every, dm.diversify(host, sel, sharpe, 1.5, 256), 256)
    assert every.exhausted and every.effective_trials == every.num_candidates == every.num_picked
    one = by.diversified(1, periods=sel, max_corr=1.5)
    assert one.effective_trials is None and one.remaining == one.num_candidates - 1
    # min_steps: strategies below it are no candidates, as top() does not rank them
    pooled = host["steps"][:, sel].sum(axis=1)
    cut = int(np.sort(pooled)[S // 2]) + 1
    masked = np.where(pooled >= cut, sharpe, np.nan)
    same(by.diversified(4, periods=sel, min_steps=cut), dm.diversify(host, sel, masked, 0.7, 4), 4)
    # the overrides: other correlation periods, another metric, explicit scores from NumPy and from torch
    same(by.diversified(4, "mean_reward", periods=sel, corr_periods=corr_sel, max_corr=0.2),
         dm.diversify(host, corr_sel, by.score("mean_reward", sel).cpu().numpy(), 0.2, 4), 4)
    mine = np.arange(S, dtype=np.float64)[::-1].copy()
    mine[3] = np.nan
    same(by.diversified(5, corr_periods=corr_sel, max_corr=0.5, scores=mine),
         dm.diversify(host, corr_sel, mine, 0.5, 5), 5)
    same(by.diversified(5, periods=sel, max_corr=-0.5, scores=torch.from_numpy(mine).to(res.picks.device)),
         dm.diversify(host, sel, mine, -0.5, 5), 5)
    assert by.numpy().tobytes() == host.tobytes()       # nothing here changes a record
    env.close()


def test_diversified_example():
    """examples/backtest_diversified.py runs at a small shape in a child process and exits 0, both shortlists and the
    count of clusters printed"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "backtest_diversified.py"), "--fast", "3",
                        "--slow", "3", "--replicas", "16", "--steps", "900", "--rows", "1500", "--periods", "12",
                        "--top", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "diversified()" in r.stdout and "mean test Sharpe" in r.stdout and "candidates" in r.stdout
