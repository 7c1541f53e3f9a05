"""The probability of backtest overfitting on the device (gte_cscv, include/gte.h) against its model
(tests/cscv_model.py), bit for bit on every output, NaN as NaN: S x B x G over the wave, tile and register-variant
edges with generated, hand-made and purged split tables across the split chunk's edge and all three metrics; crafted
records (ineligible, never trading, constant, duplicate strategies, -0.0, nobody eligible); single-period groups
against the existing ranking kernel; determinism and isolation; every refusal, with the outputs untouched; the
Python pipeline end to end; the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import cscv_model as cm
from gym_trading_env_amd import _abi, periods
from leaderboard_gpu import GUARD, assert_arrays_same, board as _board, device_records, guarded, make_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = (("best", np.int32), ("is_score", np.float64), ("oos_score", np.float64), ("below", np.int32),
           ("equal", np.int32), ("ranked", np.int32))
CHUNK = _abi.GTE_CSCV_CHUNK
METRICS = (cm.MEAN_REWARD, cm.SHARPE, cm.REWARD_SUM)


@pytest.fixture(scope="module")
def env():
    e = make_env()
    yield e
    e.close()


def random_splits(G, n, seed, purge):
    """n hand-made splits over G groups: every group in sample, out of sample or (with `purge`) in neither; both sides
    non-empty"""
    rng = np.random.default_rng(seed)
    is_g, oos_g = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for c in range(n):
        while True:
            side = rng.choice(3, G, p=[0.4, 0.4, 0.2] if purge else [0.5, 0.5, 0.0])
            if (side == 0).any() and (side == 1).any():
                break
        is_g[c] = sum(1 << g for g in np.flatnonzero(side == 0))
        oos_g[c] = sum(1 << g for g in np.flatnonzero(side == 1))
    return is_g, oos_g


def craft(S, B, seed, groups, dead=False):
    """[S, B] strategy period records: period returns over twelve decades with sums of squares and steps of their
    own; a row that dominates and its duplicates (a tie goes to the lowest index); rows that never trade (Sharpe
    0 / 0: eligible, not ranked); rows of a constant reward (Sharpe +inf and -inf); -0.0; ineligible rows (NaN, +inf,
    -inf in a grouped period; a group without steps); and NaN / inf / no step in periods of NO group, which must
    not matter"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (S, B)) * 10.0 ** rng.integers(-6, 6, (S, 1))
    steps = rng.integers(1, 50, (S, B))
    sq = x * x / steps * rng.uniform(1.0, 4.0, (S, B))
    grouped = np.array(sorted(b for row in groups for b in cm.periods_of(row)))
    free = np.setdiff1d(np.arange(B), grouped)
    first_group, last_group = cm.periods_of(groups[0]), cm.periods_of(groups[-1])

    def row(k, xs, sqs=None, st=None):
        if k < S:
            x[k] = xs
            sq[k] = xs * xs if sqs is None else sqs
            if st is not None:
                steps[k] = st
    if S > 3:
        lead = np.abs(rng.normal(0, 1, B)) * 1e7 + 1e8
        for k in (3, 17, 40):                                       # 17 and 40 duplicate 3, which wins before them
            row(k, lead, lead * lead * 1.5, np.full(B, 7))
    row(5, np.zeros(B), np.zeros(B))                                # never trades
    row(6, np.full(B, 0.25) * 4, np.full(B, 0.0625) * 4, np.full(B, 4))      # 0.25 at every step: Sharpe +inf
    row(7, np.full(B, -0.5) * 2, np.full(B, 0.25) * 2, np.full(B, 2))        # -0.5 at every step: Sharpe -inf
    row(8, np.where(np.arange(B) % 2 == 0, -0.0, 0.0), np.zeros(B))          # -0.0
    for k, bad in ((11, np.nan), (12, np.inf), (13, -np.inf)):
        if k < S:
            x[k, grouped[k % len(grouped)]] = bad
    if 15 < S:
        steps[14, last_group] = 0                                   # a group without steps
        sq[15, first_group[0]] = np.inf                             # a sum of squares that is not finite
    if len(free):
        x[:, free[0]] = np.nan
        sq[::2, free[-1]] = np.inf
        steps[:, free[-1]] = 0
    if dead:
        steps[:, first_group] = 0
    return cm.records(x, sq, steps)


def run_cscv(env, stats, groups, is_g, oos_g, metric, clobber=False):
    """gte_cscv over host-made records and tables -> dict of host arrays, like the model's; every output stands between
    guard words, which must come back untouched"""
    import torch
    dev = env._t["obs"].device
    S, B = stats.shape
    n = len(is_g)
    d_stats = device_records(env, stats)
    whole, out = {}, {}
    for k, t in OUTPUTS:
        whole[k], out[k] = guarded(torch, dev, n, getattr(torch, np.dtype(t).name), -7)
    whole["summary"], out["summary"] = guarded(torch, dev, 24, torch.uint8, 0xAB)   # (8 bytes on either side)
    ptrs = _abi.GteCscvOut(**{k: v.data_ptr() for k, v in out.items()})
    groups, is_g, oos_g = (np.ascontiguousarray(a).copy() for a in (groups, is_g, oos_g))
    torch.cuda.synchronize()
    _abi.check(env._lib, env._lib.gte_cscv(
        env._h, C.c_void_p(d_stats.data_ptr()), S, B, C.c_void_p(groups.ctypes.data), len(groups),
        C.c_void_p(is_g.ctypes.data), C.c_void_p(oos_g.ctypes.data), n, metric, C.byref(ptrs)))
    if clobber:     # the tables are the caller's again when the call returns
        groups[:], is_g[:], oos_g[:] = 0, 0, 0
    env.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["summary"] = got["summary"].view(cm.SUMMARY)
    got["stats_after"] = d_stats.cpu().numpy().tobytes()
    for k, v in whole.items():
        edge = torch.cat((v[:GUARD], v[-GUARD:])).cpu().numpy()
        assert (edge == (0xAB if k == "summary" else -7)).all(), f"guard words of {k} were written"
    return got


def assert_same(got, want, tag):
    assert_arrays_same(got, want, [k for k, _ in OUTPUTS], [k for k, t in OUTPUTS if t is np.float64], tag, dict(OUTPUTS))
    assert got["summary"].tobytes() == want["summary"].tobytes(), (tag, got["summary"], want["summary"])


def _groups(B, G, rng):
    """G groups over B periods: contiguous ones over all periods, or (B = 128) over a scattered subset with bits in both
    words, so that some periods are in no group"""
    if B == 128 and G < 32:
        ids = np.sort(rng.choice(128, 90, replace=False))
        ids = np.union1d(ids, [0, 63, 64, 127])
        return periods.cscv_groups(ids, G)
    if B == 7 and G == 2:
        return periods.cscv_groups([0, 1, 2, 4, 6], 2)
    return periods.cscv_groups(range(B), G)


@pytest.mark.parametrize("B", [2, 7, 128])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 1000])
def test_every_output_equals_the_model(env, S, B):
    """Per (S, B): G = 2, 7, 8 and 32 where B has that many periods (the 8-, 16- and 32-register variants of the two
    passes: 2, 7 and 8 take the first, 32 the last; test_crafted_records runs the middle one), the generated table for
    even G, hand-made and purged tables of 1, chunk - 1, chunk and chunk + 1 splits, the three metrics in turn.  S
    below, at and above a wavefront, a tile of 256 and several tiles."""
    rng = np.random.default_rng(S * 131 + B)
    calls = 0
    used = set()
    for G in (2, 7, 8, 32):
        if G > B:
            continue
        groups = _groups(B, G, rng)
        tables = []
        if G in (2, 8):
            tables.append(("all", periods.cscv_splits(G)))
        sizes = {2: (1,), 7: (CHUNK - 1, CHUNK + 1), 8: (CHUNK,), 32: (1, CHUNK + 1)}[G]
        for n in sizes:
            if G == 2:      # two groups: the two splits there are, again and again
                tables.append((f"hand{n}", (np.array([1, 2] * n, np.uint32)[:n], np.array([2, 1] * n, np.uint32)[:n])))
            else:
                tables.append((f"hand{n}", random_splits(G, n, S + B + G + n, purge=(n != CHUNK))))
        for name, (is_g, oos_g) in tables:
            metric = METRICS[calls % 3]
            calls += 1
            used.add(metric)
            stats = craft(S, B, S + B + G, groups)
            got = run_cscv(env, stats, groups, is_g, oos_g, metric)
            want = cm.cscv(stats, groups, is_g, oos_g, metric)
            assert_same(got, want, f"S={S} B={B} G={G} {name} metric={metric}")
            assert got["stats_after"] == stats.tobytes()
    assert calls >= 2 and (len(used) == 3 or B == 2)


@pytest.mark.parametrize("metric", METRICS)
def test_crafted_records(env, metric):
    """S = 300, B = 24, G = 12 (the 16-register variant), all 924 splits: what each crafted row is there for is seen"""
    S, B, G = 300, 24, 12
    groups = periods.cscv_groups([b for b in range(B) if b not in (5, 20)], G)
    is_g, oos_g = periods.cscv_splits(G)
    stats = craft(S, B, 77, groups)
    got = run_cscv(env, stats, groups, is_g, oos_g, metric)
    want = cm.cscv(stats, groups, is_g, oos_g, metric)
    assert_same(got, want, f"crafted metric={metric}")
    elig = want["eligible"]
    assert not elig[[11, 12, 13, 14, 15]].any() and elig[[3, 5, 6, 7, 8, 17, 40]].all()
    assert got["summary"][0]["eligible"] == S - 5 and got["summary"][0]["valid"] == len(is_g)
    if metric == cm.SHARPE:
        assert (got["best"] == 6).all() and (got["is_score"] == np.inf).all() and (got["oos_score"] == np.inf).all()
        assert (got["ranked"] == S - 5 - 2).all()             # rows 5 and 8 never trade: 0 / 0, eligible, unranked
        assert (got["equal"] == 1).all() and (got["below"] == S - 5 - 2 - 1).all()
    else:
        assert (got["best"] == 3).all() and (got["equal"] == 3).all()       # 3 wins before its duplicates 17 and 40
        assert (got["ranked"] == S - 5).all() and (got["below"] == S - 5 - 3).all()
    assert got["summary"][0]["overfit"] == 0 and got["summary"][0]["loss"] == 0


def test_nobody_eligible(env):
    groups = periods.cscv_groups(range(7), 4)
    is_g, oos_g = periods.cscv_splits(4)
    stats = craft(300, 7, 1, groups, dead=True)
    got = run_cscv(env, stats, groups, is_g, oos_g, cm.SHARPE)
    assert_same(got, cm.cscv(stats, groups, is_g, oos_g, cm.SHARPE), "dead")
    assert (got["best"] == -1).all() and np.isnan(got["is_score"]).all() and np.isnan(got["oos_score"]).all()
    assert not got["below"].any() and not got["equal"].any() and not got["ranked"].any()
    assert tuple(got["summary"][0]) == (6, 0, 0, 0, 0, 0)


def test_winners_that_lose_out_of_sample(env):
    """records made so that the in-sample winner is the out-of-sample loser in every split: PBO 1, and the
    probability of loss 1"""
    S, G = 70, 6
    x = np.random.default_rng(2).normal(0, 1e-3, (S, G))
    for g in range(G):      # strategy g is far ahead in group g alone and far behind everywhere else
        x[g] = -1.0
        x[g, g] = 50.0
    stats = cm.records(x, x * x + 1.0)                # one step per period
    groups = periods.cscv_groups(range(G), G)
    is_g = np.array([1 << g for g in range(G)], np.uint32)
    oos_g = (np.uint32(63) & ~is_g).astype(np.uint32)
    got = run_cscv(env, stats, groups, is_g, oos_g, cm.MEAN_REWARD)
    want = cm.cscv(stats, groups, is_g, oos_g, cm.MEAN_REWARD)
    assert_same(got, want, "losers")
    assert got["best"].tolist() == list(range(G)) and tuple(got["summary"][0]) == (G, G, G, G, S, 0)
    assert (got["oos_score"] == -1.0).all() and (got["equal"] == 1).all() and not got["below"].any()
    assert (got["ranked"] == S).all()


# ---- single-period groups: the existing ranking kernel says the same ---------------------------------------------

@pytest.mark.parametrize("metric", ["mean_reward", "sharpe", "reward_sum"])
def test_single_period_groups_agree_with_the_ranking(env, metric):
    S, B = 333, 8
    rng = np.random.default_rng(9)
    x = rng.normal(0, 1, (S, B))
    steps = rng.integers(5, 60, (S, B))
    stats = cm.records(x, x * x / steps * rng.uniform(1.5, 4.0, (S, B)), steps)
    board = _board(env, stats)
    check = board.cscv(groups=B, metric=metric)                 # eight groups of one period
    assert check.num_groups == B and check.num_splits == 70 and check.metric == metric
    best, is_score = check.best.cpu().numpy(), check.is_score.cpu().numpy()
    oos_score = check.oos_score.cpu().numpy()
    assert check.num_eligible == S
    for c in (0, 1, 17, 35, 68, 69):
        is_periods = cm.groups_of(check.is_groups[c], B)
        oos_periods = cm.groups_of(check.oos_groups[c], B)
        scores = board.score(metric, periods=is_periods).cpu().numpy()
        assert scores[best[c]].tobytes() == is_score[c].tobytes(), c
        assert board.score(metric, periods=oos_periods).cpu().numpy()[best[c]].tobytes() == oos_score[c].tobytes(), c
        index, top = board.top(1, metric, periods=is_periods)
        assert int(index[0]) == best[c] and float(top[0]) == is_score[c], c


# ---- determinism and isolation ---------------------------------------------------------------------------------

def test_determinism_and_isolation(env):
    S, B, G = 700, 70, 10
    groups = periods.cscv_groups([b for b in range(B) if b % 3], G)
    is_g, oos_g = periods.cscv_splits(G)
    stats = craft(S, B, 5, groups)
    keys = [k for k, _ in OUTPUTS] + ["summary"]
    first = run_cscv(env, stats, groups, is_g, oos_g, cm.SHARPE, clobber=True)
    again = run_cscv(env, stats, groups, is_g, oos_g, cm.SHARPE)
    for k in keys:
        assert first[k].tobytes() == again[k].tobytes(), k
    assert first["stats_after"] == stats.tobytes()
    assert_same(first, cm.cscv(stats, groups, is_g, oos_g, cm.SHARPE), "clobbered tables")
    # a reality check and a ranking in between, a larger call that makes the library take new scratch, a smaller one
    board = _board(env, stats)
    mask = np.arange(B) % 3 != 0
    rc0 = board.reality_check(periods=mask, n_resamples=100, seed=3).numpy()
    top0 = [t.cpu().numpy() for t in board.top(5, "reward_sum", periods=mask)]
    big_groups = periods.cscv_groups(range(128), 32)
    run_cscv(env, craft(3000, 128, 6, big_groups), big_groups, *random_splits(32, 600, 1, True), cm.MEAN_REWARD)
    small = periods.cscv_groups(range(3), 2)
    run_cscv(env, craft(5, 3, 7, small), small, *periods.cscv_splits(2), cm.REWARD_SUM)
    third = run_cscv(env, stats, groups, is_g, oos_g, cm.SHARPE)
    for k in keys:
        assert first[k].tobytes() == third[k].tobytes(), k
    rc1 = board.reality_check(periods=mask, n_resamples=100, seed=3).numpy()
    top1 = [t.cpu().numpy() for t in board.top(5, "reward_sum", periods=mask)]
    for k in ("mean", "boot_sum", "boot_sq_sum", "count_ge", "count_adj", "max_stats", "max_index"):
        assert rc0[k].tobytes() == rc1[k].tobytes(), k
    assert rc0["p_value"] == rc1["p_value"] or (np.isnan(rc0["p_value"]) and np.isnan(rc1["p_value"]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(top0, top1))
    assert board.numpy().tobytes() == stats.tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------

def test_refusals_leave_every_output_untouched(env):
    import torch
    lib, h = env._lib, env._h
    dev = env._t["obs"].device
    err = lambda: lib.gte_last_error().decode()
    S, B, G = 10, 6, 4
    groups = periods.cscv_groups([0, 1, 3, 4, 5], G)          # period 2 in no group
    is_g, oos_g = periods.cscv_splits(G)
    n = len(is_g)
    stats = craft(S, B, 1, groups)
    d_stats = device_records(env, stats)
    out = {k: torch.full((n * 8,), 0x5A, dtype=torch.uint8, device=dev) for k, _ in OUTPUTS}
    out["summary"] = torch.full((24,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ptrs = lambda **over: _abi.GteCscvOut(**{**{k: v.data_ptr() for k, v in out.items()}, **over})
    st = C.c_void_p(d_stats.data_ptr())
    held = []       # (every host table a call is given stays alive until the test ends)

    def hp(a):
        held.append(a)
        return C.c_void_p(a.ctypes.data)
    INVALID = _abi.GTE_ERR_INVALID
    good = ptrs()
    call = lib.gte_cscv

    def refused(what, *args):
        assert call(*args) == INVALID, what
        assert what in err(), (what, err())
    SH = cm.SHARPE
    refused("env is NULL", None, st, S, B, hp(groups), G, hp(is_g), hp(oos_g), n, SH, C.byref(good))
    refused("n_strategies must be >= 1", h, st, 0, B, hp(groups), G, hp(is_g), hp(oos_g), n, SH, C.byref(good))
    for bad_B in (0, -1, 129):
        refused("n_periods", h, st, S, bad_B, hp(groups), G, hp(is_g), hp(oos_g), n, SH, C.byref(good))
    for bad_G in (1, 0, -3, 33):
        refused("n_groups", h, st, S, B, hp(groups), bad_G, hp(is_g), hp(oos_g), n, SH, C.byref(good))
    for bad_n in (0, -1, 65537):
        refused("n_splits", h, st, S, B, hp(groups), G, hp(is_g), hp(oos_g), bad_n, SH, C.byref(good))
    for bad_metric in (3, 4, 5, -1, 6):
        refused("metric", h, st, S, B, hp(groups), G, hp(is_g), hp(oos_g), n, bad_metric, C.byref(good))
    refused("stats_device", h, None, S, B, hp(groups), G, hp(is_g), hp(oos_g), n, SH, C.byref(good))
    refused("stats_device must be a 16-byte aligned", h, C.c_void_p(d_stats.data_ptr() + 8), S, B, hp(groups), G,
            hp(is_g), hp(oos_g), n, SH, C.byref(good))
    refused("group_masks", h, st, S, B, None, G, hp(is_g), hp(oos_g), n, SH, C.byref(good))
    refused("group_masks", h, st, S, B, C.c_void_p(groups.ctypes.data + 4), G, hp(is_g), hp(oos_g), n, SH, C.byref(good))
    refused("is_groups and oos_groups", h, st, S, B, hp(groups), G, None, hp(oos_g), n, SH, C.byref(good))
    refused("is_groups and oos_groups", h, st, S, B, hp(groups), G, hp(is_g), None, n, SH, C.byref(good))
    refused("is_groups and oos_groups", h, st, S, B, hp(groups), G, hp(is_g), C.c_void_p(oos_g.ctypes.data + 2), n - 1,
            SH, C.byref(good))
    refused("out is NULL", h, st, S, B, hp(groups), G, hp(is_g), hp(oos_g), n, SH, None)
    for k in out:
        refused("out:", h, st, S, B, hp(groups), G, hp(is_g), hp(oos_g), n, SH, C.byref(ptrs(**{k: None})))
    refused("4-byte aligned device pointers", h, st, S, B, hp(groups), G, hp(is_g), hp(oos_g), n, SH,
            C.byref(ptrs(below=out["below"].data_ptr() + 2)))
    refused("out: is_score and oos_score must be 8-byte", h, st, S, B, hp(groups), G, hp(is_g), hp(oos_g), n, SH,
            C.byref(ptrs(oos_score=out["oos_score"].data_ptr() + 4)))
    # wrong in several ways: the check that stands first reports
    refused("n_strategies must be >= 1", h, None, 0, 0, None, 0, None, None, 0, 9, None)
    refused("n_periods 0 outside [1, 128]", h, None, S, 0, None, 0, None, None, 0, 9, None)
    refused("n_groups 0 outside [2, 32]", h, None, S, B, None, 0, None, None, 0, 9, None)
    # the group table: the message names the first offending group
    def with_group(g, w0, w1=0):
        t = groups.copy()
        t[g] = (w0, w1)
        return t
    refused("group 2 is empty", h, st, S, B, hp(with_group(2, 0)), G, hp(is_g), hp(oos_g), n, SH, C.byref(good))
    for bit in (6, 63):
        refused(f"group 1 selects period {bit}, at or above n_periods 6", h, st, S, B,
                hp(with_group(1, int(groups[1, 0]) | 1 << bit)), G, hp(is_g), hp(oos_g), n, SH, C.byref(good))
    refused("group 3 selects period 64", h, st, S, B, hp(with_group(3, int(groups[3, 0]), 1)), G, hp(is_g), hp(oos_g),
            n, SH, C.byref(good))
    refused("group 2 shares a period with an earlier group", h, st, S, B,
            hp(with_group(2, int(groups[2, 0]) | int(groups[0, 0]))), G, hp(is_g), hp(oos_g), n, SH, C.byref(good))
    refused("group 1 is empty", h, st, S, B, hp(with_group(3, 1 << 2) * np.array([[1], [0], [1], [1]], np.uint64)), G,
            hp(is_g), hp(oos_g), n, SH, C.byref(good))      # groups 1 is empty AND 3 is fine: the first is named
    # the split tables: the message names the first offending split
    def with_split(c, a, b):
        i2, o2 = is_g.copy(), oos_g.copy()
        i2[c], o2[c] = a, b
        return i2, o2
    for c, a, b, what in ((4, 0, 3, "split 4 has an empty in-sample side"),
                          (0, 3, 0, "split 0 has an empty out-of-sample side"),
                          (5, 3, 16, "split 5 uses a group at or above n_groups 4"),
                          (5, 1 << 31, 1, "split 5 uses a group at or above n_groups 4"),
                          (2, 3, 6, "split 2 has a group on both sides")):
        i2, o2 = with_split(c, a, b)
        refused(what, h, st, S, B, hp(groups), G, hp(i2), hp(o2), n, SH, C.byref(good))
    i2, o2 = with_split(1, 3, 3)
    i2[3] = 0
    refused("split 1 has a group on both sides", h, st, S, B, hp(groups), G, hp(i2), hp(o2), n, SH, C.byref(good))
    env.synchronize()
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v == 0x5A).all()), f"{k} was written by a refused call"
    assert d_stats.cpu().numpy().tobytes() == stats.tobytes()
    # the Python side: what it refuses before any call is made, and what it hands to the library
    board = _board(env, stats)
    with pytest.raises(ValueError, match="cscv scores by"):
        board.cscv(metric="worst_period")
    with pytest.raises(ValueError, match="unknown metric"):
        board.cscv(metric="calmar")
    with pytest.raises(ValueError, match="at least two"):
        board.cscv(periods=[1])
    with pytest.raises(ValueError):
        board.cscv(groups=7)                    # more groups than periods
    with pytest.raises(ValueError, match="even"):
        board.cscv(groups=3)                    # an odd G has no generated table
    with pytest.raises(ValueError, match="shape"):
        board.cscv(groups=np.zeros((3, 3), np.uint64))
    with pytest.raises(ValueError, match="two arrays"):
        board.cscv(groups=3, splits=(np.array([1, 2], np.uint32), np.array([2], np.uint32)))
    with pytest.raises(_abi.GteError, match="split 0 has a group on both sides"):
        board.cscv(groups=3, splits=([3], [1]))
    assert board.cscv(groups=3, splits=([1, 2], [6, 4])).num_valid >= 0     # an odd G with a caller's table
    # inside a stream capture: refused, nothing launched
    seen = []

    def body(i):
        try:
            board.cscv(groups=2)
        except _abi.GteError as e:
            seen.append(e)
            raise
    env.reset()
    with pytest.raises(Exception):
        env.capture_steps(body, 2)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].status == _abi.GTE_ERR_STATE and "stream capture" in str(seen[0])


# ---- end to end -----------------------------------------------------------------------------------------------

def test_pipeline_backtest_to_overfit_check():
    """256 envs, 16 strategies, 6 periods: backtest_signals -> period_stats.by_strategy().cscv(groups=4) equals the
    model applied to .numpy() of the same fold; the derived figures are the stated formulas on the model's counts."""
    import gym_trading_env_amd as gte
    import torch
    N, S, T = 256, 16, 400
    rng = np.random.default_rng(11)
    close = 100.0 * np.exp(np.cumsum(rng.normal(0, 1e-2, T)))
    feat = rng.normal(0, 1, (T, 3)).astype(np.float32)
    env = gte.BatchedTradingEnv((feat, close), num_envs=N, positions=[-1, 0, 1], windows=None, trading_fees=1e-4,
                                max_episode_duration=40, autoreset="next_step", seed=4)
    table = np.repeat(rng.integers(0, 3, (S, T // 4)), 4, axis=1).astype(np.int8)
    table[5] = -1                                      # strategy 5 holds its first position
    env.bind_signals(table)
    env.reset()
    env.track_periods(periods.blocks(T, 6))
    by = env.backtest_signals(150).period_stats.by_strategy()
    host = by.numpy()
    check = by.cscv(groups=4)
    assert isinstance(check, gte.OverfitCheck) and check.num_groups == 4 and check.num_splits == 6
    assert check.metric == "sharpe" and check.best.is_cuda and check.rel_rank.is_cuda and check.logit.is_cuda
    groups = periods.cscv_groups(range(6), 4)
    assert np.array_equal(check.groups, groups)
    is_g, oos_g = periods.cscv_splits(4)
    want = cm.cscv(host, groups, is_g, oos_g, cm.SHARPE)
    got = check.numpy()
    for k, t in OUTPUTS:
        assert (cm.same_f64(got[k], want[k]) if t is np.float64 else np.array_equal(got[k], want[k])), k
    s = want["summary"][0]
    assert s["valid"] >= 1 and s["eligible"] >= 2
    assert (check.num_valid, check.num_eligible) == (int(s["valid"]), int(s["eligible"]))
    assert check.pbo == cm.pbo(want) and check.prob_loss == cm.prob_loss(want) and 0.0 <= check.pbo <= 1.0
    valid, rel_rank, logit, line = cm.derived(want)
    np.testing.assert_array_equal(got["valid"], valid)
    np.testing.assert_allclose(got["rel_rank"], rel_rank, rtol=1e-12, atol=0.0, equal_nan=True)
    np.testing.assert_allclose(got["logit"], logit, rtol=1e-12, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(check.degradation(), line, rtol=1e-12, atol=1e-12, equal_nan=True)
    # other selections, metrics and tables go the same way: periods, a [G, 2] table, a caller's purged splits
    sel = [0, 1, 3, 4, 5]
    for kw, (g2, m2, sp2) in (
            (dict(periods=sel, groups=2, metric="mean_reward"), (periods.cscv_groups(sel, 2), cm.MEAN_REWARD, None)),
            (dict(groups=groups, metric="reward_sum"), (groups, cm.REWARD_SUM, None)),
            (dict(groups=torch.from_numpy(groups.astype(np.int64)), splits=([1, 2, 4], [8, 12, 3])),
             (groups, cm.SHARPE, (np.array([1, 2, 4], np.uint32), np.array([8, 12, 3], np.uint32)))),
            (dict(), (periods.cscv_groups(range(6), 6), cm.SHARPE, None))):     # None: six periods, six groups
        c2 = by.cscv(**kw)
        i2, o2 = sp2 if sp2 is not None else periods.cscv_splits(len(g2))
        w2 = cm.cscv(host, g2, i2, o2, m2)
        got2 = c2.numpy()
        for k, t in OUTPUTS:
            assert (cm.same_f64(got2[k], w2[k]) if t is np.float64 else np.array_equal(got2[k], w2[k])), (kw, k)
        assert (got2["num_valid"], got2["num_overfit"], got2["num_loss"]) == tuple(int(w2["summary"][0][f]) for f in
                                                                                 ("valid", "overfit", "loss"))
        pb = cm.pbo(w2)
        assert c2.pbo == pb or (np.isnan(pb) and np.isnan(c2.pbo))
    assert by.numpy().tobytes() == host.tobytes()       # the check changes no record
    env.close()


def test_overfitting_example(capsys):
    """examples/backtest_overfitting.py runs at a small shape and prints, for both cases, a PBO in [0, 1] that is the
    result object's and the model's."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import backtest_overfitting as ex
    finally:
        sys.path.pop(0)
    out = ex.main(n_fast=3, n_slow=3, replicas=16, K=900, T=1500, n_periods=12, groups=6, n_resamples=100)
    text = capsys.readouterr().out
    lines = [l for l in text.splitlines() if " PBO " in l]
    assert len(lines) == 2 and lines[0].startswith("random walk") and lines[1].startswith("one real edge")
    groups = periods.cscv_groups(range(12), 6)
    is_g, oos_g = periods.cscv_splits(6)
    for line, case in zip(lines, (out["noise"], out["edge"])):
        shown = float(line.split(" PBO ")[1].split()[0])
        assert 0.0 <= shown <= 1.0 and abs(shown - case["pbo"]) < 5.1e-4
        assert case["splits"] == 20 and case["valid"] == 20 and case["eligible"] == case["strategies"]
        want = cm.cscv(case["by_strategy"], groups, is_g, oos_g, cm.SHARPE)
        assert case["pbo"] == cm.pbo(want) and case["prob_loss"] == cm.prob_loss(want)
        assert np.array_equal(case["check"].best.cpu().numpy(), want["best"])
    peek = out["edge"]["strategies"] - 1
    assert out["edge"]["strategies"] == out["noise"]["strategies"] + 1
    assert out["edge"]["winners"].tolist() == [peek] and out["edge"]["pbo"] == 0.0 and out["edge"]["prob_loss"] == 0.0
