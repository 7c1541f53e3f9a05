"""The test for superior predictive ability and its step-down on the device (gte_spa_test, include/gte.h) against its
model (tests/spa_model.py), bit for bit on every output, NaN as NaN: the boards of test_gpu_bootstrap.py (`craft`:
twelve decades, wild, ineligible and duplicate rows) with a zero-variance row and a few winners added, over S across
a tile of 256, n in (3, 8, 12, 65) with masks in both words, R across the chunk of 16 and the slab of 256, with and
without a benchmark, caller-made weights, crit_rank at both ends, max_rounds 1 and 8; the board that rejects in two
rounds, one that rejects everybody and one with nobody studentised; the nested reality check against
gte_reality_check called alone; determinism and isolation; every refusal, with the outputs untouched; the Python
pipeline end to end; the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bootstrap_model as bm
import spa_model as sm
from gym_trading_env_amd import _abi
from leaderboard_gpu import assert_arrays_same, device_records, make_env, mask_words
from test_gpu_bootstrap import OUTPUTS as RC_OUTPUTS, craft, run_check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (0x5BA << 32) | 777   # the high word set
OUTPUTS = (("t_stat", np.float64), ("std_error", np.float64), ("recentred", np.uint8), ("count_adj", np.int32),
           ("rejected_round", np.int32), ("max_stat", np.float64), ("max_index", np.int32), ("crit", np.float64),
           ("round_rejected", np.int32))
TWO_ROUND_SEED = 1           # test_spa_model_cpu.py asserts of the model that this board rejects in rounds 0 and 1


@pytest.fixture(scope="module")
def env():
    e = make_env()
    yield e
    e.close()


def lengths(S, R, rounds):
    return dict(t_stat=S, std_error=S, recentred=S, count_adj=S, rejected_round=S, max_stat=3 * R, max_index=3 * R,
                crit=rounds, round_rejected=rounds)


def run_spa(env, stats, mask, benchmark, w, threshold, rank, rounds):
    """gte_spa_test over host-made records and weights -> dict of host arrays, like the model's ("rc": the nested
    reality check's)"""
    import torch
    dev = env._t["obs"].device
    S, B = stats.shape
    R = w.shape[0]
    d_stats = device_records(env, stats)
    d_w = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    d_b = None if benchmark is None else torch.from_numpy(np.ascontiguousarray(benchmark)).to(dev)
    rc = {k: torch.full((S if k not in ("max_stat", "max_index") else R,), -7, dtype=getattr(torch, np.dtype(t).name),
                        device=dev) for k, t in RC_OUTPUTS}
    rc["summary"] = torch.full((24,), 0xAB, dtype=torch.uint8, device=dev)
    size = lengths(S, R, rounds)
    out = {k: torch.full((size[k],), 9, dtype=getattr(torch, np.dtype(t).name), device=dev) for k, t in OUTPUTS}
    out["summary"] = torch.full((40,), 0xAB, dtype=torch.uint8, device=dev)
    rc_ptrs = _abi.GteRealityCheckOut(**{k: v.data_ptr() for k, v in rc.items()})
    ptrs = _abi.GteSpaOut(**{k: v.data_ptr() for k, v in out.items()})
    torch.cuda.synchronize()
    _abi.check(env._lib, env._lib.gte_spa_test(
        env._h, C.c_void_p(d_stats.data_ptr()), S, B, mask_words(mask), None if d_b is None else C.c_void_p(d_b.data_ptr()),
        C.c_void_p(d_w.data_ptr()), R, float(threshold), int(rank), int(rounds), C.byref(rc_ptrs), C.byref(ptrs)))
    env.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["summary"] = got["summary"].view(sm.SUMMARY)
    got["rc"] = {k: v.cpu().numpy() for k, v in rc.items()}
    got["rc"]["summary"] = got["rc"]["summary"].view(bm.SUMMARY)
    got["stats_after"] = d_stats.cpu().numpy().tobytes()
    got["weights_after"] = d_w.cpu().numpy().tobytes()
    return got


def assert_rc_same(got, want, tag):
    assert_arrays_same(got, want, [k for k, _ in RC_OUTPUTS], [k for k, t in RC_OUTPUTS if t is np.float64], tag,
                       dict(RC_OUTPUTS))
    gs, ws = got["summary"][0], want["summary"][0]
    for f in ("best", "count_rc", "eligible", "reserved"):
        assert gs[f] == ws[f], (tag, f, gs, ws)
    assert bm.same_f64(np.array([gs["best_mean"]]), np.array([ws["best_mean"]])), (tag, gs, ws)


def assert_same(got, want, tag):
    assert_arrays_same(got, want, [k for k, _ in OUTPUTS], [k for k, t in OUTPUTS if t is np.float64], tag, dict(OUTPUTS))
    gs, ws = got["summary"][0], want["summary"][0]
    for f in sm.SUMMARY.names[1:]:
        assert gs[f] == ws[f], (tag, f, gs, ws)
    assert bm.same_f64(np.array([gs["statistic"]]), np.array([ws["statistic"]])), (tag, gs, ws)
    assert_rc_same(got["rc"], want["rc"], tag + " (nested reality check)")


def board(S, B, seed, mask, wild):
    """`craft`'s records with a zero-variance row (19: a constant of few mantissa bits, its deviation is 0.0 exactly)
    and winners of graded strength (21 .. 26), so that the step-down has somebody to reject, early and late"""
    stats = craft(S, B, seed, mask, wild)
    x, steps = stats["reward_sum"].copy(), stats["steps"].copy()
    rng = np.random.default_rng(seed + 1000)
    if S > 19:
        x[19] = 0.25
    if S > 6 and not wild:     # (the subnormal row's 1 / se is +inf and so is every other maximum: the wild boards keep it)
        x[6] = rng.normal(0, 1e-3, B)
    for k in range(21, min(S, 27)):
        x[k] = rng.normal(0.5 + 0.25 * (k - 21), 1.0, B)
    return bm.records(x, steps)


def selection(B, n):
    """n of B periods, the first and the last among them: with B > 64 bits in both words"""
    mask = np.zeros(B, bool)
    mask[np.unique(np.linspace(0, B - 1, n).astype(int))] = True
    assert mask.sum() == n
    return mask


# (B, n, R, benchmark, weights, crit_rank, max_rounds, threshold, wild)
CASES = [(7, 3, 1, False, "made", 0, 1, None, False),
         (8, 8, 17, True, "own", 16, 8, 0.0, False),
         (70, 12, 255, False, "made2", 229, 8, None, True),
         (128, 65, 256, True, "made", 200, 8, np.inf, True),
         (9, 8, 257, False, "made2", 0, 8, 1.0, False),
         (70, 12, 300, True, "made2", 269, 8, None, False),
         (128, 65, 300, False, "own", 299, 1, None, True)]


@pytest.mark.parametrize("S", [1, 16, 255, 256, 257, 600])
def test_spa_equals_the_model(env, S):
    """Seven calls per S: n = 3, 8 (a power of two: the reciprocal instead of the division), 12 and 65, R below, at
    and above a chunk and the slab, S below, at and above a tile and several tiles."""
    rng = np.random.default_rng(S * 17)
    rounds_seen, rejected_seen, zero_se = set(), 0, False
    for B, n, R, with_benchmark, kind, rank, rounds, threshold, wild in CASES:
        mask = selection(B, n)
        stats = board(S, B, S + B + R, mask, wild)
        if kind == "own":      # a caller's table: zeros, non-integers, a jackknife row, a negative weight
            w = rng.choice([0.0, 0.5, 1.0, 2.25, 1e-3], (R, n)) * rng.choice([1.0, 1.0, 3.0], (R, 1))
            w[0] = n / (n - 1.0)
            w[0, 0] = 0.0
            w[min(1, R - 1), n - 1] = -1.5
        else:
            w = bm.weights(n, R, 2.0 if kind == "made2" else 1.0, SEED)
        benchmark = None
        if with_benchmark:
            benchmark = rng.normal(0, 1e-1, B)
            benchmark[~mask] = np.nan             # an unselected period's entry is never used
        thr = sm.default_threshold(n) if threshold is None else threshold
        got = run_spa(env, stats, mask, benchmark, w, thr, rank, rounds)
        want = sm.spa_test(stats, mask, benchmark, w, thr, rank, rounds)
        assert_same(got, want, f"S={S} B={B} n={n} R={R}")
        assert got["stats_after"] == stats.tobytes() and got["weights_after"] == w.tobytes()
        rounds_seen.add(int(want["summary"][0]["rounds_run"]))
        rejected_seen += int(want["summary"][0]["num_rejected"])
        zero_se = zero_se or (S > 19 and want["std_error"][19] == 0.0 and not want["studentised"][19])
        assert int(want["summary"][0]["rounds_run"]) <= rounds
    assert len(rounds_seen) >= 2 or S <= 19, rounds_seen
    assert (zero_se and rejected_seen > 0) or S <= 19


def test_two_rounds_everybody_and_nobody(env):
    mask = np.ones(12, bool)
    w = bm.weights(12, 300, 2.0, 3)
    thr, rank = sm.default_threshold(12), sm.crit_rank(0.1, 300)
    stats = sm.two_round_board(TWO_ROUND_SEED)
    want = sm.spa_test(stats, mask, None, w, thr, rank, 8)
    assert (want["round_rejected"][:2] > 0).all() and want["summary"][0]["rounds_run"] == 3
    assert_same(run_spa(env, stats, mask, None, w, thr, rank, 8), want, "two rounds")
    for rounds in (1, 2, 64):                     # cut short at either round, and with rounds to spare
        assert_same(run_spa(env, stats, mask, None, w, thr, rank, rounds),
                    sm.spa_test(stats, mask, None, w, thr, rank, rounds), f"max_rounds={rounds}")
    winners = bm.records(np.random.default_rng(5).normal(5e-3, 1e-3, (9, 12)))
    want = sm.spa_test(winners, mask, None, w, thr, rank, 8)
    assert want["summary"][0]["num_rejected"] == 9
    got = run_spa(env, winners, mask, None, w, thr, rank, 8)
    assert_same(got, want, "everybody")
    assert (got["rejected_round"] >= 0).all() and got["summary"][0]["rounds_run"] == got["rejected_round"].max() + 1
    # nobody studentised: nobody eligible, and everybody eligible with a deviation of exactly zero
    sel = np.arange(7) != 2
    w6 = bm.weights(6, 40, 2.0, SEED)
    flat = bm.records(np.repeat(np.arange(-150, 150)[:, None] / 1024.0, 7, axis=1))
    for tag, dead in (("dead", craft(300, 7, 1, sel, True, dead=True)), ("flat", flat)):
        got = run_spa(env, dead, sel, None, w6, 1.0, 37, 8)
        assert_same(got, sm.spa_test(dead, sel, None, w6, 1.0, 37, 8), tag)
        s = got["summary"][0]
        assert s["best"] == -1 and s["studentised"] == 0 and s["rounds_run"] == 0 and s["num_rejected"] == 0
        assert s["statistic"] == 0.0 and all(np.isnan(p) for p in sm.p_values(got, 40))
        assert np.isnan(got["t_stat"]).all() and np.isnan(got["crit"]).all() and not got["round_rejected"].any()
        assert not got["max_stat"].any() and (got["max_index"] == -1).all() and (got["rejected_round"] == -1).all()


def test_nested_reality_check_determinism_and_isolation(env):
    mask = np.arange(70) % 3 != 0
    n = int(mask.sum())
    stats = board(700, 70, 5, mask, True)
    w = bm.weights(n, 300, 3.0, SEED)
    bench = np.random.default_rng(1).normal(0, 1, 70)
    thr, rank = sm.default_threshold(n), 284
    keys = [k for k, _ in OUTPUTS] + ["summary"]
    first = run_spa(env, stats, mask, bench, w, thr, rank, 8)
    again = run_spa(env, stats, mask, bench, w, thr, rank, 8)
    alone = run_check(env, stats, mask, bench, w)
    for k in keys:
        assert first[k].tobytes() == again[k].tobytes(), k
    for k in [k for k, _ in RC_OUTPUTS] + ["summary"]:
        assert first["rc"][k].tobytes() == again["rc"][k].tobytes() == alone[k].tobytes(), k
    assert first["stats_after"] == stats.tobytes() and first["weights_after"] == w.tobytes()
    # unrelated launches in between: a larger test that makes the library take new scratch, a smaller one, a reality check
    big = board(3000, 128, 6, np.ones(128, bool), False)
    run_spa(env, big, np.ones(128, bool), None, bm.weights(128, 17, 1.0, 3), 1.0, 16, 2)
    run_spa(env, board(5, 3, 7, np.ones(3, bool), False), np.ones(3, bool), None, bm.weights(3, 600, 1.0, 3), 0.5, 0, 3)
    run_check(env, big, np.ones(128, bool), None, bm.weights(128, 17, 1.0, 3))
    third = run_spa(env, stats, mask, bench, w, thr, rank, 8)
    for k in keys:
        assert first[k].tobytes() == third[k].tobytes(), k


# ---- refusals -------------------------------------------------------------------------------------------------

def test_refusals_leave_every_output_untouched(env):
    import torch
    lib, h = env._lib, env._h
    dev = env._t["obs"].device
    err = lambda: lib.gte_last_error().decode()
    S, B, R, n, rounds = 10, 6, 20, 4, 8
    mask = np.array([1, 1, 0, 1, 1, 0], bool)
    stats = craft(S, B, 1, mask, False)
    d_stats = device_records(env, stats)
    d_w = torch.from_numpy(bm.weights(n, R, 1.0, 1)).to(dev)
    filled = lambda nbytes: torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    rc = {k: filled((S if k not in ("max_stat", "max_index") else R) * np.dtype(t).itemsize) for k, t in RC_OUTPUTS}
    rc["summary"] = filled(24)
    size = lengths(S, R, rounds)
    out = {k: filled(size[k] * np.dtype(t).itemsize) for k, t in OUTPUTS}
    out["summary"] = filled(40)
    torch.cuda.synchronize()
    rcp = lambda **over: _abi.GteRealityCheckOut(**{**{k: v.data_ptr() for k, v in rc.items()}, **over})
    ptrs = lambda **over: _abi.GteSpaOut(**{**{k: v.data_ptr() for k, v in out.items()}, **over})
    st, wp, words = C.c_void_p(d_stats.data_ptr()), C.c_void_p(d_w.data_ptr()), mask_words(mask)
    INVALID = _abi.GTE_ERR_INVALID
    good_rc, good = rcp(), ptrs()

    def call(env_h=h, stats_p=st, s=S, b=B, m=words, bench=None, weights=wp, r=R, thr=1.0, rank=10, nr=rounds,
             rc_p=good_rc, out_p=good):
        return lib.gte_spa_test(env_h, stats_p, s, b, m, bench, weights, r, thr, rank, nr,
                                None if rc_p is None else C.byref(rc_p), None if out_p is None else C.byref(out_p))
    # what gte_reality_check refuses, in its order
    assert call(env_h=None) == INVALID and "env is NULL" in err()
    assert call(stats_p=None) == INVALID and "stats_device" in err()
    assert call(stats_p=C.c_void_p(d_stats.data_ptr() + 8)) == INVALID and "16-byte aligned" in err()
    assert call(s=0) == INVALID and "n_strategies" in err()
    for bad_B in (0, -1, 129):
        assert call(b=bad_B) == INVALID and "n_periods" in err()
    assert call(m=None) == INVALID and "period_mask" in err()
    for bad_mask in (np.zeros(6, bool), np.array([0, 0, 1, 0, 0, 0], bool)):
        assert call(m=mask_words(bad_mask)) == INVALID and "at least two" in err()
    for bit in (6, 64, 127):
        over = mask_words(mask)
        over[bit >> 6] |= 1 << (bit & 63)
        assert call(m=over) == INVALID and "at or above n_periods" in err()
    for bad_R in (0, -5, 65537):
        assert call(r=bad_R) == INVALID and "n_resamples" in err()
    assert call(weights=None) == INVALID and "weights_device" in err()
    assert call(bench=C.c_void_p(d_w.data_ptr() + 4)) == INVALID and "benchmark_device must be 8-byte aligned" in err()
    assert call(rc_p=None) == INVALID and "rc is NULL" in err()
    for k in rc:
        assert call(rc_p=rcp(**{k: None})) == INVALID and "rc:" in err(), k
    assert call(rc_p=rcp(count_ge=rc["count_ge"].data_ptr() + 2)) == INVALID and "4-byte aligned" in err()
    # its own
    for bad_thr in (float("nan"), -0.5, -float("inf")):
        assert call(thr=bad_thr) == INVALID and "threshold" in err()
    for bad_rank in (-1, R, R + 5):
        assert call(rank=bad_rank) == INVALID and "crit_rank" in err()
    for bad_rounds in (0, -1, 65):
        assert call(nr=bad_rounds) == INVALID and "max_rounds" in err()
    assert call(out_p=None) == INVALID and "out is NULL" in err()
    for k in out:
        assert call(out_p=ptrs(**{k: None})) == INVALID and "out:" in err(), k
    assert call(out_p=ptrs(t_stat=out["t_stat"].data_ptr() + 4)) == INVALID and "8-byte aligned" in err()
    assert call(out_p=ptrs(round_rejected=out["round_rejected"].data_ptr() + 2)) == INVALID and "4-byte aligned" in err()
    # wrong in several ways: the check that stands first reports
    assert call(s=0, r=0, thr=-1.0, rc_p=None, out_p=None) == INVALID and "n_strategies must be >= 1" in err()
    assert call(thr=-1.0, rank=-1, out_p=None) == INVALID and "threshold" in err()
    env.synchronize()
    torch.cuda.synchronize()
    for k, v in [("rc." + k, v) for k, v in rc.items()] + list(out.items()):
        assert bool((v == 0x5A).all()), f"{k} was written by a refused call"
    assert d_stats.cpu().numpy().tobytes() == stats.tobytes()
    # the good call goes through (+inf is a threshold), and inside a stream capture it is refused with nothing launched
    assert call(thr=float("inf")) == _abi.GTE_OK
    env.synchronize()
    seen = []
    by = None

    own = torch.ones((10, B), dtype=torch.float64, device=dev)

    def body(i):
        try:
            by.spa(weights=own)      # (a caller's table: gte_spa_test is the first call into the library)
        except _abi.GteError as e:
            seen.append(e)
            raise
    from leaderboard_gpu import board as as_board
    by = as_board(env, stats)
    env.reset()
    with pytest.raises(Exception):
        env.capture_steps(body, 2)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].status == _abi.GTE_ERR_STATE and "stream capture" in str(seen[0])


# ---- end to end -----------------------------------------------------------------------------------------------

def test_pipeline_backtest_to_spa():
    """256 envs, 16 strategies, 6 periods: backtest_signals -> period_stats.by_strategy().spa(...) equals the model
    applied to .numpy() of the same fold; a benchmark and a caller's table go the same way."""
    import gym_trading_env_amd as gte
    import torch
    from gym_trading_env_amd import periods
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
    sel = [0, 1, 2, 4]
    mask = np.isin(np.arange(6), sel)
    spa = by.spa(periods=sel, n_resamples=300, block=2, seed=7, alpha=0.1, max_rounds=4)
    assert isinstance(spa, gte.SpaTest) and isinstance(spa.reality_check, gte.RealityCheck)
    assert spa.num_resamples == 300 and spa.periods == sel and spa.crit_rank == 269 and spa.max_rounds == 4
    assert spa.threshold == sm.default_threshold(4) and spa.alpha == 0.1
    w = bm.weights(4, 300, 2.0, 7)
    assert spa.weights.cpu().numpy().tobytes() == w.tobytes()
    want = sm.spa_test(host, mask, None, w, sm.default_threshold(4), 269, 4)
    got = spa.numpy()
    for k in ("t_stat", "std_error", "crit"):
        assert bm.same_f64(got[k], want[k]), k
    assert bm.same_f64(got["max_stats"], want["max_stat"].reshape(3, 300))
    np.testing.assert_array_equal(got["max_index"], want["max_index"].reshape(3, 300))
    for k in ("count_adj", "rejected_round", "round_rejected", "studentised"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got["recentred"], want["recentred"] != 0)
    np.testing.assert_array_equal(got["rejected"], want["rejected_round"] >= 0)
    ws = want["summary"][0]
    ok = want["studentised"]
    assert ok.sum() >= 8 and spa.num_studentised == int(ok.sum()) and spa.best == int(ws["best"]) >= 0
    assert (spa.p_lower, spa.p_consistent, spa.p_upper) == sm.p_values(want, 300) and spa.p_value == spa.p_consistent
    assert spa.statistic == float(ws["statistic"]) and spa.rounds_run == int(ws["rounds_run"]) >= 1
    assert spa.num_rejected == int(ws["num_rejected"])
    np.testing.assert_array_equal(spa.superior().cpu().numpy(), np.flatnonzero(want["rejected_round"] >= 0))
    np.testing.assert_array_equal(got["p_adjusted"][ok], (want["count_adj"] / 300)[ok])
    assert np.isnan(got["p_adjusted"][~ok]).all() and spa.p_adjusted.is_cuda and spa.t_stat.is_cuda
    # the nested reality check is the one reality_check() gives for the same weights
    rc, alone = spa.reality_check.numpy(), by.reality_check(periods=sel, n_resamples=300, block=2, seed=7).numpy()
    for k in ("mean", "boot_sum", "boot_sq_sum", "max_stats", "max_index", "count_ge", "count_adj", "std_error"):
        assert rc[k].tobytes() == alone[k].tobytes(), k
    assert rc["p_value"] == alone["p_value"] and rc["best"] == alone["best"]
    np.testing.assert_allclose(got["std_error"][ok], rc["std_error"][ok], rtol=1e-12, atol=0.0)
    # a benchmark (NumPy, then torch), a caller's table and a threshold
    bench = rng.normal(0, 1e-3, 6)
    own = rng.choice([0.0, 1.0, 2.0, 0.5], (77, 4))
    want = sm.spa_test(host, mask, bench, own, 0.25, sm.crit_rank(0.05, 77), 8)
    for b_arg, w_arg in ((bench, own), (torch.from_numpy(bench).cuda(), torch.from_numpy(own).cuda())):
        s2 = by.spa(periods=mask, benchmark=b_arg, weights=w_arg, threshold=0.25)
        assert s2.num_resamples == 77 and s2.crit_rank == sm.crit_rank(0.05, 77)
        got = s2.numpy()
        assert bm.same_f64(got["t_stat"], want["t_stat"]) and bm.same_f64(got["crit"], want["crit"])
        assert bm.same_f64(got["max_stats"], want["max_stat"].reshape(3, 77))
        np.testing.assert_array_equal(got["rejected_round"], want["rejected_round"])
        assert (s2.p_lower, s2.p_consistent, s2.p_upper) == sm.p_values(want, 77)
    with pytest.raises(ValueError, match="at least two"):
        by.spa(periods=[3])
    with pytest.raises(ValueError, match="at least three"):
        by.spa(periods=[1, 3])
    assert by.spa(periods=[1, 3], threshold=0.5, n_resamples=10).num_resamples == 10
    with pytest.raises(ValueError, match="weights must have shape"):
        by.spa(periods=sel, weights=np.ones((5, 3)))
    with pytest.raises(ValueError, match="benchmark must have shape"):
        by.spa(periods=sel, benchmark=np.ones(5))
    for bad in (dict(alpha=1.5), dict(max_rounds=0), dict(max_rounds=65), dict(threshold=-1.0), dict(n_resamples=0)):
        with pytest.raises(ValueError):
            by.spa(periods=sel, **bad)
    assert by.numpy().tobytes() == host.tobytes()       # the test changes no record
    env.close()


def test_spa_example(capsys):
    """examples/backtest_spa.py runs at a small shape and prints the Reality Check's p-value next to the three of the
    SPA test, which are the result object's and the model's; the step-down keeps the cautious strategies with an edge."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import backtest_spa as ex
    finally:
        sys.path.pop(0)
    out = ex.main(n_fast=3, n_slow=3, n_edge=2, replicas=16, K=900, T=1500, n_periods=12, n_resamples=200)
    text = capsys.readouterr().out
    line = [l for l in text.splitlines() if l.startswith("Reality Check p-value")]
    assert len(line) == 1
    rc = float(line[0].split("Reality Check p-value")[1].split()[0])
    lo, co, up = (float(v) for v in line[0].split("SPA p-values (lower, consistent, upper)")[1].split()[:3])
    spa = out["spa"]
    assert abs(rc - out["p_reality"]) < 5.1e-4 and abs(co - spa.p_consistent) < 5.1e-4
    assert abs(lo - spa.p_lower) < 5.1e-4 and abs(up - spa.p_upper) < 5.1e-4
    assert spa.num_resamples == 200 and spa.periods == list(range(12))
    want = sm.spa_test(out["by_strategy"], np.ones(12, bool), None, bm.weights(12, 200, 2.0, 7), sm.default_threshold(12),
                       sm.crit_rank(0.05, 200), 8)
    assert (spa.p_lower, spa.p_consistent, spa.p_upper) == sm.p_values(want, 200)
    assert out["p_reality"] == bm.p_values(want["rc"], 200)[0]
    assert out["superior"] == list(np.flatnonzero(want["rejected_round"] >= 0))
    # the strategies with a real but small edge are the last n_edge: the step-down keeps them (a crossover that this
    # stretch of the walk favoured may stay with them), and the studentised p-value is not above the Reality Check's
    S = out["strategies"]
    assert out["crossovers"] == S - 2 and {S - 2, S - 1} <= set(out["superior"])
    assert spa.p_consistent <= 0.05 and spa.p_consistent <= out["p_reality"]
