"""Trade statistics (gte_track_trades, include/gte.h) without a GPU: tests/trade_model.py, the statement as a
Python loop, held to hand-worked answers; what the reference's own traces make it exercise; the fold and the
scores on crafted records; and the register budget of the kernels that carry the record (csrc/gte_trades.hip)."""
import ctypes as C
import os

import numpy as np
import pytest

import backtest_model as bm
import replay
import strategy_model as sm
import trade_model as tm
from gym_trading_env_amd import _abi

NAN, INF = float("nan"), float("inf")


def T(v, p, terminated=False, truncated=False):
    return dict(stepped=True, reset=False, v=v, p=p, r=0.0, terminated=terminated, truncated=truncated)


def R(v0, p0):
    return dict(stepped=False, reset=True, v0=v0, p0=p0)


def check(rec, **want):
    for f, w in want.items():
        x = rec[f]
        assert (np.isnan(x) and np.isnan(w)) or x == w, (f, x, w)


def test_abi_mirrors_the_header():
    assert np.dtype(_abi.TRADE_DTYPE).itemsize == 128 == C.sizeof(_abi.GteTradeStats)
    assert np.dtype(_abi.STRATEGY_TRADE_DTYPE).itemsize == 128 == C.sizeof(_abi.GteStrategyTradeStats)
    assert np.dtype(_abi.TRADE_DTYPE).fields["exposure"][1] == 64 and np.dtype(_abi.TRADE_DTYPE).fields["closed"][1] == 80
    assert np.dtype(_abi.STRATEGY_TRADE_DTYPE).fields["gross_profit"][1] == 56
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gte.h")).read()
    for i, name in enumerate(_abi.TRADE_METRICS):
        assert f"GTE_TRADE_METRIC_{name.upper()} = {i}" in hdr, name
        assert getattr(_abi, "TRADE_METRIC_" + name.upper()) == i


def test_exit_to_flat_pays_the_fees_of_entering_and_leaving():
    # decided at 1000; 999 after the entry's fees; sold at 1125 after the fees of leaving
    rec = tm.run(tm.new_record(1000.0, 0.0), [T(999.0, 1.0), T(1100.0, 1.0), T(1125.0, 0.0), T(1125.0, 0.0)])
    check(rec, closed=1, wins=1, losses=0, forced=0, reversals=0, dropped=0, gross_profit=0.125, gross_loss=0.0,
          ret_sq_sum=0.015625, best_trade=0.125, worst_trade=0.125, exposure=2, hold_sum=2, max_len=2, open_len=0,
          open_position=0.0, open_value=1100.0, last_valuation=1125.0, loss_streak=0, max_loss_streak=0)


def test_reversal_closes_at_the_valuation_before_and_enters_there():
    rec = tm.run(tm.new_record(1000.0, 1.0), [T(1250.0, 1.0), T(1240.0, -1.0)])
    check(rec, closed=1, wins=1, reversals=1, gross_profit=0.25, open_position=-1.0, open_value=1250.0, open_len=1,
          exposure=2, hold_sum=1, last_valuation=1240.0)
    tm.run(rec, [T(625.0, 0.0)])  # the flip's fees (1250 -> 1240) count against the short: 625 / 1250 - 1
    check(rec, closed=2, wins=1, losses=1, reversals=1, gross_profit=0.25, gross_loss=-0.5, ret_sq_sum=0.3125,
          best_trade=0.25, worst_trade=-0.5, hold_sum=2, max_len=1, exposure=2, loss_streak=1, max_loss_streak=1,
          open_position=0.0)
    # a resize is a reversal too
    rec = tm.run(tm.new_record(1000.0, 1.0), [T(1500.0, 1.0), T(1400.0, 0.5), T(700.0, 0.5)])
    check(rec, closed=1, reversals=1, gross_profit=0.5, open_position=0.5, open_value=1500.0, open_len=2, exposure=3)


def test_forced_close_at_an_episode_end():
    for flags in (dict(terminated=True), dict(truncated=True), dict(terminated=True, truncated=True)):
        rec = tm.run(tm.new_record(1000.0, 1.0), [T(1000.0, 1.0), T(500.0, 1.0, **flags)])
        check(rec, closed=1, forced=1, losses=1, gross_loss=-0.5, worst_trade=-0.5, best_trade=-0.5, exposure=2,
              hold_sum=2, max_len=2, open_position=0.0, last_valuation=500.0, dropped=0)
        tm.run(rec, [R(1000.0, 1.0)])  # the reset that follows drops nothing: the end closed the trade
        check(rec, dropped=0, open_position=1.0, open_value=1000.0, open_len=0, loss_streak=1)
    # flat at the end: nothing to close
    rec = tm.run(tm.new_record(1000.0, 0.0), [T(1000.0, 0.0, truncated=True)])
    check(rec, closed=0, forced=0, exposure=0, best_trade=-INF, worst_trade=INF)


def test_reversal_on_the_ending_transition_closes_twice():
    rec = tm.run(tm.new_record(1000.0, 1.0), [T(2000.0, 1.0), T(1000.0, -1.0, truncated=True)])
    check(rec, closed=2, wins=1, losses=1, reversals=1, forced=1, gross_profit=1.0, gross_loss=-0.5, ret_sq_sum=1.25,
          hold_sum=2, max_len=1, exposure=2, open_position=0.0, best_trade=1.0, worst_trade=-0.5, loss_streak=1)


def test_a_reset_in_mid_trade_drops_it():
    rec = tm.run(tm.new_record(1000.0, 1.0), [T(1100.0, 1.0), R(1000.0, 0.0)])
    check(rec, closed=0, dropped=1, exposure=1, hold_sum=0, open_position=0.0, open_value=1000.0, last_valuation=1000.0,
          open_len=0, best_trade=-INF)
    tm.run(rec, [R(1000.0, 1.0), R(1000.0, 1.0)])  # flat at the first; in the (unstarted) trade of p_0 at the second
    check(rec, dropped=2)


def test_zero_and_nan_returns_count_as_closed_only():
    lose = [T(500.0, 0.0)]
    rec = tm.run(tm.new_record(1000.0, 1.0), lose + [T(500.0, 1.0), T(500.0, 0.0)])  # 500 / 500 - 1 == 0.0
    check(rec, closed=2, wins=0, losses=1, gross_profit=0.0, gross_loss=-0.5, ret_sq_sum=0.25, best_trade=0.0,
          worst_trade=-0.5, loss_streak=1, max_loss_streak=1)
    rec = tm.run(tm.new_record(1000.0, 1.0), lose + [T(500.0, 1.0), T(NAN, 0.0)])
    check(rec, closed=2, wins=0, losses=1, gross_profit=0.0, gross_loss=-0.5, ret_sq_sum=0.25, best_trade=-0.5,
          worst_trade=-0.5, loss_streak=1, max_loss_streak=1, last_valuation=NAN)
    # an infinite return is a value like any other
    rec = tm.run(tm.new_record(1000.0, 1.0), [T(INF, 0.0)])
    check(rec, closed=1, wins=1, gross_profit=INF, ret_sq_sum=INF, best_trade=INF, worst_trade=INF)


def test_loss_streaks():
    def trade(v_in, v_out):
        return [T(v_in, 1.0), T(v_out, 0.0)]
    steps = trade(1000.0, 500.0) + trade(500.0, 250.0) + trade(250.0, 500.0) + trade(500.0, 250.0) + \
        trade(250.0, 125.0) + [T(125.0, 1.0), R(1000.0, 0.0)] + trade(1000.0, 500.0)
    rec = tm.run(tm.new_record(1000.0, 0.0), steps)
    # L L W L L (dropped) L: the win ends the first streak, the dropped trade and the reset end nothing
    check(rec, closed=6, wins=1, losses=5, dropped=1, loss_streak=3, max_loss_streak=3, gross_profit=1.0,
          gross_loss=-2.5, exposure=7, hold_sum=6, max_len=1)


def test_transitions_after_the_end_change_nothing():
    rec = tm.run(tm.new_record(1000.0, 1.0), [T(500.0, 1.0, terminated=True)])
    before = dict(rec)
    tm.run(rec, [T(800.0, 1.0), T(900.0, 0.0), T(950.0, -1.0, truncated=True)])
    assert {k: v for k, v in rec.items()} == before
    tm.run(rec, [R(700.0, 1.0), T(1400.0, 0.0)])
    check(rec, closed=2, wins=1, losses=1, dropped=0, gross_profit=1.0)


COVERAGE = ("c1_btc_example", "drawdown_done", "limit_orders", "multidataset_k3", "no_autoreset", "numeric_03",
            "numeric_07", "numeric_09", "slide_03", "sweep_15", "sweep_17", "reward_clipped_nodyn")


@pytest.mark.parametrize("name", COVERAGE)
def test_the_reference_traces_exercise_every_kind_of_close(name):
    """From the trace's columns alone: run whole, every one of the twelve closes winning and losing trades, forced
    closes, reversals and exits to flat; three of them trades with a NaN return; none drops a trade."""
    g = replay.load(name)
    tot = dict(wins=0, losses=0, forced=0, reversals=0, closed=0, dropped=0, nan=0)
    for e in range(g["op"].shape[1]):
        rec = tm.new_record(g["portfolio_valuation"][0, e], g["position"][0, e])
        rec["returns"] = []
        tm.run(rec, bm.trace_steps(g, e))
        for f in ("wins", "losses", "forced", "reversals", "closed", "dropped"):
            tot[f] += rec[f]
        tot["nan"] += int(np.isnan(rec["returns"]).sum())
        assert len(rec["returns"]) == rec["closed"]
    flat = tot["closed"] - tot["reversals"] - tot["forced"]
    print(f"[trade-coverage] {name}: {tot}, exits to flat {flat}")
    assert tot["wins"] >= 10 and tot["losses"] >= 10 and tot["forced"] >= 3 and tot["reversals"] >= 10 and flat >= 10, tot
    assert tot["dropped"] == 0
    if name in ("numeric_07", "numeric_09", "slide_03"):
        assert tot["nan"] >= 49, tot


def test_fold_and_scores_on_crafted_records():
    rec = tm.craft_records(300, seed=3)
    groups = sm.default_groups(300, 7) + [[], [5, -1, 300, 5, 299]]
    out = tm.reduce_loop(rec, groups)
    assert out["envs"].tolist()[-2:] == [0, 3] and out["best_trade"][-2] == -INF and out["worst_trade"][-2] == INF
    assert int(out["closed"].sum()) == int(rec["closed"].astype(np.int64).sum()) + 2 * int(rec["closed"][5]) + int(rec["closed"][299])
    assert (out["envs_traded"] <= out["envs"]).all()
    t = tm.craft_stats(64, seed=1)
    for metric in tm.METRICS:
        s = tm.scores_loop(t, metric)
        index, top = tm.rank_loop(t, s, 2, 80)
        r = int((index >= 0).sum())
        assert r == int(((t["closed"] >= 2) & ~np.isnan(s)).sum()) and (index[r:] == -1).all() and np.isnan(top[r:]).all()
        assert all(top[i] > top[i + 1] or (top[i] == top[i + 1] and index[i] < index[i + 1]) for i in range(r - 1))
    pf = tm.scores_loop(t, "profit_factor")
    assert np.isinf(pf).any() and np.isnan(pf).any()


@pytest.mark.parametrize("source,min_occupancy", [("gte_trades.hip", 2), ("gte_trade_strategy.hip", 2)])
def test_trade_kernel_register_budget(source, min_occupancy):
    """The three from-registers kernels of gte_trades.hip carry an env, its statistics record and its trade record
    through all fused steps: no scratch, and two waves per SIMD (a launch of 65 536 envs is one wave per SIMD).
    gte_trade_strategy.hip: no scratch, and the two waves per SIMD its workgroup of eight wavefronts needs."""
    import test_host_cpu
    kernels = test_host_cpu._resource_usage(source)
    assert len(kernels) >= 3
    for k in kernels:
        assert k["scratch"] == 0, k
        assert k["occupancy"] >= min_occupancy, k
    if source == "gte_trades.hip":
        test_host_cpu._assert_kernels_found(
            kernels, ("gte_trade_backtest_kernel", "gte_trade_signal_kernel", "gte_trade_exit_kernel"), 2)
