"""The period statistics' model (tests/period_model.py, restating include/gte.h) against hand-worked answers,
the identities the header states on the twelve reference traces of tests/test_gpu_trades.py, what those traces
exercise under the period map the GPU tests use, the record layouts against the C header, the host-side helpers
of gym_trading_env_amd.periods, the fold and the scores on crafted records, and the register budget of the two
new translation units.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import backtest_model as bm
import period_model as pm
import replay
import strategy_model as sm
from gym_trading_env_amd import _abi, periods

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
ROWS = [np.array([0, 0, 1, 1, -1, 2, 2, 0, 9, 1], dtype=np.int8)]   # B = 3: row 4 is an embargo row, 9 >= B


def T(row, r, p=0.0, v=1000.0, terminated=False, truncated=False, dataset=0, **more):
    return dict(stepped=True, reset=False, v=v, p=p, r=r, terminated=terminated, truncated=truncated, row=row,
                dataset=dataset, **more)


def R(v0=1000.0, p0=0.0):
    return dict(stepped=False, reset=True, v0=v0, p0=p0, row=0, dataset=0)


def run(steps, B=3, p=0.0, ended=False, rows=ROWS):
    recs, stats = pm.new_records(B), bm.new_record(1000.0, p, ended=ended)
    pm.run(recs, stats, steps, rows)
    return recs, stats


def fields(rec):
    return rec["steps"], float(rec["reward_sum"]), float(rec["reward_sq_sum"]), rec["trades"], rec["episodes"]


def test_a_period_change_splits_the_sums():
    recs, stats = run([T(0, 0.5), T(1, 0.25), T(2, -1.0), T(3, 2.0)])
    assert fields(recs[0]) == (2, 0.75, 0.3125, 0, 0)
    assert fields(recs[1]) == (2, 1.0, 5.0, 0, 0)
    assert fields(recs[2]) == (0, 0.0, 0.0, 0, 0)
    assert stats["steps"] == 4 and stats["reward_sum"] == 1.75


def test_a_revisit_after_a_reset_continues_the_stored_sums():
    """period 0, then 1, a reset back into period 0: its sum goes on from 0.1 + 0.2, left to right — not from a
    partial sum made from zero (0.1 + 0.2 + 0.3 != 0.1 + (0.2 + 0.3) in f64)"""
    steps = [T(0, 0.1), T(1, 0.2), T(2, 7.0, terminated=True), R(), T(0, 0.3)]
    recs, _ = run(steps)
    assert recs[0]["steps"] == 3 and recs[0]["reward_sum"] == (np.float64(0.1) + 0.2) + 0.3
    assert recs[0]["reward_sum"] != np.float64(0.1) + (np.float64(0.2) + 0.3)
    assert fields(recs[1]) == (1, 7.0, 49.0, 0, 1)


def test_uncounted_rows_count_nowhere():
    recs, stats = run([T(3, 1.0), T(4, 100.0, p=1.0), T(8, 100.0), T(5, 2.0)])
    assert [r["steps"] for r in recs] == [0, 1, 1] and stats["steps"] == 4
    # the trade of the embargo row is nobody's; the one of row 8 (1.0 -> 0.0) neither; row 5 changes nothing
    assert [r["trades"] for r in recs] == [0, 0, 0] and stats["trades"] == 2
    assert recs[2]["reward_sum"] == 2.0


def test_an_episode_end_is_counted_once():
    """auto-reset off: the env steps on after the end; the later flags count no episode, the steps still count"""
    recs, stats = run([T(5, 1.0, terminated=True), T(6, 1.0, truncated=True), T(7, 1.0, terminated=True)])
    assert fields(recs[2]) == (2, 2.0, 2.0, 0, 1)
    assert fields(recs[0]) == (1, 1.0, 1.0, 0, 0)
    assert stats["episodes"] == 1 and stats["steps"] == 3


def test_a_trade_on_a_periods_first_transition_belongs_to_that_period():
    recs, _ = run([T(1, 0.0, p=0.0), T(2, 0.0, p=1.0), T(3, 0.0, p=1.0), T(5, 0.0, p=-1.0)])
    assert [r["trades"] for r in recs] == [0, 1, 1]


def test_a_nan_reward_stays_inside_its_period():
    recs, stats = run([T(0, 1.0), T(2, np.nan), T(3, 1.0), T(5, 4.0), T(7, 2.0)])
    assert np.isnan(recs[1]["reward_sum"]) and np.isnan(recs[1]["reward_sq_sum"]) and recs[1]["steps"] == 2
    assert fields(recs[0]) == (2, 3.0, 5.0, 0, 0) and fields(recs[2]) == (1, 4.0, 16.0, 0, 0)
    assert np.isnan(stats["reward_sum"])


def test_transitions_after_an_episodes_end_and_a_started_ended_env():
    """an env that had already ended when the records were cleared: its transitions count steps and sums, its
    flags no episode; a next-step reset step is no transition"""
    recs, stats = run([T(0, 1.0, terminated=True), R(), T(1, 2.0, truncated=True)], ended=True)
    assert fields(recs[0]) == (2, 3.0, 5.0, 0, 1)
    assert stats["episodes"] == 1


def test_a_row_map_per_dataset():
    rows = [np.array([0, 0, 0], np.int8), np.array([1, 1, 1], np.int8)]
    recs, _ = run([T(1, 1.0), T(1, 2.0, dataset=1), T(2, 4.0, dataset=1)], B=2, rows=rows)
    assert fields(recs[0])[:2] == (1, 1.0) and fields(recs[1])[:2] == (2, 6.0)


# ---- the twelve traces -------------------------------------------------------------------------------------------

NAMES = ("c1_btc_example", "drawdown_done", "limit_orders", "multidataset_k3", "no_autoreset", "numeric_03",
         "numeric_07", "numeric_09", "slide_03", "sweep_15", "sweep_17", "reward_clipped_nodyn")


def _whole(g, rows, B):
    out = []
    for e in range(g["op"].shape[1]):
        recs, stats = pm.new_records(B), bm.new_record(g["portfolio_valuation"][0, e], g["position"][0, e])
        pm.run(recs, stats, pm.trace_steps(g, e), rows)
        out.append((recs, stats))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_identities_on_the_reference_traces(name):
    g = replay.load(name)
    one = [np.zeros(len(ds[1]), np.int8) for ds in g["datasets"]]
    for recs, stats in _whole(g, one, 1):
        for f in ("steps", "trades", "episodes"):
            assert recs[0][f] == stats[f]
        for f in ("reward_sum", "reward_sq_sum"):
            assert replay.same_bits(np.array([recs[0][f]]), np.array([stats[f]])).all(), f
    every = [(np.arange(len(ds[1])) + d) % 5 for d, ds in enumerate(g["datasets"])]
    for recs, stats in _whole(g, every, 5):
        for f in ("steps", "trades", "episodes"):
            assert sum(r[f] for r in recs) == stats[f], f


def _map_facts(g):
    rows = pm.trace_rows(g)
    changes = uncounted = piece_starts = 0
    used = set()
    for e in range(g["op"].shape[1]):
        last = None
        for s in pm.trace_steps(g, e):
            if not s["stepped"]:
                continue
            b = int(rows[s["dataset"]][s["row"]])
            if b < 0:
                uncounted += 1
                continue
            used.add(b)
            if last is not None and b != last:
                changes += 1
                piece_starts += s["row"] % 16 == 0
            last = b
    return changes, uncounted, len(used), piece_starts


def test_what_the_traces_exercise_under_the_test_map():
    """Under the map of the GPU tests every trace changes period often, has uncounted transitions and uses all
    seven periods; on all but (at most) two a change falls on the first row of a 16-byte piece, where the
    register copy of the period bytes has just been fetched again."""
    facts = {name: _map_facts(replay.load(name)) for name in NAMES}
    for name, (changes, uncounted, used, starts) in facts.items():
        print(f"[period-coverage] {name}: {changes} period changes, {uncounted} uncounted transitions, "
              f"{used} periods, {starts} changes on a piece's first row")
        assert changes >= 50 and uncounted >= 100 and used == 7, (name, facts[name])
    assert sum(f[3] >= 4 for f in facts.values()) >= 10, facts


# ---- layout ---------------------------------------------------------------------------------------------------

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gte.h"
#define F(t, f) printf(#t " " #f " %zu %zu\n", offsetof(t, f), sizeof(((t*)0)->f));
int main(void) {
  printf("sizeof %zu %zu %d %d\n", sizeof(gte_period_stats), sizeof(gte_strategy_period_stats), GTE_MAX_PERIODS,
         GTE_ABI_VERSION);
  printf("metrics %d %d %d %d %d %d\n", GTE_PERIOD_METRIC_MEAN_REWARD, GTE_PERIOD_METRIC_SHARPE,
         GTE_PERIOD_METRIC_REWARD_SUM, GTE_PERIOD_METRIC_PERIOD_SHARPE, GTE_PERIOD_METRIC_WORST_PERIOD,
         GTE_PERIOD_METRIC_POSITIVE_SHARE);
  F(gte_period_stats, reward_sum) F(gte_period_stats, reward_sq_sum) F(gte_period_stats, steps)
  F(gte_period_stats, trades) F(gte_period_stats, episodes)
  F(gte_strategy_period_stats, reward_sum) F(gte_strategy_period_stats, reward_sq_sum)
  F(gte_strategy_period_stats, steps) F(gte_strategy_period_stats, trades) F(gte_strategy_period_stats, episodes)
  F(gte_strategy_period_stats, envs_stepped) F(gte_strategy_period_stats, reserved)
  return 0;
}
"""


def test_record_layouts_and_metric_constants_match_the_c_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).split("\n")
    assert lines[0].split()[1:] == ["32", "48", "128", "5"] and _abi.GTE_ABI_VERSION == 5
    assert C.sizeof(_abi.GtePeriodStats) == pm.PERIOD.itemsize == 32
    assert C.sizeof(_abi.GteStrategyPeriodStats) == pm.STRATEGY_PERIOD.itemsize == 48
    assert _abi.GTE_MAX_PERIODS == periods.MAX_PERIODS == 128
    codes = [int(x) for x in lines[1].split()[1:]]
    assert codes == [_abi.PERIOD_METRIC_MEAN_REWARD, _abi.PERIOD_METRIC_SHARPE, _abi.PERIOD_METRIC_REWARD_SUM,
                     _abi.PERIOD_METRIC_PERIOD_SHARPE, _abi.PERIOD_METRIC_WORST_PERIOD,
                     _abi.PERIOD_METRIC_POSITIVE_SHARE] == list(range(6))
    assert len(_abi.PERIOD_METRICS) == 6
    for struct, ct, dt in (("gte_period_stats", _abi.GtePeriodStats, pm.PERIOD),
                           ("gte_strategy_period_stats", _abi.GteStrategyPeriodStats, pm.STRATEGY_PERIOD)):
        c_fields = [(n, int(o), int(s)) for t, n, o, s in (ln.split() for ln in lines[2:] if ln) if t == struct]
        assert c_fields == [(n, getattr(ct, n).offset, getattr(ct, n).size) for n, _ in ct._fields_]
        assert c_fields == [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names]
    for name in ("gte_bind_periods", "gte_track_periods", "gte_read_period_stats", "gte_reduce_period_stats",
                 "gte_rank_period_stats"):
        assert _abi.SYMBOLS[name][0] is C.c_int


# ---- helpers ---------------------------------------------------------------------------------------------------

def test_blocks():
    b = periods.blocks(10, 3)
    assert b.dtype == np.int8 and b.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert periods.blocks(128, 128).tolist() == list(range(128))
    sizes = np.bincount(periods.blocks(1003, 7))
    assert len(sizes) == 7 and sizes.max() - sizes.min() <= 1
    for T_, n in ((10, 0), (3, 4), (1000, 129)):
        with pytest.raises(ValueError):
            periods.blocks(T_, n)


def test_split():
    s = periods.split(10, (0.6, 0.4))
    assert s.dtype == np.int8 and s.tolist() == [0] * 6 + [1] * 4
    assert periods.split(10, (0.6, 0.4), embargo=2).tolist() == [0] * 6 + [-1, -1, 1, 1]
    assert periods.split(10, (0.5, 0.3, 0.2), embargo=1).tolist() == [0] * 5 + [-1, 1, 1, -1, 2]
    assert periods.split(10, (0.6, 0.4), embargo=9).tolist() == [0] * 6 + [-1] * 4   # the embargo swallows a segment
    assert periods.split(7, (1.0,)).tolist() == [0] * 7
    for bad in ((0.5, 0.4), (1.2, -0.2), ()):
        with pytest.raises(ValueError):
            periods.split(10, bad)
    with pytest.raises(ValueError):
        periods.split(10, (0.99, 0.01))   # an empty segment


def test_from_index():
    import pandas as pd  # a dependency of the package (DataFrame datasets): missing, this fails, it does not skip
    idx = pd.date_range("2021-11-29", periods=70, freq="D")
    m = periods.from_index(idx, "M")
    assert m.dtype == np.int8 and m.tolist() == [0] * 2 + [1] * 31 + [2] * 31 + [3] * 6
    gap = idx[:2].append(idx[40:])      # December has no row: it takes no id
    assert periods.from_index(gap, "M").tolist() == [0] * 2 + [1] * 24 + [2] * 6
    assert periods.from_index(idx, "Y").tolist() == [0] * 33 + [1] * 37
    with pytest.raises(ValueError):
        periods.from_index(pd.date_range("2021-01-01", periods=200, freq="D"), "D")


# ---- fold and scores ---------------------------------------------------------------------------------------------

def test_fold_on_crafted_records():
    N, B = 300, 5
    rec = pm.craft_records(N, B, seed=3)
    groups = sm.default_groups(N, 7) + [[], [5, -1, N, 5, 299]]
    out = pm.reduce_loop(rec, groups)
    assert out.shape == (9, B) and not out["reserved"].any()
    assert not out[-2]["steps"].any() and not out[-2]["envs_stepped"].any()
    for b in range(B):
        assert int(out["steps"][:7, b].sum()) == int(rec["steps"][:, b].sum())
        assert int(out["steps"][-1, b]) == 2 * int(rec["steps"][5, b]) + int(rec["steps"][299, b])
        assert out["envs_stepped"][-1, b] == 2 * (rec["steps"][5, b] > 0) + (rec["steps"][299, b] > 0)
    # the fixed order, per (strategy, period): eight interleaved accumulators
    g, b = groups[2], 1
    acc = [np.float64(0.0)] * 8
    with np.errstate(all="ignore"):
        for j, e in enumerate(g):
            acc[j % 8] = acc[j % 8] + rec["reward_sum"][e, b]
        want = acc[0]
        for a in acc[1:]:
            want = want + a
    assert sm.same_f64(np.array([out["reward_sum"][2, b]]), np.array([want]))


def test_scores_on_hand_worked_records():
    t = np.zeros((2, 4), dtype=pm.STRATEGY_PERIOD)
    t["steps"][0] = [10, 0, 30, 10]
    t["reward_sum"][0] = [1.0, 0.0, -0.5, 2.0]
    t["reward_sq_sum"][0] = [0.5, 0.0, 0.75, 1.0]
    every, some, none = np.ones(4, bool), np.array([1, 1, 0, 1], bool), np.array([0, 1, 0, 0], bool)
    assert pm.scores_loop(t, "reward_sum", every)[0] == 2.5
    assert pm.scores_loop(t, "mean_reward", every)[0] == 2.5 / 50
    assert pm.scores_loop(t, "mean_reward", some)[0] == 3.0 / 20
    m, q = 2.5 / 50, 2.25 / 50
    assert pm.scores_loop(t, "sharpe", every)[0] == m / np.sqrt(q - m * m)
    assert pm.scores_loop(t, "worst_period", every)[0] == -0.5 and pm.scores_loop(t, "worst_period", some)[0] == 1.0
    assert pm.scores_loop(t, "positive_share", every)[0] == 2 / 3      # the empty period is no period
    mp, qp = 2.5 / 3, (1.0 + 0.25 + 4.0) / 3
    assert pm.scores_loop(t, "period_sharpe", every)[0] == mp / np.sqrt(qp - mp * mp)
    for metric in pm.METRICS:
        s = pm.scores_loop(t, metric, none)
        assert (s[0] == 0.0 if metric == "reward_sum" else np.isnan(s[0])), metric
        assert pm.rank_loop(t, s, none, 0, 2)[0].tolist() == [-1, -1]     # an all-empty selection is unranked
    assert pm.rank_loop(t, pm.scores_loop(t, "reward_sum", every), every, 0, 3)[0].tolist() == [0, -1, -1]


def test_ranking_on_crafted_records():
    t = pm.craft_stats(64, 7, seed=1)
    masks = [np.ones(7, bool), np.arange(7) < 4, np.arange(7) == 6]
    seen_nan = seen_tie = False
    for mask in masks:
        n = pm.selected_steps(t, mask)
        for metric in pm.METRICS:
            s = pm.scores_loop(t, metric, mask)
            index, top = pm.rank_loop(t, s, mask, 20, 80)
            r = int((index >= 0).sum())
            assert r == int(((n >= 20) & ~np.isnan(s)).sum()) and (index[r:] == -1).all() and np.isnan(top[r:]).all()
            assert all(top[i] > top[i + 1] or (top[i] == top[i + 1] and index[i] < index[i + 1]) for i in range(r - 1))
            seen_nan = seen_nan or bool(np.isnan(s).any())
            seen_tie = seen_tie or any(top[i] == top[i + 1] for i in range(r - 1))
    assert seen_nan and seen_tie


@pytest.mark.parametrize("source", ["gte_periods.hip", "gte_period_strategy.hip"])
def test_period_kernel_register_budget(source):
    """The three from-registers kernels of gte_periods.hip carry an env, its statistics record, the open period's
    record and the period bytes through all fused steps: no scratch, and two waves per SIMD (a launch of 65 536
    envs is one wave per SIMD).  gte_period_strategy.hip: no scratch, at least two waves per SIMD."""
    import test_host_cpu
    kernels = test_host_cpu._resource_usage(source)
    assert len(kernels) >= (4 if source == "gte_periods.hip" else 2)
    for k in kernels:
        assert k["scratch"] == 0, k
        assert k["occupancy"] >= 2, k
    if source == "gte_periods.hip":
        test_host_cpu._assert_kernels_found(
            kernels, ("gte_period_backtest_kernel", "gte_period_signal_kernel", "gte_period_exit_kernel"), 2)
