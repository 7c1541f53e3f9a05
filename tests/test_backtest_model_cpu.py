"""The backtest statistics model (tests/backtest_model.py) over the reference's own golden traces
and a hand-computed sequence, and the ABI struct's layout against the C header.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import backtest_model as bm
import replay
from gym_trading_env_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRACES = ["c2_nowindow", "drawdown_done", "no_autoreset", "limit_orders", "multidataset_k3", "numeric_07"]


@pytest.fixture(scope="module")
def traces():
    return {n: replay.load(n) for n in TRACES}


def _transitions(g, e):
    """Calls of env e that are transitions: a step() call that moved `step`."""
    K = g["op"].shape[0]
    return [k for k in range(1, K) if g["op"][k, e] == 1 and g["step"][k, e] != g["step"][k - 1, e]]


@pytest.mark.parametrize("name", TRACES)
def test_model_over_a_golden_trace(traces, name):
    g = traces[name]
    K, E = g["op"].shape
    total_eps = 0
    for e in range(E):
        rec = bm.trace_record(g, e)
        ks = _transitions(g, e)
        assert rec["steps"] == len(ks)
        # first episode ends: a raised flag on a transition, none raised since the last reset
        first_ends, terms, ended = 0, 0, False
        for k in range(1, K):
            if g["op"][k, e] == 0:
                ended = False
            elif k in ks and (g["done"][k, e] or g["truncated"][k, e]):
                first_ends += not ended
                terms += bool(g["done"][k, e]) and not ended
                ended = True
        assert rec["episodes"] == first_ends and rec["terminations"] == terms
        total_eps += first_ends
        seq = np.float64(0.0)
        with np.errstate(all="ignore"):
            for k in ks:
                seq = seq + np.float64(g["reward"][k, e])
        assert replay.same_value(np.array([rec["reward_sum"]]), np.array([seq])).all()
        pos = g["position"][:, e]
        assert rec["trades"] == sum(1 for k in ks if pos[k] != pos[k - 1])  # np.diff(history['position']) != 0
        if np.isfinite(rec["peak"]) and np.isfinite(rec["valuation_last"]):
            assert rec["peak"] >= rec["valuation_last"]
        assert rec["max_drawdown"] >= 0
        if ks:
            assert replay.same_value(np.array([rec["valuation_last"]]),
                                     np.array([g["portfolio_valuation"][ks[-1], e]])).all()
    assert total_eps > 0, "the trace ends no episode: nothing was checked about episodes"


def test_stepping_after_done_counts_transitions_and_ends_no_further_episode(traces):
    g = traces["no_autoreset"]
    after_done = 0
    for e in range(g["op"].shape[1]):
        rec = bm.trace_record(g, e)
        flags = (g["done"][1:, e] | g["truncated"][1:, e]).astype(bool)
        assert (g["op"][1:, e] == 1).all() and flags.any()
        assert rec["episodes"] == 1 and rec["steps"] == len(_transitions(g, e))
        after_done += rec["steps"] - (int(np.argmax(flags)) + 1)
    assert after_done > 0


def test_nan_valuations_change_neither_peak_nor_drawdown(traces):
    g = traces["numeric_07"]
    seen = 0
    for e in range(g["op"].shape[1]):
        rec = bm.new_record(g["portfolio_valuation"][0, e], g["position"][0, e])
        for s in bm.trace_steps(g, e):
            before = (rec["peak"], rec["max_drawdown"])
            bm.run(rec, [s])
            if s["stepped"] and np.isnan(s["v"]):
                seen += 1
                assert replay.same_value(np.array(before), np.array([rec["peak"], rec["max_drawdown"]])).all()
                assert np.isnan(rec["valuation_last"])
    assert seen > 0, "numeric_07 has no NaN valuation on a transition"


def test_hand_computed_sequence():
    """100 -> 128 -> 96 (truncated) | reset at 100 short | 50 (terminated) -> 75 -> NaN (truncated
    again: the episode has already ended).  All values are exact in binary."""
    steps = [
        dict(stepped=True, v=128.0, p=1.0, r=0.5, terminated=False, truncated=False),
        dict(stepped=True, v=96.0, p=1.0, r=-0.25, terminated=False, truncated=True),
        dict(stepped=False, reset=True, v0=100.0, p0=-1.0),
        dict(stepped=True, v=50.0, p=-1.0, r=-1.0, terminated=True, truncated=False),
        dict(stepped=True, v=75.0, p=0.0, r=0.5, terminated=False, truncated=False),
        dict(stepped=True, v=float("nan"), p=0.0, r=0.25, terminated=False, truncated=True),
    ]
    rec = bm.run(bm.new_record(100.0, 0.0), steps)
    assert (rec["steps"], rec["trades"], rec["episodes"], rec["terminations"]) == (5, 2, 2, 1)
    assert rec["reward_sum"] == 0.0 and rec["reward_sq_sum"] == 1.625
    assert rec["peak"] == 100.0 and rec["max_drawdown"] == 0.5
    assert rec["cur_return"] == 0.75
    assert rec["ep_return_sum"] == -0.75 and rec["ep_return_sq_sum"] == 1.0625
    assert np.isnan(rec["valuation_last"]) and rec["prev_position"] == 0.0
    # after the second step alone: one episode of return 0.25, drawdown 1 - 96/128
    rec = bm.run(bm.new_record(100.0, 0.0), steps[:2])
    assert (rec["steps"], rec["trades"], rec["episodes"], rec["terminations"]) == (2, 1, 1, 0)
    assert rec["max_drawdown"] == 0.25 and rec["cur_return"] == 0.0 and rec["ep_return_sum"] == 0.25
    # a frozen step changes nothing; a same-step reset follows its transition
    frozen = bm.run(dict(rec), [dict(stepped=False)])
    assert frozen == rec
    rec = bm.run(bm.new_record(128.0, 0.0), [dict(stepped=True, v=64.0, p=1.0, r=-0.5, terminated=True,
                                                   truncated=False, reset=True, v0=100.0, p0=0.0),
                                              dict(stepped=True, v=80.0, p=0.0, r=-0.25, terminated=False,
                                                   truncated=False)])
    assert rec["peak"] == 100.0 and rec["max_drawdown"] == 0.5  # 1 - 64/128, against the FIRST episode's peak
    assert (rec["episodes"], rec["terminations"], rec["trades"]) == (1, 1, 1)
    assert rec["cur_return"] == -0.25 and rec["valuation_last"] == 80.0


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gte.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(gte_backtest_stats, f), sizeof(((gte_backtest_stats*)0)->f));
int main(void) {
  printf("sizeof %zu %d\n", sizeof(gte_backtest_stats), GTE_ABI_VERSION);
  F(steps) F(reward_sum) F(reward_sq_sum) F(peak) F(max_drawdown) F(cur_return) F(ep_return_sum)
  F(ep_return_sq_sum) F(valuation_last) F(prev_position) F(trades) F(episodes) F(terminations) F(ended)
  F(episode_seen) F(step_seen) F(reserved)
  return 0;
}
"""


def test_backtest_stats_layout_matches_the_c_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).split("\n")
    size, version = map(int, lines[0].split()[1:])
    assert size == C.sizeof(_abi.GteBacktestStats) == np.dtype(_abi.BACKTEST_DTYPE).itemsize == 128
    assert version == _abi.GTE_ABI_VERSION
    c_fields = [(n, int(o), int(s)) for n, o, s in (ln.split() for ln in lines[1:] if ln)]
    ct = [(n, getattr(_abi.GteBacktestStats, n).offset, getattr(_abi.GteBacktestStats, n).size)
          for n, _ in _abi.GteBacktestStats._fields_]
    assert c_fields == ct
    dt = np.dtype(_abi.BACKTEST_DTYPE)
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == c_fields
    # the model names the public fields of the record, and no other
    assert set(bm.FIELDS) == {n for n, _ in _abi.BACKTEST_FIELDS} - {"ended", "episode_seen", "step_seen"}

