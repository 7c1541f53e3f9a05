"""The exit rules of include/gte.h as tests/exit_model.py states them: hand-made valuation paths that
trip each exit alone, the order of the four, the latch, rules that are off, a fill as an entry, the memo
and the step-gap fold; the reference-made fixtures (tests/golden/make_exit_golden.py); the host-side
builders of gym_trading_env_amd.signals; the layout of the two structs; the new kernels' registers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exit_model as xm
import replay
from gym_trading_env_amd import _abi, signals as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 3        # positions [-1, 0, 1]: index 1 is flat
LONG, FLAT = 2, 1


class Walk:
    """One env walked by hand: `row()` shows the model the env's record, `step()` moves it."""

    def __init__(self, rule, v0=1000.0, pos=LONG, episode=1):
        self.m = xm.ExitModel(1, rule, P, [0])
        self.episode, self.t, self.v, self.pos, self.nr = episode, 0, v0, pos, False

    def ask(self, raw=LONG):
        return int(self.m.actions([raw], [self.episode], [self.t], [self.v], [self.pos], [self.nr])[0])

    def step(self, v, pos=None, n=1):
        self.t += n
        self.v = v
        self.pos = self.pos if pos is None else pos

    def reset(self, v0=1000.0, pos=LONG):
        self.episode, self.t, self.v, self.pos, self.nr = self.episode + 1, 0, v0, pos, False

    @property
    def s(self):
        return self.m.state[0]


def _follow(w, action):
    """the env does what it was told (no fees in these hand-made paths)"""
    return w.pos if action < 0 else action


def test_stop_loss_alone():
    w = Walk(xm.make_rules(stop_loss=0.05, exit_position=FLAT))
    assert w.ask() == LONG and w.s["entry"] == 1000.0 and w.s["held"] == 0
    w.step(960.0)
    assert w.ask() == LONG                      # 4 % under the entry
    # the threshold is entry * (1.0 - (double)f32(0.05)), a little under 950: 950.0 itself does not trip it
    thr = np.float64(1000.0) * (np.float64(1.0) - np.float64(np.float32(0.05)))
    assert thr < 950.0
    w.step(950.0)
    assert w.ask() == LONG
    w.step(float(thr))                          # <= holds with equality
    assert w.ask() == FLAT
    assert w.s["exits"].tolist() == [1, 0, 0, 0] and w.s["latched"] == 1 and w.s["latched_raw"] == LONG


def test_trailing_alone_follows_the_peak():
    w = Walk(xm.make_rules(trailing=0.05, exit_position=FLAT))
    w.ask()
    for v in (1050.0, 1100.0, 1060.0):
        w.step(v)
        assert w.ask() == LONG
    assert w.s["peak"] == 1100.0 and w.s["entry"] == 1000.0
    w.step(1040.0)                              # 5.45 % under 1100, yet above the entry
    assert w.ask() == FLAT and w.s["exits"].tolist() == [0, 1, 0, 0]


def test_take_profit_alone():
    w = Walk(xm.make_rules(take_profit=0.10, exit_position=FLAT))
    w.ask()
    w.step(1099.0)
    assert w.ask() == LONG
    w.step(1101.0)
    assert w.ask() == FLAT and w.s["exits"].tolist() == [0, 0, 1, 0]


def test_time_exit_alone_counts_transitions_since_the_position_changed():
    w = Walk(xm.make_rules(max_hold=3, exit_position=FLAT), pos=FLAT)
    assert w.ask(LONG) == LONG                  # flat on the reset row: nothing to leave
    w.step(999.0, pos=LONG)                     # the entry: held = 1, entry = the valuation it was decided at
    assert w.ask() == LONG and w.s["held"] == 1 and w.s["entry"] == 1000.0 and w.s["peak"] == 1000.0
    w.step(1001.0)
    assert w.ask() == LONG and w.s["held"] == 2
    w.step(1002.0)
    assert w.s["held"] == 2 and w.ask() == FLAT and w.s["held"] == 3
    assert w.s["exits"].tolist() == [0, 0, 0, 1]


def test_priority_is_stop_trail_target_time():
    # stop, trail and time all hold after a fall: STOP is counted
    w = Walk(xm.make_rules(stop_loss=0.01, trailing=0.01, max_hold=1, exit_position=FLAT))
    w.ask()
    w.step(900.0)
    assert w.ask() == FLAT and w.s["exits"].tolist() == [1, 0, 0, 0]
    # trail, target and time hold (up to 1200, back to 1100, entry 1000; exits armed late by max_hold alone
    # would fire at once, so the rule's trail is wide enough to survive the way up): TRAIL is counted
    w = Walk(xm.make_rules(trailing=0.05, take_profit=0.5, exit_position=FLAT))
    w.ask()
    w.step(1200.0)
    assert w.ask() == LONG
    w.m.rules = xm.make_rules(trailing=0.05, take_profit=0.05, max_hold=1, exit_position=FLAT)
    w.step(1100.0)
    assert w.ask() == FLAT and w.s["exits"].tolist() == [0, 1, 0, 0]
    # target and time hold: TARGET is counted
    w = Walk(xm.make_rules(take_profit=0.01, max_hold=1, exit_position=FLAT))
    w.ask()
    w.step(1200.0)
    assert w.ask() == FLAT and w.s["exits"].tolist() == [0, 0, 1, 0]


def test_latch_holds_on_an_unchanged_byte_and_rearms_on_a_changed_one():
    w = Walk(xm.make_rules(stop_loss=0.05, exit_position=FLAT))
    w.ask()
    w.step(900.0)
    assert w.ask(LONG) == FLAT
    w.step(899.0, pos=FLAT)
    for v in (898.0, 897.0):                    # the table still says LONG: hold, stay flat
        assert w.ask(LONG) == -1 and w.s["latched"] == 1
        w.step(v)
    assert w.ask(0) == 0 and w.s["latched"] == 0    # the byte moved (to short): the table decides again
    w.step(896.0, pos=0)
    assert w.s["exits"].tolist() == [1, 0, 0, 0]
    assert w.ask(LONG) == LONG and w.s["entry"] == 897.0   # the short was decided at 897
    # a byte that moves to an out-of-range value re-arms too: the comparison is on the raw byte
    w = Walk(xm.make_rules(stop_loss=0.05, exit_position=FLAT))
    w.ask()
    w.step(900.0)
    assert w.ask(LONG) == FLAT
    w.step(899.0, pos=FLAT)
    assert w.ask(-128) == -1 and w.s["latched"] == 0
    # a reset clears the latch, the counters go on
    w = Walk(xm.make_rules(stop_loss=0.05, exit_position=FLAT))
    w.ask()
    w.step(900.0)
    assert w.ask(LONG) == FLAT
    w.reset()
    assert w.ask(LONG) == LONG and w.s["latched"] == 0 and w.s["exits"].tolist() == [1, 0, 0, 0]


@pytest.mark.parametrize("rule", [
    dict(stop_loss=0.05, exit_position=3), dict(stop_loss=0.05, exit_position=-1),
    dict(stop_loss=0.05, exit_position=127), dict(stop_loss=0.0, take_profit=-1.0, trailing=np.nan, max_hold=0),
    dict(stop_loss=np.nan, take_profit=np.nan, trailing=-0.0, max_hold=-5, exit_position=FLAT)])
def test_rules_that_are_off_leave_the_table_in_charge(rule):
    w = Walk(xm.make_rules(**rule))
    for v, raw in ((1000.0, LONG), (500.0, LONG), (2000.0, 7), (100.0, 0), (100.0, -128)):
        want = raw if 0 <= raw < P else -1
        assert w.ask(raw) == want
        w.step(v, pos=_follow(w, want))
    assert w.s["exits"].sum() == 0 and w.s["latched"] == 0


def test_nan_valuation_trips_nothing_and_already_at_exit_position_is_no_exit():
    w = Walk(xm.make_rules(stop_loss=0.05, trailing=0.05, take_profit=0.05, exit_position=FLAT))
    w.ask()
    w.step(np.nan)
    assert w.ask() == LONG and w.s["exits"].sum() == 0
    w = Walk(xm.make_rules(stop_loss=0.05, max_hold=1, exit_position=FLAT), pos=FLAT)
    w.ask(FLAT)
    w.step(100.0)
    assert w.ask(FLAT) == FLAT and w.s["exits"].sum() == 0


def test_a_limit_order_fill_is_an_entry():
    w = Walk(xm.make_rules(stop_loss=0.05, exit_position=FLAT), pos=FLAT)
    assert w.ask(-1) == -1                      # the table holds: the env stays flat ...
    w.step(1003.0, pos=LONG)                    # ... but an order filled: the position changed anyway
    assert w.ask(-1) == -1 and w.s["entry"] == 1000.0 and w.s["held"] == 1 and w.s["peak"] == 1003.0
    w.step(940.0)
    assert w.ask(-1) == FLAT and w.s["exits"].tolist() == [1, 0, 0, 0]


def test_a_repeated_decision_returns_the_memo_and_changes_nothing():
    w = Walk(xm.make_rules(stop_loss=0.05, exit_position=FLAT))
    w.ask()
    w.step(900.0)
    first = w.ask(LONG)
    before = w.m.state.copy()
    assert first == FLAT and w.ask(LONG) == FLAT and w.ask(0) == FLAT   # (even with another byte: the row decided)
    assert w.m.state.tobytes() == before.tobytes()
    w.nr = True                                 # an env that needs a reset: hold, and that is memoised too
    w.step(890.0, pos=FLAT)
    assert w.ask(LONG) == -1 and w.s["decided_action"] == -1 and w.s["latched"] == 1
    assert w.s["held"] == 1 and w.s["entry"] == 900.0   # (the state was still brought up to date)


def test_step_gap_folds_as_one_transition():
    w = Walk(xm.make_rules(max_hold=10, exit_position=FLAT))
    w.ask()
    w.step(1010.0, n=4)                         # four steps without a decision, same position
    assert w.ask() == LONG and w.s["held"] == 4 and w.s["peak"] == 1010.0 and w.s["step_seen"] == 4
    w.step(990.0, pos=0, n=3)                   # three more, and the position changed somewhere in them
    assert w.ask(0) == 0 and w.s["held"] == 3 and w.s["entry"] == 1010.0 and w.s["peak"] == 1010.0
    w.s["held"] = xm.INT32_MAX - 1
    w.step(991.0, n=5)
    w.ask(0)
    assert w.s["held"] == xm.INT32_MAX          # saturating


def test_rule_of_env_and_default_map():
    np.testing.assert_array_equal(xm.rule_of(7, 3, None, 5), (np.arange(7) % 5) % 3)
    np.testing.assert_array_equal(xm.rule_of(4, 3, [4, 0, 7, 2], 8), [1, 0, 1, 2])
    np.testing.assert_array_equal(xm.rule_of(4, 3, [4, 0, 7, 2], 8, rule_of_env=[2, 2, 0, 1]), [2, 2, 0, 1])


@pytest.mark.parametrize("name", ["exit_trace", "exit_trace_multi"])
def test_reference_fixture_conditions(name):
    """What tests/golden/make_exit_golden.py promises of a fixture, checked on the file: the recorded
    actions are the model's over the trace's own rows, every comparison the model made is further
    than 1e-9 (relative) from its threshold, every kind of exit occurs at least five times, and the
    file is small."""
    g = replay.load(name)
    assert os.path.getsize(os.path.join(replay.GOLDEN_DIR, name + ".npz")) <= 200 * 1024
    actions, margin, counts, model = xm.trace_actions(g)
    np.testing.assert_array_equal(actions, g["action"])
    assert margin > 1e-9 and margin == float(g["min_margin"]), (margin, float(g["min_margin"]))
    np.testing.assert_array_equal(counts, g["exit_counts"])
    assert (counts >= 5).all(), counts
    assert g["cfg"]["positions"] == [-1, 0, 1] and g["cfg"]["trading_fees"] > 0
    assert g["cfg"]["initial_position"] == "random" and len(set(g["pos_index"][0].tolist())) > 1
    # an exit really changed what the env did: somewhere the action differs from the table's
    import signal_model as sm
    table_only = sm.trace_actions(dict(g, signals_0=g["signals_0"]))
    assert (table_only != g["action"]).sum() >= counts.sum()


def test_struct_layouts_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "gte.h")).read()
    assert "sizeof(gte_exit_rule) == 32 && sizeof(gte_exit_state) == 80" in hdr
    rule, state = np.dtype(_abi.EXIT_RULE_DTYPE), np.dtype(_abi.EXIT_STATE_DTYPE)
    assert rule.itemsize == C.sizeof(_abi.GteExitRule) == 32 and state.itemsize == C.sizeof(_abi.GteExitState) == 80
    assert state.itemsize % 16 == 0
    for dt, cls in ((rule, _abi.GteExitRule), (state, _abi.GteExitState)):
        for name in dt.names:
            assert dt.fields[name][1] == getattr(cls, name).offset, name
    body = re.search(r"typedef struct gte_exit_state \{(.*?)\} gte_exit_state;", hdr, re.S).group(1)
    declared = re.findall(r"\b(?:double|int32_t)\s+(\w+)", body)
    assert declared == [n for n in state.names], declared
    assert xm.STATE_DTYPE == state and xm.RULE_DTYPE == rule == sig.EXIT_DTYPE
    assert _abi.EXIT_KINDS == xm.KINDS


def test_exit_rules_builder_broadcasts_and_checks():
    r = sig.exit_rules(stop_loss=[0.02, 0.05], take_profit=0.1, max_hold=[[12], [48]], exit_position=1)
    assert r.dtype == sig.EXIT_DTYPE and r.shape == (4,)
    assert r["stop_loss"].tolist() == pytest.approx([0.02, 0.05, 0.02, 0.05]) and r["max_hold"].tolist() == [12, 12, 48, 48]
    assert (r["exit_position"] == 1).all() and (r["trailing"] == 0).all() and not r["reserved"].any()
    assert sig.exit_rules().shape == (1,)
    np.testing.assert_array_equal(r.view(np.uint8), xm.make_rules([0.02, 0.05, 0.02, 0.05], 0.1, 0.0,
                                                                  [12, 12, 48, 48], 1).view(np.uint8))
    with pytest.raises(TypeError):
        sig.exit_rules(max_hold=1.5)
    with pytest.raises(TypeError):
        sig.exit_rules(stop_loss="x")
    with pytest.raises(ValueError):
        sig.exit_rules(exit_position=200)
    sig.check_exit_rules(r, 3)
    with pytest.raises(IndexError):
        sig.check_exit_rules(sig.exit_rules(exit_position=3), 3)
    with pytest.raises(IndexError):
        sig.check_exit_rules(sig.exit_rules(exit_position=-1), 3)


def test_exit_kernels_use_no_scratch():
    """The fused exit kernel carries an env, its statistics record and its exit state through all its
    steps: it must stay in registers (the compiler's resource remarks for gfx950)."""
    import test_host_cpu as th
    kernels = {k["name"]: k for k in th._resource_usage("gte_exits.hip")}
    assert any("gte_backtest_exit_kernel" in n for n in kernels) and any("gte_exit_actions_kernel" in n for n in kernels)
    for k in kernels.values():
        assert k["scratch"] == 0, k
        assert k["occupancy"] >= 2, k
    th._assert_kernels_found(list(kernels.values()), ("gte_backtest_exit_kernel",), 2)
