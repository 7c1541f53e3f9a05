"""Signal tables without a GPU: the reference-made fixtures against the lookup model, their replay
on the two restatements, the records the GPU test expects, the ABI surface and the row padding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import backtest_model as bm
import replay
import signal_model as sm
from gym_trading_env_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACES = ["signal_trace", "signal_trace_multi"]
ENTRY_POINTS = {"gte_bind_signals": 5, "gte_signal_actions": 3, "gte_backtest_signals": 5}


@pytest.mark.parametrize("name", TRACES)
def test_fixture_is_a_trace_with_tables(name):
    path = os.path.join(replay.GOLDEN_DIR, name + ".npz")
    assert os.path.getsize(path) <= 200 * 1024
    assert name in replay.golden_names()  # so every test that walks the traces replays it too
    g = replay.load(name)
    tables = sm.trace_tables(g)
    K, E = g["op"].shape
    P = len(g["cfg"]["positions"])
    assert len(tables) == len(g["datasets"]) and g["strategy"].shape == (E,)
    for t, ds in zip(tables, g["datasets"]):
        assert t.dtype == np.int8 and t.shape == (3, len(ds[1]))
        for v in (-1, -128, 127, 3):
            assert (t == v).any(), f"the table lacks {v}"
    assert P == 3 and ((0 <= g["strategy"]) & (g["strategy"] < 3)).all()
    # every env sees several episodes, next-step convention
    assert ((g["op"] == 0).sum(axis=0) >= 3).all()
    if name == "signal_trace":
        assert (E, tables[0].shape[1]) == (6, 200) and K >= 100
    else:
        assert [t.shape[1] for t in tables] == [150, 210]
        assert set(np.unique(g["dataset"])) == {0, 1}


@pytest.mark.parametrize("name", TRACES)
def test_recorded_actions_are_what_the_lookup_model_gives(name):
    """The reference was driven with a = signals[strategy[e]][env._idx]; the model, fed the rows the
    trace recorded, gives the same action at every step — out-of-range entries as hold."""
    g = replay.load(name)
    want = sm.trace_actions(g)
    np.testing.assert_array_equal(g["action"], want)
    step = g["op"] == 1
    assert (g["action"][step] == -1).any() and (g["action"][step] >= 0).any()
    # ... and holds come from out-of-range table entries only, each kind of them
    tables, seen = sm.trace_tables(g), set()
    for k in range(1, g["op"].shape[0]):
        for e in np.nonzero(step[k])[0]:
            raw = int(tables[g["dataset"][k - 1, e]][g["strategy"][e], g["idx"][k - 1, e]])
            assert (g["action"][k, e] == -1) == (not 0 <= raw < 3)
            if g["action"][k, e] == -1:
                seen.add(raw)
    if name == "signal_trace":
        assert seen == {-1, -128, 127, 3}


def test_lookup_model_rule():
    t0 = np.array([[0, 1, 2, 3], [-1, 2, 127, 0]], np.int8)
    t1 = np.array([[2, 2, -128, 1, 0], [1, 0, 0, 0, 5]], np.int8)
    got = sm.lookup([t0, t1], [0, 1, 1, 0], idx=[3, 1, 4, 2], dataset=[0, 0, 1, 1], n_positions=3)
    np.testing.assert_array_equal(got, [-1, 2, -1, -1])
    np.testing.assert_array_equal(sm.lookup(t0, None, [1, 1, 1], [0, 0, 0], 3), [1, 2, 1])  # e % S
    np.testing.assert_array_equal(sm.default_strategy(5, 3, env_id_base=4), [1, 2, 0, 1, 2])
    with pytest.raises(AssertionError):
        sm.lookup(t0, [2], [0], [0], 3)


@pytest.mark.parametrize("name", TRACES)
def test_fixture_replays_on_the_c_oracle(oracle_mod, name):
    from test_oracle_golden import OracleAdapter
    g = replay.load(name)
    g["action"] = sm.trace_actions(g)  # driven by the model's actions, not the recorded ones
    worst = replay.replay(OracleAdapter(oracle_mod, g), g, rtol=1e-12, reward_ulps=replay.reward_ulp_bound(g))
    assert worst == 0.0


def test_fixture_replays_on_the_python_loop():
    from test_oracle_golden import PyLoopAdapter
    g = replay.load("signal_trace")
    g["action"] = sm.trace_actions(g)
    assert replay.replay(PyLoopAdapter(g), g, rtol=1e-12, reward_ulps=replay.reward_ulp_bound(g)) == 0.0


@pytest.mark.parametrize("name", TRACES)
def test_backtest_model_over_the_fixture(name):
    """The records the GPU test expects from backtest_signals over the fixture: every env finished
    its episodes by truncation, traded, and counts one transition per step call."""
    g = replay.load(name)
    K, E = g["op"].shape
    for e in range(E):
        rec = bm.trace_record(g, e)
        assert rec["steps"] == int((g["op"][1:, e] == 1).sum())
        assert rec["episodes"] == int((g["done"][:, e] | g["truncated"][:, e]).sum()) >= 3
        assert rec["terminations"] == 0 and rec["trades"] > 0
        assert np.isfinite(rec["ep_return_sum"]) and rec["max_drawdown"] > 0


def test_header_declares_the_entry_points_and_version_5():
    hdr = open(os.path.join(ROOT, "include", "gte.h")).read()
    assert re.search(r"#define GTE_ABI_VERSION 5\b", hdr) and _abi.GTE_ABI_VERSION == 5
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in ENTRY_POINTS.items():
        m = re.search(rf"\bint {name}\s*\(([^)]*)\)\s*;", code)
        assert m, f"include/gte.h does not declare {name}"
        assert len(m.group(1).split(",")) == n_args, name
        restype, argtypes = _abi.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
    sig = re.search(r"int gte_bind_signals\s*\(([^)]*)\)", code).group(1)
    assert "const int8_t* signals_device" in sig and "int64_t row_stride" in sig
    # each entry cites the reference lines it batches
    for name in ENTRY_POINTS:
        comment = hdr[:hdr.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert re.search(r"environments\.py:\d+", comment), name


def test_library_exports_the_entry_points():
    lib = _abi.load_library()
    assert lib.gte_abi_version() == 5
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)
    # refusals that need no device
    assert lib.gte_bind_signals(None, 0, None, 1, 16) == _abi.GTE_ERR_INVALID
    assert lib.gte_signal_actions(None, None, None) == _abi.GTE_ERR_INVALID
    assert lib.gte_backtest_signals(None, None, 1, 1, None) == _abi.GTE_ERR_INVALID
    assert "env is NULL" in lib.gte_last_error().decode()


@pytest.mark.parametrize("T,stride", [(1, 16), (15, 16), (16, 16), (17, 32)])
def test_rows_are_padded_to_16_bytes(T, stride):
    from gym_trading_env_amd import signals
    assert signals.row_stride(T) == stride
    table = (np.arange(3 * T).reshape(3, T) % 7 - 2).astype(np.int64)
    a = signals.as_int8_table(table)
    assert a.dtype == np.int8 and a.shape == (3, T)
    p = signals.pad_rows(a)
    assert p.dtype == np.int8 and p.shape == (3, stride) and p.flags.c_contiguous
    assert p.strides == (stride, 1) and stride % 16 == 0 and stride >= T and stride - T < 16
    np.testing.assert_array_equal(p[:, :T], table)
    assert (p[:, T:] == -1).all()  # hold, and never looked up


def test_tables_are_checked_on_the_host():
    from gym_trading_env_amd import signals
    with pytest.raises(ValueError, match="fit int8"):
        signals.as_int8_table([[0, 128]])
    with pytest.raises(ValueError, match="fit int8"):
        signals.as_int8_table([[-129, 0]])
    with pytest.raises(TypeError, match="integers"):
        signals.as_int8_table([[0.5, 1.0]])
    with pytest.raises(ValueError, match=r"shape \(S, T\)"):
        signals.as_int8_table([0, 1, 2])
    with pytest.raises(ValueError):
        signals.row_stride(0)
    assert signals.as_int8_table(np.array([[127, -128]], np.int16)).tolist() == [[127, -128]]
