"""The rows of a backtest (struct gte_curve_bufs, include/gte.h) as tests/curve_model.py states them, held to
themselves on the CPU: rows at a stride from the stride-1 rows; the drawdown column against max_drawdown and the
reward column against reward_sum of backtest_model; the valuation rows against the reference's golden traces; the
struct and the flag bits between the header and _abi.py; the register budget of csrc/gte_curves.hip."""
import os
import re

import numpy as np
import pytest

import backtest_model as bm
import curve_model as cm
import replay
from gym_trading_env_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSITIONS = np.array([-1.0, 0.0, 1.0])
MODES = [None, "next_step", "same_step"]


def _timeline(rng, K, mode):
    """(record before the call, step dicts) of one env: random valuations, rewards (a few -0.0 and NaN
    valuations among them), episode ends; next-step reset rows, same-step ends, and with auto-reset off envs that
    freeze or go on stepping after their episode ended."""
    v, i, pi = np.float64(1000.0), int(rng.integers(0, 20)), int(rng.integers(0, 3))
    ended = bool(rng.random() < 0.2)
    frozen = bool(rng.random() < 0.5)
    rec = bm.new_record(v, POSITIONS[pi], ended=ended)
    steps = []
    for _ in range(K):
        if ended and mode == "next_step":
            v, i, pi = np.float64(rng.uniform(500, 2000)), int(rng.integers(0, 20)), int(rng.integers(0, 3))
            steps.append(dict(stepped=False, reset=True, v0=v, p0=POSITIONS[pi], i0=i, pi0=pi))
            ended = False
            continue
        if ended and mode is None and frozen:
            steps.append(dict(stepped=False, v=v, i=i, pi=pi))
            continue
        before = v
        v = np.float64(v * np.exp(rng.normal(0, 0.05)))
        if rng.random() < 0.03:
            v = np.float64("nan")
        i += 1
        if rng.random() < 0.4:
            pi = int(rng.integers(0, 3))
        with np.errstate(all="ignore"):
            r = np.float64(-0.0) if rng.random() < 0.1 else np.log(v / before)
        term, trunc = bool(rng.random() < 0.08), bool(rng.random() < 0.12)
        s = dict(stepped=True, v=v, p=POSITIONS[pi], r=r, terminated=term, truncated=trunc, i=i, pi=pi)
        if np.isnan(v):
            v = before
        if term or trunc:
            if mode == "same_step":
                v, i, pi = np.float64(rng.uniform(500, 2000)), int(rng.integers(0, 20)), int(rng.integers(0, 3))
                s.update(reset=True, v0=v, p0=POSITIONS[pi])
            else:
                ended = True
                frozen = bool(rng.random() < 0.5)
        steps.append(s)
    return rec, steps


def _same(a, b, tag):
    for c in cm.COLUMNS:
        if a[c].dtype.kind == "f":
            replay.assert_same_value(a[c], b[c], f"{tag}: {c}")
        else:
            np.testing.assert_array_equal(a[c], b[c], err_msg=f"{tag}: {c}")


@pytest.mark.parametrize("mode", MODES, ids=str)
def test_rows_at_a_stride_follow_from_the_stride_1_rows(mode):
    rng = np.random.default_rng(5)
    K = 35
    seen = 0
    for n in range(40):
        rec, steps = _timeline(rng, K, mode)
        one = cm.rows(dict(rec), steps, 1)
        seen |= int(np.bitwise_or.reduce(one["flags"]))
        for stride in (1, 2, 3, 16, K, K + 3):
            got = cm.rows(dict(rec), steps, stride)
            assert all(got[c].shape == (cm.n_rows(K, stride),) for c in cm.COLUMNS)
            _same(got, cm.restride(one, K, stride), f"{mode} timeline {n} stride {stride}")
    want = {None: 1 | 2 | 8, "next_step": 1 | 2 | 4, "same_step": 1 | 2 | 4}[mode]
    assert seen == want, f"the timelines raised flags {seen}, expected {want}"


@pytest.mark.parametrize("mode", MODES, ids=str)
def test_the_columns_add_up_to_the_record(mode):
    """max over the drawdown column == max_drawdown and the ordered sum of the stride-1 reward column ==
    reward_sum of backtest_model.run over the same timeline, bitwise; the record curve_model advances is that
    record."""
    rng = np.random.default_rng(6)
    nonzero = 0
    for n in range(60):
        rec, steps = _timeline(rng, 41, mode)
        want = bm.run(dict(rec), steps)
        for stride in (1, 3, 16):
            mine = dict(rec)
            got = cm.rows(mine, steps, stride)
            for f in bm.FIELDS:
                assert replay.same_value(np.array([mine[f]], np.float64), np.array([want[f]], np.float64)).all(), f
            dd = np.float64(0.0)
            for d in got["drawdown"]:
                if d > dd:
                    dd = d
            assert replay.same_value(np.array([dd]), np.array([want["max_drawdown"]])).all(), (n, stride)
            assert not np.isnan(got["drawdown"]).any()
        total = np.float64(0.0)
        with np.errstate(all="ignore"):
            for r in cm.rows(dict(rec), steps, 1)["reward"]:
                total = total + r
        assert replay.same_value(np.array([total]), np.array([want["reward_sum"]])).all(), n
        nonzero += int(want["max_drawdown"] > 0)
    assert nonzero > 30


def test_a_lone_negative_zero_reward_becomes_positive_zero():
    rec = bm.new_record(100.0, 0.0)
    s = dict(stepped=True, v=100.0, p=0.0, r=np.float64(-0.0), terminated=False, truncated=False, i=4, pi=1)
    got = cm.rows(rec, [s], 1)
    assert got["reward"][0] == 0.0 and not np.signbit(got["reward"][0])
    assert (got["row"][0], got["position"][0], got["flags"][0], got["drawdown"][0]) == (4, 1, 0, 0.0)


@pytest.mark.parametrize("name", ["c2_nowindow", "drawdown_done", "limit_orders"])
def test_valuation_rows_are_the_reference_trace(name):
    g = replay.load(name)
    K, E = g["op"].shape
    for e in range(E):
        rec = bm.new_record(g["portfolio_valuation"][0, e], g["position"][0, e])
        got = cm.rows(rec, cm.trace_steps(g, e), 1)
        replay.assert_same_bits(got["valuation"], np.ascontiguousarray(g["portfolio_valuation"][1:, e]),
                                f"{name} env {e}")
        np.testing.assert_array_equal(got["row"], g["idx"][1:, e])
        np.testing.assert_array_equal(got["position"], g["pos_index"][1:, e])
        want = bm.trace_record(g, e)
        assert replay.same_value(np.array([got["drawdown"].max()]), np.array([want["max_drawdown"]])).all()


def test_the_struct_and_the_flags_agree_between_header_and_abi():
    hdr = open(os.path.join(ROOT, "include", "gte.h")).read()
    body = re.search(r"typedef struct gte_curve_bufs \{(.*?)\} gte_curve_bufs;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(double|int32_t|uint8_t)\s+(.*)", decl.strip(), re.S)
        if m:
            fields += [(n.strip().lstrip("*"), m.group(1)) for n in m.group(2).split(",")]
    ctype = {"float64": "double", "int32": "int32_t", "uint8": "uint8_t"}
    assert fields == [(n, ctype[t]) for n, t in _abi.CURVE_COLUMNS]
    assert [n for n, _ in _abi.GteCurveBufs._fields_] == [n for n, _ in fields]
    assert tuple(n for n, _ in fields) == ("valuation", "drawdown", "reward", "position", "row", "flags")
    bits = dict(re.findall(r"#define GTE_CURVE_(\w+) (\d+)", hdr))
    assert {k: int(v) for k, v in bits.items()} == dict(TERMINATED=_abi.CURVE_TERMINATED, TRUNCATED=_abi.CURVE_TRUNCATED,
                                                         RESET=_abi.CURVE_RESET, FROZEN=_abi.CURVE_FROZEN)
    assert (cm.TERMINATED, cm.TRUNCATED, cm.RESET, cm.FROZEN) == (1, 2, 4, 8) == tuple(
        int(bits[k]) for k in ("TERMINATED", "TRUNCATED", "RESET", "FROZEN"))
    assert "gte_backtest_curves" in _abi.SYMBOLS and hasattr(_abi.load_library(), "gte_backtest_curves")


def test_curve_kernels_register_budget():
    """csrc/gte_curves.hip for gfx950: the four kernels by name, no scratch, at least 2 waves/SIMD (the figures
    are in DESIGN.md, "Curves")."""
    import test_host_cpu as th
    kernels = th._resource_usage("gte_curves.hip")
    th._assert_kernels_found(kernels, ("gte_curve_backtest_kernel", "gte_curve_signal_kernel",
                                       "gte_curve_exit_kernel", "gte_curve_fold_kernel"), 2)
    src = open(os.path.join(ROOT, "gym-trading-env_amd", "csrc", "gte_curves.hip")).read()
    assert src.count("summary_body(") == 3 and "phase_a<" not in src and "#define GTE_HOT_ONLY" not in src
    assert "__syncthreads" not in src and "__shared__" not in src and "atomic" not in src
