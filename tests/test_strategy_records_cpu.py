"""What the record families share, without a GPU: the helpers of gym_trading_env_amd/strategy_records.py, and
csrc/gte_members.h — the member rule include/gte.h promises and the period mask's bit test — compiled for the host
(tests/members_check.cpp, its own main, run as a child process) and held to tests/strategy_model.py."""
import os
import subprocess

import numpy as np
import pytest

import strategy_model as sm
from gym_trading_env_amd import _abi
from gym_trading_env_amd.strategy_records import mask_words, metric_code, resolve_strategy_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
FAMILIES = ((_abi.STRATEGY_METRICS, "METRIC"), (_abi.TRADE_METRICS, "TRADE_METRIC"),
            (_abi.PERIOD_METRICS, "PERIOD_METRIC"))


@pytest.mark.parametrize("names,prefix", FAMILIES, ids=[p for _, p in FAMILIES])
def test_metric_code(names, prefix):
    assert [metric_code(n, names, prefix) for n in names] == list(range(len(names)))
    assert [metric_code(n.upper(), names, prefix) for n in names] == list(range(len(names)))
    for c in range(len(names)):
        assert metric_code(c, names, prefix) == c and metric_code(np.int32(c), names, prefix) == c
        assert getattr(_abi, f"{prefix}_{names[c].upper()}") == c  # the constants ARE the indices
    with pytest.raises(ValueError, match=f"unknown metric 'median': one of {names[0]}, "):
        metric_code("median", names, prefix)
    with pytest.raises(ValueError, match=rf"unknown metric {len(names)}: 0 \.\. {len(names) - 1}"):
        metric_code(len(names), names, prefix)
    with pytest.raises(ValueError):
        metric_code(-1, names, prefix)
    for bad in (1.5, 1.0, True):
        with pytest.raises(TypeError, match=rf"metric must be a name or a {prefix}_\* constant"):
            metric_code(bad, names, prefix)


def test_resolve_strategy_map():
    captured, mine = ("the call's map", 7), object()
    assert resolve_strategy_map(captured, None, None) == captured
    with pytest.raises(ValueError, match=r"by_strategy\(\) of a backtest\(\) result needs n_strategies"):
        resolve_strategy_map(None, None, None)
    assert resolve_strategy_map(captured, mine, None) == (mine, 7)
    with pytest.raises(ValueError, match=r"by_strategy\(strategy=\.\.\.\) needs n_strategies"):
        resolve_strategy_map(None, mine, None)
    for given in (captured, None):  # both arguments: as given, whatever was captured
        assert resolve_strategy_map(given, mine, 3) == (mine, 3)
        assert resolve_strategy_map(given, None, 3) == (None, 3)


def _mask(*bits):
    m = np.zeros(128, dtype=bool)
    m[list(bits)] = True
    return m


def test_mask_words():
    assert list(mask_words(_mask())) == [0, 0]
    assert list(mask_words(_mask(0))) == [1, 0]
    assert list(mask_words(_mask(63))) == [1 << 63, 0]
    assert list(mask_words(_mask(64))) == [0, 1]
    assert list(mask_words(_mask(127))) == [0, 1 << 63]
    assert list(mask_words(_mask(0, 63, 64, 127))) == [1 | 1 << 63, 1 | 1 << 63]
    assert list(mask_words(np.ones(5, dtype=bool))) == [31, 0]  # (a mask is as long as the records have periods)


@pytest.fixture(scope="module")
def members_check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("members") / "members_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "members_check.cpp"), "-o", out], check=True, cwd=ROOT)

    def run(*args):
        r = subprocess.run([out, *map(str, args)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (args, r.returncode, r.stderr[-2000:])
        return r.stdout
    return run


def _lists(out):
    """members_check's lines `s: e e e` -> the list of every strategy, in order"""
    rows = [line.split(":") for line in out.splitlines()]
    assert [int(s) for s, _ in rows] == list(range(len(rows)))
    return [[int(e) for e in places.split()] for _, places in rows]


@pytest.mark.parametrize("base", [0, 5, -3])
@pytest.mark.parametrize("N", [1, 64, 65])
@pytest.mark.parametrize("S", [1, 7, 8])
def test_default_map_members(members_check, S, N, base):
    got = _lists(members_check("members", N, S, base))
    assert got == sm.default_groups(N, S, base)
    assert sorted(e for g in got for e in g) == list(range(N))  # every env belongs to exactly one strategy


def test_explicit_list_members(members_check):
    """An empty strategy, entries outside [0, N) (they hold their place: -1 here, skipped by the sums), and offsets
    that include/gte.h says are clamped into [0, N] and made non-decreasing."""
    N = 300
    groups = sm.default_groups(N - 5, 7) + [[], [5, -1, N, 5, 299]]  # (N entries: offsets[S] <= N, include/gte.h)
    offsets, envs = sm.csr(groups)
    assert offsets[-1] == N
    got = _lists(members_check("members", N, len(groups), 0, *offsets, *envs))
    assert got == [[e if 0 <= e < N else -1 for e in g] for g in groups]
    # offsets as a careless caller might leave them (N entries exist): list s is [lo, max(lo, hi)) of the clamped
    # offsets[s], offsets[s + 1]
    envs = list(range(9, -1, -1))
    got = _lists(members_check("members", 10, 4, 0, -2, 3, 1, 12, 10, *envs))
    assert got == [envs[0:3], [], envs[1:10], []]


def test_period_mask_bit_test_reads_what_mask_words_packs(members_check):
    for bits in ((), (0,), (63,), (64,), (127,), (0, 5, 63, 64, 100, 127)):
        w = mask_words(_mask(*bits))
        assert [int(b) for b in members_check("mask", w[0], w[1]).split()] == list(bits)
