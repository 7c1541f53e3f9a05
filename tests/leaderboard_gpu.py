"""What the GPU tests of the three leaderboard analyses share (test_gpu_bootstrap.py, test_gpu_cscv.py,
test_gpu_diversify.py, test_gpu_leaderboard_scratch.py): the small env their calls run on, guarded output tensors, the
two words of a period selection, host-made [S, B] records on the device, alone or as a `StrategyPeriodStats`, and the
bit-for-bit comparison of a call's arrays with its model's.  Each file keeps its own `env` fixture around `make_env`
and its own `assert_same` around `assert_arrays_same`: the summaries differ."""
import ctypes as C

import numpy as np
import pytest

from strategy_model import same_f64

GUARD = 8          # elements of guard on either side of every output


def make_env():
    """64 envs over 60 rows: what the analyses need of an env is its library handle, its stream and its device"""
    from gym_trading_env_amd.batched import BatchedTradingEnv
    rng = np.random.default_rng(0)
    close = 100.0 * np.exp(np.cumsum(rng.normal(0, 1e-2, 60)))
    feat = rng.normal(0, 1, (60, 3)).astype(np.float32)
    return BatchedTradingEnv((feat, close), num_envs=64, positions=[-1, 0, 1], windows=None)


def guarded(torch, dev, n, dtype, fill):
    """(the whole tensor, its n elements between the guards), every element `fill`"""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n]


def mask_words(mask):
    """the two words of a bool mask over the periods, as the libgte calls take them"""
    return id_words(np.flatnonzero(mask))


def id_words(ids):
    """the same for a list of period ids: bit b & 63 of word b >> 6"""
    w = (C.c_uint64 * 2)(0, 0)
    for b in ids:
        w[int(b) >> 6] |= 1 << (int(b) & 63)
    return w


def device_records(env, stats):
    """host-made [S, B] strategy period records as the uint8 [S * B, 48] array on the env's device the calls read"""
    import torch
    S, B = stats.shape
    return torch.from_numpy(stats.view(np.uint8).reshape(S * B, 48).copy()).to(env._t["obs"].device)


def board(env, stats):
    """... as the `StrategyPeriodStats` a fold would have made"""
    from gym_trading_env_amd.period_stats import StrategyPeriodStats
    return StrategyPeriodStats(env, device_records(env, stats), stats.shape[1])


def assert_arrays_same(got, want, names, floats, tag, dtypes=None):
    """got[name] equals want[name] for every name: dtype (`dtypes[name]`, or the model's), shape and every element,
    those of `floats` bit for bit with NaN as NaN; a difference is reported with its first five places"""
    for name in names:
        g, w = got[name], want[name]
        assert g.dtype == (dtypes[name] if dtypes else w.dtype) and g.shape == w.shape, (tag, name, g.dtype, g.shape)
        if same_f64(g, w) if name in floats else np.array_equal(g, w):
            continue
        gf, wf = g.reshape(-1), w.reshape(-1)
        bad = [i for i in range(len(wf)) if not (same_f64(gf[i:i + 1], wf[i:i + 1]) if name in floats else gf[i] == wf[i])]
        pytest.fail(f"{tag}: {name} differs at {len(bad)} of {len(wf)} places, first {[(i, gf[i], wf[i]) for i in bad[:5]]}")
