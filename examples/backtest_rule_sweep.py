#!/usr/bin/env python3
"""The crossover sweep of examples/backtest_signals.py with the signal table BUILT ON THE DEVICE
(`build_signals` + `backtest_signals`): the host computes a small bank of moving averages, one row
per window length, and writes one 32-byte rule per strategy — which two averages to compare, a band
around zero, and whether to latch (stay long until the difference falls below -band, stay short until
it rises above +band) — and the device writes the int8 [strategies, T] table.  No table exists on the
host and none is copied.  Prints the mean episode return per strategy.

    python examples/backtest_rule_sweep.py [--strategies 512] [--replicas 8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402


def grid(strategies, seed=0):
    """(fast, slow, band, latch) per strategy: window lengths as in backtest_signals.py, a band of
    0 to 0.4 % of the price level of make_frame, every other strategy latched."""
    rng = np.random.default_rng(seed)
    fast = rng.integers(3, 40, strategies)
    slow = fast + rng.integers(5, 200, strategies)
    band = rng.choice([0.0, 0.1, 0.2, 0.4], strategies).astype(np.float32)
    latch = np.arange(strategies) % 2 == 1
    return fast, slow, band, latch


def host_table(bank, a, b, band, latch, warmup):
    """The table the rules ask for, by crossover_table-style NumPy over the same f32 bank: int8 [S, T]
    with 2 (long) above the band, 0 (short) below it, -1 (hold) inside it or, latched, the last of
    the two; -1 during the warm-up."""
    T = bank.shape[1]
    t = np.arange(T)[None, :]
    with np.errstate(invalid="ignore"):
        d = bank[a] - bank[b]                                                  # [S, T] f32
    z = np.where(d > band[:, None], 1, np.where(d < -band[:, None], -1, 0))
    z[t < warmup[:, None]] = 0
    last = np.maximum.accumulate(np.where(z != 0, t, 0), axis=1)               # the last row outside the band
    q = np.where(latch[:, None], np.take_along_axis(z, last, axis=1), z)
    table = np.where(q > 0, 2, np.where(q < 0, 0, -1)).astype(np.int8)
    table[t < warmup[:, None]] = -1
    return table


def main(strategies=512, replicas=8, K=1000, duration=168, details=False):
    import gym_trading_env_amd as gte
    from gym_trading_env_amd import signals
    df = make_frame(T=6000, seed=3)
    close = df["close"].to_numpy()
    fast, slow, band, latch = grid(strategies)
    windows = np.unique(np.concatenate([fast, slow]))
    bank = signals.sma_bank(close, windows)                                    # f32 [windows, T]
    rules = signals.rules(a=np.searchsorted(windows, fast), b=np.searchsorted(windows, slow), hi=band, lo=-band,
                          warmup=slow - 1, pos_up=2, pos_down=0, pos_neutral=-1, latch=latch)
    N = strategies * replicas
    env = gte.BatchedTradingEnv(df, num_envs=N, positions=[-1, 0, 1], windows=None,
                                trading_fees=1e-4, borrow_interest_rate=3e-6, initial_position=0,
                                max_episode_duration=duration, autoreset="next_step", seed=5)
    table = env.build_signals(bank, rules)                 # written on the device, and bound
    env.reset()
    stats = env.backtest_signals(K // 2)                   # env e follows strategy e % strategies
    stats = env.backtest_signals(K - K // 2, resume=True)  # ... in chunks, the statistics carry on
    by_strategy = lambda x: x.cpu().numpy().reshape(replicas, strategies).sum(0)
    episodes = by_strategy(stats.episodes)
    mean_return = by_strategy(stats.ep_return_sum) / np.maximum(episodes, 1)
    trades = by_strategy(stats.trades)
    drawdown = stats.max_drawdown.cpu().numpy().reshape(replicas, strategies).max(0)
    order = np.argsort(-mean_return)
    print(f"{strategies} strategies x {replicas} envs x {K} steps, episodes of {duration} rows from random starts; "
          f"table built on the device from {len(windows)} moving averages")
    for s in list(order[:3]) + list(order[-1:]):
        print(f"  SMA({fast[s]:2d}) / SMA({slow[s]:3d}) band {band[s]:.1f}{' latched' if latch[s] else '        '}: "
              f"mean episode return {mean_return[s]:+.4f} over {episodes[s]} episodes, "
              f"max drawdown {drawdown[s]:.1%}, {trades[s]} trades")
    assert (episodes > 0).all() and np.isfinite(mean_return).all()
    table = table.cpu().numpy() if details else None
    env.close()
    return (mean_return, table, (bank, rules, band)) if details else mean_return


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--strategies", type=int, default=512)
    ap.add_argument("--replicas", type=int, default=8)
    a = ap.parse_args()
    main(a.strategies, a.replicas)
