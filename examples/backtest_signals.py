#!/usr/bin/env python3
"""Backtest a sweep of strategies over RANDOM episodes (`bind_signals` + `backtest_signals`):
every strategy is a moving-average crossover written as one row of a signal table — the position
it wants on each market row — and the device looks each step's action up at the row the env
stands on.  So the envs keep what the environment models: random episode starts,
`max_episode_duration` and next-step auto-reset; several envs follow each strategy, and no
[steps, envs] action tensor exists.  Prints the mean episode return per strategy.

    python examples/backtest_signals.py [--strategies 512] [--replicas 8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402


def crossover_table(close, fast, slow):
    """int8 [S, T]: on row t strategy s wants position index 2 (long) when SMA(fast) > SMA(slow),
    else 0 (short), for positions [-1, 0, 1]; -1 (hold) while the slow average has no history."""
    T = len(close)
    c = np.concatenate([[0.0], np.cumsum(close)])
    t = np.arange(T)[None, :]                                              # [1, T]
    sma = lambda w: (c[t + 1] - c[np.maximum(t + 1 - w, 0)]) / w           # [S, T]
    table = np.where(sma(fast[:, None]) > sma(slow[:, None]), 2, 0).astype(np.int8)
    table[t + 1 < slow[:, None]] = -1
    return table


def main(strategies=512, replicas=8, K=1000, duration=168):
    import gym_trading_env_amd as gte
    df = make_frame(T=6000, seed=3)
    close = df["close"].to_numpy()
    rng = np.random.default_rng(0)
    fast = rng.integers(3, 40, strategies)
    slow = fast + rng.integers(5, 200, strategies)
    N = strategies * replicas
    env = gte.BatchedTradingEnv(df, num_envs=N, positions=[-1, 0, 1], windows=None,
                                trading_fees=1e-4, borrow_interest_rate=3e-6, initial_position=0,
                                max_episode_duration=duration, autoreset="next_step", seed=5)
    env.bind_signals(crossover_table(close, fast, slow))
    env.reset()
    stats = env.backtest_signals(K // 2)                   # env e follows strategy e % strategies
    stats = env.backtest_signals(K - K // 2, resume=True)  # ... in chunks, the statistics carry on
    by_strategy = lambda x: x.cpu().numpy().reshape(replicas, strategies).sum(0)
    episodes = by_strategy(stats.episodes)
    mean_return = by_strategy(stats.ep_return_sum) / np.maximum(episodes, 1)
    trades = by_strategy(stats.trades)
    drawdown = stats.max_drawdown.cpu().numpy().reshape(replicas, strategies).max(0)
    order = np.argsort(-mean_return)
    print(f"{strategies} strategies x {replicas} envs x {K} steps, episodes of {duration} rows from random starts")
    for s in list(order[:3]) + list(order[-1:]):
        print(f"  SMA({fast[s]:2d}) / SMA({slow[s]:3d}): mean episode return {mean_return[s]:+.4f} over "
              f"{episodes[s]} episodes, max drawdown {drawdown[s]:.1%}, {trades[s]} trades")
    assert (episodes > 0).all() and np.isfinite(mean_return).all()
    env.close()
    return mean_return


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--strategies", type=int, default=512)
    ap.add_argument("--replicas", type=int, default=8)
    a = ap.parse_args()
    main(a.strategies, a.replicas)
