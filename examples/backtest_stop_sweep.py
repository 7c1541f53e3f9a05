#!/usr/bin/env python3
"""A few SMA-crossover strategies x a grid of stop-losses and take-profits, backtested in one fused
launch: the signal table has one row per crossover (built on the device, as in backtest_rule_sweep.py),
`bind_exits` adds one 32-byte exit rule per (stop, target) cell, and two explicit maps give every env
its pair — `strategy[e]` the table row, `rule_of_env[e]` the exit rule.  The table stays `rows` rows
however fine the grid is: exits decide from the env's own path (the valuation it entered at), which no
table row can hold.  `by_strategy(pair_id, n_pairs).top(k)` ranks the pairs on the device.

    python examples/backtest_stop_sweep.py [--rows 4] [--stops 6] [--targets 6] [--replicas 16]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402


def main(rows=4, stops=6, targets=6, replicas=16, K=1000, duration=168, top=5, details=False):
    import gym_trading_env_amd as gte
    from gym_trading_env_amd import signals
    df = make_frame(T=6000, seed=3)
    close = df["close"].to_numpy()
    fast = np.array([5, 8, 13, 21, 34, 55, 89, 144])[:rows]
    slow = fast * 4
    windows = np.unique(np.concatenate([fast, slow]))
    rules = signals.rules(a=np.searchsorted(windows, fast), b=np.searchsorted(windows, slow), warmup=slow - 1,
                          pos_up=2, pos_down=1, pos_neutral=-1)            # long above, flat below
    stop = np.linspace(0.002, 0.012, stops)       # make_frame moves about 0.1 % a row, 2 % an episode
    target = np.linspace(0.004, 0.024, targets)
    grid_stop, grid_target = (g.reshape(-1) for g in np.meshgrid(stop, target, indexing="ij"))
    exits = signals.exit_rules(stop_loss=grid_stop, take_profit=grid_target, exit_position=1)   # leave for flat
    R = len(exits)
    n_pairs = rows * R
    N = n_pairs * replicas
    pair = np.arange(N, dtype=np.int32) % n_pairs            # env e backtests pair e % n_pairs
    strategy, rule_of_env = pair // R, pair % R
    env = gte.BatchedTradingEnv(df, num_envs=N, positions=[-1, 0, 1], windows=None,
                                trading_fees=1e-4, borrow_interest_rate=3e-6, initial_position=0,
                                max_episode_duration=duration, autoreset="next_step", seed=5)
    env.build_signals(signals.sma_bank(close, windows), rules)   # rows x T bytes: the whole table
    env.bind_exits(exits, rule_of_env=rule_of_env)
    env.reset()
    stats = env.backtest_signals(K, strategy=strategy)
    board = stats.by_strategy(pair, n_pairs)
    index, score = board.top(top, "mean_episode_return", min_episodes=4)
    index, score = index.cpu().numpy(), score.cpu().numpy()
    fired = env.exit_state().exits.sum(0).cpu().numpy()
    print(f"{rows} crossovers x {stops} stops x {targets} targets = {n_pairs} pairs over {N} envs x {K} steps; "
          f"exits fired: " + ", ".join(f"{k} {int(n)}" for k, n in zip(signals.EXIT_KINDS, fired)))
    for p, v in zip(index, score):
        if p < 0:
            continue
        s, r = divmod(int(p), R)
        print(f"  SMA({fast[s]:3d}) / SMA({slow[s]:3d})  stop {grid_stop[r]:.2%}  target {grid_target[r]:.2%}: "
              f"mean episode return {v:+.5f}")
    out = (index, score, stats.numpy(), env.exit_state().numpy(), (strategy, rule_of_env, exits)) if details \
        else (index, score)
    env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--stops", type=int, default=6)
    ap.add_argument("--targets", type=int, default=6)
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--top", type=int, default=5)
    a = ap.parse_args()
    main(a.rows, a.stops, a.targets, a.replicas, top=a.top)
