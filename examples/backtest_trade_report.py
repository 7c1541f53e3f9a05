#!/usr/bin/env python3
"""A trade report for a stop-loss x take-profit grid: the SMA-crossover rows and exit rules of
backtest_stop_sweep.py, backtested in one fused launch with trade tracking on, so that every env also keeps
its round-trip trade statistics (closed trades, wins, gross profit and loss, holding times) in registers while it
steps.  `trade_stats.by_strategy(pair, n_pairs).top(10)` folds them per (crossover, stop, target) pair and
ranks the pairs by profit factor on the device; the table adds win rate, trade count and mean holding time —
the first check against a leaderboard whose score comes from three lucky trades.

    python examples/backtest_trade_report.py [--rows 4] [--stops 6] [--targets 6] [--replicas 16]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402


def main(rows=4, stops=6, targets=6, replicas=16, K=1000, T=6000, duration=168, top=10, min_trades=8):
    import gym_trading_env_amd as gte
    from gym_trading_env_amd import signals
    df = make_frame(T=T, seed=3)
    close = df["close"].to_numpy()
    fast = np.array([5, 8, 13, 21, 34, 55, 89, 144])[:rows]
    slow = fast * 4
    windows = np.unique(np.concatenate([fast, slow]))
    rules = signals.rules(a=np.searchsorted(windows, fast), b=np.searchsorted(windows, slow), warmup=slow - 1,
                          pos_up=2, pos_down=1, pos_neutral=-1)            # long above, flat below
    stop = np.linspace(0.002, 0.012, stops)
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
    env.build_signals(signals.sma_bank(close, windows), rules)
    env.bind_exits(exits, rule_of_env=rule_of_env)
    env.reset()
    env.track_trades()                                       # from here on every backtest keeps trade records too
    stats = env.backtest_signals(K, strategy=strategy)
    board = stats.trade_stats.by_strategy(pair, n_pairs)
    index, score = board.top(top, "profit_factor", min_trades=min_trades)
    win_rate, mean_hold = board.score("win_rate"), board.hold_sum.double() / board.closed.double()
    print(f"{rows} crossovers x {stops} stops x {targets} targets = {n_pairs} pairs over {N} envs x {K} steps; "
          f"{int(board.closed.sum())} trades closed, {int(board.forced.sum())} of them by an episode's end")
    print("rank pair   fast slow   stop%  target%   profit_factor  win%  trades  mean_hold")
    for place, (p, v) in enumerate(zip(index.cpu().numpy().tolist(), score.cpu().numpy().tolist()), 1):
        s, r = divmod(p, R)
        print(f"{place:4d} {p:4d}   {fast[s]:4d} {slow[s]:4d}   {100 * grid_stop[r]:5.2f}  {100 * grid_target[r]:7.2f}   "
              f"{v:13.4f}  {100 * float(win_rate[p]):4.1f}  {int(board.closed[p]):6d}  {float(mean_hold[p]):9.1f}")
    env.close()
    return dict(index=index, score=score, by_strategy=board, min_trades=min_trades)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--stops", type=int, default=6)
    ap.add_argument("--targets", type=int, default=6)
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--top", type=int, default=10)
    a = ap.parse_args()
    main(a.rows, a.stops, a.targets, a.replicas, top=a.top)
