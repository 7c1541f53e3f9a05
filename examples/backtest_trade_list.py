#!/usr/bin/env python3
"""The trades behind a leaderboard: a sweep of SMA crossovers backtested in one fused launch with trade tracking
and the per-trade list on (`track_trades(list_capacity=...)`), ranked by profit factor on the device, and then
the first trades of the winner as a table — when each was entered and left, at what valuation, how long it was
held and how it ended.  The list is written where a trade closes, from values the kernel holds in registers; its
returns are the very numbers the leaderboard's sums were made of.

    python examples/backtest_trade_list.py [--rows 8] [--replicas 16] [--capacity 32] [--show 12]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402

KINDS = ("flat", "reversal", "forced")


def stamp(date):
    """an index value as one column of the table"""
    return str(date)[:19].replace(" ", "T")


def main(rows=8, replicas=16, K=1000, T=6000, duration=168, capacity=32, show=12, min_trades=8):
    import gym_trading_env_amd as gte
    from gym_trading_env_amd import signals
    df = make_frame(T=T, seed=3)
    close = df["close"].to_numpy()
    fast = np.array([5, 8, 13, 21, 34, 55, 89, 144])[:rows]
    slow = fast * 4
    windows = np.unique(np.concatenate([fast, slow]))
    rules = signals.rules(a=np.searchsorted(windows, fast), b=np.searchsorted(windows, slow), warmup=slow - 1,
                          pos_up=2, pos_down=0, pos_neutral=-1)            # long above, short below
    S = len(fast)
    N = S * replicas                                         # env e backtests crossover e % S
    env = gte.BatchedTradingEnv(df, num_envs=N, positions=[-1, 0, 1], windows=None,
                                trading_fees=1e-4, borrow_interest_rate=3e-6, initial_position=0,
                                max_episode_duration=duration, autoreset="next_step", seed=5)
    env.build_signals(signals.sma_bank(close, windows), rules)
    env.reset()
    env.track_trades(list_capacity=capacity)                 # trade records AND the first `capacity` trades per env
    stats = env.backtest_signals(K)
    board = stats.trade_stats.by_strategy()
    index, score = board.top(3, "profit_factor", min_trades=min_trades)
    winner = int(index[0])
    trades = stats.trade_stats.trades(strategy=winner)       # the lists of the winner's member envs, one transfer
    print(f"{S} crossovers over {N} envs x {K} steps; winner {winner} (SMA {fast[winner]} / {slow[winner]}), profit "
          f"factor {float(score[0]):.4f} over {int(board.closed[winner])} trades; {len(trades)} of them listed, "
          f"{int(trades.truncated.sum())} of {len(trades.env_ids)} lists truncated at {capacity}")
    print(" env  entry                exit                 hold  position   open_value  close_value    ret%  ended")
    dates = trades.entry_date is not None
    for i in range(min(show, len(trades))):
        entry = stamp(trades.entry_date[i]) if dates else str(trades.entry_row[i])
        leave = stamp(trades.exit_date[i]) if dates else str(trades.exit_row[i])
        print(f"{trades.env[i]:4d}  {entry:19s}  {leave:19s}  {trades.hold[i]:4d}  {trades.position[i]:8.2f}  "
              f"{trades.open_value[i]:11.4f}  {trades.close_value[i]:11.4f}  {100 * trades.ret[i]:6.2f}  "
              f"{KINDS[trades.kind[i]]}")
    env.close()
    return dict(index=index, score=score, by_strategy=board, trades=trades, min_trades=min_trades, winner=winner)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--capacity", type=int, default=32)
    ap.add_argument("--show", type=int, default=12)
    a = ap.parse_args()
    main(a.rows, a.replicas, capacity=a.capacity, show=a.show)
