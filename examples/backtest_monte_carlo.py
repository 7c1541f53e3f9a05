#!/usr/bin/env python3
"""How bad can the winners get?  A sweep of SMA crossovers backtested in one fused launch with the per-trade list on
(`track_trades(list_capacity=64)`), the ten best by profit factor picked on the device, and then a Monte Carlo over
the closed trades of each: trades drawn with replacement from its list and compounded, a thousand times.  The
realised drawdown of a backtest is ONE ordering of its trades; the table shows the 5 % / 50 % / 95 % quantiles of the
maximum drawdown over the resampled orderings and the risk of halving the account.  The ranking's index goes into the
Monte Carlo as it is: nothing but the number of trades visits the host before the table is printed.

    python examples/backtest_monte_carlo.py [--strategies 24] [--replicas 8] [--resamples 1000]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402

CAPACITY = 64


def crossovers(count):
    """`count` (fast, slow) window pairs: six fast windows, each against slow windows 2, 3, 4, ... times as long"""
    fast = np.array([5, 8, 13, 21, 34, 55])
    pairs = [(f, f * ratio) for ratio in range(2, 2 + (count + len(fast) - 1) // len(fast)) for f in fast]
    return np.array(pairs[:count])


def main(strategies=24, K=1000, replicas=8, T=6000, duration=168, top=10, resamples=1000, ruin=0.5, min_trades=8,
         seed=7):
    import gym_trading_env_amd as gte
    from gym_trading_env_amd import signals
    df = make_frame(T=T, seed=3)
    close = df["close"].to_numpy()
    pairs = crossovers(strategies)
    fast, slow = pairs[:, 0], pairs[:, 1]
    windows = np.unique(pairs)
    rules = signals.rules(a=np.searchsorted(windows, fast), b=np.searchsorted(windows, slow), warmup=slow - 1,
                          pos_up=2, pos_down=0, pos_neutral=-1)            # long above, short below
    S = len(pairs)
    N = S * replicas                                         # env e backtests crossover e % S
    env = gte.BatchedTradingEnv(df, num_envs=N, positions=[-1, 0, 1], windows=None,
                                trading_fees=1e-4, borrow_interest_rate=3e-6, initial_position=0,
                                max_episode_duration=duration, autoreset="next_step", seed=5)
    env.build_signals(signals.sma_bank(close, windows), rules)
    env.reset()
    env.track_trades(list_capacity=CAPACITY)                 # the first 64 trades of every env
    stats = env.backtest_signals(K)
    board = stats.trade_stats.by_strategy()
    index, score = board.top(top, "profit_factor", min_trades=min_trades)
    mc = board.monte_carlo(index, n_resamples=resamples, seed=seed, ruin=ruin, keep=("final", "max_drawdown"))
    quantiles = mc.quantile("max_drawdown", (0.05, 0.5, 0.95)).cpu().numpy()
    final = mc.quantile("final", 0.5).cpu().numpy()
    risk, truncated, size = mc.risk_of_ruin.cpu().numpy(), mc.truncated.cpu().numpy(), mc.pool_size.cpu().numpy()
    ids, score = index.cpu().numpy(), score.cpu().numpy()
    print(f"{S} crossovers over {N} envs x {K} steps; the {len(ids)} best by profit factor, {resamples} resampled "
          f"orderings of each one's trades")
    print(" strategy   SMA        profit factor  trades   drawdown 5%    50%    95%   median final  risk of ruin")
    for i, s in enumerate(ids):
        print(f"{s:9d}  {fast[s]:3d} / {slow[s]:3d}  {score[i]:13.4f}  {size[i]:6d}  {100 * quantiles[i, 0]:11.2f}  "
              f"{100 * quantiles[i, 1]:5.2f}  {100 * quantiles[i, 2]:5.2f}  {final[i]:13.4f}  {100 * risk[i]:11.2f}%")
    cut = [int(s) for s, t in zip(ids, truncated) if t]
    print(f"lists truncated at {CAPACITY} trades: " +
          (", ".join(f"strategy {s} ({int(t)} of its envs)" for s, t in zip(ids, truncated) if t) if cut else "none"))
    env.close()
    return dict(index=index, score=score, by_strategy=board, monte_carlo=mc, quantiles=quantiles, truncated=cut)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--strategies", type=int, default=24)
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--resamples", type=int, default=1000)
    a = ap.parse_args()
    main(a.strategies, replicas=a.replicas, resamples=a.resamples)
