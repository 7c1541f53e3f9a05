#!/usr/bin/env python3
"""The sweep of backtest_indicator_sweep.py (the same grid of EMA, RSI and z-score strategies, built on the
device from specs and rules) closed on the device as well: `backtest_signals(K).by_strategy()` folds the
per-env records into one record per strategy (`gte_reduce_backtest_stats`) and `.top(k, metric)` ranks
them (`gte_rank_strategies`).  The env count is NOT a multiple of the strategy count — the strategies get
`N // S` or `N // S + 1` envs each, which the fold takes from the map the backtest ran with — and the only
arrays that reach the host are the k leaders per metric.

    python examples/backtest_leaderboard.py [--strategies 384] [--envs 3000] [--top 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from backtest_indicator_sweep import grid  # noqa: E402
from batched_random_policy import make_frame  # noqa: E402

METRICS = ("mean_episode_return", "episode_sharpe", "sharpe", "neg_max_drawdown", "worst_reward_sum")


def main(strategies=384, envs=3000, K=1000, duration=168, top=5, details=False):
    import gym_trading_env_amd as gte
    assert envs % strategies != 0, "the point of this example: N is no multiple of S"
    df = make_frame(T=6000, seed=3)
    specs, rules, family, label = grid(strategies)
    env = gte.BatchedTradingEnv(df, num_envs=envs, positions=[-1, 0, 1], windows=None,
                                trading_fees=1e-4, borrow_interest_rate=3e-6, initial_position=0,
                                max_episode_duration=duration, autoreset="next_step", seed=5)
    env.build_signals(env.build_indicators(specs), rules)   # bank and table: device only, bound
    env.reset()
    stats = env.backtest_signals(K)                         # env e follows strategy e % strategies
    board = stats.by_strategy()                             # one record per strategy, on the device
    print(f"{strategies} strategies over {envs} envs x {K} steps ({int(board.envs.min())} to {int(board.envs.max())} "
          f"envs each), episodes of {duration} rows from random starts")
    leaders = {}
    for metric in METRICS:
        index, score = board.top(top, metric, min_episodes=4)
        leaders[metric] = (index.cpu().numpy(), score.cpu().numpy())
        print(f"  by {metric}:")
        for s, v in zip(*leaders[metric]):
            print(f"    {label[s]:32s} {v:+.5f}")
    out = (leaders, stats.numpy(), board.numpy()) if details else leaders
    env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--strategies", type=int, default=384)
    ap.add_argument("--envs", type=int, default=3000)
    ap.add_argument("--top", type=int, default=5)
    a = ap.parse_args()
    main(a.strategies, a.envs, top=a.top)
