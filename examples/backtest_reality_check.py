#!/usr/bin/env python3
"""Is the winner of a sweep better than what luck alone gives the best of that many tries?  The crossover sweep of
backtest_walk_forward.py runs on a random walk, where no crossover has an edge, with the market rows cut into
equal periods: the first two thirds are training periods, the rest is kept for a test (a strategy takes part only if
it stepped in every training period, hence enough replicas and steps to visit them all).  `reality_check()` then
bootstraps the training periods on the device (White's Reality Check: the maximum over ALL strategies of their
centred mean period return, resample by resample) and two p-values are printed side by side: the best NAIVE one —
the winner judged as if it had been the only strategy tried — and the Reality Check's, which knows how many were.

The second case is the same sweep with one more strategy that has a real edge: it sees the sign of the next return,
right four times out of five.  Its adjusted p-value stays small although it competes with the whole sweep.

    python examples/backtest_reality_check.py [--fast 16] [--slow 16] [--replicas 16] [--resamples 1000]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402


def sweep(df, fast, slow, replicas, K, duration, n_periods, n_train, n_resamples, block, seed, edge):
    """One sweep and its reality check over the training periods; `edge`: append the strategy that peeks."""
    import gym_trading_env_amd as gte
    from gym_trading_env_amd import periods, signals
    close = df["close"].to_numpy()
    T = len(close)
    pair_fast, pair_slow = (g.reshape(-1) for g in np.meshgrid(fast, slow, indexing="ij"))
    windows = np.unique(np.concatenate([fast, slow]))
    bank = signals.sma_bank(close, windows)
    a, b = np.searchsorted(windows, pair_fast), np.searchsorted(windows, pair_slow)
    warmup = pair_slow - 1
    if edge:   # one more indicator row: the sign of the NEXT return, flipped one time in five
        rng = np.random.default_rng(seed)
        peek = np.sign(np.append(np.diff(close), 0.0)) * np.where(rng.random(T) < 0.8, 1.0, -1.0)
        bank = np.concatenate([bank, peek[None, :].astype(np.float32)])
        a, b, warmup = np.append(a, len(windows)), np.append(b, -1), np.append(warmup, 0)
    rules = signals.rules(a=a, b=b, warmup=warmup, pos_up=2, pos_down=0, pos_neutral=-1)   # long above, short below
    S = len(rules)
    env = gte.BatchedTradingEnv(df, num_envs=S * replicas, positions=[-1, 0, 1], windows=None, trading_fees=1e-4,
                                borrow_interest_rate=3e-6, initial_position=1, max_episode_duration=duration,
                                autoreset="next_step", seed=5)
    env.build_signals(bank, rules)
    env.reset()
    env.track_periods(periods.blocks(T, n_periods))
    board = env.backtest_signals(K).period_stats.by_strategy()      # fields [S, n_periods]
    rc = board.reality_check(periods=range(n_train), n_resamples=n_resamples, block=block, seed=seed)
    out = dict(check=rc, p_naive=float(rc.p_individual[rc.eligible].min()) if rc.num_eligible else float("nan"),
               p_reality=rc.p_value, best=rc.best, strategies=S, eligible=rc.num_eligible,
               p_adjusted=rc.p_adjusted.cpu().numpy(), by_strategy=board.numpy())
    env.close()
    return out


def main(n_fast=16, n_slow=16, replicas=16, K=2000, T=6000, duration=168, n_periods=24, n_train=16, n_resamples=1000,
         block=2.0, seed=7):
    df = make_frame(T=T, seed=3)
    fast = np.unique(np.linspace(3, 40, n_fast).astype(int))
    slow = np.unique(np.linspace(50, 200, n_slow).astype(int))
    args = (df, fast, slow, replicas, K, duration, n_periods, n_train, n_resamples, block, seed)
    noise, edge = sweep(*args, edge=False), sweep(*args, edge=True)
    print(f"{noise['strategies']} crossovers on a random walk, {n_train} training periods, {n_resamples} resamples "
          f"(mean block {block:g} periods); {noise['eligible']} strategies stepped in every training period")
    print(f"random walk:     best naive p-value {noise['p_naive']:.3f}   Reality Check p-value {noise['p_reality']:.3f}"
          f"   (leader: strategy {noise['best']})")
    peek = edge["strategies"] - 1
    print(f"one real edge:   best naive p-value {edge['p_naive']:.3f}   Reality Check p-value {edge['p_reality']:.3f}"
          f"   (leader: strategy {edge['best']}; adjusted p-value of the one that peeks, strategy {peek}: "
          f"{edge['p_adjusted'][peek]:.3f})")
    return dict(noise=noise, edge=edge)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fast", type=int, default=16)
    ap.add_argument("--slow", type=int, default=16)
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--resamples", type=int, default=1000)
    a = ap.parse_args()
    main(a.fast, a.slow, a.replicas, n_resamples=a.resamples)
