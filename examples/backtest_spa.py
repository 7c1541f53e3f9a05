#!/usr/bin/env python3
"""Which strategies of a sweep are better than luck — when most of the sweep is poor and noisy?  The crossover sweep
of backtest_reality_check.py runs on a random walk at twice the capital (positions -2 and 2): no crossover has an
edge, every one of them pays fees and borrow interest, and their period returns swing widely.  A few cautious
strategies are added that do have an edge: they see the sign of the next return, right seven times out of ten, and
go long with a tenth of the capital or stay out.  Their mean period return is small next to the swings of the
crossovers, so White's Reality Check, whose statistic is the raw maximum of centred means, cannot tell them from
luck: the noisy losers widen its null distribution.  Hansen's SPA test (`spa()`) measures every strategy in its own
bootstrap deviation and leaves the clearly poor ones out of the null; its step-down then says which strategies beat
doing nothing.  The Reality Check's p-value is printed next to the three of the SPA test, and the strategies the
step-down keeps.

    python examples/backtest_spa.py [--fast 16] [--slow 16] [--edge 3] [--replicas 16] [--resamples 1000]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402


def main(n_fast=16, n_slow=16, n_edge=3, replicas=16, K=2000, T=6000, duration=168, n_periods=24, n_resamples=1000,
         block=2.0, seed=7, alpha=0.05):
    import gym_trading_env_amd as gte
    from gym_trading_env_amd import periods, signals
    df = make_frame(T=T, seed=3)
    close = df["close"].to_numpy()
    fast = np.unique(np.linspace(3, 40, n_fast).astype(int))
    slow = np.unique(np.linspace(50, 200, n_slow).astype(int))
    pair_fast, pair_slow = (g.reshape(-1) for g in np.meshgrid(fast, slow, indexing="ij"))
    windows = np.unique(np.concatenate([fast, slow]))
    bank = signals.sma_bank(close, windows)
    a, b = np.searchsorted(windows, pair_fast), np.searchsorted(windows, pair_slow)
    n_cross = len(a)
    # the cautious strategies: one indicator row each, the sign of the NEXT return flipped three times in ten
    rng = np.random.default_rng(seed)
    up = np.sign(np.append(np.diff(close), 0.0))
    peeks = np.stack([up * np.where(rng.random(T) < 0.7, 1.0, -1.0) for _ in range(n_edge)]).astype(np.float32)
    bank = np.concatenate([bank, peeks])
    a = np.concatenate([a, len(windows) + np.arange(n_edge)])
    b = np.concatenate([b, np.full(n_edge, -1)])
    warmup = np.concatenate([pair_slow - 1, np.zeros(n_edge, int)])
    # positions [-2, 0, 0.1, 2]: a crossover is long 2 above and short 2 below, a cautious one long 0.1 or out
    pos_up = np.concatenate([np.full(n_cross, 3), np.full(n_edge, 2)])
    pos_down = np.concatenate([np.full(n_cross, 0), np.full(n_edge, 1)])
    rules = signals.rules(a=a, b=b, warmup=warmup, pos_up=pos_up, pos_down=pos_down, pos_neutral=-1)
    S = len(rules)
    env = gte.BatchedTradingEnv(df, num_envs=S * replicas, positions=[-2, 0, 0.1, 2], windows=None, trading_fees=1e-4,
                                borrow_interest_rate=3e-6, initial_position=0, max_episode_duration=duration,
                                autoreset="next_step", seed=5)
    env.build_signals(bank, rules)
    env.reset()
    env.track_periods(periods.blocks(T, n_periods))
    board = env.backtest_signals(K).period_stats.by_strategy()      # fields [S, n_periods]
    spa = board.spa(n_resamples=n_resamples, block=block, seed=seed, alpha=alpha)
    rc = spa.reality_check
    superior = [int(s) for s in spa.superior().cpu().numpy()]
    print(f"{n_cross} crossovers at twice the capital and {n_edge} cautious strategies with an edge, {n_periods} periods, "
          f"{n_resamples} resamples (mean block {block:g} periods); {spa.num_studentised} strategies take part")
    print(f"Reality Check p-value {rc.p_value:.3f} (leader by mean: strategy {rc.best})   "
          f"SPA p-values (lower, consistent, upper) {spa.p_lower:.3f} {spa.p_consistent:.3f} {spa.p_upper:.3f} "
          f"(leader by t-statistic: strategy {spa.best}, t = {spa.statistic:.2f})")
    print(f"step-down at level {alpha:g}: {spa.num_rejected} of {S} strategies beat doing nothing, in "
          f"{spa.rounds_run} rounds: {superior}  (the cautious ones are {list(range(n_cross, S))})")
    out = dict(spa=spa, p_reality=rc.p_value, strategies=S, crossovers=n_cross, superior=superior,
               by_strategy=board.numpy())
    env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fast", type=int, default=16)
    ap.add_argument("--slow", type=int, default=16)
    ap.add_argument("--edge", type=int, default=3)
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--resamples", type=int, default=1000)
    a = ap.parse_args()
    main(a.fast, a.slow, a.edge, a.replicas, n_resamples=a.resamples)
