#!/usr/bin/env python3
"""How much does picking the winner of a sweep overfit?  The crossover sweep of backtest_walk_forward.py runs on a
random walk, where no crossover has an edge, with the market rows cut into equal periods.  One train / test split is
a single draw; `cscv()` makes every draw there is (combinatorially symmetric cross-validation: the periods are cut
into G groups, every way of taking half of them in sample is a split) on the device and reports

  - the probability of backtest overfitting (PBO): the share of splits whose in-sample winner lands in the lower half
    of all strategies out of sample — about one half when the winner was picked for its luck;
  - the probability that the selected strategy loses out of sample;
  - the performance-degradation line: the winner's out-of-sample Sharpe ratio against its in-sample one,

next to the Reality Check p-value of the same leaderboard (`reality_check()`: is the best of S tries better than what
luck gives the best of S tries?).  The second case adds one strategy with a real edge — it sees the sign of the next
return, right four times out of five — and the PBO falls to zero.

    python examples/backtest_overfitting.py [--fast 16] [--slow 16] [--replicas 16] [--groups 12]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402


def sweep(df, fast, slow, replicas, K, duration, n_periods, groups, n_resamples, seed, edge):
    """One sweep, its overfit check and its reality check over all periods; `edge`: append the strategy that peeks."""
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
    check = board.cscv(groups=groups, metric="sharpe")              # enqueued, like the reality check after it
    rc = board.reality_check(n_resamples=n_resamples, block=2.0, seed=seed)
    slope, intercept = check.degradation()
    out = dict(check=check, pbo=check.pbo, prob_loss=check.prob_loss, slope=slope, intercept=intercept,
               valid=check.num_valid, splits=check.num_splits, eligible=check.num_eligible, strategies=S,
               winners=np.unique(check.best.cpu().numpy()), p_reality=rc.p_value, by_strategy=board.numpy())
    env.close()
    return out


def main(n_fast=16, n_slow=16, replicas=16, K=2000, T=6000, duration=168, n_periods=24, groups=12, n_resamples=1000,
         seed=7):
    df = make_frame(T=T, seed=3)
    fast = np.unique(np.linspace(3, 40, n_fast).astype(int))
    slow = np.unique(np.linspace(50, 200, n_slow).astype(int))
    args = (df, fast, slow, replicas, K, duration, n_periods, groups, n_resamples, seed)
    noise, edge = sweep(*args, edge=False), sweep(*args, edge=True)
    print(f"{noise['strategies']} crossovers on a random walk, {n_periods} periods in {groups} groups, "
          f"{noise['splits']} splits; {noise['eligible']} strategies stepped in every group")
    for name, case in (("random walk:  ", noise), ("one real edge:", edge)):
        print(f"{name} PBO {case['pbo']:.3f}   probability of loss {case['prob_loss']:.3f}   degradation line "
              f"OOS = {case['intercept']:+.4f} {case['slope']:+.3f} * IS   ({len(case['winners'])} different winners "
              f"in {case['valid']} valid splits)   Reality Check p-value {case['p_reality']:.3f}")
    return dict(noise=noise, edge=edge)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fast", type=int, default=16)
    ap.add_argument("--slow", type=int, default=16)
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--groups", type=int, default=12)
    a = ap.parse_args()
    main(a.fast, a.slow, a.replicas, groups=a.groups)
