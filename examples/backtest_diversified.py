#!/usr/bin/env python3
"""Ten leaders or one bet ten times?  The crossover sweep of backtest_walk_forward.py runs with the market rows cut
into equal periods, the first two thirds of them for training.  `top(10)` of such a sweep is mostly one crossover
under ten neighbouring parameterisations.  `diversified(10)` picks greedily on the device instead: the best strategy,
everything whose training-period returns correlate with it above `--max-corr` dropped, the best of what is left, and
so on.  The two shortlists are printed side by side, the second with the size of the cluster every pick removed, and
then both shortlists' Sharpe ratios on the test periods.  Run until nothing is left, the number of picks says how
many independent things the sweep tried at that threshold.

    python examples/backtest_diversified.py [--fast 16] [--slow 16] [--replicas 8] [--top 10] [--max-corr 0.7]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402


def main(n_fast=16, n_slow=16, replicas=8, K=1500, T=6000, duration=168, top=10, n_periods=24, max_corr=0.7,
         min_steps=200):
    import gym_trading_env_amd as gte
    from gym_trading_env_amd import periods, signals
    df = make_frame(T=T, seed=3)
    close = df["close"].to_numpy()
    fast = np.unique(np.linspace(3, 40, n_fast).astype(int))
    slow = np.unique(np.linspace(50, 200, n_slow).astype(int))
    pair_fast, pair_slow = (g.reshape(-1) for g in np.meshgrid(fast, slow, indexing="ij"))
    windows = np.unique(np.concatenate([fast, slow]))
    rules = signals.rules(a=np.searchsorted(windows, pair_fast), b=np.searchsorted(windows, pair_slow),
                          warmup=pair_slow - 1, pos_up=2, pos_down=0, pos_neutral=-1)   # long above, short below
    S = len(rules)
    N = S * replicas
    env = gte.BatchedTradingEnv(df, num_envs=N, positions=[-1, 0, 1], windows=None, trading_fees=1e-4,
                                borrow_interest_rate=3e-6, initial_position=1, max_episode_duration=duration,
                                autoreset="next_step", seed=5)
    env.build_signals(signals.sma_bank(close, windows), rules)
    env.reset()
    env.track_periods(periods.blocks(T, n_periods))
    board = env.backtest_signals(K).period_stats.by_strategy()          # fields [S, n_periods]
    train = list(range(2 * n_periods // 3))
    test = list(range(2 * n_periods // 3, n_periods))
    index, train_sharpe = board.top(top, "sharpe", periods=train, min_steps=min_steps)
    pick = board.diversified(top, "sharpe", periods=train, max_corr=max_corr, min_steps=min_steps)
    every = board.diversified(gte._abi.GTE_RANK_MAX, "sharpe", periods=train, max_corr=max_corr, min_steps=min_steps)
    test_sharpe = board.select(test).sharpe().cpu().numpy()
    lead = index.cpu().numpy().tolist()
    got = pick.numpy()
    chosen = [int(s) for s in got["picks"] if s >= 0]
    print(f"{len(fast)} fast x {len(slow)} slow = {S} crossovers over {N} envs x {K} steps, {n_periods} periods: "
          f"{len(train)} train, {len(test)} test; {pick.num_candidates} candidates, correlations above {max_corr} "
          f"count as the same bet")
    print("            top()                          |            diversified()")
    print("rank strategy fast slow train_sharpe  test  | strategy fast slow train_sharpe  test  cluster")
    cell = lambda s, a: f"{s:8d} {pair_fast[s]:4d} {pair_slow[s]:4d} {a:12.4f} {test_sharpe[s]:6.3f}"
    for place in range(max(len(lead), len(chosen))):
        left = cell(lead[place], float(train_sharpe[place])) if place < len(lead) else " " * 38
        right = (cell(chosen[place], float(got["scores"][place])) + f" {int(got['cluster_size'][place]):7d}"
                 if place < len(chosen) else "")
        print(f"{place + 1:4d} {left}  | {right}")
    mean = lambda ids: float(np.nanmean(test_sharpe[ids])) if len(ids) else float("nan")
    pairs = got["corr"][:len(chosen), :len(chosen)][~np.eye(len(chosen), dtype=bool)]
    print(f"mean test Sharpe: top() {mean(lead):+.4f}, diversified() {mean(chosen):+.4f}; the highest correlation "
          f"between two picks is {pairs.max() if len(pairs) else float('nan'):.3f}")
    trials = every.effective_trials
    print(f"{every.num_picked} picks " + (f"exhaust the {every.num_candidates} candidates: about {trials} independent "
                                          f"strategies at {max_corr}" if trials is not None else
                                          f"leave {every.remaining} of {every.num_candidates} candidates: more than "
                                          f"{every.num_picked} independent strategies at {max_corr}"))
    host = board.numpy()
    env.close()
    return dict(top=lead, picks=chosen, result=pick, every=every, test_sharpe=test_sharpe, by_strategy=host,
                train=train, test=test)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fast", type=int, default=16)
    ap.add_argument("--slow", type=int, default=16)
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--max-corr", type=float, default=0.7)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--periods", type=int, default=24)
    a = ap.parse_args()
    main(a.fast, a.slow, a.replicas, K=a.steps, T=a.rows, top=a.top, n_periods=a.periods, max_corr=a.max_corr)
