#!/usr/bin/env python3
"""Show a strategy.  The crossover sweep of backtest_diversified.py ranks a few hundred crossovers and picks five
that are not the same bet; this example then LOOKS at the five: a second, small env follows one pick per env over the
whole table, and `backtest_curves` keeps its equity curve and its underwater curve (the deepest drawdown of every
window of `--stride` steps against the running peak) while it steps — the rows are written by the launch that holds
the step in registers, no [K, N] action tensor and no host loop.  A few sampled rows are printed beside
`stats.max_drawdown`, which the maximum of the underwater column equals to the bit.

    python examples/backtest_equity_curves.py [--fast 12] [--slow 12] [--replicas 8] [--stride 24] [--show 10]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402


def main(n_fast=12, n_slow=12, replicas=8, K=1500, T=6000, duration=168, picks=5, n_periods=24, max_corr=0.7,
         min_steps=200, stride=24, show=10):
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
    kw = dict(positions=[-1, 0, 1], windows=None, trading_fees=1e-4, borrow_interest_rate=3e-6, initial_position=1)
    bank = signals.sma_bank(close, windows)
    # 1. the sweep: random starts, short episodes, statistics per period -> five decorrelated picks
    env = gte.BatchedTradingEnv(df, num_envs=S * replicas, max_episode_duration=duration, autoreset="next_step",
                                seed=5, **kw)
    env.build_signals(bank, rules)
    env.reset()
    env.track_periods(periods.blocks(T, n_periods))
    board = env.backtest_signals(K).period_stats.by_strategy()
    got = board.diversified(picks, "sharpe", max_corr=max_corr, min_steps=min_steps).numpy()
    chosen = [int(s) for s in got["picks"] if s >= 0]
    env.close()
    if not chosen:
        raise SystemExit("diversified() found no candidate (a strategy must step in every period): nothing to follow")
    # 2. the shortlist: env e follows pick e from the first row of the table to its last
    book = gte.BatchedTradingEnv(df, num_envs=len(chosen), autoreset=None, seed=5, **kw)
    book.build_signals(bank, rules[chosen])
    book.reset()
    steps = T - 1 - int(book.state("idx").max())
    curves = book.backtest_curves(steps, stride=stride, drawdown=True, row=True)
    equity, under = curves.valuation.cpu().numpy(), curves.drawdown.cpu().numpy()
    dates = curves.dates(book)[:, 0]
    stats = curves.stats.numpy()
    print(f"{S} crossovers swept over {S * replicas} envs x {K} steps; {len(chosen)} picks followed over {steps} "
          f"steps, one row per {stride}: {curves.rows} rows")
    head = "  ".join(f"{pair_fast[s]:>3d}/{pair_slow[s]:<3d} equity  under" for s in chosen)
    print(f"{'date':>19s}  {head}")
    for j in np.unique(np.linspace(0, curves.rows - 1, show).astype(int)):
        cells = "  ".join(f"{equity[j, e]:14.2f} {-100 * under[j, e]:5.1f}%" for e in range(len(chosen)))
        print(f"{str(dates[j])[:19]:>19s}  {cells}")
    print(f"{'max drawdown':>19s}  " + "  ".join(f"{'':14s} {-100 * stats['max_drawdown'][e]:5.1f}%"
                                                 for e in range(len(chosen))))
    assert (under.max(axis=0) == stats["max_drawdown"]).all()  # the column's maximum IS the record's, to the bit
    book.close()
    return dict(picks=chosen, curves=curves, equity=equity, underwater=under, dates=dates, stats=stats)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fast", type=int, default=12)
    ap.add_argument("--slow", type=int, default=12)
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--picks", type=int, default=5)
    ap.add_argument("--max-corr", type=float, default=0.7)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--stride", type=int, default=24)
    ap.add_argument("--show", type=int, default=10)
    a = ap.parse_args()
    main(a.fast, a.slow, a.replicas, K=a.steps, T=a.rows, picks=a.picks, max_corr=a.max_corr, stride=a.stride,
         show=a.show)
