#!/usr/bin/env python3
"""A sweep over three strategy families with NOTHING BUT SPECS AND RULES on the host
(`build_indicators` + `build_signals` + `backtest_signals`): the device computes the indicator bank from
the market data it already holds — one 16-byte spec per row — then the int8 [strategies, T] table from
one 32-byte rule per strategy, then the per-env statistics.  No indicator, no table and no price series
is computed on or copied from the host.

  * an EMA crossover with a latched band: long while EMA(fast) - EMA(slow) stayed above +band since it
    was last below -band, short the other way round;
  * an RSI(n) band: long once RSI falls below 30, short once it rises above 70, keep the position in
    between (latched, one indicator alone: b = -1);
  * a z-score breakout: long above +z standard deviations of the last n closes, short below -z, flat
    in between.

Prints the best strategies of each family.

    python examples/backtest_indicator_sweep.py [--strategies 384] [--replicas 8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402

FAMILIES = ("EMA crossover", "RSI band", "z-score breakout")


def grid(strategies, seed=0):
    """(specs, rules, family, label): the bank rows every family needs, each once, and one rule per
    strategy that names them."""
    from gym_trading_env_amd import signals
    rng = np.random.default_rng(seed)
    family = np.arange(strategies) % 3
    n_ema, n_rsi, n_z = ((family == f).sum() for f in range(3))
    fast = rng.integers(3, 40, n_ema)
    slow = fast + rng.integers(5, 200, n_ema)
    band = rng.choice([0.0, 0.1, 0.2, 0.4], n_ema).astype(np.float32)
    rsi_n = rng.integers(5, 40, n_rsi)
    z_n = rng.integers(10, 200, n_z)
    z_hi = rng.choice([1.0, 1.5, 2.0, 2.5], n_z).astype(np.float32)
    # the bank: every (kind, n) once, in a fixed order
    ema_ns, rsi_ns, z_ns = np.unique(np.concatenate([fast, slow])), np.unique(rsi_n), np.unique(z_n)
    specs = np.concatenate([signals.indicators("ema", ema_ns), signals.indicators("rsi", rsi_ns),
                            signals.indicators("zscore", z_ns)])
    ema_row = lambda n: np.searchsorted(ema_ns, n)
    rsi_row = lambda n: len(ema_ns) + np.searchsorted(rsi_ns, n)
    z_row = lambda n: len(ema_ns) + len(rsi_ns) + np.searchsorted(z_ns, n)
    rules = np.zeros(strategies, dtype=signals.RULE_DTYPE)
    rules[family == 0] = signals.rules(a=ema_row(fast), b=ema_row(slow), hi=band, lo=-band, warmup=slow,
                                       pos_up=2, pos_down=0, pos_neutral=-1, latch=True)
    rules[family == 1] = signals.rules(a=rsi_row(rsi_n), b=-1, hi=70.0, lo=30.0, warmup=rsi_n,
                                       pos_up=0, pos_down=2, pos_neutral=-1, latch=True)
    rules[family == 2] = signals.rules(a=z_row(z_n), b=-1, hi=z_hi, lo=-z_hi, warmup=z_n - 1,
                                       pos_up=2, pos_down=0, pos_neutral=1, latch=False)
    label = np.empty(strategies, dtype=object)
    label[family == 0] = [f"EMA({f}) / EMA({s}) band {b:.1f}" for f, s, b in zip(fast, slow, band)]
    label[family == 1] = [f"RSI({n}) 30 / 70" for n in rsi_n]
    label[family == 2] = [f"z({n}) +-{z:.1f}" for n, z in zip(z_n, z_hi)]
    return specs, rules, family, label


def main(strategies=384, replicas=8, K=1000, duration=168, details=False):
    import gym_trading_env_amd as gte
    df = make_frame(T=6000, seed=3)
    specs, rules, family, label = grid(strategies)
    N = strategies * replicas
    env = gte.BatchedTradingEnv(df, num_envs=N, positions=[-1, 0, 1], windows=None,
                                trading_fees=1e-4, borrow_interest_rate=3e-6, initial_position=0,
                                max_episode_duration=duration, autoreset="next_step", seed=5)
    bank = env.build_indicators(specs)            # f32 [rows, T], written on the device from `close`
    table = env.build_signals(bank, rules)        # int8 [strategies, T], read from the bank in place, and bound
    env.reset()
    stats = env.backtest_signals(K)               # env e follows strategy e % strategies
    by_strategy = lambda x: x.cpu().numpy().reshape(replicas, strategies).sum(0)
    episodes = by_strategy(stats.episodes)
    mean_return = by_strategy(stats.ep_return_sum) / np.maximum(episodes, 1)
    trades = by_strategy(stats.trades)
    print(f"{strategies} strategies x {replicas} envs x {K} steps, episodes of {duration} rows from random starts; "
          f"{len(specs)} indicator rows and the table built on the device")
    for f, name in enumerate(FAMILIES):
        mine = np.flatnonzero(family == f)
        print(f"  {name}:")
        for s in mine[np.argsort(-mean_return[mine])][:3]:
            print(f"    {label[s]:32s} mean episode return {mean_return[s]:+.4f} over {episodes[s]} episodes, "
                  f"{trades[s]} trades")
    assert (episodes > 0).all() and np.isfinite(mean_return).all()
    out = (mean_return, family, bank.cpu().numpy(), table.cpu().numpy(), specs, rules) if details else mean_return
    env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--strategies", type=int, default=384)
    ap.add_argument("--replicas", type=int, default=8)
    a = ap.parse_args()
    main(a.strategies, a.replicas)
