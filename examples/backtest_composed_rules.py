#!/usr/bin/env python3
"""Strategies COMPOSED on the device from a few clause rows (`compose_signals`): specs -> indicator bank
(`build_indicators`) -> clause table (`build_signals(..., bind=False)` with `signals.clauses`, zone codes
0 / 1 / 2) -> composed table (`compose_signals`) -> `backtest_signals` -> `by_strategy().top()`.  Two
families over the same clause rows:

  trend AND entry   long while EMA(fast) > EMA(slow) AND the RSI is not overbought, flat otherwise
                    — every (trend clause, RSI clause) pair is one strategy
  enter / exit      go long on a z-score breakout, leave only when a slower trend clause turns down, and
                    keep the position in between (`signals.KEEP`)

A handful of clause rows gives trends x entries strategies; no [S, T] array exists on the host.

    python examples/backtest_composed_rules.py [--envs 2048] [--top 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batched_random_policy import make_frame  # noqa: E402

FAST, SLOW = (5, 8, 13, 21), (34, 55, 89, 144)
RSI_N, RSI_CAP = (7, 14, 21), (65.0, 70.0, 80.0)
Z_N, Z_ENTER = (20, 50, 100), (1.0, 2.0)
SHORT, FLAT, LONG = 0, 1, 2  # indices into positions=[-1, 0, 1]


def clause_rows():
    """(indicator specs, clause rules, labels, the clause rows of each kind)"""
    from gym_trading_env_amd import signals
    specs = np.concatenate([signals.indicators("ema", list(FAST + SLOW)), signals.indicators("rsi", list(RSI_N)),
                            signals.indicators("zscore", list(Z_N))])
    ema = {n: i for i, n in enumerate(FAST + SLOW)}
    rsi = {n: len(ema) + i for i, n in enumerate(RSI_N)}
    z = {n: len(ema) + len(rsi) + i for i, n in enumerate(Z_N)}
    rules, labels, kinds = [], [], {"trend": [], "rsi": [], "breakout": []}
    for f in FAST:      # UP while the fast average is above the slow one
        for s in SLOW:
            kinds["trend"].append(len(rules))
            rules.append(signals.clauses(a=ema[f], b=ema[s], hi=0.0, lo=0.0, warmup=s))
            labels.append(f"EMA{f}>EMA{s}")
    for n in RSI_N:     # UP while overbought
        for cap in RSI_CAP:
            kinds["rsi"].append(len(rules))
            rules.append(signals.clauses(a=rsi[n], hi=cap, lo=cap, warmup=n))
            labels.append(f"RSI{n}>{cap:.0f}")
    for n in Z_N:       # UP on a breakout above the band
        for k in Z_ENTER:
            kinds["breakout"].append(len(rules))
            rules.append(signals.clauses(a=z[n], hi=k, lo=-k, warmup=n))
            labels.append(f"z{n}>{k}")
    return specs, np.concatenate(rules), labels, kinds


def strategies(labels, kinds):
    """(COMPOSE_DTYPE [S], labels): the two families"""
    from gym_trading_env_amd import signals
    UP, DOWN, KEEP = signals.UP, signals.DOWN, signals.KEEP
    pairs = np.array([(t, r) for t in kinds["trend"] for r in kinds["rsi"]])
    trend_and_entry = signals.compose(pairs, lambda trend, overbought: LONG if trend == UP and overbought != UP else FLAT,
                                      initial=FLAT)
    pairs2 = np.array([(b, t) for b in kinds["breakout"] for t in kinds["trend"]])
    enter_exit = signals.compose(pairs2, lambda breakout, trend: LONG if breakout == UP else FLAT if trend == DOWN else KEEP,
                                 initial=FLAT)
    names = [f"{labels[t]} and not {labels[r]}" for t, r in pairs] + \
            [f"enter {labels[b]}, exit not {labels[t]}" for b, t in pairs2]
    return np.concatenate([trend_and_entry, enter_exit]), names


def main(envs=2048, K=1000, duration=168, top=5, details=False):
    import gym_trading_env_amd as gte
    df = make_frame(T=6000, seed=3)
    specs, rules, labels, kinds = clause_rows()
    composed, names = strategies(labels, kinds)
    env = gte.BatchedTradingEnv(df, num_envs=envs, positions=[-1, 0, 1], windows=None,
                                trading_fees=1e-4, borrow_interest_rate=3e-6, initial_position=0,
                                max_episode_duration=duration, autoreset="next_step", seed=5)
    clauses = env.build_signals(env.build_indicators(specs), rules, bind=False)   # int8 [R, T] of zone codes
    table = env.compose_signals(clauses, composed)                                # int8 [S, T], bound
    env.reset()
    board = env.backtest_signals(K).by_strategy()
    print(f"{len(composed)} strategies composed from {len(rules)} clause rows, {envs} envs x {K} steps, "
          f"episodes of {duration} rows from random starts")
    leaders = {}
    for family, members in (("trend and entry", slice(0, len(kinds["trend"]) * len(kinds["rsi"]))),
                            ("enter / exit", slice(len(kinds["trend"]) * len(kinds["rsi"]), len(composed)))):
        index, score = board.top(len(composed), "mean_episode_return", min_episodes=2)  # (240 <= the 256 ranked)
        index, score = index.cpu().numpy(), score.cpu().numpy()
        inside = (index >= members.start) & (index < members.stop)
        leaders[family] = (index[inside][:top], score[inside][:top])
        print(f"  {family}, by mean episode return:")
        for s, v in zip(*leaders[family]):
            print(f"    {names[s]:44s} {v:+.5f}")
    out = (leaders, table.cpu().numpy(), clauses.cpu().numpy(), composed) if details else leaders
    env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--top", type=int, default=5)
    a = ap.parse_args()
    main(a.envs, top=a.top)
