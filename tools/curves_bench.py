#!/usr/bin/env python3
"""What the rows of `backtest_curves` cost, us per step of the whole batch, S = 64.

Shape A, 65 536 envs on bench.py's c3 shape, K = 512: `backtest_signals(K)` — the yardstick, measured in the SAME
process — against `backtest_curves(K)` with the valuation column alone and with all six, at stride 1 and 16, each
without and with 256 exit rules bound:

  signals / v1 / v16 / all1 / all16           gte_backtest_signal_kernel  /  gte_curve_signal_kernel
  signals+exits / v1+exits / ... / all16+exits  gte_backtest_exit_kernel  /  gte_curve_exit_kernel

and, for what a user had before: `loop`, signal_actions() + step() + state("portfolio_valuation") per step (over
--loop-steps steps), and for the action source `rollout(actions, valuation=True)` against
`backtest_curves(actions=actions)` with the valuation column (`rollout v` / `actions v1`).

Shape B, the shortlist: 64 envs that walk the whole table once (auto-reset off, no episode limit), the same legs
without exits.  One wavefront's worth of work per step: this shape is bound by the latency of a step, not by
bandwidth, so the rows cost what their stores add to the dependent chain.

One process; episodes out of phase (bench.desynchronise, shape A); the legs are interleaved pass by pass and timed
with device events on the env's stream; every leg is preceded by its switches (rules) and one untimed call of
itself.  The spread of a leg is its min .. max over the passes.

    python tools/curves_bench.py [--k 512] [--reps 9] [--loop-steps 64]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from signal_bench import random_table  # noqa: E402
from trade_bench import make_env  # noqa: E402

ALL = dict(valuation=True, drawdown=True, reward=True, position=True, row=True, flags=True)
ONE = dict(valuation=True, flags=False)
COLUMNS = (("v", ONE), ("all", ALL))
STRIDES = (1, 16)


def time_legs(legs, reps):
    """legs: (name, env, before, run, steps) -> {name: [us per step, ...]}; pass 0 is the warm-up"""
    times = {n: [] for n, *_ in legs}
    for rep in range(reps + 1):
        for n, e, before, f, steps in legs:
            before()
            e.timer_start()
            f()
            t = e.timer_stop() * 1e3 / steps
            if rep:
                times[n].append(t)
    return times


def curve_legs(env, K, exits, rules, tail=""):
    """the yardstick and the four curve legs of one source; the result of a leg's untimed call is its `out`"""
    def switch():
        if rules is not None:
            env.bind_exits(rules if exits else None)

    def plain():
        switch()
        env.backtest_signals(K)
    legs = [("signals" + tail, env, plain, lambda: env.backtest_signals(K), K)]
    for label, keep in COLUMNS:
        for stride in STRIDES:
            held = {}

            def before(held=held, keep=keep, stride=stride):
                switch()
                held["out"] = env.backtest_curves(K, stride=stride, out=held.get("out"), **keep)
            legs.append((f"{label}{stride}{tail}", env, before,
                         lambda held=held, keep=keep, stride=stride: env.backtest_curves(K, stride=stride,
                                                                                         out=held["out"], **keep), K))
    return legs


def report(shape, N, K, legs, times, reps):
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    for n, *_ in legs:
        print(f"{shape} {N:6d} envs K={K}  {n:15s} {med[n]:8.3f} us/step  (min {min(times[n]):.3f}, "
              f"max {max(times[n]):.3f}, {reps} interleaved passes)", flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-steps", type=int, default=64)
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi, signals
    from gym_trading_env_amd.batched import BatchedTradingEnv
    if not torch.cuda.is_available():
        sys.exit("curves_bench needs the GPU: nothing here can be timed without it")
    K, R = a.k, 256
    rng = np.random.default_rng(0)
    rules = signals.exit_rules(stop_loss=rng.uniform(0.002, 0.02, R), take_profit=rng.uniform(0.004, 0.04, R),
                               trailing=rng.uniform(0.002, 0.02, R), max_hold=rng.integers(8, 96, R), exit_position=1)
    d_rules = torch.from_numpy(rules.view(np.uint8).reshape(R, 32).copy()).cuda()
    wl = bench.WORKLOADS["c3"]
    results = {}

    # --- shape A
    N = 65_536
    env = make_env(torch, wl, N, K)
    torch.manual_seed(1)
    acts = torch.randint(0, len(env.positions), (K, N), dtype=torch.int32, device="cuda")
    legs = curve_legs(env, K, False, d_rules) + curve_legs(env, K, True, d_rules, "+exits")
    off = lambda: env.bind_exits(None)
    held = {}

    def loop():
        for _ in range(a.loop_steps):
            env.step(env.signal_actions())
            env.state("portfolio_valuation")

    def before_rollout():
        off()
        held["rollout"] = env.rollout(acts, valuation=True, out=held.get("rollout"))

    def before_actions():
        off()
        held["curves"] = env.backtest_curves(actions=acts, out=held.get("curves"), **ONE)
    legs += [("loop", env, lambda: (off(), loop()), loop, a.loop_steps),
             ("rollout v", env, before_rollout, lambda: env.rollout(acts, valuation=True, out=held["rollout"]), K),
             ("actions v1", env, before_actions,
              lambda: env.backtest_curves(actions=acts, out=held["curves"], **ONE), K)]
    times = time_legs(legs, a.reps)
    med = report("c3", N, K, legs, times, a.reps)
    for tail in ("", "+exits"):
        base = med["signals" + tail]
        print(f"c3 {N:6d} envs K={K}  rows cost over signals{tail}: " + "   ".join(
            f"{l}{s}{tail} {med[f'{l}{s}{tail}'] - base:+.3f}" for l, _ in COLUMNS for s in STRIDES) + "  us/step",
            flush=True)
    print(f"c3 {N:6d} envs K={K}  loop / v1 {med['loop'] / med['v1']:.1f}x   rollout v / actions v1 "
          f"{med['rollout v'] / med['actions v1']:.3f}", flush=True)
    results["A"] = dict(shape="c3", envs=N, K=K, reps=a.reps, rules=R, strategies=64, loop_steps=a.loop_steps,
                        us_per_step=med, us_per_step_min={n: min(t) for n, t in times.items()},
                        us_per_step_max={n: max(t) for n, t in times.items()})
    env.close()
    del acts, held

    # --- shape B: the shortlist, 64 envs over the whole table
    N = 64
    kw = dict(bench.env_kwargs(wl), max_episode_duration="max", autoreset=None, initial_position=1)
    book = BatchedTradingEnv(bench.synthetic_dataset(0, wl["T"], wl["n_static"]), num_envs=N, seed=1, output="torch",
                             **kw)
    book.bind_signals(random_table(torch, 64, wl["T"]))
    book.reset()
    KB = wl["T"] - 1 - int(book.state("idx").max())
    # (every call, untimed or timed, starts from the first row)
    legs = [(n, e, (lambda before=before: (book.reset(), before(), book.reset())), f, steps)
            for n, e, before, f, steps in curve_legs(book, KB, False, None)]
    times = time_legs(legs, max(3, a.reps // 3))
    med = report("c3", N, KB, legs, times, max(3, a.reps // 3))
    print(f"c3 {N:6d} envs K={KB}  rows cost over signals: " + "   ".join(
        f"{l}{s} {med[f'{l}{s}'] - med['signals']:+.3f}" for l, _ in COLUMNS for s in STRIDES) +
        "  us/step (latency-bound: one wavefront per step)", flush=True)
    results["B"] = dict(shape="c3", envs=N, K=KB, reps=max(3, a.reps // 3), strategies=64, us_per_step=med,
                        us_per_step_min={n: min(t) for n, t in times.items()},
                        us_per_step_max={n: max(t) for n, t in times.items()})
    book.close()
    print(json.dumps({"curves_bench": dict(library=os.path.basename(_abi.LIB_PATH), shapes=results)}))


if __name__ == "__main__":
    main()
