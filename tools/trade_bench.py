#!/usr/bin/env python3
"""What trade tracking costs, us per step of the whole batch: backtest_signals(K), S = 64, with
`track_trades` off and on, each without and with 256 exit rules bound, at 65 536 envs on bench.py's c3 shape
and at 4 096 on its c2 shape:

  off / on                gte_backtest_signal_kernel  /  gte_trade_signal_kernel
  off+exits / on+exits    gte_backtest_exit_kernel    /  gte_trade_exit_kernel

The comparison is on against off in the same run.  With --parent LIB (a build of libgte from the parent commit)
the two off legs are also run through that library in the same process, on a second env of the same seed
(tools/lib_ab.py's way): they launch the same kernels, so they should tie within the spread of the passes.

One process; episodes out of phase (bench.desynchronise); the legs are interleaved pass by pass and timed with
device events on the env's stream; every leg is preceded by its switches (tracking, rules) and one untimed call
of itself, which also takes the clearing a switch of tracking asks for.  The spread of a leg is its min .. max
over the passes.

    python tools/trade_bench.py [--k 512] [--reps 9] [--parent libgte_parent.so]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from signal_bench import random_table  # noqa: E402

SHAPES = (("c3", 65_536), ("c2", 4_096))


def make_env(torch, wl, N, K, library=None):
    from gym_trading_env_amd import _abi
    from gym_trading_env_amd.batched import BatchedTradingEnv
    data = bench.synthetic_dataset(0, wl["T"], wl["n_static"])
    kw = dict(bench.env_kwargs(wl))
    full = dict(_abi.SYMBOLS)
    if library:  # an older build lacks the newer entry points: they are not bound (tools/lib_ab.py)
        have = C.CDLL(library)
        _abi.SYMBOLS = {k: v for k, v in full.items() if hasattr(have, k)}
        kw["library_path"] = library
    try:
        env = BatchedTradingEnv(data, num_envs=N, seed=1, output="torch", **kw)
    finally:
        _abi.SYMBOLS = full
    env.reset()
    torch.manual_seed(0)
    bench.desynchronise(env, torch.randint(0, len(env.positions), (K, N), dtype=torch.int32, device="cuda"),
                        wl["max_episode_duration"])
    env.bind_signals(random_table(torch, 64, wl["T"]))
    return env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent", default=None, help="libgte.so built from the parent commit: its off legs as well")
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi, signals
    if not torch.cuda.is_available():
        sys.exit("trade_bench needs the GPU: nothing here can be timed without it")
    K, R = a.k, 256
    rng = np.random.default_rng(0)
    rules = signals.exit_rules(stop_loss=rng.uniform(0.002, 0.02, R), take_profit=rng.uniform(0.004, 0.04, R),
                               trailing=rng.uniform(0.002, 0.02, R), max_hold=rng.integers(8, 96, R), exit_position=1)
    d_rules = torch.from_numpy(rules.view(np.uint8).reshape(R, 32).copy()).cuda()
    results = {}
    for shape, N in SHAPES:
        wl = bench.WORKLOADS[shape]
        env = make_env(torch, wl, N, K)
        parent = make_env(torch, wl, N, K, os.path.abspath(a.parent)) if a.parent else None

        def leg(e, track, exits):
            def before():
                if track is not None:
                    e.track_trades(track)
                e.bind_exits(d_rules if exits else None)
                e.backtest_signals(K)
            return before, lambda: e.backtest_signals(K)

        legs = [("off", *leg(env, False, False)), ("on", *leg(env, True, False)),
                ("off+exits", *leg(env, False, True)), ("on+exits", *leg(env, True, True))]
        if parent is not None:
            legs += [("parent off", *leg(parent, None, False)), ("parent off+exits", *leg(parent, None, True))]
        times = {n: [] for n, _, _ in legs}
        for rep in range(a.reps + 1):  # pass 0 is the warm-up: allocations, code objects, geometry choices
            for n, before, f in legs:
                e = parent if n.startswith("parent") else env
                before()
                e.timer_start()
                f()
                t = e.timer_stop() * 1e3 / K
                if rep:
                    times[n].append(t)
        env.track_trades(True)
        env.bind_exits(d_rules)
        stats = env.backtest_signals(K)
        trades = stats.trade_stats
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        results[shape] = dict(envs=N, K=K, reps=a.reps, rules=R, strategies=64, us_per_step=med,
                              us_per_step_min={n: min(t) for n, t in times.items()},
                              us_per_step_max={n: max(t) for n, t in times.items()},
                              transitions_last_call=int(stats.steps.sum().item()),
                              closed_last_call=int(trades.closed.sum().item()),
                              exposure_last_call=int(trades.exposure.sum().item()))
        for n, _, _ in legs:
            print(f"{shape} {N:6d} envs K={K}  {n:17s} {med[n]:8.3f} us/step  (min {min(times[n]):.3f}, "
                  f"max {max(times[n]):.3f}, {a.reps} interleaved passes)", flush=True)
        print(f"{shape} {N:6d} envs K={K}  on / off {med['on'] / med['off']:.3f}   on+exits / off+exits "
              f"{med['on+exits'] / med['off+exits']:.3f}   ({results[shape]['closed_last_call']} trades closed in "
              f"{results[shape]['transitions_last_call']} transitions of the last call)", flush=True)
        env.close()
        if parent is not None:
            parent.close()
    print(json.dumps({"trade_bench": dict(library=os.path.basename(_abi.LIB_PATH),
                                          parent=os.path.basename(a.parent) if a.parent else None, shapes=results)}))


if __name__ == "__main__":
    main()
