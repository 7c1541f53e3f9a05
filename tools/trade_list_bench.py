#!/usr/bin/env python3
"""What the per-trade list costs, us per step of the whole batch: backtest_signals(K), S = 64, with
`track_trades()` alone — the yardstick, measured in the SAME process — and with `list_capacity` 16 and 64, each
without and with 256 exit rules bound, at 65 536 envs on bench.py's c3 shape and at 4 096 on its c2 shape:

  track / list16 / list64                  gte_trade_signal_kernel  /  gte_trade_list_signal_kernel
  track+exits / list16+exits / list64+exits  gte_trade_exit_kernel  /  gte_trade_list_exit_kernel

and the seconds `trade_stats.trades(strategy=top 64)` takes at capacity 16 (the gather on the device, one transfer,
the host's columns).  With --parent LIB (a build of libgte from the parent commit) the two list-off legs are also run
through that library in the same process, on a second env of the same seed (tools/lib_ab.py's way): they launch
the same kernels, so they should tie within the spread of the passes.

One process; episodes out of phase (bench.desynchronise); the legs are interleaved pass by pass and timed with
device events on the env's stream; every leg is preceded by its switches (capacity, rules) and one untimed call
of itself, which also takes the clearing a switch asks for.  The spread of a leg is its min .. max over the passes.

    python tools/trade_list_bench.py [--k 512] [--reps 9] [--parent libgte_parent.so]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from trade_bench import SHAPES, make_env  # noqa: E402

CAPACITIES = (16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent", default=None, help="libgte.so built from the parent commit: its list-off legs as well")
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi, signals
    if not torch.cuda.is_available():
        sys.exit("trade_list_bench needs the GPU: nothing here can be timed without it")
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
        if parent is not None:
            parent.track_trades()

        def leg(e, capacity, exits):
            def before():
                if capacity is not None:
                    e.track_trades(list_capacity=capacity)
                e.bind_exits(d_rules if exits else None)
                e.backtest_signals(K)
            return before, lambda: e.backtest_signals(K)

        legs = []
        for exits, tail in ((False, ""), (True, "+exits")):
            legs.append(("track" + tail, *leg(env, 0, exits)))
            legs += [(f"list{c}{tail}", *leg(env, c, exits)) for c in CAPACITIES]
            if parent is not None:
                legs.append(("parent track" + tail, *leg(parent, None, exits)))
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
        env.track_trades(list_capacity=CAPACITIES[0])
        env.bind_exits(d_rules)
        stats = env.backtest_signals(K)
        board = stats.trade_stats.by_strategy()
        index, _ = board.top(64, "profit_factor")
        reads = []
        for _ in range(3):
            env.synchronize()
            t0 = time.perf_counter()
            lists = stats.trade_stats.trades(strategy=index)
            reads.append(time.perf_counter() - t0)
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        results[shape] = dict(envs=N, K=K, reps=a.reps, rules=R, strategies=64, us_per_step=med,
                              us_per_step_min={n: min(t) for n, t in times.items()},
                              us_per_step_max={n: max(t) for n, t in times.items()},
                              closed_last_call=int(stats.trade_stats.closed.sum().item()),
                              read=dict(strategies=int(len(index)), envs=int(len(lists.env_ids)), trades=len(lists),
                                        truncated=int(lists.truncated.sum()), capacity=CAPACITIES[0],
                                        seconds=sorted(reads)[1], seconds_min=min(reads), seconds_max=max(reads)))
        for n, _, _ in legs:
            print(f"{shape} {N:6d} envs K={K}  {n:19s} {med[n]:8.3f} us/step  (min {min(times[n]):.3f}, "
                  f"max {max(times[n]):.3f}, {a.reps} interleaved passes)", flush=True)
        for tail in ("", "+exits"):
            print(f"{shape} {N:6d} envs K={K}  " + "   ".join(
                f"list{c}{tail} / track{tail} {med[f'list{c}{tail}'] / med['track' + tail]:.3f}" for c in CAPACITIES),
                flush=True)
        r = results[shape]["read"]
        print(f"{shape} {N:6d} envs  trades(strategy=top {r['strategies']}): {r['trades']} trades of {r['envs']} envs "
              f"({r['truncated']} lists truncated at {r['capacity']}) in {r['seconds'] * 1e3:.2f} ms "
              f"(min {r['seconds_min'] * 1e3:.2f}, max {r['seconds_max'] * 1e3:.2f}, 3 reads)", flush=True)
        env.close()
        if parent is not None:
            parent.close()
    print(json.dumps({"trade_list_bench": dict(library=os.path.basename(_abi.LIB_PATH),
                                               parent=os.path.basename(a.parent) if a.parent else None,
                                               shapes=results)}))


if __name__ == "__main__":
    main()
