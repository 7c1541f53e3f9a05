#!/usr/bin/env python3
"""The nine from-registers backtest kernels (csrc/gte_summary_body.h: three action sources x three trackers) of
this build against a libgte built from another commit, us per step of the whole batch, at 65 536 envs on
bench.py's c3 shape:

  source    actions: backtest(actions [K, N])    signal: backtest_signals(K), S = 64    exit: ... with 256 rules bound
  tracker   none / track_trades / track_periods (B = 64, equal blocks of the market rows)

One process, both libraries loaded, one env of the same seed on each (tools/trade_bench.py's make_env); for each
kernel the legs of the two builds are interleaved pass by pass and timed with device events on the env's stream;
every leg is preceded by its switches (tracking, rules) and one untimed call of itself, which also takes the
clearing a switch of tracking asks for.  The spread of a leg is its min .. max over the passes; `within` says
whether this build's median exceeds the parent's by no more than the parent leg's own spread.

    python tools/summary_body_bench.py --parent libgte_parent.so [--k 512] [--reps 9] [--parent-first]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from trade_bench import make_env  # noqa: E402

SHAPE, N, B = "c3", 65_536, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent", required=True, help="libgte.so built from the commit to compare against")
    ap.add_argument("--parent-first", action="store_true", help="create the parent's env first and run its leg first")
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi, periods, signals
    if not torch.cuda.is_available():
        sys.exit("summary_body_bench needs the GPU: nothing here can be timed without it")
    K, R = a.k, 256
    rng = np.random.default_rng(0)
    rules = signals.exit_rules(stop_loss=rng.uniform(0.002, 0.02, R), take_profit=rng.uniform(0.004, 0.04, R),
                               trailing=rng.uniform(0.002, 0.02, R), max_hold=rng.integers(8, 96, R), exit_position=1)
    d_rules = torch.from_numpy(rules.view(np.uint8).reshape(R, 32).copy()).cuda()
    wl = bench.WORKLOADS[SHAPE]
    # (which env is created first decides where its buffers land and which leg of a pass runs first: --parent-first
    # is the control for that, as is a --parent that is a copy of this build)
    order = ("parent", "new") if a.parent_first else ("new", "parent")
    envs = {b: make_env(torch, wl, N, K, os.path.abspath(a.parent) if b == "parent" else None) for b in order}
    rows = periods.blocks(wl["T"], B)
    torch.manual_seed(1)
    acts = torch.randint(0, len(envs["new"].positions), (K, N), dtype=torch.int32, device="cuda")

    def leg(e, source, tracker):
        run = (lambda: e.backtest(acts)) if source == "actions" else (lambda: e.backtest_signals(K))

        def before():  # (the two trackers are never on together: the other one goes first)
            if tracker != "trades":
                e.track_trades(False)
            e.track_periods(rows if tracker == "periods" else None, B if tracker == "periods" else None)
            if tracker == "trades":
                e.track_trades(True)
            e.bind_exits(d_rules if source == "exit" else None)
            run()
        return before, run

    results = {}
    for tracker in ("none", "trades", "periods"):
        for source in ("actions", "signal", "exit"):
            legs = {build: leg(e, source, tracker) for build, e in envs.items()}
            times = {build: [] for build in legs}
            for rep in range(a.reps + 1):  # pass 0 is the warm-up: allocations, code objects, geometry choices
                for build, (before, run) in legs.items():
                    before()
                    envs[build].timer_start()
                    run()
                    t = envs[build].timer_stop() * 1e3 / K
                    if rep:
                        times[build].append(t)
            med = {b: sorted(t)[len(t) // 2] for b, t in times.items()}
            spread = max(times["parent"]) - min(times["parent"])
            within = med["new"] <= med["parent"] + spread
            results[f"{source}/{tracker}"] = dict(us_per_step=med, us_per_step_min={b: min(t) for b, t in times.items()},
                                                  us_per_step_max={b: max(t) for b, t in times.items()},
                                                  parent_spread=spread, within=within)
            for b in ("parent", "new"):
                print(f"{SHAPE} {N} envs K={K}  {source:7s} x {tracker:7s} {b:6s} {med[b]:8.3f} us/step  "
                      f"(min {min(times[b]):.3f}, max {max(times[b]):.3f}, {a.reps} interleaved passes)", flush=True)
            print(f"{SHAPE} {N} envs K={K}  {source:7s} x {tracker:7s} new - parent {med['new'] - med['parent']:+.3f}, "
                  f"parent spread {spread:.3f}: {'within' if within else 'OUTSIDE'}", flush=True)
    for e in envs.values():
        e.close()
    print(json.dumps({"summary_body_bench": dict(library=os.path.basename(_abi.LIB_PATH),
                                                 parent=os.path.basename(a.parent), first=order[0], shape=SHAPE, envs=N, K=K,
                                                 reps=a.reps, periods=B, kernels=results)}))


if __name__ == "__main__":
    main()
