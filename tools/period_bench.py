#!/usr/bin/env python3
"""What period tracking costs, us per step of the whole batch: backtest_signals(K), S = 64, with
`track_periods` off, on with B = 4 and on with B = 64 (equal blocks of the market rows), each without and with
256 exit rules bound, at 65 536 envs on bench.py's c3 shape and at 4 096 on its c2 shape:

  off / on                gte_backtest_signal_kernel  /  gte_period_signal_kernel
  off+exits / on+exits    gte_backtest_exit_kernel    /  gte_period_exit_kernel

The comparison is on against off in the same run.  With --parent LIB (a build of libgte from the parent commit)
the two off legs are also run through that library in the same process, on a second env of the same seed
(tools/lib_ab.py's way): they launch the same kernels, so they should tie within the spread of the passes.

One process; episodes out of phase (bench.desynchronise); the legs are interleaved pass by pass and timed with
device events on the env's stream; every leg is preceded by its switches (tracking, rules) and one untimed call
of itself, which also takes the clearing a switch of tracking asks for.  The spread of a leg is its min .. max
over the passes.  Beside B = 64: how many periods an env touched in one more call — every entry is a store and
a dependent load of 32 bytes — and the share of the rows that start a block.

Then the fold: the 65 536 x 64 records into 4 096 x 64 (`period_stats.by_strategy(n_strategies=4096)`, device
events on the env's stream around the call) against the torch formulation over the same records,
`reshape(R, S, B).sum(0)` per field (device events on torch's stream), and its bytes over its time against the
HBM peak.

    python tools/period_bench.py [--k 512] [--reps 9] [--parent libgte_parent.so]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from trade_bench import make_env  # noqa: E402

SHAPES = (("c3", 65_536), ("c2", 4_096))
HBM_PEAK = 8.0e12  # bytes / s, MI355X data sheet


def fold_bench(torch, env, stats, reps):
    """-> dict: the device fold and the torch formulation over the env's own [N, 64] records, us"""
    per = stats.period_stats
    N, B, S = env.num_envs, per.num_periods, 4096
    R = N // S
    fields = [getattr(per, f) for f in per.FIELDS]

    def by_torch():
        return [f.reshape(R, S, B).sum(0) for f in fields]

    def torch_us(f):
        out = []
        for rep in range(reps + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            env.synchronize()
            torch.cuda.synchronize()
            t0.record()
            keep = f()
            t1.record()
            torch.cuda.synchronize()
            if rep:
                out.append(t0.elapsed_time(t1) * 1e3)
            del keep
        return sorted(out)

    def library_us(f):
        out = []
        for rep in range(reps + 1):
            torch.cuda.synchronize()
            env.timer_start()   # (device events on the env's stream, where the library's launch runs)
            keep = f()
            t = env.timer_stop() * 1e3
            if rep:
                out.append(t)
            del keep
        return sorted(out)

    lib = library_us(lambda: per.by_strategy(n_strategies=S))
    tor = torch_us(by_torch)
    board = per.by_strategy(n_strategies=S)
    same = all(bool((getattr(board, f) == t).all()) for f, t in zip(per.FIELDS, by_torch()) if f in ("steps", "trades", "episodes"))
    moved = N * B * 32 + S * B * 48
    return dict(envs=N, periods=B, strategies=S, bytes=moved, library_us=lib[len(lib) // 2], library_us_min=lib[0],
                library_us_max=lib[-1], torch_us=tor[len(tor) // 2], torch_us_min=tor[0], torch_us_max=tor[-1],
                library_bytes_per_s=moved / (lib[len(lib) // 2] * 1e-6), hbm_peak=HBM_PEAK, counters_equal_torch=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent", default=None, help="libgte.so built from the parent commit: its off legs as well")
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi, periods, signals
    if not torch.cuda.is_available():
        sys.exit("period_bench needs the GPU: nothing here can be timed without it")
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
        rows = {B: periods.blocks(wl["T"], B) for B in (4, 64)}

        def leg(e, B, exits):
            def before():
                if B is not None:
                    e.track_periods(rows[B] if B else None, B or None)
                e.bind_exits(d_rules if exits else None)
                e.backtest_signals(K)
            return before, lambda: e.backtest_signals(K)

        legs = [("off", *leg(env, 0, False)), ("on B=4", *leg(env, 4, False)), ("on B=64", *leg(env, 64, False)),
                ("off+exits", *leg(env, 0, True)), ("on B=4+exits", *leg(env, 4, True)),
                ("on B=64+exits", *leg(env, 64, True))]
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
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        # how often a step crosses a block edge: the share of the rows whose id differs from the row before
        # (envs are spread over the rows); the records of one more call say how many periods an env entered
        change_rate = {B: float((rows[B][1:] != rows[B][:-1]).mean()) for B in rows}
        env.bind_exits(None)
        env.track_periods(rows[64], 64)
        stats = env.backtest_signals(K)
        per = stats.period_stats
        touched = float((per.steps > 0).sum(dim=1).double().mean().item())
        results[shape] = dict(envs=N, K=K, reps=a.reps, rules=R, strategies=64, us_per_step=med,
                              us_per_step_min={n: min(t) for n, t in times.items()},
                              us_per_step_max={n: max(t) for n, t in times.items()},
                              transitions_last_call=int(stats.steps.sum().item()),
                              counted_last_call=int(per.steps.sum().item()),
                              periods_touched_per_env_last_call=touched, map_changes_per_row=change_rate)
        for n, _, _ in legs:
            print(f"{shape} {N:6d} envs K={K}  {n:17s} {med[n]:8.3f} us/step  (min {min(times[n]):.3f}, "
                  f"max {max(times[n]):.3f}, {a.reps} interleaved passes)", flush=True)
        print(f"{shape} {N:6d} envs K={K}  on / off: B=4 {med['on B=4'] / med['off']:.3f}, B=64 {med['on B=64'] / med['off']:.3f}"
              f"   with exits: B=4 {med['on B=4+exits'] / med['off+exits']:.3f}, B=64 {med['on B=64+exits'] / med['off+exits']:.3f}"
              f"   (B=64, last call: {touched:.2f} periods touched per env in {K} steps — every entry a store and a "
              f"dependent load; an episode's reset lands in another period more often than a row crosses a block "
              f"edge: {change_rate[64]:.5f} of the rows start a block)", flush=True)
        if shape == "c3":
            fb = fold_bench(torch, env, stats, a.reps)
            results["fold"] = fb
            print(f"fold {fb['envs']} x {fb['periods']} -> {fb['strategies']} x {fb['periods']}: library "
                  f"{fb['library_us']:.1f} us (min {fb['library_us_min']:.1f}, max {fb['library_us_max']:.1f}), "
                  f"{fb['bytes'] / 1e6:.1f} MB -> {fb['library_bytes_per_s'] / 1e12:.2f} TB/s, "
                  f"{100 * fb['library_bytes_per_s'] / HBM_PEAK:.0f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak; "
                  f"torch reshape(R, S, B).sum(0) per field {fb['torch_us']:.1f} us (min {fb['torch_us_min']:.1f}, "
                  f"max {fb['torch_us_max']:.1f}); counters equal: {fb['counters_equal_torch']}", flush=True)
        env.close()
        if parent is not None:
            parent.close()
    print(json.dumps({"period_bench": dict(library=os.path.basename(_abi.LIB_PATH),
                                           parent=os.path.basename(a.parent) if a.parent else None, shapes=results)}))


if __name__ == "__main__":
    main()
