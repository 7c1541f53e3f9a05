#!/usr/bin/env python3
"""What exit rules cost, us per step of the whole batch, at 65 536 envs (bench.py's c3 shape):

  (a) signals64   backtest_signals(K), S = 64, no exit rules bound: the leg of the same name of
                  tools/signal_bench.py, and the yardstick;
  (b) exits       the same call with 256 exit rules bound (stop-loss + take-profit + trailing + time,
                  rule of env e = strategy % 256): gte_backtest_exit_kernel;
  (a') signals64-first   leg (a) timed back to back at the start of the process, before any exit rule is
                  bound: whether the interleaved (a) differs from it is a question of the states and the
                  launches around it, the kernel being the same;
  (c) torch-loop  what the feature replaces: for each of the K steps signal_actions(), a stop-loss /
                  take-profit formula in torch over the env's state tensors, step().

One process, one env; episodes out of phase (bench.desynchronise); the legs are interleaved pass by
pass and timed with device events on the env's stream; each fused leg is preceded by one untimed call
of itself (the host-bound torch loop leaves the device idle, and the launches after an idle stretch are
slower than the steady state).  Every leg continues from the state the previous one left.  The spread of a leg is its min .. max over the passes.

    python tools/exit_bench.py [--k 512] [--reps 9] [--loop-k 64]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from signal_bench import random_table  # noqa: E402

N = 65_536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-k", type=int, default=64, help="steps of the torch loop per pass (it is slow)")
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi, signals
    from gym_trading_env_amd.batched import BatchedTradingEnv
    if not torch.cuda.is_available():
        sys.exit("exit_bench needs the GPU: nothing here can be timed without it")
    wl = bench.WORKLOADS["c3"]
    data = bench.synthetic_dataset(0, wl["T"], wl["n_static"])
    env = BatchedTradingEnv(data, num_envs=N, seed=1, output="torch", **bench.env_kwargs(wl))
    env.reset()
    K, T, P = a.k, wl["T"], len(env.positions)
    torch.manual_seed(0)
    bench.desynchronise(env, torch.randint(0, P, (K, N), dtype=torch.int32, device="cuda"),
                        wl["max_episode_duration"])
    env.bind_signals(random_table(torch, 64, T))
    # leg (a) before any exit rule was bound and any exit leg ran: the same launches from the states the
    # plain backtest itself leaves (what tools/signal_bench.py times), back to back
    first = []
    for rep in range(a.reps + 1):
        env.timer_start()
        env.backtest_signals(K)
        t = env.timer_stop() * 1e3 / K
        if rep:
            first.append(t)
    rng = np.random.default_rng(0)
    R = 256
    rules = signals.exit_rules(stop_loss=rng.uniform(0.002, 0.02, R), take_profit=rng.uniform(0.004, 0.04, R),
                               trailing=rng.uniform(0.002, 0.02, R), max_hold=rng.integers(8, 96, R),
                               exit_position=1)
    d_rules = torch.from_numpy(rules.view(np.uint8).reshape(R, 32).copy()).cuda()
    exit_pos = 1  # flat
    stop = torch.from_numpy(rules["stop_loss"].astype(np.float64)).cuda()[torch.arange(N, device="cuda") % 64 % R]
    target = torch.from_numpy(rules["take_profit"].astype(np.float64)).cuda()[torch.arange(N, device="cuda") % 64 % R]
    entry = env.state_tensor("portfolio_valuation").clone()
    last_pos = env.state_tensor("position_index").clone()
    step_buf = torch.empty(N, dtype=torch.int32, device="cuda")

    def torch_loop():
        nonlocal entry, last_pos
        for _ in range(a.loop_k):
            act = env.signal_actions(out=step_buf)
            pv, pos = env.state_tensor("portfolio_valuation"), env.state_tensor("position_index")
            entry = torch.where(pos != last_pos, pv, entry)
            last_pos = pos.clone()
            leave = (pos != exit_pos) & ((pv <= entry * (1.0 - stop)) | (pv >= entry * (1.0 + target)))
            env.step(torch.where(leave, torch.full_like(act, exit_pos), act))

    def bind_rules(on):
        env.bind_exits(d_rules if on else None)

    def fused_after(on):
        """bind or unbind, then one untimed call: the torch loop before it leaves the device mostly idle, and
        the first launches after an idle stretch run slower than the steady state this leg is about"""
        bind_rules(on)
        env.backtest_signals(K)

    legs = (("signals64", lambda: fused_after(False), lambda: env.backtest_signals(K), K),
            ("exits", lambda: fused_after(True), lambda: env.backtest_signals(K), K),
            ("torch-loop", lambda: bind_rules(False), torch_loop, a.loop_k))
    times = {n: [] for n, _, _, _ in legs}
    times["signals64-first"] = first
    for rep in range(a.reps + 1):  # pass 0 is the warm-up: allocations, code objects, geometry choices
        for n, before, f, steps in legs:
            before()
            env.timer_start()
            f()
            t = env.timer_stop() * 1e3 / steps
            if rep:
                times[n].append(t)
    bind_rules(True)
    stats = env.backtest_signals(K)
    fired = env.exit_state().exits.sum(0).cpu().numpy()
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    res = dict(shape="c3", envs=N, K=K, loop_K=a.loop_k, T=T, reps=a.reps, rules=R, strategies=64,
               library=os.path.basename(_abi.LIB_PATH), us_per_step=med,
               us_per_step_min={n: min(t) for n, t in times.items()},
               us_per_step_max={n: max(t) for n, t in times.items()},
               transitions_last_call=int(stats.steps.sum().item()),
               exits_last_call=dict(zip(signals.EXIT_KINDS, (int(x) for x in fired))))
    for n in ["signals64-first"] + [n for n, _, _, _ in legs]:
        print(f"c3 {N:6d} envs K={K}  {n:15s} {med[n]:8.3f} us/step  (min {min(times[n]):.3f}, "
              f"max {max(times[n]):.3f}, {a.reps} interleaved passes)", flush=True)
    env.close()
    print(json.dumps({"exit_bench": res}))


if __name__ == "__main__":
    main()
