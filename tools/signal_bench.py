#!/usr/bin/env python3
"""What looking the action up on the device costs, us per step of the whole batch:

  (a) actions     backtest(acts) with the [K, N] int32 actions materialised from the same tables:
                  the way to run signals before backtest_signals, and the yardstick;
  (b) signals     backtest_signals(K), default strategy, S = N: every env its own row of the table;
  (c) signals64   the same with S = 64: a table that stays in L2;
  (d) per-step    signal_actions() + step() for each of the K steps, for scale.

One process, one env per shape; episodes out of phase (bench.desynchronise); the legs are
interleaved pass by pass and timed with device events on the env's stream.  Every leg continues
from the state the previous one left: all of them advance the env K steps.  The actions of leg (a)
are those the tables gave on the first K steps after the prologue; the timed passes run them from
other rows, which changes what is traded and not what is computed.

    python tools/signal_bench.py [--k 512] [--reps 9] [--shapes c3 c2]

GTE_LIBRARY=<another build of libgte.so> times that build.  (At commit 5644e99 the fused kernel had a
byte-per-step variant behind a macro, built with `make libgte_exp.so EXP=-DGTE_SIGNAL_BYTE_LOAD=1` and timed
this way; the A/B is finished, profiles/signal_bench.log keeps it, and the macro no longer exists.)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

SHAPES = (("c3", 65_536), ("c2", 4_096))


def random_table(torch, S, T):
    """int8 [S, T] on the device: runs of 8 rows (a signal holds for a while) of a position index or
    -1 (out of range: hold)."""
    runs = torch.randint(-1, 3, (S, (T + 7) // 8), dtype=torch.int8, device="cuda")
    return runs.repeat_interleave(8, dim=1)[:, :T].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", nargs="+", default=[s for s, _ in SHAPES])
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi
    from gym_trading_env_amd.batched import BatchedTradingEnv
    if not torch.cuda.is_available():
        sys.exit("signal_bench needs the GPU: nothing here can be timed without it")
    results = []
    for name, N in SHAPES:
        if name not in a.shapes:
            continue
        wl = bench.WORKLOADS[name]
        data = bench.synthetic_dataset(0, wl["T"], wl["n_static"])
        env = BatchedTradingEnv(data, num_envs=N, seed=1, output="torch", **bench.env_kwargs(wl))
        env.reset()
        K, T = a.k, wl["T"]
        torch.manual_seed(0)
        wide, narrow = random_table(torch, N, T), random_table(torch, 64, T)
        bench.desynchronise(env, torch.randint(0, 3, (K, N), dtype=torch.int32, device="cuda"),
                            wl["max_episode_duration"])
        env.bind_signals(wide)
        wide_bound = env._signals[0]
        del wide
        acts = torch.empty((K, N), dtype=torch.int32, device="cuda")
        for k in range(K):  # leg (a)'s actions: what the tables give, materialised
            env.step(env.signal_actions(out=acts[k]))

        def bind(buf):  # the padded tensor bind_signals made: rebinding it copies nothing
            _abi.check(env._lib, env._lib.gte_bind_signals(env._h, 0, buf.data_ptr(), int(buf.shape[0]),
                                                           int(buf.shape[1])))
        env.bind_signals(narrow)
        narrow_bound = env._signals[0]
        del narrow
        step_buf = torch.empty(N, dtype=torch.int32, device="cuda")

        def per_step():
            for _ in range(K):
                env.step(env.signal_actions(out=step_buf))

        # (name, what runs before the bracket, the timed call); binding waits for the stream
        legs = (("actions", None, lambda: env.backtest(acts)),
                ("signals", lambda: bind(wide_bound), lambda: env.backtest_signals(K)),
                ("signals64", lambda: bind(narrow_bound), lambda: env.backtest_signals(K)),
                ("per-step", None, per_step))
        times = {n: [] for n, _, _ in legs}
        for rep in range(a.reps + 1):  # pass 0 is the warm-up: allocations, code objects, geometry choices
            for n, before, f in legs:
                if before:
                    before()
                env.timer_start()
                f()
                t = env.timer_stop() * 1e3 / K
                if rep:
                    times[n].append(t)
        stats = env.backtest_signals(K)
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        res = dict(shape=name, envs=N, K=K, T=T, reps=a.reps, library=os.path.basename(_abi.LIB_PATH),
                   us_per_step=med, us_per_step_min={n: min(t) for n, t in times.items()},
                   us_per_step_max={n: max(t) for n, t in times.items()},
                   action_bytes_per_call=K * N * 4, table_bytes_wide=int(wide_bound.numel()),
                   table_bytes_narrow=int(narrow_bound.numel()),
                   transitions_last_call=int(stats.steps.sum().item()),
                   episodes_last_call=int(stats.episodes.sum().item()))
        results.append(res)
        for n, _, _ in legs:
            print(f"{name} {N:6d} envs K={K}  {n:9s} {med[n]:8.3f} us/step  (min {min(times[n]):.3f}, "
                  f"max {max(times[n]):.3f}, {a.reps} interleaved passes)", flush=True)
        env.close()
        del acts, wide_bound, narrow_bound
        torch.cuda.empty_cache()
    print(json.dumps({"signal_bench": results}))


if __name__ == "__main__":
    main()
