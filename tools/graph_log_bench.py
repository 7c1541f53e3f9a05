#!/usr/bin/env python3
"""Logged envs and Python callables: eager steps against the same steps replayed as a HIP graph
(`capture_steps`, 64 steps per graph), alternated round by round in one process; and the eager
logged step of two BUILDS of libgte, alternated the same way.

    python3 tools/graph_log_bench.py callables [envs ...]        (default 65536 4096)
    python3 tools/graph_log_bench.py ab libA.so libB.so [envs]   (eager step, log_steps=2)

Config-3 shape (window 20 x 32 features), episodes out of phase; us per step, 3 rounds."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

K = 64  # steps per graph
ROUNDS, REPLAYS = 3, 4


def reward_function(history):  # the reference's vectorised example (examples/example_vectorized_environment.py)
    return np.log(history["portfolio_valuation", -1] / history["portfolio_valuation", -2])


def dyn_last_position(history):
    return history["position", -1]


def dyn_real_position(history):
    return history["real_position", -1]


def _env(envs, library_path=None, **kw):
    from gym_trading_env_amd.batched import BatchedTradingEnv
    wl = dict(bench.WORKLOADS["c3"], envs=envs)
    feat, close = bench.synthetic_dataset(0, wl["T"], wl["n_static"])
    k = dict(bench.env_kwargs(wl))
    k.update(kw)
    return BatchedTradingEnv((feat, close), num_envs=envs, seed=1, output="torch", verbose=0,
                             library_path=library_path, **k), wl


def callables(sizes):
    import torch
    cases = [("Python reward_function", dict(reward_function=reward_function)),
             ("Python reward + 2 Python dynamic features",
              dict(reward_function=reward_function,
                   dynamic_feature_functions=[dyn_last_position, dyn_real_position]))]
    for envs in sizes:
        for name, kw in cases:
            env, wl = _env(envs, **kw)
            acts = torch.randint(0, 3, (K, envs), dtype=torch.int32, device="cuda")
            env.reset()
            bench.desynchronise(env, acts, wl["max_episode_duration"])
            g = env.capture_steps(lambda i: env.step(acts[i]), K)
            eager, graph = [], []
            for r in range(ROUNDS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(REPLAYS):
                    for i in range(K):
                        env.step(acts[i])
                torch.cuda.synchronize()
                eager.append((time.perf_counter() - t0) / (REPLAYS * K) * 1e6)
                t0 = time.perf_counter()
                for _ in range(REPLAYS):
                    g.replay()
                torch.cuda.synchronize()
                graph.append((time.perf_counter() - t0) / (REPLAYS * K) * 1e6)
            print(f"{envs:6d} envs  {name:42s} eager " + " ".join(f"{x:7.2f}" for x in eager) +
                  "   graph " + " ".join(f"{x:7.2f}" for x in graph) + "  us/step", flush=True)
            del g
            env.close()


def ab(libs, envs):
    """The eager logged step (kernel-written row, log_steps=2) of several builds; a build with an
    older ABI version is created with that version in its config (gte_config is unchanged)."""
    import torch
    from gym_trading_env_amd import _abi
    full, version = dict(_abi.SYMBOLS), _abi.GTE_ABI_VERSION
    runs = []
    for p in libs:
        have = C.CDLL(p)
        _abi.SYMBOLS = {k: v for k, v in full.items() if hasattr(have, k)}
        _abi.GTE_ABI_VERSION = have.gte_abi_version()
        _abi._lib = None
        env, wl = _env(envs, library_path=p, log_steps=2)
        acts = torch.randint(0, 3, (K, envs), dtype=torch.int32, device="cuda")
        env.reset()
        bench.desynchronise(env, acts, wl["max_episode_duration"])
        runs.append((p, env, acts, []))
    _abi.SYMBOLS, _abi.GTE_ABI_VERSION, _abi._lib = full, version, None
    for r in range(ROUNDS):
        for p, env, acts, ts in runs:
            for i in range(50):
                env.step(acts[i % K])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(400):
                env.step(acts[i % K])
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / 400 * 1e6)
    for p, env, acts, ts in runs:
        print(f"{envs:6d} envs  eager logged step  {os.path.basename(p):24s} " +
              " ".join(f"{x:7.2f}" for x in ts) + "  us/step", flush=True)
        env.close()


if __name__ == "__main__":
    if sys.argv[1] == "callables":
        callables([int(x) for x in sys.argv[2:]] or [65536, 4096])
    elif sys.argv[1] == "ab":
        libs = [os.path.abspath(p) for p in sys.argv[2:4]]
        ab(libs, int(sys.argv[4]) if len(sys.argv) > 4 else 65536)
    else:
        raise SystemExit(__doc__)
