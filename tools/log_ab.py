import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench
import torch
from gym_trading_env_amd import _abi
from gym_trading_env_amd.batched import BatchedTradingEnv
for envs in (8192, 16384, 32768, 65536):
    wl = dict(bench.WORKLOADS["c3"], envs=envs)
    feat, close = bench.synthetic_dataset(0, wl["T"], wl["n_static"])
    acts = torch.randint(0, 3, (64, envs), dtype=torch.int32, device="cuda")
    for name, kw in (("kernel row", dict(log_steps=2)), ("separate launch", dict(log_steps=2, kernel_variant=_abi.KV_LOG_SEPARATE)),
                     ("kernel row, affinity off", dict(log_steps=2, affinity_period=-1)),
                     ("separate, affinity off", dict(log_steps=2, kernel_variant=_abi.KV_LOG_SEPARATE, affinity_period=-1))):
        k = dict(bench.env_kwargs(wl)); k.update(kw)
        env = BatchedTradingEnv((feat, close), num_envs=envs, seed=1, output="torch", **k)
        env.reset(); bench.desynchronise(env, acts, wl["max_episode_duration"])
        for i in range(100): env.step(acts[i % 64])
        torch.cuda.synchronize(); ts = []
        for rep in range(3):
            t0 = time.perf_counter()
            for i in range(300): env.step(acts[i % 64])
            torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) / 300 * 1e6)
        print(f"{envs:6d} envs  {name:28s} " + "  ".join(f"{x:7.2f}" for x in ts), flush=True)
        env.close()
