#!/usr/bin/env python3
"""What a trade Monte Carlo costs on the device (gte_trade_monte_carlo, csrc/gte_montecarlo.hip): the whole call — the
walk launch and the close launch — at Q = 10, 256 and 4 096 pools, R = 1 000 resamples, pools of 100, 1 000,
GTE_MC_LDS_POOL and 4 x GTE_MC_LDS_POOL trade factors, paths of min(P, 1 000) trades, with the `final` and
`max_drawdown` columns kept; against the same computation in torch in the same process:

  library  gte_trade_monte_carlo.  A pool of at most GTE_MC_LDS_POOL factors is staged into LDS and the walk reads
           LDS; a larger one is read in place.  The two largest pool sizes sit on either side of that threshold.
  torch    `torch.randint` indices [q, R, L], a gather out of the pools, `cumprod` along the path, `cummax` for the
           running peak, and the reductions: final, maximum drawdown, lowest equity, their sums and squares, the counts
           of losses, ruins and drawdown levels.  (No losing streak: torch has no scan for it.)  [q, R, L] tensors do not
           fit for many pools, so torch takes the pools in chunks of at most --chunk elements; its peak of temporaries
           is what torch's allocator reports above what was live before.

One process, one small env; the legs are interleaved pass by pass; every leg is timed with device events on the env's
stream (torch's), `--inner` calls per timing window.  Per leg: median and min-max over the passes, per call, and walk
steps (Q x R x L) per second.  Before anything is timed the two sides are compared: they draw different random
numbers, so what is compared is the mean maximum drawdown over all paths, within six standard errors.  No ratio is
promised: the numbers are printed as they come out, sizes where torch is faster included.

    python tools/trade_mc_bench.py [--reps 5] [--inner 2] [--chunk 67108864]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

POOLS = (10, 256, 4096)
R = 1000
MAX_LEN = 1000
RUIN = 0.5
LEVELS = (0.1, 0.2, 0.3, 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=1 << 26, help="most [q, R, L] elements of a torch chunk")
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi
    from gym_trading_env_amd.batched import BatchedTradingEnv
    if not torch.cuda.is_available():
        sys.exit("trade_mc_bench needs the GPU: nothing here can be timed without it")
    feat, close = bench.synthetic_dataset(0, 2000, 2)
    env = BatchedTradingEnv((feat, close), num_envs=64, positions=[-1, 0, 1], windows=None, seed=1, output="torch")
    lib, h, dev = env._lib, env._h, env._t["obs"].device
    f64t, i32t = torch.float64, torch.int32
    sizes = (100, 1000, _abi.GTE_MC_LDS_POOL, 4 * _abi.GTE_MC_LDS_POOL)
    host_levels = (C.c_double * len(LEVELS))(*LEVELS)
    levels_t = torch.tensor(LEVELS, dtype=f64t, device=dev)
    results = []
    for Q in POOLS:
        for P in sizes:
            L = min(P, MAX_LEN)
            rng = np.random.default_rng(Q + P)
            pools = torch.from_numpy(np.exp(rng.normal(2e-4, 0.02, (Q, P)))).to(dev)    # [Q, P]: trades of about 2 %
            first = torch.arange(Q + 1, dtype=torch.int64, device=dev) * P
            out = dict(final=torch.empty((Q * R,), dtype=f64t, device=dev),
                       max_drawdown=torch.empty((Q * R,), dtype=f64t, device=dev),
                       pool=torch.empty((Q * 48,), dtype=torch.uint8, device=dev),
                       dd_count=torch.empty((Q * len(LEVELS),), dtype=i32t, device=dev))
            ptrs = _abi.GteMcOut(**{name: v.data_ptr() for name, v in out.items()})
            qc = max(1, min(Q, a.chunk // (R * L)))
            torch.cuda.synchronize()

            def library():
                _abi.check(lib, lib.gte_trade_monte_carlo(h, C.c_void_p(pools.data_ptr()), C.c_void_p(first.data_ptr()),
                                                          None, Q, R, L, 12345, RUIN, host_levels, len(LEVELS),
                                                          C.byref(ptrs)))

            def with_torch():
                final = torch.empty((Q, R), dtype=f64t, device=dev)
                mdd = torch.empty((Q, R), dtype=f64t, device=dev)
                low = torch.empty((Q, R), dtype=f64t, device=dev)
                for q0 in range(0, Q, qc):
                    q1 = min(q0 + qc, Q)
                    idx = torch.randint(0, P, (q1 - q0, R, L), device=dev)
                    f = torch.gather(pools[q0:q1].unsqueeze(1).expand(q1 - q0, R, P), 2, idx)
                    e = torch.cumprod(f, dim=2)
                    peak = torch.cummax(e, dim=2).values.clamp(min=1.0)
                    final[q0:q1] = e[:, :, -1]
                    mdd[q0:q1] = (1.0 - e / peak).amax(dim=2).clamp(min=0.0)
                    low[q0:q1] = e.amin(dim=2).clamp(max=1.0)
                sums = (final.sum(1), (final * final).sum(1), mdd.sum(1), (mdd * mdd).sum(1))
                counts = ((final < 1.0).sum(1), (low <= RUIN).sum(1), (mdd.unsqueeze(2) >= levels_t).sum(1))
                return final, mdd, sums, counts

            res = dict(Q=Q, P=P, L=L, R=R, staged_in_lds=P <= _abi.GTE_MC_LDS_POOL, steps=Q * R * L, reps=a.reps,
                       inner=a.inner, torch_chunk_pools=qc, us={}, us_min={}, us_max={})
            # the two sides say the same, as far as two random streams can
            library()
            env.synchronize()
            _, mdd, _, _ = with_torch()
            torch.cuda.synchronize()
            rec = out["pool"].cpu().numpy().view(np.dtype(_abi.MC_POOL_DTYPE))
            n = Q * R
            lib_mean = float(rec["mdd_sum"].sum()) / n
            lib_sd = float(np.sqrt(max(float(rec["mdd_sq_sum"].sum()) / n - lib_mean ** 2, 0.0)))
            torch_mean = float(mdd.mean())
            res["mean_max_drawdown"] = dict(library=lib_mean, torch=torch_mean, standard_error=lib_sd / np.sqrt(n))
            assert abs(lib_mean - torch_mean) <= 6.0 * lib_sd * np.sqrt(2.0 / n) + 1e-12, (Q, P, lib_mean, torch_mean)
            del mdd
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            live_bytes = torch.cuda.memory_allocated(dev)
            with_torch()
            torch.cuda.synchronize()
            res["torch_peak_temporary_bytes"] = int(torch.cuda.max_memory_allocated(dev) - live_bytes)
            legs = (("library", library), ("torch", with_torch))
            times = {name: [] for name, _ in legs}
            for rep in range(a.reps + 1):   # pass 0 is the warm-up: allocations, code objects
                for name, f in legs:
                    env.timer_start()
                    for _ in range(a.inner):
                        f()
                    t = env.timer_stop() * 1e3 / a.inner
                    if rep:
                        times[name].append(t)
            for name, _ in legs:
                t = times[name]
                res["us"][name], res["us_min"][name], res["us_max"][name] = sorted(t)[len(t) // 2], min(t), max(t)
            res["library_steps_per_s"] = res["steps"] / (res["us"]["library"] * 1e-6)
            print(f"Q={Q:5d} P={P:6d} L={L:5d} {'LDS' if res['staged_in_lds'] else 'L2 ':3s}  library "
                  f"{res['us']['library']:11.1f} us (min {res['us_min']['library']:.1f}, max {res['us_max']['library']:.1f}), "
                  f"{res['library_steps_per_s'] / 1e9:7.2f} G steps/s;  torch {res['us']['torch']:12.1f} us (min "
                  f"{res['us_min']['torch']:.1f}, max {res['us_max']['torch']:.1f}), chunks of {qc} pools, peak temporaries "
                  f"{res['torch_peak_temporary_bytes'] / 2 ** 20:8.1f} MiB;  torch / library = "
                  f"{res['us']['torch'] / res['us']['library']:.2f};  mean max drawdown {lib_mean:.5f} / {torch_mean:.5f}",
                  flush=True)
            results.append(res)
            del pools, first, out
            torch.cuda.empty_cache()
    env.close()
    print(json.dumps({"trade_mc_bench": results}))


if __name__ == "__main__":
    main()
