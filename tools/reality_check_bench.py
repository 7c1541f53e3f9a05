#!/usr/bin/env python3
"""What the bootstrap reality check costs on the device (gte_bootstrap_weights, gte_reality_check,
csrc/gte_bootstrap.hip) at the size of a large sweep, S = 65 536 strategies, n = B = 64 periods, R = 1 000
resamples, and at S = 4 096, against the formulation a user would write with torch in the same process:

  weights   gte_bootstrap_weights: the [R, n] table, one launch;
  check     gte_reality_check: gather, resample pass, the three closing launches — five launches;
  torch     `C = (W @ D) / n - mean` in f64 ([R, S], rocBLAS), `C.max(0)` for the maxima and their indices,
            `C.sum`, `(C * C).sum`, `(C >= mean).sum` for the moments, and the adjusted counts from the sorted maxima;
            its peak temporary memory is what torch's allocator reports above what was live before.

One process, one small env; the legs are interleaved pass by pass; every leg is timed with device events on the env's
stream (torch's), `--inner` calls per timing window.  Per leg: median and min-max over the passes, per call.  The
resample pass does 2 * R * S * n f64 operations (one multiply, one add per weight and strategy): "f64 rate" is that
count over the whole check's time — an end-to-end figure, not the kernel's.  Before anything is timed the two
formulations are held equal within the rounding of a 64-term f64 sum.  No ratio is promised: the library path is
kept for its fixed bits and for never making the [R, S] matrix; where rocBLAS is faster this says so.

    python tools/reality_check_bench.py [--reps 9] [--inner 10]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

SHAPES = ((65_536, 64, 1000), (4_096, 64, 1000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi
    from gym_trading_env_amd.batched import BatchedTradingEnv
    if not torch.cuda.is_available():
        sys.exit("reality_check_bench needs the GPU: nothing here can be timed without it")
    feat, close = bench.synthetic_dataset(0, 2000, 2)
    env = BatchedTradingEnv((feat, close), num_envs=64, positions=[-1, 0, 1], windows=None, seed=1, output="torch")
    lib, h, dev = env._lib, env._h, env._t["obs"].device
    dt = np.dtype(_abi.STRATEGY_PERIOD_DTYPE)
    results = []
    for S, B, R in SHAPES:
        n = B
        rng = np.random.default_rng(S)
        host = np.zeros((S, B), dtype=dt)
        host["reward_sum"] = rng.normal(0, 1e-2, (S, B))
        host["steps"] = 100
        rec = torch.from_numpy(host.view(np.uint8).reshape(S * B, 48).copy()).to(dev)
        x = torch.from_numpy(np.ascontiguousarray(host["reward_sum"])).to(dev)            # [S, B] for torch
        benchmark = torch.from_numpy(rng.normal(0, 1e-2, B)).to(dev)
        w = torch.empty((R, n), dtype=torch.float64, device=dev)
        f64 = lambda k: torch.empty((k,), dtype=torch.float64, device=dev)
        i32 = lambda k: torch.empty((k,), dtype=torch.int32, device=dev)
        out = dict(mean=f64(S), boot_sum=f64(S), boot_sq_sum=f64(S), count_ge=i32(S), count_adj=i32(S), max_stat=f64(R),
                   max_index=i32(R), summary=torch.empty((24,), dtype=torch.uint8, device=dev))
        ptrs = _abi.GteRealityCheckOut(**{k: v.data_ptr() for k, v in out.items()})
        words = (C.c_uint64 * 2)(2 ** 64 - 1 if B >= 64 else (1 << B) - 1, 0)
        torch.cuda.synchronize()

        def weights():
            _abi.check(lib, lib.gte_bootstrap_weights(h, n, R, 2.0, 7, C.c_void_p(w.data_ptr())))

        def check():
            _abi.check(lib, lib.gte_reality_check(h, C.c_void_p(rec.data_ptr()), S, B, words,
                                                  C.c_void_p(benchmark.data_ptr()), C.c_void_p(w.data_ptr()), R,
                                                  C.byref(ptrs)))

        def with_torch():
            d = (x - benchmark).t().contiguous()            # [n, S]
            mean = d.sum(0) / n
            c = (w @ d) / n - mean                          # [R, S]
            top = c.max(1)
            moments = c.sum(0), (c * c).sum(0), (c >= mean).sum(0)
            adj = R - torch.searchsorted(top.values.sort().values, mean, right=False)
            return mean, top.values, top.indices, moments, adj

        weights()
        check()
        env.synchronize()
        mean, top, top_index, moments, adj = with_torch()
        torch.cuda.synchronize()
        scale = float(x.abs().max()) * 4                    # |w d| sums to at most n * this per resample, / n
        tol = 64 * 2.0 ** -52 * scale * 4
        assert float((out["mean"] - mean).abs().max()) <= tol
        assert float((out["max_stat"] - top).abs().max()) <= tol
        assert float((out["boot_sum"] - moments[0]).abs().max()) <= R * tol
        assert float((out["max_index"] != top_index).sum()) <= 2 and int((out["count_adj"] - adj).abs().max()) <= 2
        del mean, top, top_index, moments, adj
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        live = torch.cuda.memory_allocated(dev)
        with_torch()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - live

        legs = [("weights", weights), ("check", check), ("torch", with_torch)]
        times = {name: [] for name, _ in legs}
        for rep in range(a.reps + 1):   # pass 0 is the warm-up: allocations, code objects, rocBLAS's choice
            for name, f in legs:
                env.timer_start()
                for _ in range(a.inner):
                    f()
                t = env.timer_stop() * 1e3 / a.inner
                if rep:
                    times[name].append(t)
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
        ops = 2.0 * R * S * n
        res = dict(S=S, n=n, B=B, R=R, reps=a.reps, inner=a.inner, us=med, us_min={k: min(t) for k, t in times.items()},
                   us_max={k: max(t) for k, t in times.items()}, f64_ops=ops,
                   check_f64_rate_tflops=round(ops / (med["check"] * 1e-6) / 1e12, 3),
                   torch_over_check=round(med["torch"] / med["check"], 3), torch_peak_temporary_bytes=int(peak),
                   matrix_bytes=8 * R * S)
        for name, _ in legs:
            print(f"S={S} n={n} R={R}  {name:8s} {med[name]:10.1f} us per call  (min {min(times[name]):.1f}, max "
                  f"{max(times[name]):.1f}, {a.reps} interleaved passes of {a.inner} calls, device events)", flush=True)
        print(f"S={S} n={n} R={R}  check: {ops:.3g} f64 operations, {res['check_f64_rate_tflops']} Top/s end to end; "
              f"torch / check = {res['torch_over_check']}; torch's peak temporary memory {peak / 2 ** 20:.1f} MiB "
              f"(the [R, S] matrix alone is {8 * R * S / 2 ** 20:.1f} MiB), the library's scratch holds no [R, S] array",
              flush=True)
        results.append(res)
        del rec, x, w, out
        torch.cuda.empty_cache()
    env.close()
    print(json.dumps({"reality_check_bench": results}))


if __name__ == "__main__":
    main()
