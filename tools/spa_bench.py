#!/usr/bin/env python3
"""What the test for superior predictive ability costs on the device (gte_spa_test, csrc/gte_spa.hip) at the size of
a large sweep, S = 65 536 strategies, n = B = 64 periods, R = 1 000 resamples, and at S = 4 096, next to the reality
check it contains and to the formulation a user would write with torch in the same process:

  check     gte_reality_check alone: five launches;
  spa1      gte_spa_test with max_rounds = 1: the reality check, then the pass with its three recentrings and the
            close of round 0 (by operation count about twice the reality check: the chain a = a + w * d is made again);
  spa2      ... with max_rounds = 2 on a board whose round 0 rejects: one further LIVE round (spa2 - spa1);
  spa10     ... with max_rounds = 10 on the same board, whose round 1 rejects nothing: eight IDLE rounds behind the
            done flag ((spa10 - spa2) / 8 each);
  torch     `Q = (W @ D) / n` in f64 chunk by chunk over the resamples (rocBLAS), `((Q - g_j) * rse).max(1)` for the
            three recentrings, `kthvalue` for the critical value of round 0 (no further round, no reality check);
            its peak temporary memory is what torch's allocator reports above what was live before.

One process, one small env; the legs are interleaved pass by pass; every leg is timed with device events on the env's
stream (torch's), `--inner` calls per timing window.  Per leg: median and min-max over the passes, per call.  Before
anything is timed the library's maxima are held equal to torch's within the rounding of a 64-term f64 sum.  No ratio is
promised: where torch is the faster side this says so.  The lines go to `--log` as well (profiles/spa_bench.log).

    python tools/spa_bench.py [--reps 7] [--inner 5] [--log profiles/spa_bench.log]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SHAPES = ((65_536, 64, 1000), (4_096, 64, 1000))
WINNERS = 8       # rows with a mean of 1.5 deviations per period: round 0 rejects them, round 1 nothing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "spa_bench.log"))
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi
    from gym_trading_env_amd.batched import BatchedTradingEnv
    if not torch.cuda.is_available():
        sys.exit("spa_bench needs the GPU: nothing here can be timed without it")
    log = open(a.log, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()
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
        host["reward_sum"][:WINNERS] += 1.5e-2
        host["steps"] = 100
        rec = torch.from_numpy(host.view(np.uint8).reshape(S * B, 48).copy()).to(dev)
        x = torch.from_numpy(np.ascontiguousarray(host["reward_sum"])).to(dev)            # [S, B] for torch
        w = torch.empty((R, n), dtype=torch.float64, device=dev)
        f64 = lambda k: torch.empty((k,), dtype=torch.float64, device=dev)
        i32 = lambda k: torch.empty((k,), dtype=torch.int32, device=dev)
        rc = dict(mean=f64(S), boot_sum=f64(S), boot_sq_sum=f64(S), count_ge=i32(S), count_adj=i32(S), max_stat=f64(R),
                  max_index=i32(R), summary=torch.empty((24,), dtype=torch.uint8, device=dev))
        out = dict(t_stat=f64(S), std_error=f64(S), recentred=torch.empty((S,), dtype=torch.uint8, device=dev),
                   count_adj=i32(S), rejected_round=i32(S), max_stat=f64(3 * R), max_index=i32(3 * R),
                   crit=f64(_abi.GTE_SPA_MAX_ROUNDS), round_rejected=i32(_abi.GTE_SPA_MAX_ROUNDS),
                   summary=torch.empty((40,), dtype=torch.uint8, device=dev))
        rc_ptrs = _abi.GteRealityCheckOut(**{k: v.data_ptr() for k, v in rc.items()})
        ptrs = _abi.GteSpaOut(**{k: v.data_ptr() for k, v in out.items()})
        words = (C.c_uint64 * 2)(2 ** 64 - 1 if B >= 64 else (1 << B) - 1, 0)
        thr, rank = math.sqrt(2.0 * math.log(math.log(n))), math.ceil(0.95 * R) - 1
        _abi.check(lib, lib.gte_bootstrap_weights(h, n, R, 2.0, 7, C.c_void_p(w.data_ptr())))
        torch.cuda.synchronize()

        def check():
            _abi.check(lib, lib.gte_reality_check(h, C.c_void_p(rec.data_ptr()), S, B, words, None,
                                                  C.c_void_p(w.data_ptr()), R, C.byref(rc_ptrs)))

        def spa(rounds):
            def call():
                _abi.check(lib, lib.gte_spa_test(h, C.c_void_p(rec.data_ptr()), S, B, words, None,
                                                 C.c_void_p(w.data_ptr()), R, thr, rank, rounds, C.byref(rc_ptrs),
                                                 C.byref(ptrs)))
            return call

        def with_torch(chunk=250):
            # (the mean and the deviation are the reality check's: this leg is the studentised pass alone)
            d = x.t().contiguous()                           # [n, S]
            mean, rse = rc["mean"], 1.0 / out["std_error"]
            t = mean * rse
            zero = torch.zeros_like(mean)
            g = (torch.where(mean > 0, mean, zero), torch.where(t >= -thr, mean, zero), mean)
            tops = [[], [], []]
            for r0 in range(0, R, chunk):
                q = (w[r0:r0 + chunk] @ d) / n               # [chunk, S]
                for j in range(3):
                    tops[j].append(((q - g[j]) * rse).max(1).values.clamp(min=0.0))
            M = torch.stack([torch.cat(tj) for tj in tops])
            return M, torch.kthvalue(M[1], rank + 1).values

        spa(10)()
        env.synchronize()
        summary = out["summary"].cpu().numpy().view(np.dtype(_abi.SPA_SUMMARY_DTYPE))[0]
        assert int(summary["rounds_run"]) == 2 and int(summary["num_rejected"]) >= 1, summary
        M, crit = with_torch()
        torch.cuda.synchronize()
        got = out["max_stat"].view(3, R)
        tol = 64 * 2.0 ** -52 * 16 * float(M.max())          # a 64-term sum, then one subtraction and one product
        assert float((got - M).abs().max()) <= tol and abs(float(out["crit"][0]) - float(crit)) <= tol
        del M, crit
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        live = torch.cuda.memory_allocated(dev)
        with_torch()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - live

        legs = [("check", check), ("spa1", spa(1)), ("spa2", spa(2)), ("spa10", spa(10)), ("torch", with_torch)]
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
                   us_max={k: max(t) for k, t in times.items()}, f64_ops_per_pass=ops,
                   spa1_over_check=round(med["spa1"] / med["check"], 3),
                   live_round_us=round(med["spa2"] - med["spa1"], 1),
                   idle_round_us=round((med["spa10"] - med["spa2"]) / 8, 2),
                   torch_over_spa_pass=round(med["torch"] / (med["spa1"] - med["check"]), 3),
                   torch_peak_temporary_bytes=int(peak), matrix_bytes=8 * R * S)
        for name, _ in legs:
            say(f"S={S} n={n} R={R}  {name:6s} {med[name]:10.1f} us per call  (min {min(times[name]):.1f}, max "
                f"{max(times[name]):.1f}, {a.reps} interleaved passes of {a.inner} calls, device events)")
        say(f"S={S} n={n} R={R}  spa1 / check = {res['spa1_over_check']}; one further live round "
            f"{res['live_round_us']} us, one idle round {res['idle_round_us']} us; torch / (spa1 - check) = "
            f"{res['torch_over_spa_pass']}; torch's peak temporary memory {peak / 2 ** 20:.1f} MiB (the [R, S] matrix "
            f"alone is {8 * R * S / 2 ** 20:.1f} MiB), the library's scratch holds no [R, S] array")
        results.append(res)
        del rec, x, w, out, rc
        torch.cuda.empty_cache()
    env.close()
    say(json.dumps({"spa_bench": results}))
    log.close()


if __name__ == "__main__":
    main()
