#!/usr/bin/env python3
"""What the probability of backtest overfitting costs on the device (gte_cscv, csrc/gte_cscv.hip) at the size of a
large sweep, S = 65 536 strategies, B = 64 periods in G = 16 groups, all C(16, 8) = 12 870 splits, Sharpe ratio, and at
S = 4 096, against the formulation a user would write with torch in the same process:

  cscv      gte_cscv: the copy of the three host tables and six launches (fold, IS/OOS pass, winners, rank pass,
            close, summary);
  torch     the group sums as `masks [G, B] @ field [B, S]` per field, then, for a chunk of splits at a time,
            `side [c, G] @ sums [G, S]` per field and side in f64, the Sharpe formulas, `argmax` over the strategies,
            the winner's out-of-sample score by `gather`, and comparisons against it summed for below / equal /
            ranked.  The chunk is the largest with chunk * S <= 2^24, so that one [chunk, S] f64 temporary is 128 MiB;
            its peak temporary memory is what torch's allocator reports above what was live before.
  reality   gte_reality_check at the same S (n = B = 64, R = 1 000, its weights made before), for scale.

One process, one small env; the legs are interleaved pass by pass; every leg is timed with device events on the env's
stream (torch's), `--inner` calls per timing window.  Per leg: median and min-max over the passes, per call.  A
(split, strategy) pair is scored twice in the first pass and once in the second: "pair scores per second" is
3 * C * S over the whole call's time — an end-to-end figure, not a kernel's.  Before anything is timed the two
formulations are compared: the winners agree except where two in-sample scores differ by rounding alone, the scores
within the rounding of a 16-term f64 sum.  No ratio is promised: the library path is kept for its fixed bits and for
never making a [C, S] matrix; where torch is faster this says so.

    python tools/cscv_bench.py [--reps 7] [--inner 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

SHAPES = ((4_096, 64, 16), (65_536, 64, 16))
R = 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi, periods
    from gym_trading_env_amd.batched import BatchedTradingEnv
    if not torch.cuda.is_available():
        sys.exit("cscv_bench needs the GPU: nothing here can be timed without it")
    feat, close = bench.synthetic_dataset(0, 2000, 2)
    env = BatchedTradingEnv((feat, close), num_envs=64, positions=[-1, 0, 1], windows=None, seed=1, output="torch")
    lib, h, dev = env._lib, env._h, env._t["obs"].device
    dt = np.dtype(_abi.STRATEGY_PERIOD_DTYPE)
    f64t = torch.float64
    results = []
    for S, B, G in SHAPES:
        rng = np.random.default_rng(S)
        host = np.zeros((S, B), dtype=dt)
        host["reward_sum"] = rng.normal(0, 0.1, (S, B))             # 100 steps of N(0, 0.01^2) per period
        host["reward_sq_sum"] = 0.01 * rng.chisquare(100, (S, B)) / 100
        host["steps"] = 100
        rec = torch.from_numpy(host.view(np.uint8).reshape(S * B, 48).copy()).to(dev)
        fields = [torch.from_numpy(np.ascontiguousarray(host[k]).astype(np.float64).T.copy()).to(dev)     # [B, S]
                  for k in ("reward_sum", "reward_sq_sum", "steps")]
        groups = periods.cscv_groups(range(B), G)
        is_g, oos_g = periods.cscv_splits(G)
        n = len(is_g)
        member = np.array([[(int(groups[g, b >> 6]) >> (b & 63)) & 1 for b in range(B)] for g in range(G)], np.float64)
        member = torch.from_numpy(member).to(dev)                                                       # [G, B]
        bits = lambda w: torch.from_numpy(((w[:, None] >> np.arange(G, dtype=np.uint32)) & 1).astype(np.float64)).to(dev)
        is_m, oos_m = bits(is_g), bits(oos_g)                                                           # [C, G]
        i32 = lambda: torch.empty((n,), dtype=torch.int32, device=dev)
        f64 = lambda: torch.empty((n,), dtype=f64t, device=dev)
        out = dict(best=i32(), is_score=f64(), oos_score=f64(), below=i32(), equal=i32(), ranked=i32(),
                   summary=torch.empty((24,), dtype=torch.uint8, device=dev))
        ptrs = _abi.GteCscvOut(**{k: v.data_ptr() for k, v in out.items()})
        w = torch.empty((R, B), dtype=f64t, device=dev)
        rc = dict(mean=torch.empty((S,), dtype=f64t, device=dev), boot_sum=torch.empty((S,), dtype=f64t, device=dev),
                  boot_sq_sum=torch.empty((S,), dtype=f64t, device=dev),
                  count_ge=torch.empty((S,), dtype=torch.int32, device=dev),
                  count_adj=torch.empty((S,), dtype=torch.int32, device=dev), max_stat=torch.empty((R,), dtype=f64t, device=dev),
                  max_index=torch.empty((R,), dtype=torch.int32, device=dev),
                  summary=torch.empty((24,), dtype=torch.uint8, device=dev))
        rc_ptrs = _abi.GteRealityCheckOut(**{k: v.data_ptr() for k, v in rc.items()})
        words = (C.c_uint64 * 2)(2 ** 64 - 1 if B >= 64 else (1 << B) - 1, 0)
        _abi.check(lib, lib.gte_bootstrap_weights(h, B, R, 2.0, 7, C.c_void_p(w.data_ptr())))
        chunk = max(1, min(n, 2 ** 24 // S))
        torch.cuda.synchronize()

        def cscv():
            _abi.check(lib, lib.gte_cscv(h, C.c_void_p(rec.data_ptr()), S, B, C.c_void_p(groups.ctypes.data), G,
                                         C.c_void_p(is_g.ctypes.data), C.c_void_p(oos_g.ctypes.data), n,
                                         _abi.PERIOD_METRIC_SHARPE, C.byref(ptrs)))

        def reality():
            _abi.check(lib, lib.gte_reality_check(h, C.c_void_p(rec.data_ptr()), S, B, words, None,
                                                  C.c_void_p(w.data_ptr()), R, C.byref(rc_ptrs)))

        def sharpe(side, sums):
            s1, s2, cnt = (side @ t for t in sums)          # [c, S] each
            m = s1 / cnt
            return m / torch.sqrt(torch.clamp(s2 / cnt - m * m, min=0.0))

        def with_torch():
            sums = [member @ t for t in fields]             # [G, S] each
            res = [[] for _ in range(6)]
            for lo in range(0, n, chunk):
                IS = sharpe(is_m[lo:lo + chunk], sums)
                best = IS.argmax(dim=1)
                OOS = sharpe(oos_m[lo:lo + chunk], sums)
                won = OOS.gather(1, best[:, None])
                for k, v in enumerate((best, IS.gather(1, best[:, None])[:, 0], won[:, 0], (OOS < won).sum(1),
                                       (OOS == won).sum(1), (OOS == OOS).sum(1))):
                    res[k].append(v)
            return [torch.cat(v) for v in res]

        cscv()
        env.synchronize()
        best, is_score, oos_score, below, equal, ranked = with_torch()
        torch.cuda.synchronize()
        same = out["best"].long() == best
        tol = 16 * 2.0 ** -52 * 8           # relative: sixteen additions and the five operations after them
        rel = ((out["is_score"] - is_score).abs() / is_score.abs())[same]
        agree = float(same.double().mean())
        assert agree >= 0.99 and float(rel.max()) <= tol, (agree, float(rel.max()))
        assert int((out["ranked"].long() - ranked).abs().max()) == 0
        assert int((out["below"].long() - below)[same].abs().max()) <= 2
        pbo_torch = float(((2 * below + equal) <= ranked).double().mean())
        summary = out["summary"].cpu().numpy().view(np.dtype(_abi.CSCV_SUMMARY_DTYPE))[0]
        pbo = float(summary["overfit"]) / float(summary["valid"])
        del best, is_score, oos_score, below, equal, ranked, same, rel
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        live = torch.cuda.memory_allocated(dev)
        with_torch()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - live

        legs = [("cscv", cscv), ("torch", with_torch), ("reality", reality)]
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
        pairs = 3.0 * n * S
        res = dict(S=S, B=B, G=G, splits=n, R=R, reps=a.reps, inner=a.inner, us=med,
                   us_min={k: min(t) for k, t in times.items()}, us_max={k: max(t) for k, t in times.items()},
                   pair_scores=pairs, cscv_pair_scores_per_s=round(pairs / (med["cscv"] * 1e-6), 0),
                   torch_over_cscv=round(med["torch"] / med["cscv"], 3), torch_chunk=chunk,
                   torch_peak_temporary_bytes=int(peak), matrix_bytes=8 * n * S, winners_agree=agree, pbo=pbo,
                   pbo_torch=pbo_torch)
        for name, _ in legs:
            print(f"S={S} B={B} G={G} C={n}  {name:8s} {med[name]:11.1f} us per call  (min {min(times[name]):.1f}, max "
                  f"{max(times[name]):.1f}, {a.reps} interleaved passes of {a.inner} calls, device events)", flush=True)
        print(f"S={S} B={B} G={G} C={n}  cscv: {pairs:.3g} pair scores, {res['cscv_pair_scores_per_s']:.3g} per second "
              f"end to end; torch / cscv = {res['torch_over_cscv']}; torch in chunks of {chunk} splits, peak temporary "
              f"memory {peak / 2 ** 20:.1f} MiB (one [C, S] f64 matrix would be {8 * n * S / 2 ** 20:.1f} MiB), the "
              f"library's scratch holds no [C, S] array; PBO {pbo:.4f} (torch {pbo_torch:.4f}), winners agree in "
              f"{agree:.4f} of the splits", flush=True)
        results.append(res)
        del rec, fields, out, rc, w, is_m, oos_m, member
        torch.cuda.empty_cache()
    env.close()
    print(json.dumps({"cscv_bench": results}))


if __name__ == "__main__":
    main()
