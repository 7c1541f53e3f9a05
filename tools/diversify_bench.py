#!/usr/bin/env python3
"""What a decorrelated leaderboard costs on the device (gte_diversify, csrc/gte_diversify.hip) at the size of a large
sweep, S = 65 536 strategies over n = 64 periods, and at S = 4 096, for k = 10, 64 and 256 rounds, against the loop a
user would write with torch in the same process:

  diversify  gte_diversify: the whole call, k + 2 launches (prepare, one per round, close);
  torch      the standardised matrix Z [S, n] in f64, then per round `where(live, scores, -inf).argmax()`, the
             mat-vec `Z @ Z[pick]`, and mask updates of live / owner / owner_corr, the pick staying on the device (no
             host read inside the loop); its peak temporary memory is what torch's allocator reports above what was
             live before.

Two inputs per shape, threshold 0.9:
  families     64 factor rows, every strategy one of them plus 0.05 x noise — a near-duplicate sweep.  Every round
               removes a family, so the live set collapses: after 64 rounds nothing is left and later rounds are empty.
  independent  rows of independent normals: a round removes its pick alone, so every round reads the whole staged
               matrix, S * n * 8 bytes (33.5 MB at the large shape: more than the 32 MiB of the eight L2s, so it is
               served by the Infinity Cache; 2.1 MB at the small one: L2).

One process, one small env; the legs are interleaved pass by pass; every leg is timed with device events on the env's
stream (torch's), `--inner` calls per timing window.  Per leg: median and min-max over the passes, per call.  For the
independent rows the cost of one more round is the slope between k = 10 and k = 256, and S * n * 8 bytes over it the
achieved rate of a round — a launch boundary included: an end-to-end figure per round, not a kernel's.  Before
anything is timed the two formulations are compared: the same picks, the same cluster sizes, the same owners.  No
ratio is promised: the library path is kept for its fixed bits; where torch is faster this says so.

    python tools/diversify_bench.py [--reps 7] [--inner 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

SHAPES = ((4_096, 64), (65_536, 64))
ROUNDS = (10, 64, 256)
FAMILIES = 64
MAX_CORR = 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi
    from gym_trading_env_amd.batched import BatchedTradingEnv
    if not torch.cuda.is_available():
        sys.exit("diversify_bench needs the GPU: nothing here can be timed without it")
    feat, close = bench.synthetic_dataset(0, 2000, 2)
    env = BatchedTradingEnv((feat, close), num_envs=64, positions=[-1, 0, 1], windows=None, seed=1, output="torch")
    lib, h, dev = env._lib, env._h, env._t["obs"].device
    dt = np.dtype(_abi.STRATEGY_PERIOD_DTYPE)
    f64t = torch.float64
    results = []
    for S, n in SHAPES:
        for kind in ("families", "independent"):
            rng = np.random.default_rng(S + len(kind))
            if kind == "families":
                factors = rng.normal(0, 1, (FAMILIES, n))
                x = (factors[rng.integers(0, FAMILIES, S)] + 0.05 * rng.normal(0, 1, (S, n))) * 1e-3
            else:
                x = rng.normal(0, 1, (S, n)) * 1e-3
            host = np.zeros((S, n), dtype=dt)
            host["reward_sum"], host["reward_sq_sum"], host["steps"] = x, x * x, 100
            rec = torch.from_numpy(host.view(np.uint8).reshape(S * n, 48).copy()).to(dev)
            X = torch.from_numpy(x).to(dev)                                     # [S, n], what torch starts from
            scores = torch.from_numpy(rng.normal(0, 1, S)).to(dev)
            words = (C.c_uint64 * 2)(2 ** 64 - 1 if n >= 64 else (1 << n) - 1, 0)
            kmax = max(ROUNDS)
            out = dict(pick=torch.empty((kmax,), dtype=torch.int32, device=dev),
                       pick_score=torch.empty((kmax,), dtype=f64t, device=dev),
                       cluster_size=torch.empty((kmax,), dtype=torch.int32, device=dev),
                       owner=torch.empty((S,), dtype=torch.int32, device=dev),
                       owner_corr=torch.empty((S,), dtype=f64t, device=dev),
                       pick_corr=torch.empty((kmax * kmax,), dtype=f64t, device=dev),
                       summary=torch.empty((20,), dtype=torch.uint8, device=dev))
            ptrs = _abi.GteDiversifyOut(**{name: v.data_ptr() for name, v in out.items()})
            ids = torch.arange(S, device=dev)
            neg = torch.full((S,), float("-inf"), dtype=f64t, device=dev)
            nan = torch.full((S,), float("nan"), dtype=f64t, device=dev)
            torch.cuda.synchronize()

            def diversify(k):
                _abi.check(lib, lib.gte_diversify(h, C.c_void_p(rec.data_ptr()), S, n, words,
                                                  C.c_void_p(scores.data_ptr()), MAX_CORR, k, C.byref(ptrs)))

            def with_torch(k):
                e = X - X.mean(dim=1, keepdim=True)
                Z = e / e.norm(dim=1, keepdim=True)
                live = torch.isfinite(Z).all(dim=1) & ~torch.isnan(scores)
                owner = torch.where(live, -1, -2).to(torch.int32)
                owner_corr = nan.clone()
                picks = torch.full((k,), -1, dtype=torch.int64, device=dev)
                sizes = torch.zeros((k,), dtype=torch.int64, device=dev)
                for r in range(k):
                    p = torch.where(live, scores, neg).argmax()
                    c = Z @ Z.index_select(0, p.view(1))[0]     # (an index that stays on the device)
                    gone = live & ((c > MAX_CORR) | (ids == p))
                    picks[r] = torch.where(live.any(), p, -1)
                    sizes[r] = gone.sum()
                    owner = torch.where(gone, r, owner)
                    owner_corr = torch.where(gone, c, owner_corr)
                    live = live & ~gone
                return picks, sizes, owner, owner_corr

            res = dict(S=S, n=n, input=kind, max_corr=MAX_CORR, reps=a.reps, inner=a.inner, matrix_bytes=8 * S * n,
                       us={}, us_min={}, us_max={}, torch_peak_temporary_bytes={}, picked={}, remaining={})
            for k in ROUNDS:    # the two formulations say the same
                diversify(k)
                env.synchronize()
                picks, sizes, owner, _ = with_torch(k)
                torch.cuda.synchronize()
                assert bool((out["pick"][:k].long() == picks).all()), (S, kind, k, "picks differ")
                assert bool((out["cluster_size"][:k].long() == sizes).all()), (S, kind, k, "cluster sizes differ")
                assert bool((out["owner"] == owner).all()), (S, kind, k, "owners differ")
                summary = out["summary"].cpu().numpy().view(np.dtype(_abi.DIVERSIFY_SUMMARY_DTYPE))[0]
                res["picked"][k], res["remaining"][k] = int(summary["picked"]), int(summary["remaining"])
                del picks, sizes, owner
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats(dev)
                live_bytes = torch.cuda.memory_allocated(dev)
                with_torch(k)
                torch.cuda.synchronize()
                res["torch_peak_temporary_bytes"][k] = int(torch.cuda.max_memory_allocated(dev) - live_bytes)
            legs = [(f"{name} k={k}", f, k) for k in ROUNDS for name, f in (("diversify", diversify), ("torch", with_torch))]
            times = {name: [] for name, _, _ in legs}
            for rep in range(a.reps + 1):   # pass 0 is the warm-up: allocations, code objects, rocBLAS's choice
                for name, f, k in legs:
                    env.timer_start()
                    for _ in range(a.inner):
                        f(k)
                    t = env.timer_stop() * 1e3 / a.inner
                    if rep:
                        times[name].append(t)
            for name, _, _ in legs:
                t = times[name]
                res["us"][name], res["us_min"][name], res["us_max"][name] = sorted(t)[len(t) // 2], min(t), max(t)
                print(f"S={S} n={n} {kind:11s} {name:16s} {res['us'][name]:11.1f} us per call  (min {min(t):.1f}, max "
                      f"{max(t):.1f}, {a.reps} interleaved passes of {a.inner} calls, device events)", flush=True)
            lo, hi = min(ROUNDS), max(ROUNDS)
            for side in ("diversify", "torch"):
                res[f"{side}_us_per_round"] = (res["us"][f"{side} k={hi}"] - res["us"][f"{side} k={lo}"]) / (hi - lo)
            per_round = res["diversify_us_per_round"]
            res["diversify_round_bytes_per_s"] = 8.0 * S * n / (per_round * 1e-6)
            print(f"S={S} n={n} {kind:11s} picks / remaining after k rounds: "
                  + ", ".join(f"k={k}: {res['picked'][k]} / {res['remaining'][k]}" for k in ROUNDS)
                  + f"; one more round costs {per_round:.2f} us (torch {res['torch_us_per_round']:.2f} us)"
                  + (f", S * n * 8 = {8 * S * n / 1e6:.1f} MB over it = {res['diversify_round_bytes_per_s'] / 1e12:.2f} "
                     f"TB/s per round, launch boundary included" if kind == "independent" else
                     " on average over rounds 10 .. 255, most of which find nothing live")
                  + "; torch / diversify = "
                  + ", ".join(f"k={k}: {res['us'][f'torch k={k}'] / res['us'][f'diversify k={k}']:.2f}" for k in ROUNDS)
                  + f"; torch's peak temporary memory {max(res['torch_peak_temporary_bytes'].values()) / 2 ** 20:.1f} "
                    f"MiB (Z alone is {8 * S * n / 2 ** 20:.1f} MiB), the library's staged matrix is as large and "
                    f"lives in its scratch", flush=True)
            results.append(res)
            del rec, X, scores, out, ids, neg, nan
            torch.cuda.empty_cache()
    env.close()
    print(json.dumps({"diversify_bench": results}))


if __name__ == "__main__":
    main()
