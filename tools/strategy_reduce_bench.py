#!/usr/bin/env python3
"""What folding N env records into S strategy records on the device costs (gte_reduce_backtest_stats,
csrc/gte_strategy.hip), and ranking them (gte_rank_strategies), at the two extremes of a sweep and in
between: N = 524 288 / S = 65 536 (8 members each), N = 65 536 / S = 64 (1 024 each), N = S = 65 536.

  dev-default   the reduction under the library's map e % S;
  dev-map       the same under an explicit shuffled map, from CSR lists built beforehand;
  lists         building those lists from the map on the device (torch: stable sort + searchsorted);
  torch-default what a user writes today for e % S: `field.reshape(R, S).sum(0)` per summed field (four f64
                sums, four counters) and `.amax(0)` for the drawdown, on the 128-byte-strided field views;
  torch-map     the same for an explicit map: `index_add_` per summed field, `scatter_reduce_` for the maximum;
  host          the `.numpy()` path: the records to the host in one transfer, then NumPy's reshape-sums,
                WALL CLOCK;
  rank-32       gte_rank_strategies(k = 32) over the S strategy records (score, candidates, selection);
  torch-topk    `torch.topk(scores, 32)` over the S scores alone (no score computed, no eligibility rule).

One process, one small env; the legs are interleaved pass by pass; the device legs are timed with device
events on the env's stream, which is torch's.  Per leg: median and min-max over the passes.  "share" is
(N + S) * 128 bytes / time against the 6.29 TB/s a 16-byte-vector copy reaches on an MI355X.  Before
anything is timed the device's counters are held equal to torch's and its f64 sums to torch's within the
summation-order bound.

    python tools/strategy_reduce_bench.py [--reps 9]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

SHAPES = ((524_288, 65_536), (65_536, 64), (65_536, 65_536))
HBM_BYTES_PER_S = 6.29e12
SUMMED = ("reward_sum", "reward_sq_sum", "ep_return_sum", "ep_return_sq_sum", "steps", "trades", "episodes",
          "terminations")


def records(N, seed=0):
    from gym_trading_env_amd import _abi
    rng = np.random.default_rng(seed)
    r = np.zeros(N, dtype=np.dtype(_abi.BACKTEST_DTYPE))
    r["steps"] = rng.integers(1, 5000, N)
    for name in ("reward_sum", "ep_return_sum"):
        r[name] = rng.normal(0, 1, N)
    for name in ("reward_sq_sum", "ep_return_sq_sum"):
        r[name] = rng.uniform(0, 2, N)
    r["max_drawdown"] = rng.uniform(0, 1, N)
    r["trades"], r["episodes"], r["terminations"] = rng.integers(0, 4000, N), rng.integers(1, 40, N), rng.integers(0, 3, N)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi
    from gym_trading_env_amd.batched import BatchedTradingEnv, _device_view
    from gym_trading_env_amd.strategy_records import strategy_groups
    if not torch.cuda.is_available():
        sys.exit("strategy_reduce_bench needs the GPU: nothing here can be timed without it")
    feat, close = bench.synthetic_dataset(0, 2000, 2)
    bt, st = np.dtype(_abi.BACKTEST_DTYPE), np.dtype(_abi.STRATEGY_DTYPE)
    results = []
    for N, S in SHAPES:
        env = BatchedTradingEnv((feat, close), num_envs=N, positions=[-1, 0, 1], windows=None, seed=1, output="torch")
        lib, h, dev = env._lib, env._h, env._t["obs"].device
        host_rec = records(N)
        rec = torch.from_numpy(host_rec.view(np.uint8).reshape(N, 128).copy()).to(dev)
        field = {n: _device_view(rec.data_ptr() + bt.fields[n][1], (N,), t, dev, (128,)) for n, t in _abi.BACKTEST_FIELDS}
        R = N // S
        m = torch.from_numpy(np.random.default_rng(1).permutation(np.arange(N) % S)).to(dev)
        offsets, members = strategy_groups(env, m, S)
        out = torch.empty((S, 128), dtype=torch.uint8, device=dev)
        idx = torch.empty((32,), dtype=torch.int32, device=dev)
        top = torch.empty((32,), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def dev_reduce(lists):
            _abi.check(lib, lib.gte_reduce_backtest_stats(
                h, C.c_void_p(rec.data_ptr()), S, C.c_void_p(offsets.data_ptr()) if lists else None,
                C.c_void_p(members.data_ptr()) if lists else None, C.c_void_p(out.data_ptr())))

        def torch_default():
            res = {n: field[n].reshape(R, S).sum(0) for n in SUMMED}
            res["max_drawdown"] = field["max_drawdown"].reshape(R, S).amax(0)
            return res

        def torch_map():
            res = {n: torch.zeros(S, dtype=field[n].dtype, device=dev).index_add_(0, m, field[n]) for n in SUMMED}
            res["max_drawdown"] = torch.zeros(S, dtype=torch.float64, device=dev).scatter_reduce_(
                0, m, field["max_drawdown"], "amax")
            return res

        def host():
            r = rec.cpu().numpy().view(bt).reshape(N)
            res = {n: r[n].reshape(R, S).sum(0) for n in SUMMED}
            res["max_drawdown"] = r["max_drawdown"].reshape(R, S).max(0)
            return res

        def rank():
            _abi.check(lib, lib.gte_rank_strategies(h, C.c_void_p(out.data_ptr()), S, _abi.METRIC_MEAN_EPISODE_RETURN, 1, 32,
                                                    C.c_void_p(idx.data_ptr()), C.c_void_p(top.data_ptr()), None))

        # the formulations agree before any is timed
        for lists, ref in ((False, torch_default()), (True, torch_map())):
            dev_reduce(lists)
            env.synchronize()
            got = out.cpu().numpy().view(st).reshape(S)
            for n in SUMMED:
                want = ref[n].cpu().numpy()
                if want.dtype.kind == "f":
                    bound = (R + 7) * 2.0 ** -52 * np.abs(host_rec[n]).reshape(R, S).sum(0).max() * 2
                    assert np.abs(got[n] - want).max() <= bound, (n, lists)
                else:
                    assert (got[n] == want).all(), (n, lists)
            assert (got["max_drawdown"] == ref["max_drawdown"].cpu().numpy()).all() and (got["envs"] == R).all()
        scores = (_device_view(out.data_ptr() + st.fields["ep_return_sum"][1], (S,), "<f8", dev, (128,)) /
                  _device_view(out.data_ptr() + st.fields["episodes"][1], (S,), "<i8", dev, (128,))).contiguous()
        rank()
        env.synchronize()
        assert torch.equal(top, torch.topk(scores, 32).values)

        legs = [("dev-default", lambda: dev_reduce(False)), ("dev-map", lambda: dev_reduce(True)),
                ("lists", lambda: strategy_groups(env, m, S)), ("torch-default", torch_default),
                ("torch-map", torch_map), ("host", host), ("rank-32", rank),
                ("torch-topk", lambda: torch.topk(scores, 32))]
        times = {n: [] for n, _ in legs}
        for rep in range(a.reps + 1):  # pass 0 is the warm-up: allocations, code objects
            for n, f in legs:
                if n == "host":
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    t = (time.perf_counter() - t0) * 1e6
                else:
                    env.timer_start()
                    f()
                    t = env.timer_stop() * 1e3
                if rep:
                    times[n].append(t)
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        need = (N + S) * 128
        share = {n: round(need / (med[n] * 1e-6) / HBM_BYTES_PER_S, 4) for n in ("dev-default", "dev-map", "torch-default",
                                                                                 "torch-map", "host")}
        res = dict(N=N, S=S, members=R, reps=a.reps, bytes_needed=need, us=med, us_min={n: min(t) for n, t in times.items()},
                   us_max={n: max(t) for n, t in times.items()}, hbm_share=share,
                   torch_over_dev_default=round(med["torch-default"] / med["dev-default"], 2),
                   torch_over_dev_map=round(med["torch-map"] / med["dev-map"], 2),
                   host_over_dev_default=round(med["host"] / med["dev-default"], 1),
                   rank_over_topk=round(med["rank-32"] / med["torch-topk"], 2))
        for n, _ in legs:
            clock = "wall clock" if n == "host" else "device events"
            extra = f"  {100 * share[n]:6.2f} % of the HBM rate" if n in share else ""
            print(f"N={N} S={S}  {n:13s} {med[n]:11.1f} us  (min {min(times[n]):.1f}, max {max(times[n]):.1f}, "
                  f"{a.reps} interleaved passes, {clock}){extra}", flush=True)
        results.append(res)
        env.close()
        del rec, field, out, m, offsets, members
    print(json.dumps({"strategy_reduce_bench": results}))


if __name__ == "__main__":
    main()
