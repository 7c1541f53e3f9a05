#!/usr/bin/env python3
"""What building a signal table on the device costs (gte_build_signals, csrc/gte_signals.hip), on the
33 259-row shape DESIGN.md argues from, with a bank of 256 moving averages:

  (a) build         gte_build_signals into a preallocated table, rules in RANDOM order, and
      build-sorted  the same rules sorted by (a, b): waves that run together read the same bank rows;
  (b) torch         the same rule in torch (`where` -> `cummax` over "last row with a non-zero zone"
                    -> `gather`), int64 [S, T] temporaries and all — only at S = 4 096, where they fit;
  (c) fill          `tensor.fill_` of the same int8 bytes: the store floor.

One process, one small env (the build needs the dataset's T and the env's stream, not its envs); the
legs are interleaved pass by pass and timed with device events on the env's stream, which is torch's.
Per leg: median and min-max over the passes, GB/s of table bytes, and (a) against (b) and (c).
Before anything is timed, (a) in both orders and (b) are held equal byte for byte.

    python tools/signal_build_bench.py [--reps 9] [--sizes 4096 65536]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

T_ROWS = 33_259
N_SMA = 256
TORCH_MAX_S = 4_096


def sweep_rules(signals, S, seed=0):
    """S crossover rules over the bank, in random order: two different averages, a band, half latched"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, N_SMA, S)
    b = (a + rng.integers(1, N_SMA, S)) % N_SMA
    band = rng.choice([0.0, 0.05, 0.1, 0.2], S).astype(np.float32)
    return signals.rules(a=a, b=b, hi=band, lo=-band, warmup=4 * N_SMA, pos_up=2, pos_down=0, pos_neutral=-1,
                         latch=rng.random(S) < 0.5)


def rule_columns(torch, rules):
    """the fields of a RULE_DTYPE array as device tensors [S] for torch_table"""
    kinds = dict(a=np.int64, b=np.int64, hi=np.float32, lo=np.float32, warmup=np.int64, pos_up=np.int8,
                 pos_down=np.int8, pos_neutral=np.int8, latch=np.bool_)
    return {k: torch.from_numpy(np.ascontiguousarray(rules[k]).astype(dt)).to(device="cuda") for k, dt in kinds.items()}


def torch_table(torch, bank, r, T):
    """the rule of include/gte.h in torch: int8 [S, T] from bank f32 [C, >= T] and the rule columns"""
    t = torch.arange(T, device=bank.device)[None, :]
    A = bank[r["a"], :T]
    d = torch.where((r["b"] >= 0)[:, None], A - bank[r["b"].clamp_min(0), :T], A)
    up = d > r["hi"][:, None]
    z = up.to(torch.int8) - ((d < r["lo"][:, None]) & ~up).to(torch.int8)
    warm = t < r["warmup"][:, None]
    z = z.masked_fill(warm, 0)
    last = torch.cummax(torch.where(z != 0, t, -1), 1).values          # int64 [S, T]
    q = torch.where(last >= 0, torch.gather(z, 1, last.clamp_min(0)), 0).to(torch.int8)
    q = torch.where(r["latch"][:, None], q, z)
    out = torch.where(q > 0, r["pos_up"][:, None], torch.where(q < 0, r["pos_down"][:, None], r["pos_neutral"][:, None]))
    return out.masked_fill(warm, -1).to(torch.int8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4_096, 65_536])
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi, signals
    from gym_trading_env_amd.batched import BatchedTradingEnv
    if not torch.cuda.is_available():
        sys.exit("signal_build_bench needs the GPU: nothing here can be timed without it")
    T = T_ROWS
    feat, close = bench.synthetic_dataset(0, T, 2)
    env = BatchedTradingEnv((feat, close), num_envs=64, positions=[-1, 0, 1], windows=None, seed=1, output="torch")
    lib, h = env._lib, env._h
    windows = 2 + 4 * np.arange(N_SMA)
    bank = torch.from_numpy(signals.pad_bank(signals.sma_bank(close, windows))).cuda()
    stride = signals.row_stride(T)
    results = []
    for S in a.sizes:
        rules = sweep_rules(signals, S)
        order = np.lexsort((rules["b"], rules["a"]))
        as_tensor = lambda r: torch.from_numpy(np.ascontiguousarray(r).view(np.uint8).reshape(-1, 32)).cuda()
        d_random, d_sorted = as_tensor(rules), as_tensor(rules[order])
        table = torch.empty((S, stride), dtype=torch.int8, device="cuda")

        def build(d_rules):
            _abi.check(lib, lib.gte_build_signals(h, 0, C.c_void_p(bank.data_ptr()), N_SMA, int(bank.shape[1]),
                                                  C.c_void_p(d_rules.data_ptr()), S, C.c_void_p(table.data_ptr()), stride))

        legs = [("build", lambda: build(d_random)), ("build-sorted", lambda: build(d_sorted)),
                ("fill", lambda: table.fill_(1))]
        with_torch = S <= TORCH_MAX_S
        if with_torch:
            cols = rule_columns(torch, rules)
            legs.insert(2, ("torch", lambda: torch_table(torch, bank, cols, T)))
            # the three ways to the table agree before any is timed
            want = torch_table(torch, bank, cols, T)
            build(d_random)
            env.synchronize()
            assert torch.equal(table[:, :T], want), "gte_build_signals and the torch formulation disagree"
            by_rule = table[:, :T].clone()
            build(d_sorted)
            env.synchronize()
            assert torch.equal(table[:, :T], by_rule[torch.from_numpy(order).cuda()]), "sorted rules: other rows"
            shares = {int(v): round(float((want == v).float().mean()), 3) for v in (-1, 0, 2)}
            del want, by_rule
        times = {n: [] for n, _ in legs}
        for rep in range(a.reps + 1):  # pass 0 is the warm-up: allocations, code objects
            for n, f in legs:
                env.timer_start()
                f()
                t = env.timer_stop() * 1e3
                if rep:
                    times[n].append(t)
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        table_bytes = S * stride
        res = dict(S=S, T=T, indicators=N_SMA, reps=a.reps, table_bytes=table_bytes, bank_bytes=int(bank.numel()) * 4,
                   us=med, us_min={n: min(t) for n, t in times.items()}, us_max={n: max(t) for n, t in times.items()},
                   table_GBps={n: round(table_bytes / (med[n] * 1e-6) / 1e9, 1) for n in med},
                   build_over_fill=round(med["build"] / med["fill"], 3),
                   sorted_over_fill=round(med["build-sorted"] / med["fill"], 3),
                   sorted_over_random=round(med["build-sorted"] / med["build"], 3))
        if with_torch:
            res.update(torch_over_build=round(med["torch"] / med["build"], 2),
                       torch_over_sorted=round(med["torch"] / med["build-sorted"], 2), table_shares=shares)
        results.append(res)
        for n, _ in legs:
            print(f"S={S:6d} T={T}  {n:12s} {med[n]:10.1f} us  (min {min(times[n]):.1f}, max {max(times[n]):.1f}, "
                  f"{a.reps} interleaved passes)  {res['table_GBps'][n]:8.1f} GB/s of table bytes", flush=True)
        del table, d_random, d_sorted
        torch.cuda.empty_cache()
    env.close()
    print(json.dumps({"signal_build_bench": results}))


if __name__ == "__main__":
    main()
