#!/usr/bin/env python3
"""What composing a signal table on the device costs (gte_compose_signals, csrc/gte_compose.hip), on the
33 259-row shape DESIGN.md argues from: 512 clause rows (zone codes, built by gte_build_signals from a bank
of 256 moving averages) and S specs of two inputs each — every spec an enter/exit table with KEEP or a
trend-AND-entry table, half and half:

  (a) compose          gte_compose_signals into a preallocated table, specs in RANDOM order,
      compose-sorted   the same specs sorted by their inputs: waves that run together read the same rows,
      compose-4in      specs of FOUR inputs (random order): twice the loads and index arithmetic;
  (b) build            gte_build_signals at the same S x T (random rule order) and
      build-sorted     sorted by (a, b): the neighbouring stage, which reads 8 bank bytes per table byte
                       where (a) reads 2;
  (c) torch            the same table in torch (`gather` of the clause rows, the truth table as an index,
                       `cummax` over "last decided row"), int64 [S, T] temporaries and all — only at
                       S = 4 096, where they fit;
  (d) fill             `tensor.fill_` of the same int8 bytes: the store floor.

One process, one small env (the stage needs the dataset's T and the env's stream, not its envs); the legs
are interleaved pass by pass and timed with device events on the env's stream, which is torch's.  Per
leg: median and min-max over the passes, GB/s of table bytes and their share of the 8 TB/s HBM peak, and
(a) against (b), (c) and (d).  Before anything is timed, (a) in both orders and (c) are held equal byte
for byte.

    python tools/signal_compose_bench.py [--reps 9] [--sizes 4096 65536]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from signal_build_bench import N_SMA, T_ROWS, TORCH_MAX_S, sweep_rules  # noqa: E402

N_CLAUSES = 512
HBM_PEAK_GBPS = 8000.0


def clause_rules(signals, seed=1):
    """512 clause rules over the bank: crossovers with a band, half latched, in zone codes"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, N_SMA, N_CLAUSES)
    b = (a + rng.integers(1, N_SMA, N_CLAUSES)) % N_SMA
    band = rng.choice([0.0, 0.05, 0.1, 0.2], N_CLAUSES).astype(np.float32)
    return signals.clauses(a=a, b=b, hi=band, lo=-band, warmup=4 * N_SMA, latch=rng.random(N_CLAUSES) < 0.5)


def sweep_specs(signals, S, n_in=2, seed=0):
    """S specs over the clause rows, in random order: a 256 x 256 grid of (trend, entry) pairs when S allows"""
    rng = np.random.default_rng(seed)
    KEEP = signals.KEEP
    inputs = np.stack([rng.integers(k * (N_CLAUSES // n_in), (k + 1) * (N_CLAUSES // n_in), S) for k in range(n_in)], 1)
    first = lambda f: (lambda *c: f(c[0], c[1]))
    enter_exit = signals.compose(inputs[:1], first(lambda x, y: 2 if x == 2 else 0 if y == 0 else KEEP))["lut"][0]
    trend_and = signals.compose(inputs[:1], first(lambda x, y: 2 if x == 2 and y != 2 else 1))["lut"][0]
    specs = signals.compose(inputs, np.zeros((3,) * n_in, np.int8), initial=1)
    specs["lut"] = np.where((rng.random(S) < 0.5)[:, None], enter_exit[None, :], trend_and[None, :])
    return specs


def spec_columns(torch, specs):
    """the fields of a COMPOSE_DTYPE array as device tensors for torch_table"""
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).to(device="cuda")
    return dict(rows=dev(specs["in"], np.int64), n_in=dev(specs["n_in"], np.int64), lut=dev(specs["lut"], np.int64),
                initial=dev(specs["initial"], np.int64), pos_invalid=dev(specs["pos_invalid"], np.int64))


def torch_table(torch, clauses, s, T, n_in, keep):
    """the rule of include/gte.h in torch: int8 [S, T] from clauses int8 [R, >= T] and the spec columns
    (specs that name clause rows, all with n_in inputs)"""
    t = torch.arange(T, device=clauses.device)[None, :]
    index = torch.zeros((s["rows"].shape[0], T), dtype=torch.int64, device=clauses.device)
    valid = torch.ones_like(index, dtype=torch.bool)
    for k in range(n_in):
        c = clauses[s["rows"][:, k], :T].to(torch.int64)           # int64 [S, T]
        ok = (c >= 0) & (c <= 2)
        valid &= ok
        index += torch.where(ok, c, 0) * 3 ** k
    e = torch.gather(s["lut"], 1, torch.where(valid, index, 0))    # the truth table as an index
    last = torch.cummax(torch.where(valid & (e != keep), t, -1), 1).values
    q = torch.where(last >= 0, torch.gather(e, 1, last.clamp_min(0)), s["initial"][:, None])
    return torch.where(valid, q, s["pos_invalid"][:, None]).to(torch.int8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4_096, 65_536])
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi, signals
    from gym_trading_env_amd.batched import BatchedTradingEnv
    if not torch.cuda.is_available():
        sys.exit("signal_compose_bench needs the GPU: nothing here can be timed without it")
    T = T_ROWS
    feat, close = bench.synthetic_dataset(0, T, 2)
    env = BatchedTradingEnv((feat, close), num_envs=64, positions=[-1, 0, 1], windows=None, seed=1, output="torch")
    lib, h = env._lib, env._h
    windows = 2 + 4 * np.arange(N_SMA)
    bank = torch.from_numpy(signals.pad_bank(signals.sma_bank(close, windows))).cuda()
    clauses = env.build_signals(bank[:, :T], clause_rules(signals), bind=False)   # int8 [512, T], rows padded
    stride = signals.row_stride(T)
    assert int(clauses.stride(0)) == stride
    results = []
    for S in a.sizes:
        specs, specs4 = sweep_specs(signals, S), sweep_specs(signals, S, n_in=4, seed=2)
        order = np.lexsort((specs["in"][:, 1], specs["in"][:, 0]))
        as_tensor = lambda r: torch.from_numpy(np.ascontiguousarray(r).view(np.uint8).reshape(len(r), -1).copy()).cuda()
        d_random, d_sorted, d_four = as_tensor(specs), as_tensor(specs[order]), as_tensor(specs4)
        rules = sweep_rules(signals, S)
        r_random, r_sorted = as_tensor(rules), as_tensor(rules[np.lexsort((rules["b"], rules["a"]))])
        table = torch.empty((S, stride), dtype=torch.int8, device="cuda")

        def compose(d_specs):
            _abi.check(lib, lib.gte_compose_signals(h, 0, C.c_void_p(clauses.data_ptr()), N_CLAUSES, stride,
                                                    C.c_void_p(d_specs.data_ptr()), S, C.c_void_p(table.data_ptr()), stride))

        def build(d_rules):
            _abi.check(lib, lib.gte_build_signals(h, 0, C.c_void_p(bank.data_ptr()), N_SMA, int(bank.shape[1]),
                                                  C.c_void_p(d_rules.data_ptr()), S, C.c_void_p(table.data_ptr()), stride))

        legs = [("compose", lambda: compose(d_random)), ("compose-sorted", lambda: compose(d_sorted)),
                ("compose-4in", lambda: compose(d_four)), ("build", lambda: build(r_random)),
                ("build-sorted", lambda: build(r_sorted)), ("fill", lambda: table.fill_(1))]
        with_torch = S <= TORCH_MAX_S
        shares = None
        if with_torch:
            cols = spec_columns(torch, specs)
            legs.insert(5, ("torch", lambda: torch_table(torch, clauses, cols, T, 2, signals.KEEP)))
            # the ways to the table agree before any is timed
            want = torch_table(torch, clauses, cols, T, 2, signals.KEEP)
            compose(d_random)
            env.synchronize()
            assert torch.equal(table[:, :T], want), "gte_compose_signals and the torch formulation disagree"
            by_spec = table[:, :T].clone()
            compose(d_sorted)
            env.synchronize()
            assert torch.equal(table[:, :T], by_spec[torch.from_numpy(order).cuda()]), "sorted specs: other rows"
            want4 = torch_table(torch, clauses, spec_columns(torch, specs4), T, 4, signals.KEEP)
            compose(d_four)
            env.synchronize()
            assert torch.equal(table[:, :T], want4), "four inputs: gte_compose_signals and torch disagree"
            shares = {int(v): round(float((want == v).float().mean()), 3) for v in (-1, 0, 1, 2)}
            del want, want4, by_spec
            torch.cuda.empty_cache()
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
        gbps = {n: round(table_bytes / (med[n] * 1e-6) / 1e9, 1) for n in med}
        res = dict(S=S, T=T, clause_rows=N_CLAUSES, reps=a.reps, table_bytes=table_bytes,
                   clause_bytes=N_CLAUSES * stride, us=med, us_min={n: min(t) for n, t in times.items()},
                   us_max={n: max(t) for n, t in times.items()}, table_GBps=gbps,
                   share_of_hbm_peak={n: round(v / HBM_PEAK_GBPS, 3) for n, v in gbps.items()},
                   compose_over_build=round(med["compose"] / med["build"], 3),
                   sorted_over_build_sorted=round(med["compose-sorted"] / med["build-sorted"], 3),
                   sorted_over_random=round(med["compose-sorted"] / med["compose"], 3),
                   four_over_two=round(med["compose-4in"] / med["compose"], 3),
                   compose_over_fill=round(med["compose"] / med["fill"], 3),
                   sorted_over_fill=round(med["compose-sorted"] / med["fill"], 3))
        if with_torch:
            res.update(torch_over_compose=round(med["torch"] / med["compose"], 2),
                       torch_over_sorted=round(med["torch"] / med["compose-sorted"], 2), table_shares=shares)
        results.append(res)
        for n, _ in legs:
            print(f"S={S:6d} T={T}  {n:15s} {med[n]:10.1f} us  (min {min(times[n]):.1f}, max {max(times[n]):.1f}, "
                  f"{a.reps} interleaved passes)  {gbps[n]:8.1f} GB/s of table bytes = "
                  f"{gbps[n] / HBM_PEAK_GBPS:.2f} of the HBM peak", flush=True)
        del table, d_random, d_sorted, d_four, r_random, r_sorted
        torch.cuda.empty_cache()
    env.close()
    print(json.dumps({"signal_compose_bench": results}))


if __name__ == "__main__":
    main()
