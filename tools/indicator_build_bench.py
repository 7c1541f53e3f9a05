#!/usr/bin/env python3
"""What building an indicator bank on the device costs (gte_build_indicators, csrc/gte_indicators.hip),
on the 33 259-row shape DESIGN.md argues from, with C = 256 specs:

  (a) dev-sma       gte_build_indicators, 256 SMAs of close (windows 2, 6, .. 1 022),
      dev-ema       256 EMAs of the same spans: one dependent f64 chain along T per row,
      dev-mixed     EMA / RSI / ZSCORE rows in the proportions of examples/backtest_indicator_sweep.py;
  (b) host-sma      today's path to the all-SMA bank: signals.sma_bank + pad_bank + the host-to-device
                    copy, WALL CLOCK (it runs on the host);
  (c) torch-sma     the SMA in torch on the device: cumsum in f64, difference, divide, cast;
  (d) fill          `tensor.fill_` of the same f32 bytes: the store floor.

One process, one small env; the legs are interleaved pass by pass; the device legs are timed with device
events on the env's stream, which is torch's.  Per leg: median and min-max over the passes.  Before
anything is timed the three SMA banks are held equal: (a) against the header's k-ordered sum on sampled
rows float for float, (b) and (c) — prefix sums, another order of summation — against (a) within
2 units of the last f32 place.

    python tools/indicator_build_bench.py [--reps 9]
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

T_ROWS = 33_259
N_SPECS = 256


def torch_sma(torch, close64, windows, T, stride):
    """f32 [C, stride] from f64 prefix sums on the device; NaN while the window has no history"""
    csum = torch.cat([torch.zeros(1, dtype=torch.float64, device=close64.device), torch.cumsum(close64, 0)])
    out = torch.zeros((len(windows), stride), dtype=torch.float32, device=close64.device)
    out[:, :T] = float("nan")
    for i, n in enumerate(windows):
        out[i, n - 1:T] = ((csum[n:] - csum[:-n]) / n).to(torch.float32)
    return out


def ulps(torch, a, b):
    """the largest distance of two f32 tensors in units of the last place (NaN only beside NaN)"""
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    ok = ~torch.isnan(a)
    ia, ib = a[ok].view(torch.int32).to(torch.int64), b[ok].view(torch.int32).to(torch.int64)
    return int((ia - ib).abs().max())   # (all values positive here: prices)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    from gym_trading_env_amd import _abi, signals
    from gym_trading_env_amd.batched import BatchedTradingEnv
    if not torch.cuda.is_available():
        sys.exit("indicator_build_bench needs the GPU: nothing here can be timed without it")
    T = T_ROWS
    feat, close = bench.synthetic_dataset(0, T, 2)
    env = BatchedTradingEnv((feat, close), num_envs=64, positions=[-1, 0, 1], windows=None, seed=1, output="torch")
    lib, h = env._lib, env._h
    windows = [int(w) for w in 2 + 4 * np.arange(N_SPECS)]
    third = N_SPECS // 3
    mixed = np.concatenate([signals.indicators("ema", windows[:N_SPECS - 2 * third]),
                            signals.indicators("rsi", windows[:third]), signals.indicators("zscore", windows[:third])])
    banks = {"dev-sma": signals.indicators("sma", windows), "dev-ema": signals.indicators("ema", windows),
             "dev-mixed": mixed}
    as_tensor = lambda s: torch.from_numpy(np.ascontiguousarray(s).view(np.uint8).reshape(-1, 16)).cuda()
    d_specs = {k: as_tensor(v) for k, v in banks.items()}
    stride = signals.bank_stride(T)
    bank = torch.empty((N_SPECS, stride), dtype=torch.float32, device="cuda")
    close64 = torch.from_numpy(close).cuda()

    def build(name):
        _abi.check(lib, lib.gte_build_indicators(h, 0, C.c_void_p(d_specs[name].data_ptr()), N_SPECS, None, 0, 0,
                                                 C.c_void_p(bank.data_ptr()), stride))

    def host_sma():
        return torch.from_numpy(signals.pad_bank(signals.sma_bank(close, windows))).cuda()

    # the ways to the all-SMA bank agree before any is timed
    build("dev-sma")
    env.synchronize()
    dev = bank.clone()
    for i in (0, 1, 17, 255):
        n = windows[i]
        s = np.zeros(T - n + 1)
        for k in range(n):
            s = s + close[k:k + T - n + 1]
        want = torch.from_numpy((s / n).astype(np.float32)).cuda()
        assert torch.equal(dev[i, n - 1:T], want) and bool(torch.isnan(dev[i, :n - 1]).all()), f"SMA({n})"
    assert bool((dev[:, T:] == 0).all())
    far = {"host-sma": ulps(torch, dev[:, :T], host_sma()[:, :T]),
           "torch-sma": ulps(torch, dev[:, :T], torch_sma(torch, close64, windows, T, stride)[:, :T])}
    assert max(far.values()) <= 2, far
    del dev

    legs = [("dev-sma", lambda: build("dev-sma")), ("dev-ema", lambda: build("dev-ema")),
            ("dev-mixed", lambda: build("dev-mixed")), ("host-sma", host_sma),
            ("torch-sma", lambda: torch_sma(torch, close64, windows, T, stride)), ("fill", lambda: bank.fill_(1.0))]
    times = {n: [] for n, _ in legs}
    for rep in range(a.reps + 1):  # pass 0 is the warm-up: allocations, code objects
        for n, f in legs:
            if n == "host-sma":
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                t = (time.perf_counter() - t0) * 1e6
            else:
                env.timer_start()
                f()
                t = env.timer_stop() * 1e3
            if rep:
                times[n].append(t)
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    bank_bytes = N_SPECS * stride * 4
    res = dict(C=N_SPECS, T=T, reps=a.reps, bank_bytes=bank_bytes, us=med,
               us_min={n: min(t) for n, t in times.items()}, us_max={n: max(t) for n, t in times.items()},
               bank_GBps={n: round(bank_bytes / (med[n] * 1e-6) / 1e9, 2) for n in med},
               ulps_from_dev_sma=far, ns_per_row_of_an_ema=round(med["dev-ema"] * 1e3 / T, 2),
               host_over_dev_sma=round(med["host-sma"] / med["dev-sma"], 2),
               torch_over_dev_sma=round(med["torch-sma"] / med["dev-sma"], 2),
               dev_sma_over_fill=round(med["dev-sma"] / med["fill"], 1))
    for n, _ in legs:
        clock = "wall clock" if n == "host-sma" else "device events"
        print(f"C={N_SPECS} T={T}  {n:10s} {med[n]:12.1f} us  (min {min(times[n]):.1f}, max {max(times[n]):.1f}, "
              f"{a.reps} interleaved passes, {clock})  {res['bank_GBps'][n]:8.2f} GB/s of bank bytes", flush=True)
    env.close()
    print(json.dumps({"indicator_build_bench": res}))


if __name__ == "__main__":
    main()
