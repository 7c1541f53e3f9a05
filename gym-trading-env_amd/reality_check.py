"""RealityCheck — what `StrategyPeriodStats.reality_check()` gives: White's Reality Check of a strategy leaderboard,
a bootstrap over time blocks of the maximum over all strategies of their centred mean period return, computed on
the device from the [S, B] period records (`gte_bootstrap_weights`, `gte_reality_check`, include/gte.h).  It says
whether the best of S tries is better than what luck alone gives the best of S tries."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .strategy_records import mask_words


def bootstrap_weights(env, n, n_resamples, block=1.0, seed=0):
    """The resampling weights of the stationary bootstrap (Politis & Romano) over `n` positions with mean block
    length `block` >= 1: a torch f64 tensor [n_resamples, n] on the env's device; entry [r, i] is how many times
    position i is drawn in resample r, every row sums to n.  The same (n, n_resamples, block, seed) give the same
    bits on every run (`gte_bootstrap_weights`).  Enqueued on the env's stream; nothing waits."""
    torch = env._torch
    if torch is None:
        raise ValueError("bootstrap weights need output='torch'")
    for name, v in (("n", n), ("n_resamples", n_resamples), ("seed", seed)):
        if isinstance(v, (bool, float)) or int(v) != v:
            raise TypeError(f"{name} must be an integer")
    if not 2 <= int(n) <= _abi.GTE_MAX_PERIODS:
        raise ValueError(f"n must lie in [2, {_abi.GTE_MAX_PERIODS}]")
    if not 1 <= int(n_resamples) <= _abi.GTE_BOOT_MAX_RESAMPLES:
        raise ValueError(f"n_resamples must lie in [1, {_abi.GTE_BOOT_MAX_RESAMPLES}]")
    if not float(block) >= 1.0:
        raise ValueError("block must be >= 1.0")
    dev = env._t["obs"].device
    with torch.cuda.device(dev):
        w = torch.empty((int(n_resamples), int(n)), dtype=torch.float64, device=dev)
    _abi.check(env._lib, env._lib.gte_bootstrap_weights(env._h, int(n), int(n_resamples), float(block),
                                                        int(seed) & (2 ** 64 - 1), C.c_void_p(w.data_ptr())))
    return w


class RealityCheck:
    """The result of `StrategyPeriodStats.reality_check()`.

    Device tensors, none of which waits: ``mean`` f64 [S] (the mean period return of each strategy over the
    selected periods, less the benchmark's; NaN for a strategy that is not eligible), ``std_error`` f64 [S] (the
    deviation of its bootstrap distribution), ``p_individual`` f64 [S] (its naive p-value, selection ignored),
    ``p_adjusted`` f64 [S] (its single-step adjusted p-value: the share of resamples whose maximum over ALL
    strategies reaches its mean), ``eligible`` bool [S], ``max_stats`` f64 [R] and ``max_index`` int32 [R] (the
    maximum of every resample and the strategy that attained it).  ``boot_sum``, ``boot_sq_sum``, ``count_ge`` and
    ``count_adj`` are the raw sums and counts of the library.

    ``p_value`` (the Reality Check p-value of the leaderboard: `p_adjusted` of the best strategy), ``best`` (its
    index, -1 when no strategy is eligible) and ``best_mean`` are read from the device's summary record: these
    three wait for the device, once.  ``num_resamples``, ``periods`` (the selected period ids) and ``weights`` (the
    [R, n] table that was used) describe the call."""

    def __init__(self, env, periods, weights, out, keep):
        self._env, self._keep = env, keep   # every tensor the launches read, alive with the result
        self.periods = list(periods)
        self.weights = weights
        self.num_resamples = R = int(weights.shape[0])
        self.mean, self.boot_sum, self.boot_sq_sum = out["mean"], out["boot_sum"], out["boot_sq_sum"]
        self.count_ge, self.count_adj = out["count_ge"], out["count_adj"]
        self.max_stats, self.max_index = out["max_stat"], out["max_index"]
        self._summary_dev, self._summary = out["summary"], None
        torch = env._torch
        owner = keep[0]  # eligible: stepped in every selected period, every period return finite (include/gte.h)
        self.eligible = (owner.steps[:, self.periods] > 0).all(dim=1) & \
            torch.isfinite(owner.reward_sum[:, self.periods]).all(dim=1)
        # (divided by a DEVICE scalar: torch turns a division by a host scalar into a multiplication by its
        # reciprocal, which is not count / R to the last bit)
        Rt = torch.full((), float(R), dtype=torch.float64, device=self.mean.device)
        m1 = self.boot_sum / Rt
        self.std_error = torch.sqrt(torch.clamp(self.boot_sq_sum / Rt - m1 * m1, min=0.0))
        nan = torch.full_like(self.mean, float("nan"))
        self.p_individual = torch.where(self.eligible, self.count_ge.to(torch.float64) / Rt, nan)
        self.p_adjusted = torch.where(self.eligible, self.count_adj.to(torch.float64) / Rt, nan)

    def _read(self):
        if self._summary is None:
            raw = self._summary_dev.cpu().numpy()
            self._summary = raw.view(np.dtype(_abi.REALITY_CHECK_SUMMARY_DTYPE))[0]
        return self._summary

    @property
    def best(self) -> int:
        return int(self._read()["best"])

    @property
    def best_mean(self) -> float:
        return float(self._read()["best_mean"])

    @property
    def num_eligible(self) -> int:
        return int(self._read()["eligible"])

    @property
    def p_value(self) -> float:
        """count_rc / R: the share of resamples whose maximum reaches the best strategy's mean; NaN when no
        strategy is eligible."""
        s = self._read()
        return float(s["count_rc"]) / self.num_resamples if int(s["best"]) >= 0 else float("nan")

    def numpy(self) -> dict:
        """Everything on the host: the arrays above by name, and the summary's scalars."""
        out = {k: getattr(self, k).cpu().numpy() for k in (
            "mean", "std_error", "p_individual", "p_adjusted", "eligible", "max_stats", "max_index", "boot_sum",
            "boot_sq_sum", "count_ge", "count_adj")}
        s = self._read()
        out.update(best=int(s["best"]), best_mean=float(s["best_mean"]), count_rc=int(s["count_rc"]),
                   num_eligible=int(s["eligible"]), p_value=self.p_value, num_resamples=self.num_resamples,
                   periods=list(self.periods))
        return out


def run(owner, periods=None, n_resamples=1000, block=1.0, seed=0, benchmark=None, weights=None) -> RealityCheck:
    """`StrategyPeriodStats.reality_check`: stage the arguments, enqueue the launches, wait for nothing."""
    env, torch = owner._env, owner._env._torch
    mask = owner._mask(periods)
    ids = [int(b) for b in np.flatnonzero(mask)]
    n = len(ids)
    if n < 2:
        raise ValueError("a reality check needs at least two selected periods")
    words = mask_words(mask)
    dev = owner._records.device
    S, B = owner.num_strategies, owner.num_periods
    if weights is None:
        weights = bootstrap_weights(env, n, n_resamples, block, seed)
    else:
        if not hasattr(weights, "is_cuda"):
            weights = torch.from_numpy(np.ascontiguousarray(np.asarray(weights, dtype=np.float64)))
        weights = weights.to(device=dev, dtype=torch.float64).contiguous()
        if weights.dim() != 2 or weights.shape[1] != n or not 1 <= weights.shape[0] <= _abi.GTE_BOOT_MAX_RESAMPLES:
            raise ValueError(f"weights must have shape [R, {n}] with 1 <= R <= {_abi.GTE_BOOT_MAX_RESAMPLES}, "
                             f"not {tuple(weights.shape)}")
    R = int(weights.shape[0])
    bench = None
    if benchmark is not None:
        if not hasattr(benchmark, "is_cuda"):
            benchmark = torch.from_numpy(np.ascontiguousarray(np.asarray(benchmark, dtype=np.float64)))
        bench = benchmark.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(bench.shape) != (B,):
            raise ValueError(f"benchmark must have shape ({B},), not {tuple(bench.shape)}")
    with torch.cuda.device(dev):
        out = {k: torch.empty((S,), dtype=torch.float64, device=dev) for k in ("mean", "boot_sum", "boot_sq_sum")}
        out.update({k: torch.empty((S,), dtype=torch.int32, device=dev) for k in ("count_ge", "count_adj")})
        out["max_stat"] = torch.empty((R,), dtype=torch.float64, device=dev)
        out["max_index"] = torch.empty((R,), dtype=torch.int32, device=dev)
        out["summary"] = torch.empty((C.sizeof(_abi.GteRealityCheckSummary),), dtype=torch.uint8, device=dev)
    # (the env launches on torch's current stream as it was when the env was made: the copies above are ordered
    # with the launches, as in StrategyStats)
    ptrs = _abi.GteRealityCheckOut(**{k: v.data_ptr() for k, v in out.items()})
    _abi.check(env._lib, env._lib.gte_reality_check(
        env._h, C.c_void_p(owner._records.data_ptr()), S, B, words, None if bench is None else C.c_void_p(bench.data_ptr()),
        C.c_void_p(weights.data_ptr()), R, C.byref(ptrs)))
    return RealityCheck(env, ids, weights, out, (owner, bench, weights))
