"""RealityCheck — what `StrategyPeriodStats.reality_check()` gives: White's Reality Check of a strategy leaderboard,
a bootstrap over time blocks of the maximum over all strategies of their centred mean period return, computed on
the device from the [S, B] period records (`gte_bootstrap_weights`, `gte_reality_check`, include/gte.h).  It says
whether the best of S tries is better than what luck alone gives the best of S tries."""
from __future__ import annotations

import ctypes as C

from . import _abi
from .strategy_records import LeaderboardResult, f64_on, is_int_in, make_outputs, mask_words


def bootstrap_weights(env, n, n_resamples, block=1.0, seed=0):
    """The resampling weights of the stationary bootstrap (Politis & Romano) over `n` positions with mean block
    length `block` >= 1: a torch f64 tensor [n_resamples, n] on the env's device; entry [r, i] is how many times
    position i is drawn in resample r, every row sums to n.  The same (n, n_resamples, block, seed) give the same
    bits on every run (`gte_bootstrap_weights`).  Enqueued on the env's stream; nothing waits."""
    torch = env._torch
    if torch is None:
        raise ValueError("bootstrap weights need output='torch'")
    for name, v in (("n", n), ("n_resamples", n_resamples), ("seed", seed)):
        if not is_int_in(v, -float("inf"), float("inf"), floats=False):
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


class RealityCheck(LeaderboardResult):
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

    SUMMARY_DTYPE = _abi.REALITY_CHECK_SUMMARY_DTYPE
    ARRAYS = ("mean", "std_error", "p_individual", "p_adjusted", "eligible", "max_stats", "max_index", "boot_sum",
              "boot_sq_sum", "count_ge", "count_adj")

    def __init__(self, env, periods, weights, out, keep):
        super().__init__(env, out, keep)
        self.periods = list(periods)
        self.weights = weights
        self.num_resamples = R = int(weights.shape[0])
        self.mean, self.boot_sum, self.boot_sq_sum = out["mean"], out["boot_sum"], out["boot_sq_sum"]
        self.count_ge, self.count_adj = out["count_ge"], out["count_adj"]
        self.max_stats, self.max_index = out["max_stat"], out["max_index"]
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

    def _scalars(self) -> dict:
        s = self._read()
        return dict(best=int(s["best"]), best_mean=float(s["best_mean"]), count_rc=int(s["count_rc"]),
                    num_eligible=int(s["eligible"]), p_value=self.p_value, num_resamples=self.num_resamples,
                    periods=list(self.periods))


def run(owner, periods=None, n_resamples=1000, block=1.0, seed=0, benchmark=None, weights=None) -> RealityCheck:
    """`StrategyPeriodStats.reality_check`: stage the arguments, enqueue the launches, wait for nothing."""
    env, torch = owner._env, owner._env._torch
    mask, ids = owner._selected(periods, 2, "a reality check needs at least two selected periods")
    n = len(ids)
    dev = owner._records.device
    S, B = owner.num_strategies, owner.num_periods
    if weights is None:
        weights = bootstrap_weights(env, n, n_resamples, block, seed)
    else:
        most = _abi.GTE_BOOT_MAX_RESAMPLES
        weights = f64_on(torch, dev, weights, lambda s: len(s) == 2 and s[1] == n and 1 <= s[0] <= most,
                         f"weights must have shape [R, {n}] with 1 <= R <= {most}")
    R = int(weights.shape[0])
    bench = None
    if benchmark is not None:
        bench = f64_on(torch, dev, benchmark, lambda s: s == (B,), f"benchmark must have shape ({B},)")
    f64, i32 = torch.float64, torch.int32
    out, ptrs = make_outputs(torch, dev, (("mean", f64, S), ("boot_sum", f64, S), ("boot_sq_sum", f64, S),
                                          ("count_ge", i32, S), ("count_adj", i32, S), ("max_stat", f64, R),
                                          ("max_index", i32, R)), _abi.GteRealityCheckOut, _abi.GteRealityCheckSummary)
    # (the env launches on torch's current stream as it was when the env was made: the copies above are ordered
    # with the launches, as in StrategyStats)
    _abi.check(env._lib, env._lib.gte_reality_check(
        env._h, C.c_void_p(owner._records.data_ptr()), S, B, mask_words(mask),
        None if bench is None else C.c_void_p(bench.data_ptr()), C.c_void_p(weights.data_ptr()), R, C.byref(ptrs)))
    return RealityCheck(env, ids, weights, out, (owner, bench, weights))
