"""SpaTest — what `StrategyPeriodStats.spa()` gives: Hansen's test for Superior Predictive Ability of a strategy
leaderboard and its step-down, computed on the device from the [S, B] period records (`gte_spa_test`,
include/gte.h).  The Reality Check studentised: every strategy is measured in its own bootstrap deviation, so that a
poor but noisy strategy no longer widens the null distribution, and the null is recentred so that clearly poor
strategies do not contribute.  The step-down says WHICH strategies beat the benchmark at a family-wise level, not
only whether the best one does."""
from __future__ import annotations

import ctypes as C
import math

from . import _abi
from .reality_check import RealityCheck, bootstrap_weights
from .strategy_records import LeaderboardResult, f64_on, is_int_in, make_outputs, mask_words


def arguments(n, R, alpha, max_rounds, threshold):
    """(threshold, crit_rank, max_rounds) as `gte_spa_test` takes them, for n selected periods and R resamples:
    crit_rank = min(R - 1, max(0, ceil((1 - alpha) * R) - 1)); threshold None = Hansen's sqrt(2 log log n)."""
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("alpha must lie in [0, 1]")
    if not is_int_in(max_rounds, -float("inf"), float("inf"), floats=False):
        raise TypeError("max_rounds must be an integer")
    if not 1 <= int(max_rounds) <= _abi.GTE_SPA_MAX_ROUNDS:
        raise ValueError(f"max_rounds must lie in [1, {_abi.GTE_SPA_MAX_ROUNDS}]")
    if threshold is None:
        if n < 3:
            raise ValueError("the default threshold sqrt(2 log log n) needs at least three selected periods: "
                             "pass threshold=")
        threshold = math.sqrt(2.0 * math.log(math.log(n)))
    if not float(threshold) >= 0.0:
        raise ValueError("threshold must be >= 0 (inf allowed)")
    rank = min(R - 1, max(0, math.ceil((1.0 - float(alpha)) * R) - 1))
    return float(threshold), int(rank), int(max_rounds)


class SpaTest(LeaderboardResult):
    """The result of `StrategyPeriodStats.spa()`.

    Device tensors, none of which waits: ``t_stat`` f64 [S] (mean / std_error; NaN for a strategy that is not
    studentised: not eligible, or a bootstrap deviation of zero), ``std_error`` f64 [S], ``recentred`` bool [S]
    (t_stat >= -threshold: the strategy keeps its mean under the consistent null), ``studentised`` bool [S],
    ``p_adjusted`` f64 [S] (the single-step adjusted p-value, studentised: the share of resamples whose consistent
    maximum reaches t_stat), ``rejected_round`` int32 [S] (the step-down round that rejected the strategy, -1 for
    none) and ``rejected`` bool [S], ``max_stats`` f64 [3, R] and ``max_index`` int32 [3, R] (the maxima of round
    0 under the lower, the consistent and the upper recentring, and who attained them), ``crit`` f64 [max_rounds]
    (the critical value of every round that ran, NaN after) and ``round_rejected`` int32 [max_rounds].
    ``count_adj`` is the raw count of the library.

    ``statistic`` (the largest t_stat, at least 0), ``best`` (its index, -1 when no strategy is studentised),
    ``p_lower``, ``p_consistent`` (= ``p_value``) and ``p_upper`` (Hansen's three p-values; NaN for best == -1),
    ``rounds_run``, ``num_rejected`` and ``num_studentised`` are read from the device's summary record: they wait for
    the device, once.  ``reality_check`` is the `RealityCheck` of the same weights, ``superior()`` the rejected
    strategies.  ``threshold``, ``alpha``, ``crit_rank``, ``max_rounds``, ``num_resamples``, ``periods`` and
    ``weights`` describe the call."""

    SUMMARY_DTYPE = _abi.SPA_SUMMARY_DTYPE
    ARRAYS = ("t_stat", "std_error", "recentred", "studentised", "p_adjusted", "rejected_round", "rejected",
              "max_stats", "max_index", "crit", "round_rejected", "count_adj")

    def __init__(self, env, check, out, keep, threshold, alpha, crit_rank, max_rounds):
        super().__init__(env, out, keep)
        self.reality_check = check
        self.periods, self.weights, self.num_resamples = check.periods, check.weights, check.num_resamples
        self.threshold, self.alpha, self.crit_rank, self.max_rounds = threshold, alpha, crit_rank, max_rounds
        R = self.num_resamples
        torch = env._torch
        self.t_stat, self.std_error, self.count_adj = out["t_stat"], out["std_error"], out["count_adj"]
        self.recentred = out["recentred"] != 0
        self.studentised = check.eligible & torch.isfinite(check.mean) & torch.isfinite(self.std_error) & \
            (self.std_error > 0)
        self.rejected_round = out["rejected_round"]
        self.rejected = self.rejected_round >= 0
        self.max_stats, self.max_index = out["max_stat"].view(3, R), out["max_index"].view(3, R)
        self.crit, self.round_rejected = out["crit"], out["round_rejected"]
        # (divided by a DEVICE scalar, as RealityCheck does: count / R to the last bit)
        Rt = torch.full((), float(R), dtype=torch.float64, device=self.t_stat.device)
        nan = torch.full_like(self.t_stat, float("nan"))
        self.p_adjusted = torch.where(self.studentised, self.count_adj.to(torch.float64) / Rt, nan)

    def _p(self, field) -> float:
        s = self._read()
        return float(s[field]) / self.num_resamples if int(s["best"]) >= 0 else float("nan")

    @property
    def statistic(self) -> float:
        return float(self._read()["statistic"])

    @property
    def best(self) -> int:
        return int(self._read()["best"])

    @property
    def p_lower(self) -> float:
        return self._p("count_lower")

    @property
    def p_consistent(self) -> float:
        return self._p("count_consistent")

    @property
    def p_upper(self) -> float:
        return self._p("count_upper")

    @property
    def p_value(self) -> float:
        """Hansen's consistent p-value, `p_consistent`."""
        return self._p("count_consistent")

    @property
    def rounds_run(self) -> int:
        return int(self._read()["rounds_run"])

    @property
    def num_rejected(self) -> int:
        return int(self._read()["num_rejected"])

    @property
    def num_studentised(self) -> int:
        return int(self._read()["studentised"])

    def superior(self):
        """The indices of the strategies the step-down rejected, ascending: int64 tensor on the device."""
        return self._env._torch.nonzero(self.rejected).reshape(-1)

    def _scalars(self) -> dict:
        return dict(statistic=self.statistic, best=self.best, p_lower=self.p_lower, p_consistent=self.p_consistent,
                    p_upper=self.p_upper, p_value=self.p_value, rounds_run=self.rounds_run,
                    num_rejected=self.num_rejected, num_studentised=self.num_studentised,
                    num_resamples=self.num_resamples, periods=list(self.periods), threshold=self.threshold,
                    alpha=self.alpha, crit_rank=self.crit_rank, max_rounds=self.max_rounds)


def run(owner, periods=None, n_resamples=1000, block=1.0, seed=0, benchmark=None, weights=None, alpha=0.05,
        max_rounds=8, threshold=None) -> SpaTest:
    """`StrategyPeriodStats.spa`: stage the arguments, enqueue the launches, wait for nothing."""
    env, torch = owner._env, owner._env._torch
    mask, ids = owner._selected(periods, 2, "an SPA test needs at least two selected periods")
    n = len(ids)
    dev = owner._records.device
    S, B = owner.num_strategies, owner.num_periods
    if weights is None:
        if not is_int_in(n_resamples, 1, _abi.GTE_BOOT_MAX_RESAMPLES, floats=False):
            raise ValueError(f"n_resamples must be an integer in [1, {_abi.GTE_BOOT_MAX_RESAMPLES}]")
        thr, rank, rounds = arguments(n, int(n_resamples), alpha, max_rounds, threshold)
        weights = bootstrap_weights(env, n, n_resamples, block, seed)
    else:
        most = _abi.GTE_BOOT_MAX_RESAMPLES
        weights = f64_on(torch, dev, weights, lambda s: len(s) == 2 and s[1] == n and 1 <= s[0] <= most,
                         f"weights must have shape [R, {n}] with 1 <= R <= {most}")
        thr, rank, rounds = arguments(n, int(weights.shape[0]), alpha, max_rounds, threshold)
    R = int(weights.shape[0])
    bench = None
    if benchmark is not None:
        bench = f64_on(torch, dev, benchmark, lambda s: s == (B,), f"benchmark must have shape ({B},)")
    f64, i32 = torch.float64, torch.int32
    rc_out, rc_ptrs = make_outputs(torch, dev, (("mean", f64, S), ("boot_sum", f64, S), ("boot_sq_sum", f64, S),
                                                ("count_ge", i32, S), ("count_adj", i32, S), ("max_stat", f64, R),
                                                ("max_index", i32, R)), _abi.GteRealityCheckOut,
                                   _abi.GteRealityCheckSummary)
    out, ptrs = make_outputs(torch, dev, (("t_stat", f64, S), ("std_error", f64, S), ("recentred", torch.uint8, S),
                                          ("count_adj", i32, S), ("rejected_round", i32, S), ("max_stat", f64, 3 * R),
                                          ("max_index", i32, 3 * R), ("crit", f64, rounds),
                                          ("round_rejected", i32, rounds)), _abi.GteSpaOut, _abi.GteSpaSummary)
    _abi.check(env._lib, env._lib.gte_spa_test(
        env._h, C.c_void_p(owner._records.data_ptr()), S, B, mask_words(mask),
        None if bench is None else C.c_void_p(bench.data_ptr()), C.c_void_p(weights.data_ptr()), R, thr, rank, rounds,
        C.byref(rc_ptrs), C.byref(ptrs)))
    keep = (owner, bench, weights)
    check = RealityCheck(env, ids, weights, rc_out, keep)
    return SpaTest(env, check, out, keep + (rc_out,), thr, float(alpha), rank, rounds)
