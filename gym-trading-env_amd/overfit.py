"""OverfitCheck — what `StrategyPeriodStats.cscv()` gives: the probability of backtest overfitting (PBO) of a
strategy leaderboard by combinatorially symmetric cross-validation (Bailey, Borwein, Lopez de Prado, Zhu), computed
on the device from the [S, B] period records (`gte_cscv`, include/gte.h).  The periods are cut into groups; every
split takes some groups as in-sample and others as out-of-sample, picks the in-sample winner and looks where it
ranks out of sample among all strategies.  It says how much the SELECTION overfits: a winner that is as likely to
land in the lower half out of sample as in the upper one was picked for its luck."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, periods as period_rows
from .strategy_records import LeaderboardResult, make_outputs, metric_code


class OverfitCheck(LeaderboardResult):
    """The result of `StrategyPeriodStats.cscv()`.

    Device tensors over the C splits, none of which waits: ``best`` int32 (the in-sample winner, -1 when no
    strategy could win), ``is_score`` and ``oos_score`` f64 (its score on the two sides), ``ranked`` int32 (the
    eligible strategies with an out-of-sample score that is not NaN), ``below`` and ``equal`` int32 (how many of
    those score below the winner out of sample, and the same as it, itself included), ``valid`` bool (a winner
    with an out-of-sample score), ``rel_rank`` f64 (the winner's mid-rank relative rank
    w = (below + (equal + 1) / 2) / (ranked + 1), NaN where the split is not valid) and ``logit`` f64
    (ln(w / (1 - w)): negative where the winner lands in the lower half).

    ``pbo`` (overfit / valid: the share of valid splits with w <= 1/2), ``prob_loss`` (loss / valid: the share whose
    winner has a negative out-of-sample score), ``num_valid`` and ``num_eligible`` are read from the device's summary
    record: these wait for the device, once; the two shares are NaN without a valid split.  ``num_splits``,
    ``metric``, ``groups`` (the [G, 2] mask table), ``is_groups`` and ``oos_groups`` (the split tables, host) describe
    the call."""

    SUMMARY_DTYPE = _abi.CSCV_SUMMARY_DTYPE
    ARRAYS = ("best", "is_score", "oos_score", "below", "equal", "ranked", "valid", "rel_rank", "logit")

    def __init__(self, env, metric, groups, is_groups, oos_groups, out, keep):
        super().__init__(env, out, keep)
        self.metric = _abi.PERIOD_METRICS[metric]
        self.groups, self.is_groups, self.oos_groups = groups, is_groups, oos_groups
        self.num_groups, self.num_splits = int(groups.shape[0]), int(is_groups.shape[0])
        self.best, self.is_score, self.oos_score = out["best"], out["is_score"], out["oos_score"]
        self.below, self.equal, self.ranked = out["below"], out["equal"], out["ranked"]
        torch = env._torch
        f64 = torch.float64
        self.valid = (self.best >= 0) & ~torch.isnan(self.oos_score)
        w = (self.below.to(f64) + (self.equal.to(f64) + 1.0) / 2.0) / (self.ranked.to(f64) + 1.0)
        self.rel_rank = torch.where(self.valid, w, torch.full_like(w, float("nan")))
        self.logit = torch.log(self.rel_rank / (1.0 - self.rel_rank))

    @property
    def num_valid(self) -> int:
        return int(self._read()["valid"])

    @property
    def num_eligible(self) -> int:
        return int(self._read()["eligible"])

    @property
    def pbo(self) -> float:
        """overfit / valid: the probability of backtest overfitting; NaN without a valid split."""
        s = self._read()
        return float(s["overfit"]) / float(s["valid"]) if int(s["valid"]) > 0 else float("nan")

    @property
    def prob_loss(self) -> float:
        """loss / valid: the share of valid splits whose winner scores below zero out of sample; NaN without one."""
        s = self._read()
        return float(s["loss"]) / float(s["valid"]) if int(s["valid"]) > 0 else float("nan")

    def degradation(self):
        """The performance-degradation line: ``(slope, intercept)`` of the least-squares line of `oos_score` on
        `is_score` over the valid splits whose two scores are finite, computed in torch on the device
        (slope = sum (x - mx)(y - my) / sum (x - mx)^2, intercept = my - slope * mx) and read back as two floats.
        NaN with fewer than two such splits or when their in-sample scores are all the same."""
        torch = self._env._torch
        x, y = self.is_score, self.oos_score
        use = self.valid & torch.isfinite(x) & torch.isfinite(y)
        zero = torch.zeros_like(x)
        n = use.sum().to(torch.float64)
        mx, my = torch.where(use, x, zero).sum() / n, torch.where(use, y, zero).sum() / n
        dx, dy = torch.where(use, x - mx, zero), torch.where(use, y - my, zero)
        slope = (dx * dy).sum() / (dx * dx).sum()
        slope = torch.where(n >= 2.0, slope, torch.full_like(slope, float("nan")))
        both = torch.stack((slope, my - slope * mx)).cpu()
        return float(both[0]), float(both[1])

    def _scalars(self) -> dict:
        s = self._read()
        return dict(pbo=self.pbo, prob_loss=self.prob_loss, num_valid=int(s["valid"]), num_overfit=int(s["overfit"]),
                    num_loss=int(s["loss"]), num_eligible=int(s["eligible"]), num_splits=self.num_splits,
                    num_groups=self.num_groups, metric=self.metric)


def _table(a, dtype, what):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    a = np.asarray(a)
    if a.dtype.kind not in "iu" or (a.size and int(a.min()) < 0):
        raise TypeError(f"{what} must hold unsigned integers")
    return np.ascontiguousarray(a.astype(dtype))


def run(owner, periods=None, groups=None, metric="sharpe", splits=None) -> OverfitCheck:
    """`StrategyPeriodStats.cscv`: make the tables, enqueue the launches, wait for nothing."""
    env, torch = owner._env, owner._env._torch
    code = metric_code(metric, _abi.PERIOD_METRICS, "PERIOD_METRIC")
    if _abi.PERIOD_METRICS[code] not in _abi.CSCV_METRICS:
        raise ValueError(f"cscv scores by one of {', '.join(_abi.CSCV_METRICS)}, not {_abi.PERIOD_METRICS[code]}")
    if groups is None or isinstance(groups, (int, np.integer)) and not isinstance(groups, bool):
        _, ids = owner._selected(periods, 2 if groups is None else 0, "cscv needs at least two selected periods")
        if groups is None:
            groups = min(len(ids), 16) // 2 * 2
        table = period_rows.cscv_groups(ids, int(groups))
    else:
        table = _table(groups, np.uint64, "groups")
        if table.ndim != 2 or table.shape[1] != 2 or not 2 <= table.shape[0] <= _abi.GTE_CSCV_MAX_GROUPS:
            raise ValueError(f"groups must have shape [G, 2] with 2 <= G <= {_abi.GTE_CSCV_MAX_GROUPS}, "
                             f"not {tuple(table.shape)}")
    G = int(table.shape[0])
    if splits is None:
        is_groups, oos_groups = period_rows.cscv_splits(G)
    else:
        is_groups, oos_groups = (_table(a, np.uint32, "splits") for a in splits)
        if is_groups.ndim != 1 or is_groups.shape != oos_groups.shape or \
                not 1 <= is_groups.shape[0] <= _abi.GTE_CSCV_MAX_SPLITS:
            raise ValueError(f"splits must be two arrays [C] with 1 <= C <= {_abi.GTE_CSCV_MAX_SPLITS}")
    n_splits = int(is_groups.shape[0])
    dev = owner._records.device
    S, B = owner.num_strategies, owner.num_periods
    spec = [(name, torch.int32, n_splits) for name in ("best", "below", "equal", "ranked")] + \
           [(name, torch.float64, n_splits) for name in ("is_score", "oos_score")]
    out, ptrs = make_outputs(torch, dev, spec, _abi.GteCscvOut, _abi.GteCscvSummary)
    # (the library copies the three host tables before it returns; the env launches on torch's current stream as it
    # was when the env was made, as in StrategyStats)
    _abi.check(env._lib, env._lib.gte_cscv(
        env._h, C.c_void_p(owner._records.data_ptr()), S, B, C.c_void_p(table.ctypes.data), G,
        C.c_void_p(is_groups.ctypes.data), C.c_void_p(oos_groups.ctypes.data), n_splits, code, C.byref(ptrs)))
    return OverfitCheck(env, code, table, is_groups, oos_groups, out, (owner,))
