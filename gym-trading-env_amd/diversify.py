"""Diversified — what `StrategyPeriodStats.diversified()` gives: a decorrelated leaderboard picked greedily on the
device from the [S, B] period records (`gte_diversify`, include/gte.h).  The best strategy by score, everything whose
period returns correlate with it above `max_corr` dropped, the best of what is left, and so on: the picks are a
shortlist of different bets, what a pick dropped is its cluster, and once nothing is left the number of picks is the
number of independent strategies the sweep held at that threshold."""
from __future__ import annotations

import ctypes as C

from . import _abi
from .strategy_records import LeaderboardResult, f64_on, is_int_in, make_outputs, mask_words


class Diversified(LeaderboardResult):
    """The result of `StrategyPeriodStats.diversified()`.

    Device tensors, none of which waits: ``picks`` int32 [k] (the strategy picked in every round, -1 from the round
    on in which no candidate was left), ``scores`` f64 [k] (its score, NaN beside a -1), ``cluster_size`` int32 [k]
    (how many candidates the round removed, the pick included), ``owner`` int32 [S] (the round that removed each
    strategy; -1 for a candidate no round removed, -2 for a strategy that was no candidate: not stepped in every
    correlation period, a period return that is not finite, a constant row, or a NaN score), ``owner_corr`` f64 [S]
    (its correlation with the pick that removed it, NaN where ``owner`` < 0) and ``corr`` f64 [k, k] (the correlations
    of the picks with one another, NaN beside a -1).

    ``num_picked``, ``num_candidates``, ``num_eligible`` and ``remaining`` (the candidates still there after the
    last round) are read from the device's summary record: these wait for the device, once.  ``exhausted`` is
    ``remaining == 0``; ``effective_trials`` is then ``num_picked``, the number of clusters at this threshold, and
    None while candidates remain.  ``k``, ``max_corr`` and ``corr_periods`` (the period ids the correlations are
    taken over) describe the call."""

    SUMMARY_DTYPE = _abi.DIVERSIFY_SUMMARY_DTYPE
    ARRAYS = ("picks", "scores", "cluster_size", "owner", "owner_corr", "corr")

    def __init__(self, env, k, max_corr, corr_periods, out, keep):
        super().__init__(env, out, keep)
        self.k, self.max_corr, self.corr_periods = int(k), float(max_corr), list(corr_periods)
        self.picks, self.scores, self.cluster_size = out["pick"], out["pick_score"], out["cluster_size"]
        self.owner, self.owner_corr = out["owner"], out["owner_corr"]
        self.corr = out["pick_corr"].view(self.k, self.k)

    @property
    def num_picked(self) -> int:
        return int(self._read()["picked"])

    @property
    def num_candidates(self) -> int:
        return int(self._read()["candidates"])

    @property
    def num_eligible(self) -> int:
        return int(self._read()["eligible"])

    @property
    def remaining(self) -> int:
        return int(self._read()["remaining"])

    @property
    def exhausted(self) -> bool:
        return self.remaining == 0

    @property
    def effective_trials(self):
        """`num_picked` once every candidate belongs to a cluster, else None: with candidates left the count is
        only a lower bound."""
        return self.num_picked if self.exhausted else None

    def members(self, r):
        """The strategies round `r` removed — the pick and what correlated with it above `max_corr` — as an int64
        index tensor on the device, ascending."""
        if isinstance(r, bool) or int(r) != r or not 0 <= int(r) < self.k:
            raise IndexError(f"round {r} outside [0, {self.k})")
        return (self.owner == int(r)).nonzero().flatten()

    def _scalars(self) -> dict:
        return dict(num_picked=self.num_picked, num_candidates=self.num_candidates, num_eligible=self.num_eligible,
                    remaining=self.remaining, exhausted=self.exhausted, effective_trials=self.effective_trials,
                    k=self.k, max_corr=self.max_corr, corr_periods=list(self.corr_periods))


def run(owner, k, metric="sharpe", periods=None, max_corr=0.7, min_steps=1, corr_periods=None, scores=None) -> Diversified:
    """`StrategyPeriodStats.diversified`: stage the arguments, enqueue the launches, wait for nothing."""
    env, torch = owner._env, owner._env._torch
    if not is_int_in(k, 1, _abi.GTE_RANK_MAX):
        raise ValueError(f"k must lie in [1, {_abi.GTE_RANK_MAX}]")
    k = int(k)
    max_corr = float(max_corr)
    if max_corr != max_corr:
        raise ValueError("max_corr must not be NaN")
    mask, ids = owner._selected(periods if corr_periods is None else corr_periods, 3,
                                "a correlation needs at least three selected periods")
    dev = owner._records.device
    S, B = owner.num_strategies, owner.num_periods
    if scores is None:
        pooled, pooled_ids = owner._selected(periods)
        scores = owner.score(metric, pooled)
        steps = owner.steps[:, pooled_ids].sum(dim=1)
        scores = torch.where(steps >= max(1, int(min_steps)), scores, torch.full_like(scores, float("nan")))
    else:
        scores = f64_on(torch, dev, scores, lambda s: s == (S,), f"scores must have shape ({S},)")
    f64, i32 = torch.float64, torch.int32
    out, ptrs = make_outputs(torch, dev, (("pick", i32, k), ("pick_score", f64, k), ("cluster_size", i32, k),
                                          ("owner", i32, S), ("owner_corr", f64, S), ("pick_corr", f64, k * k)),
                             _abi.GteDiversifyOut, _abi.GteDiversifySummary)
    # (the env launches on torch's current stream as it was when the env was made: the tensors made above are
    # ordered with the launches, as in StrategyStats)
    _abi.check(env._lib, env._lib.gte_diversify(
        env._h, C.c_void_p(owner._records.data_ptr()), S, B, mask_words(mask), C.c_void_p(scores.data_ptr()), max_corr, k,
        C.byref(ptrs)))
    return Diversified(env, k, max_corr, ids, out, (owner, scores))
