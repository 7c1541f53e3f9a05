"""PeriodStats — the statistics of a backtest split by market period (`BacktestStats.period_stats`, kept while
`BatchedTradingEnv.track_periods` is on): the per-(env, period) records of libgte (struct gte_period_stats,
include/gte.h) as torch views of device memory; and StrategyPeriodStats, the same folded per strategy and ranked
over any subset of the periods on the device — rank on the training periods, read the same strategies on the
test periods."""
from __future__ import annotations

import numpy as np

from . import _abi
from .strategy_records import StrategyRecords, field_views, mask_words, resolve_strategy_map


class PeriodStats:
    """Per-env, per-period statistics.

    Every field of the record is an attribute (``reward_sum``, ``reward_sq_sum``, ``steps``, ``trades``,
    ``episodes``): a torch tensor [N, B] that is a strided VIEW of the env's records, so it shows the next
    ``backtest(..., resume=True)`` as well — clone what has to outlive it.

    The records live until `track_periods()` is called with another `n_periods`: the library then frees them
    and allocates new ones.  From then on this object is STALE — every field, `numpy()` and `by_strategy()`
    raise `RuntimeError` instead of touching freed memory.  (A field tensor taken out of the object before
    that is a raw view like any other and is the caller's to drop.)"""

    FIELDS = tuple(n for n, _ in _abi.PERIOD_FIELDS)

    def __init__(self, env, ptr: int, n_periods: int, generation: int, strategy_map=None):
        self._env = env
        self._ptr, self._generation = int(ptr), int(generation)  # which allocation of the env's these records are
        self._map = strategy_map  # what the call that made these records ran with
        self._views = {}
        self.num_periods = int(n_periods)
        self._alive()

    def _alive(self):
        """Raise unless the env's period records are still the allocation this object was made over."""
        e = self._env
        if e._period_generation != self._generation or e._period_records != (self._ptr, self.num_periods):
            raise RuntimeError(
                f"these period statistics ({self.num_periods} periods) are stale: track_periods() has since been "
                "called with another n_periods, which freed their records (clone the fields or take .numpy() "
                "before changing the period count)")

    def __getattr__(self, name):  # the record's fields: views made on first use, checked on every use
        if name.startswith("_") or name not in self.FIELDS:
            raise AttributeError(name)
        self._alive()
        if name not in self._views:
            e = self._env
            self._views.update(field_views(self._ptr, [(name, dict(_abi.PERIOD_FIELDS)[name])], _abi.PERIOD_DTYPE,
                                           (e.num_envs, self.num_periods), e._t["obs"].device))
        return self._views[name]

    def numpy(self) -> np.ndarray:
        """The whole record array on the host, one transfer: a structured array [N, B] of `PERIOD_DTYPE`
        (`gte_read_period_stats`)."""
        self._alive()  # the read copies the live records' B per env: `out` is sized for it only while they are ours
        e = self._env
        out = np.empty((e.num_envs, self.num_periods), dtype=np.dtype(_abi.PERIOD_DTYPE))
        _abi.check(e._lib, e._lib.gte_read_period_stats(e._h, 0, e.num_envs, out.ctypes.data))
        return out

    def by_strategy(self, strategy=None, n_strategies=None) -> "StrategyPeriodStats":
        """These records folded into one record per (strategy, period), on the device
        (`gte_reduce_period_stats`): a `StrategyPeriodStats`.  `strategy` / `n_strategies` and their defaults —
        the map and the S of the `backtest_signals()` call that produced the records — are those of
        `BacktestStats.by_strategy`; like there, what is folded is what the live records hold when this runs."""
        self._alive()
        strategy, n_strategies = resolve_strategy_map(self._map, strategy, n_strategies)
        return StrategyPeriodStats._reduce(self._env, strategy, n_strategies, self.num_periods)


class PeriodSelection:
    """What `StrategyPeriodStats.select(periods)` gives: the pooled figures of the selected periods per
    strategy, [S] tensors on the device — ``steps``, ``reward_sum``, ``mean_reward`` and ``sharpe()``, as
    `gte_rank_period_stats` scores them."""

    def __init__(self, owner, mask):
        self._owner, self._mask = owner, mask
        self.periods = [b for b in range(owner.num_periods) if mask[b]]

    @property
    def steps(self):
        o = self._owner
        return o.steps[:, self.periods].sum(dim=1) if self.periods else o.steps.new_zeros((o.num_strategies,))

    @property
    def reward_sum(self):
        return self._owner.score("reward_sum", self._mask)

    @property
    def mean_reward(self):
        return self._owner.score("mean_reward", self._mask)

    def sharpe(self, periods_per_year=None):
        """mean / population deviation of the pooled step rewards of the selected periods, annualised by
        sqrt(periods_per_year) when given."""
        s = self._owner.score("sharpe", self._mask)
        return s if periods_per_year is None else s * float(periods_per_year) ** 0.5


class StrategyPeriodStats(StrategyRecords):
    """Per-strategy, per-period statistics: the period records of a `PeriodStats` folded over the members of
    each strategy by one device launch (struct gte_strategy_period_stats, include/gte.h), and the ranking of the
    strategies by a score over a subset of the periods, also on the device (`gte_rank_period_stats`).

    Every field of the record is an attribute (``reward_sum``, ``reward_sq_sum``, ``steps``, ``trades``,
    ``episodes``, ``envs_stepped``): a torch tensor [S, B] that is a strided view of the result records, which
    this object owns.  ``reward_sum`` is the [S, B] matrix of period returns everything further starts from.
    `periods` is an iterable of period ids, a bool mask [B], or None for all periods.  Launches are enqueued on
    the env's stream as in `StrategyStats`; `top()` alone waits."""

    DTYPE, RECORD_FIELDS = _abi.STRATEGY_PERIOD_DTYPE, _abi.STRATEGY_PERIOD_FIELDS
    FIELDS = tuple(n for n, _ in RECORD_FIELDS)
    METRICS, METRIC_PREFIX = _abi.PERIOD_METRICS, "PERIOD_METRIC"
    REDUCE, RANK = "gte_reduce_period_stats", "gte_rank_period_stats"

    def __init__(self, env, records, n_periods, inputs=()):
        self.num_periods = B = int(n_periods)
        super().__init__(env, records, inputs, (int(records.shape[0]) // B, B))  # records: uint8 [S * B, 48], CUDA

    @classmethod
    def _reduce(cls, env, strategy, n_strategies, n_periods):
        out, inputs = cls._fold(env, None, strategy, n_strategies, n_periods, (n_periods,))
        return cls(env, out, n_periods, inputs)

    def _mask(self, periods):
        """bool [B] on the host from an iterable of ids, a bool mask [B], or None (all)."""
        B = self.num_periods
        if periods is None:
            return np.ones(B, dtype=bool)
        if isinstance(periods, np.ndarray) and periods.dtype == bool or \
                (hasattr(periods, "dtype") and str(periods.dtype) == "torch.bool"):
            m = np.asarray(periods.cpu() if hasattr(periods, "cpu") else periods, dtype=bool)
            if m.shape != (B,):
                raise ValueError(f"a period mask must have shape ({B},), not {m.shape}")
            return m.copy()
        ids = [int(b) for b in (periods.tolist() if hasattr(periods, "tolist") else periods)]
        m = np.zeros(B, dtype=bool)
        for b in ids:
            if not 0 <= b < B:
                raise IndexError(f"period {b} outside [0, {B})")
            m[b] = True
        return m

    def _selected(self, periods, at_least=0, refusal=None):
        """`_mask(periods)` and the ids it selects, ascending; fewer than `at_least` of them: ValueError(refusal)."""
        mask = self._mask(periods)
        ids = [int(b) for b in np.flatnonzero(mask)]
        if len(ids) < at_least:
            raise ValueError(refusal)
        return mask, ids

    def _periods_args(self, periods):
        """What the rank call takes between S and the metric: B and the mask's words, made when it asks."""
        return lambda: (self.num_periods, mask_words(self._mask(periods)))

    def select(self, periods) -> PeriodSelection:
        """The pooled figures of a set of periods per strategy: `steps`, `reward_sum`, `mean_reward`,
        `sharpe()`, each [S]."""
        return PeriodSelection(self, self._mask(periods))

    def score(self, metric, periods=None):
        """The score of every strategy under `metric` (a name of `METRICS` or a `PERIOD_METRIC_*` constant) over
        `periods`, f64 [S] on the device, as `gte_rank_period_stats` computes it — NaN included."""
        code = self._code(metric)
        mask = self._mask(periods)
        return self._lazy(("score", code, mask.tobytes()),
                          lambda: self._rank(code, 1, 1, True, self._periods_args(mask))[2])

    def top(self, k, metric="sharpe", periods=None, min_steps=1):
        """The k best strategies over `periods`: ``(index int32 [r], score f64 [r])`` on the device, best first,
        r = min(k, ranked strategies).  Ranked are those with at least max(1, `min_steps`) transitions in the
        selected periods and a score that is not NaN; equal scores order by index.  Waits for the device, like
        `StrategyStats.top`."""
        return self._top(metric, min_steps, k, self._periods_args(periods))

    def reality_check(self, periods=None, n_resamples=1000, block=1.0, seed=0, benchmark=None, weights=None):
        """White's Reality Check of this leaderboard over `periods`, on the device (`gte_reality_check`): is the
        best strategy's mean period return better than what luck alone gives the best of S tries?  A
        `RealityCheck`.  `n_resamples` resamples of the stationary bootstrap with mean block length `block`
        (in periods) and `seed` — the same arguments give the same bits; `weights` (NumPy or torch, [R, n] for n
        selected periods) overrides the generated table; `benchmark` (NumPy or torch, [B]) is subtracted period by
        period, e.g. buy-and-hold's period returns.  A strategy counts only if it stepped in every selected period
        and all its period returns are finite.  Nothing here waits for the device."""
        from . import reality_check
        return reality_check.run(self, periods, n_resamples, block, seed, benchmark, weights)

    def spa(self, periods=None, n_resamples=1000, block=1.0, seed=0, benchmark=None, weights=None, alpha=0.05,
            max_rounds=8, threshold=None):
        """Hansen's test for Superior Predictive Ability of this leaderboard over `periods` and its step-down, on the
        device (`gte_spa_test`): the Reality Check studentised, so that poor but noisy strategies do not blind it,
        and WHICH strategies beat the benchmark at family-wise level `alpha`.  A `SpaTest`, which carries the
        `RealityCheck` of the same weights.  `periods`, `n_resamples`, `block`, `seed`, `benchmark` and `weights` as
        in `reality_check`; at most `max_rounds` rounds of step-down; `threshold`: a strategy whose t-statistic is
        below -threshold does not contribute to the null (None: Hansen's sqrt(2 log log n), which needs at least
        three periods).  Enqueued on the env's stream; nothing waits."""
        from . import spa
        return spa.run(self, periods, n_resamples, block, seed, benchmark, weights, alpha, max_rounds, threshold)


    def cscv(self, periods=None, groups=None, metric="sharpe", splits=None):
        """The probability of backtest overfitting of this leaderboard by combinatorially symmetric
        cross-validation over `periods`, on the device (`gte_cscv`): across every split of the period groups into
        an in-sample and an out-of-sample half, how often does the in-sample winner land in the lower half out of
        sample?  An `OverfitCheck`.  `groups`: an int G (the selected periods cut into G contiguous groups,
        `periods.cscv_groups`), a uint64 table [G, 2] of group masks (then `periods` is not used), or None for the
        largest even G <= min(selected periods, 16).  `splits=(is_groups, oos_groups)`, two uint32 arrays [C] with
        bit g = group g, overrides the generated table of all G/2-subsets (`periods.cscv_splits`) — purged splits,
        a walk-forward scheme.  `metric`: "sharpe", "mean_reward" or "reward_sum".  A strategy counts only if it
        stepped in every group and all its group sums are finite.  Nothing here waits for the device."""
        from . import overfit
        return overfit.run(self, periods, groups, metric, splits)

    def diversified(self, k, metric="sharpe", periods=None, max_corr=0.7, min_steps=1, corr_periods=None, scores=None):
        """A decorrelated leaderboard of at most `k` strategies, picked greedily on the device (`gte_diversify`):
        the best strategy, everything whose period returns correlate with it above `max_corr` dropped, the best of
        what is left, and so on.  A `Diversified`: the picks, the size of the cluster each one removed, which pick
        removed every strategy, and — once no candidate is left — the number of independent strategies the sweep
        held at this threshold.  The score is `score(metric, periods)`, with NaN for a strategy with fewer than
        max(1, `min_steps`) transitions in `periods`: the candidates are the strategies `top()` ranks, less those
        that did not step in every correlation period or whose period returns there are constant or not finite.
        `scores` (NumPy or torch, f64 [S]; NaN = no candidate) overrides the metric — a trade metric, a negated
        p-value.  The correlations are taken over `corr_periods` (default: `periods`), at least three.  The signed
        correlation decides: a mirror strategy hedges the pick and stays.  The default `max_corr` of 0.7 is a
        convention, not a finding; `effective_trials` moves with it.  Nothing here waits for the device."""
        from . import diversify
        return diversify.run(self, k, metric, periods, max_corr, min_steps, corr_periods, scores)
