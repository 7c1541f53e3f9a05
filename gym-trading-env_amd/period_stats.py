"""PeriodStats — the statistics of a backtest split by market period (`BacktestStats.period_stats`, kept while
`BatchedTradingEnv.track_periods` is on): the per-(env, period) records of libgte (struct gte_period_stats,
include/gte.h) as torch views of device memory; and StrategyPeriodStats, the same folded per strategy and ranked
over any subset of the periods on the device — rank on the training periods, read the same strategies on the
test periods."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .backtest_stats import StrategyStats


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
            from .batched import _device_view
            e, B, dt = self._env, self.num_periods, np.dtype(_abi.PERIOD_DTYPE)
            typestr = dict(_abi.PERIOD_FIELDS)[name]
            self._views[name] = _device_view(self._ptr + dt.fields[name][1], (e.num_envs, B), typestr,
                                             e._t["obs"].device, (B * dt.itemsize, dt.itemsize))
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
        if strategy is None and n_strategies is None:
            if self._map is None:
                raise ValueError("by_strategy() of a backtest() result needs n_strategies (and strategy=, unless "
                                 "env e follows strategy (env_id_base + e) % S)")
            strategy, n_strategies = self._map
        elif n_strategies is None:
            if self._map is None:
                raise ValueError("by_strategy(strategy=...) needs n_strategies")
            n_strategies = self._map[1]
        return StrategyPeriodStats._reduce(self._env, strategy, n_strategies, self.num_periods)


def _period_metric_code(metric) -> int:
    if isinstance(metric, str):
        if metric.lower() not in _abi.PERIOD_METRICS:
            raise ValueError(f"unknown metric {metric!r}: one of {', '.join(_abi.PERIOD_METRICS)}")
        return _abi.PERIOD_METRICS.index(metric.lower())
    if isinstance(metric, (bool, float)) or int(metric) != metric:
        raise TypeError("metric must be a name or a PERIOD_METRIC_* constant")
    if not 0 <= int(metric) < len(_abi.PERIOD_METRICS):
        raise ValueError(f"unknown metric {metric}: 0 .. {len(_abi.PERIOD_METRICS) - 1}")
    return int(metric)


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


class StrategyPeriodStats:
    """Per-strategy, per-period statistics: the period records of a `PeriodStats` folded over the members of
    each strategy by one device launch (struct gte_strategy_period_stats, include/gte.h), and the ranking of the
    strategies by a score over a subset of the periods, also on the device (`gte_rank_period_stats`).

    Every field of the record is an attribute (``reward_sum``, ``reward_sq_sum``, ``steps``, ``trades``,
    ``episodes``, ``envs_stepped``): a torch tensor [S, B] that is a strided view of the result records, which
    this object owns.  ``reward_sum`` is the [S, B] matrix of period returns everything further starts from.
    `periods` is an iterable of period ids, a bool mask [B], or None for all periods.  Launches are enqueued on
    the env's stream as in `StrategyStats`; `top()` alone waits."""

    FIELDS = tuple(n for n, _ in _abi.STRATEGY_PERIOD_FIELDS)
    METRICS = _abi.PERIOD_METRICS

    def __init__(self, env, records, n_periods, inputs=()):
        from .batched import _device_view
        self._env = env
        self._records = records  # uint8 [S * B, 48], CUDA
        self._keep = inputs      # what the reduction reads: alive while the launch may be in flight
        self._derived = {}
        self.num_periods = B = int(n_periods)
        self.num_strategies = S = int(records.shape[0]) // B
        dt = np.dtype(_abi.STRATEGY_PERIOD_DTYPE)
        for name, typestr in _abi.STRATEGY_PERIOD_FIELDS:
            setattr(self, name, _device_view(records.data_ptr() + dt.fields[name][1], (S, B), typestr, records.device,
                                             (B * dt.itemsize, dt.itemsize)))

    @classmethod
    def _reduce(cls, env, strategy, n_strategies, n_periods):
        torch = env._torch
        if torch is None:
            raise ValueError("strategy statistics need output='torch'")
        if isinstance(n_strategies, bool) or int(n_strategies) != n_strategies:
            raise TypeError("n_strategies must be an integer")
        S = int(n_strategies)
        if S < 1:
            raise ValueError("n_strategies must be >= 1")
        dev = env._t["obs"].device
        offsets = members = None
        if strategy is not None:
            offsets, members = StrategyStats._groups(env, strategy, S)
        with torch.cuda.device(dev):
            out = torch.empty((S * n_periods, 48), dtype=torch.uint8, device=dev)
        _abi.check(env._lib, env._lib.gte_reduce_period_stats(
            env._h, None, n_periods, S, None if offsets is None else C.c_void_p(offsets.data_ptr()),
            None if members is None else C.c_void_p(members.data_ptr()), C.c_void_p(out.data_ptr())))
        return cls(env, out, n_periods, (offsets, members))

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

    def _rank(self, metric, periods, min_steps, k, want_scores):
        env, torch = self._env, self._env._torch
        code = _period_metric_code(metric)
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= _abi.GTE_RANK_MAX:
            raise ValueError(f"k must lie in [1, {_abi.GTE_RANK_MAX}]")
        mask = self._mask(periods)
        words = (C.c_uint64 * 2)(0, 0)
        for b in np.flatnonzero(mask):
            words[int(b) >> 6] |= 1 << (int(b) & 63)
        dev = self._records.device
        with torch.cuda.device(dev):
            index = torch.empty((int(k),), dtype=torch.int32, device=dev)
            top = torch.empty((int(k),), dtype=torch.float64, device=dev)
            scores = torch.empty((self.num_strategies,), dtype=torch.float64, device=dev) if want_scores else None
        _abi.check(env._lib, env._lib.gte_rank_period_stats(
            env._h, C.c_void_p(self._records.data_ptr()), self.num_strategies, self.num_periods, words, code,
            int(min_steps), int(k), C.c_void_p(index.data_ptr()), C.c_void_p(top.data_ptr()),
            None if scores is None else C.c_void_p(scores.data_ptr())))
        return index, top, scores

    def select(self, periods) -> PeriodSelection:
        """The pooled figures of a set of periods per strategy: `steps`, `reward_sum`, `mean_reward`,
        `sharpe()`, each [S]."""
        return PeriodSelection(self, self._mask(periods))

    def score(self, metric, periods=None):
        """The score of every strategy under `metric` (a name of `METRICS` or a `PERIOD_METRIC_*` constant) over
        `periods`, f64 [S] on the device, as `gte_rank_period_stats` computes it — NaN included."""
        code = _period_metric_code(metric)
        mask = self._mask(periods)
        return self._lazy(("score", code, mask.tobytes()), lambda: self._rank(code, mask, 1, 1, True)[2])

    def _lazy(self, key, make):
        if key not in self._derived:
            self._derived[key] = make()
        return self._derived[key]

    def top(self, k, metric="sharpe", periods=None, min_steps=1):
        """The k best strategies over `periods`: ``(index int32 [r], score f64 [r])`` on the device, best first,
        r = min(k, ranked strategies).  Ranked are those with at least max(1, `min_steps`) transitions in the
        selected periods and a score that is not NaN; equal scores order by index.  Waits for the device, like
        `StrategyStats.top`."""
        index, top, _ = self._rank(metric, periods, min_steps, k, False)
        r = int((index >= 0).sum().item())
        return index[:r], top[:r]

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

    def numpy(self) -> np.ndarray:
        """The records on the host, one transfer: a structured array [S, B] of `STRATEGY_PERIOD_DTYPE`."""
        raw = self._records.cpu().numpy()
        return raw.view(np.dtype(_abi.STRATEGY_PERIOD_DTYPE)).reshape(self.num_strategies, self.num_periods).copy()
