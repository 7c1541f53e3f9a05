"""TradeStats — the round-trip trade statistics of a backtest (`BacktestStats.trade_stats`, kept while
`BatchedTradingEnv.track_trades` is on): the per-env records of libgte (struct gte_trade_stats,
include/gte.h) as torch views of device memory and the figures a backtest report gives per trade; and
StrategyTradeStats, the same folded per strategy and ranked on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .backtest_stats import StrategyStats


class TradeStats:
    """Per-env trade statistics, one value per env and field.

    Every field of the record is an attribute (``open_value``, ``open_position``, ``last_valuation``,
    ``gross_profit``, ``gross_loss``, ``ret_sq_sum``, ``best_trade``, ``worst_trade``, ``exposure``,
    ``hold_sum``, ``closed``, ``wins``, ``losses``, ``forced``, ``reversals``, ``dropped``, ``open_len``,
    ``max_len``, ``loss_streak``, ``max_loss_streak``): a torch tensor [N] that is a strided VIEW of the
    env's records, so it shows the next ``backtest(..., resume=True)`` as well — clone what has to outlive
    it.  The derived figures are computed once per object and call."""

    FIELDS = tuple(n for n, _ in _abi.TRADE_FIELDS)

    def __init__(self, env, ptr: int, steps, strategy_map=None):
        from .batched import _device_view
        self._env = env
        self._derived = {}
        self._steps = steps      # the transitions of the same records' gte_backtest_stats (exposure_share)
        self._map = strategy_map  # what the call that made these records ran with
        dev = env._t["obs"].device
        dt = np.dtype(_abi.TRADE_DTYPE)
        for name, typestr in _abi.TRADE_FIELDS:
            setattr(self, name, _device_view(ptr + dt.fields[name][1], (env.num_envs,), typestr, dev, (dt.itemsize,)))

    def _lazy(self, key, make):
        if key not in self._derived:
            self._derived[key] = make()
        return self._derived[key]

    @property
    def win_rate(self):
        """wins / closed per env (NaN where no trade closed)."""
        return self._lazy("win_rate", lambda: self.wins.double() / self.closed.double())

    @property
    def profit_factor(self):
        """gross_profit / -gross_loss per env (inf without a losing trade, NaN without any)."""
        return self._lazy("profit_factor", lambda: self.gross_profit / (0.0 - self.gross_loss))

    @property
    def expectancy(self):
        """Mean return of a closed trade per env."""
        return self._lazy("expectancy", lambda: (self.gross_profit + self.gross_loss) / self.closed.double())

    @property
    def mean_hold(self):
        """Mean number of transitions a closed trade was held."""
        return self._lazy("mean_hold", lambda: self.hold_sum.double() / self.closed.double())

    @property
    def exposure_share(self):
        """exposure / steps: the share of its transitions the env spent inside a trade."""
        return self._lazy("exposure_share", lambda: self.exposure.double() / self._steps.double())

    def numpy(self) -> np.ndarray:
        """The whole record array on the host, one transfer: a structured array [N] of `TRADE_DTYPE`
        (`gte_read_trade_stats`)."""
        e = self._env
        out = np.empty(e.num_envs, dtype=np.dtype(_abi.TRADE_DTYPE))
        _abi.check(e._lib, e._lib.gte_read_trade_stats(e._h, 0, e.num_envs, out.ctypes.data))
        return out

    def by_strategy(self, strategy=None, n_strategies=None) -> "StrategyTradeStats":
        """These records folded into one record per strategy, on the device (`gte_reduce_trade_stats`): a
        `StrategyTradeStats`.  `strategy` / `n_strategies` and their defaults — the map and the S of the
        `backtest_signals()` call that produced the records — are those of `BacktestStats.by_strategy`; like
        there, what is folded is what the live records hold when this runs."""
        if strategy is None and n_strategies is None:
            if self._map is None:
                raise ValueError("by_strategy() of a backtest() result needs n_strategies (and strategy=, unless "
                                 "env e follows strategy (env_id_base + e) % S)")
            strategy, n_strategies = self._map
        elif n_strategies is None:
            if self._map is None:
                raise ValueError("by_strategy(strategy=...) needs n_strategies")
            n_strategies = self._map[1]
        return StrategyTradeStats._reduce(self._env, strategy, n_strategies)


def _trade_metric_code(metric) -> int:
    if isinstance(metric, str):
        if metric.lower() not in _abi.TRADE_METRICS:
            raise ValueError(f"unknown metric {metric!r}: one of {', '.join(_abi.TRADE_METRICS)}")
        return _abi.TRADE_METRICS.index(metric.lower())
    if isinstance(metric, (bool, float)) or int(metric) != metric:
        raise TypeError("metric must be a name or a TRADE_METRIC_* constant")
    if not 0 <= int(metric) < len(_abi.TRADE_METRICS):
        raise ValueError(f"unknown metric {metric}: 0 .. {len(_abi.TRADE_METRICS) - 1}")
    return int(metric)


class StrategyTradeStats:
    """Per-strategy trade statistics: the trade records of a `TradeStats` folded over the members of each
    strategy by one device launch (struct gte_strategy_trade_stats, include/gte.h), and the ranking of the
    strategies by a per-trade score, also on the device (`gte_rank_trade_stats`).

    Every field of the record is an attribute (``closed``, ``wins``, ``losses``, ``forced``, ``reversals``,
    ``exposure``, ``hold_sum``, ``gross_profit``, ``gross_loss``, ``ret_sq_sum``, ``best_trade``,
    ``worst_trade``, ``max_len``, ``max_loss_streak``, ``envs``, ``envs_traded``): a torch tensor [S] that is a
    strided view of the result records, which this object owns.  Launches are enqueued on the env's stream as
    in `StrategyStats`; `top()` alone waits."""

    FIELDS = tuple(n for n, _ in _abi.STRATEGY_TRADE_FIELDS)
    METRICS = _abi.TRADE_METRICS

    def __init__(self, env, records, inputs=()):
        from .batched import _device_view
        self._env = env
        self._records = records  # uint8 [S, 128], CUDA
        self._keep = inputs      # what the reduction reads: alive while the launch may be in flight
        self._derived = {}
        self.num_strategies = int(records.shape[0])
        dt = np.dtype(_abi.STRATEGY_TRADE_DTYPE)
        for name, typestr in _abi.STRATEGY_TRADE_FIELDS:
            setattr(self, name, _device_view(records.data_ptr() + dt.fields[name][1], (self.num_strategies,), typestr,
                                             records.device, (dt.itemsize,)))

    @classmethod
    def _reduce(cls, env, strategy, n_strategies):
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
            out = torch.empty((S, 128), dtype=torch.uint8, device=dev)
        _abi.check(env._lib, env._lib.gte_reduce_trade_stats(
            env._h, None, S, None if offsets is None else C.c_void_p(offsets.data_ptr()),
            None if members is None else C.c_void_p(members.data_ptr()), C.c_void_p(out.data_ptr())))
        return cls(env, out, (offsets, members))

    def _lazy(self, key, make):
        if key not in self._derived:
            self._derived[key] = make()
        return self._derived[key]

    def _rank(self, metric, min_trades, k, want_scores):
        env, torch = self._env, self._env._torch
        code = _trade_metric_code(metric)
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= _abi.GTE_RANK_MAX:
            raise ValueError(f"k must lie in [1, {_abi.GTE_RANK_MAX}]")
        dev = self._records.device
        with torch.cuda.device(dev):
            index = torch.empty((int(k),), dtype=torch.int32, device=dev)
            top = torch.empty((int(k),), dtype=torch.float64, device=dev)
            scores = torch.empty((self.num_strategies,), dtype=torch.float64, device=dev) if want_scores else None
        _abi.check(env._lib, env._lib.gte_rank_trade_stats(
            env._h, C.c_void_p(self._records.data_ptr()), self.num_strategies, code, int(min_trades), int(k),
            C.c_void_p(index.data_ptr()), C.c_void_p(top.data_ptr()),
            None if scores is None else C.c_void_p(scores.data_ptr())))
        return index, top, scores

    def score(self, metric):
        """The score of every strategy under `metric` (a name of `METRICS` or a `TRADE_METRIC_*` constant), f64
        [S] on the device, as `gte_rank_trade_stats` computes it — NaN included."""
        code = _trade_metric_code(metric)
        return self._lazy(("score", code), lambda: self._rank(code, 1, 1, True)[2])

    def top(self, k, metric="profit_factor", min_trades=1):
        """The k best strategies: ``(index int32 [r], score f64 [r])`` on the device, best first, r = min(k,
        ranked strategies).  Ranked are those with at least max(1, `min_trades`) closed trades and a score that
        is not NaN; equal scores order by index.  Waits for the device, like `StrategyStats.top`."""
        index, top, _ = self._rank(metric, min_trades, k, False)
        r = int((index >= 0).sum().item())
        return index[:r], top[:r]

    def numpy(self) -> np.ndarray:
        """The records on the host, one transfer: a structured array [S] of `STRATEGY_TRADE_DTYPE`."""
        raw = self._records.cpu().numpy()
        return raw.view(np.dtype(_abi.STRATEGY_TRADE_DTYPE)).reshape(self.num_strategies).copy()
