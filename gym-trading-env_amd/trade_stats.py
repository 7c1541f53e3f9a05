"""TradeStats — the round-trip trade statistics of a backtest (`BacktestStats.trade_stats`, kept while
`BatchedTradingEnv.track_trades` is on): the per-env records of libgte (struct gte_trade_stats,
include/gte.h) as torch views of device memory and the figures a backtest report gives per trade; and
StrategyTradeStats, the same folded per strategy and ranked on the device."""
from __future__ import annotations

import numpy as np

from . import _abi
from .strategy_records import StrategyRecords, field_views, resolve_strategy_map


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
        self._env = env
        self._derived = {}
        self._steps = steps      # the transitions of the same records' gte_backtest_stats (exposure_share)
        self._map = strategy_map  # what the call that made these records ran with
        vars(self).update(field_views(ptr, _abi.TRADE_FIELDS, _abi.TRADE_DTYPE, (env.num_envs,),
                                      env._t["obs"].device))

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

    def trades(self, env_ids=None, strategy=None) -> "TradeList":
        """The per-trade list (`track_trades(list_capacity=...)`) of the envs `env_ids` (any order, repeats allowed;
        None: all envs), or of the member envs of the strategies `strategy` (an id or a sequence of ids, e.g.
        ``by_strategy().top(10)[0]``) under the map of the `backtest_signals()` call that made these records: a
        `TradeList`.  One gather on the device and one transfer (`gte_read_trade_list`); like `numpy()` it reads
        what the live records hold when it runs."""
        from .trade_list import TradeList
        return TradeList._read(self._env, self._map, env_ids, strategy)

    def trades_device(self, env_ids=None, max_trades=None):
        """The same gather with its results left on the device (`gte_pack_trade_list`): ``(first int64 [n + 1],
        closed int32 [n], trades uint8 [n_trades, 48])``; `env_ids`: an int32 CUDA tensor, None for all envs.
        Without `max_trades` the total is read back once to size the block (one wait); with it nothing is waited
        for, the block has `max_trades` records, and ``first[n]`` says how many there were."""
        from .trade_list import pack_trades
        return pack_trades(self._env, env_ids, max_trades)

    def by_strategy(self, strategy=None, n_strategies=None) -> "StrategyTradeStats":
        """These records folded into one record per strategy, on the device (`gte_reduce_trade_stats`): a
        `StrategyTradeStats`.  `strategy` / `n_strategies` and their defaults — the map and the S of the
        `backtest_signals()` call that produced the records — are those of `BacktestStats.by_strategy`; like
        there, what is folded is what the live records hold when this runs."""
        strategy, n_strategies = resolve_strategy_map(self._map, strategy, n_strategies)
        return StrategyTradeStats._reduce(self._env, strategy, n_strategies)


class StrategyTradeStats(StrategyRecords):
    """Per-strategy trade statistics: the trade records of a `TradeStats` folded over the members of each
    strategy by one device launch (struct gte_strategy_trade_stats, include/gte.h), and the ranking of the
    strategies by a per-trade score, also on the device (`gte_rank_trade_stats`).

    Every field of the record is an attribute (``closed``, ``wins``, ``losses``, ``forced``, ``reversals``,
    ``exposure``, ``hold_sum``, ``gross_profit``, ``gross_loss``, ``ret_sq_sum``, ``best_trade``,
    ``worst_trade``, ``max_len``, ``max_loss_streak``, ``envs``, ``envs_traded``): a torch tensor [S] that is a
    strided view of the result records, which this object owns.  Launches are enqueued on the env's stream as
    in `StrategyStats`; `top()` alone waits."""

    DTYPE, RECORD_FIELDS = _abi.STRATEGY_TRADE_DTYPE, _abi.STRATEGY_TRADE_FIELDS
    FIELDS = tuple(n for n, _ in RECORD_FIELDS)
    METRICS, METRIC_PREFIX = _abi.TRADE_METRICS, "TRADE_METRIC"
    REDUCE, RANK = "gte_reduce_trade_stats", "gte_rank_trade_stats"

    def __init__(self, env, records, inputs=()):
        super().__init__(env, records, inputs, (int(records.shape[0]),))  # records: uint8 [S, 128], CUDA

    @classmethod
    def _reduce(cls, env, strategy, n_strategies):
        return cls(env, *cls._fold(env, None, strategy, n_strategies))

    def score(self, metric):
        """The score of every strategy under `metric` (a name of `METRICS` or a `TRADE_METRIC_*` constant), f64
        [S] on the device, as `gte_rank_trade_stats` computes it — NaN included."""
        code = self._code(metric)
        return self._lazy(("score", code), lambda: self._rank(code, 1, 1, True)[2])

    def top(self, k, metric="profit_factor", min_trades=1):
        """The k best strategies: ``(index int32 [r], score f64 [r])`` on the device, best first, r = min(k,
        ranked strategies).  Ranked are those with at least max(1, `min_trades`) closed trades and a score that
        is not NaN; equal scores order by index.  Waits for the device, like `StrategyStats.top`."""
        return self._top(metric, min_trades, k)

    def monte_carlo(self, strategies, n_resamples=1000, n_trades=None, seed=0, ruin=0.5,
                    drawdown_levels=(0.1, 0.2, 0.3, 0.5), keep=("final", "max_drawdown")) -> "TradeMonteCarlo":
        """How bad can these strategies get?  A Monte Carlo over the closed trades of each of `strategies` (ids on
        the host, or an int32 CUDA tensor such as ``top(k)[0]``, which then never visits the host): `n_resamples`
        paths of `n_trades` trades (None: as many as the strategy closed) drawn with replacement from the trade lists
        of its member envs (`track_trades(list_capacity=...)`, the member lists of this fold) and compounded, all on
        the device (`gte_pool_trades`, `gte_trade_monte_carlo`).  `ruin`: the equity level whose touch counts as ruin;
        `drawdown_levels`: the drawdowns whose probability is counted; `keep`: the per-path columns to keep, of
        ``final``, ``max_drawdown``, ``low``, ``max_loss_streak``.  A strategy's paths depend on its id, the seed and
        its trades alone, not on who else was asked for; an id outside [0, S), such as a ranking's -1 padding, gives
        an empty pool.  Like `trades()` it reads what the live lists hold when it runs.  Waits once, for the number
        of trades, to size the block of factors.  Returns a `TradeMonteCarlo`."""
        from .monte_carlo import run
        return run(self, strategies, n_resamples, n_trades, seed, ruin, drawdown_levels, keep)
