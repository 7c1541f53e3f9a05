"""BacktestStats — what `BatchedTradingEnv.backtest` returns: the per-env statistics records of
libgte (struct gte_backtest_stats, include/gte.h) as torch views of device memory, and the few
figures a backtest is read for, derived from them on the device when first asked for."""
from __future__ import annotations

import numpy as np

from . import _abi
from .strategy_records import StrategyRecords, field_views, metric_code, resolve_strategy_map


class BacktestStats:
    """Per-env running statistics of a backtest, one value per env and field.

    Every field of the record is an attribute (``steps``, ``reward_sum``, ``reward_sq_sum``,
    ``peak``, ``max_drawdown``, ``cur_return``, ``ep_return_sum``, ``ep_return_sq_sum``,
    ``valuation_last``, ``prev_position``, ``trades``, ``episodes``, ``terminations``): a torch
    tensor [N] that is a strided VIEW of the env's records, so it shows the next
    ``backtest(..., resume=True)`` as well — clone what has to outlive it.  The derived figures
    are computed once per object and call."""

    FIELDS = tuple(n for n, _ in _abi.BACKTEST_FIELDS)

    def __init__(self, env, ptr: int):
        self._env = env
        self._derived = {}
        self._map = getattr(env, "_backtest_map", None)  # what the call that made these records ran with
        self._trades_ptr = getattr(env, "_trades_ptr", 0)  # the trade records, if that call kept them
        # (address, B, generation) of the period records, if that call kept them
        self._periods = getattr(env, "_periods", None)
        vars(self).update(field_views(ptr, _abi.BACKTEST_FIELDS, _abi.BACKTEST_DTYPE, (env.num_envs,),
                                      env._t["obs"].device))

    def _lazy(self, key, make):
        if key not in self._derived:
            self._derived[key] = make()
        return self._derived[key]

    @property
    def mean_reward(self):
        """Mean step reward per env (NaN where the env made no transition)."""
        return self._lazy("mean_reward", lambda: self.reward_sum / self.steps)

    @property
    def reward_std(self):
        """Population standard deviation of the step reward per env."""
        def make():
            var = self.reward_sq_sum / self.steps - self.mean_reward ** 2
            return var.clamp_min(0.0).sqrt()
        return self._lazy("reward_std", make)

    def sharpe(self, periods_per_year=None):
        """mean_reward / reward_std, annualised by sqrt(periods_per_year) when given."""
        s = self._lazy("sharpe", lambda: self.mean_reward / self.reward_std)
        return s if periods_per_year is None else s * float(periods_per_year) ** 0.5

    @property
    def mean_episode_return(self):
        """Mean over the finished episodes of their summed reward (NaN where none finished)."""
        return self._lazy("mean_episode_return", lambda: self.ep_return_sum / self.episodes)

    @property
    def total_return(self):
        """exp(reward_sum): the factor the portfolio value was multiplied by over all transitions.
        Only a sum of log returns says that: the plain and the scaled log-return rewards."""
        kind = self._env.cfg.reward_kind
        if kind == _abi.REWARD_LOG_RETURN:
            return self._lazy("total_return", lambda: self.reward_sum.exp())
        if kind == _abi.REWARD_SCALED_LOG_RETURN:
            return self._lazy("total_return", lambda: (self.reward_sum / self._env.cfg.reward_param0).exp())
        raise ValueError("total_return = exp(reward_sum) needs a log-return reward (basic_reward_function or "
                         "scaled_log_return): the sum of clipped rewards is not the log of a return")

    @property
    def trade_stats(self):
        """The round-trip trade statistics of the same transitions, a `TradeStats` — or None when the call
        that made these records ran with trade tracking off (`BatchedTradingEnv.track_trades`)."""
        if not self._trades_ptr:
            return None
        from .trade_stats import TradeStats
        return self._lazy("trade_stats", lambda: TradeStats(self._env, self._trades_ptr, self.steps, self._map))

    @property
    def period_stats(self):
        """The same transitions split by market period, a `PeriodStats` with fields [N, B] — or None when the
        call that made these records ran with period tracking off (`BatchedTradingEnv.track_periods`)."""
        if not self._periods:
            return None
        from .period_stats import PeriodStats
        return self._lazy("period_stats", lambda: PeriodStats(self._env, *self._periods, self._map))

    def numpy(self) -> np.ndarray:
        """The whole record array on the host, one transfer: a structured array [N] with the
        record's field names (`gte_read_backtest_stats`)."""
        e = self._env
        out = np.empty(e.num_envs, dtype=np.dtype(_abi.BACKTEST_DTYPE))
        _abi.check(e._lib, e._lib.gte_read_backtest_stats(e._h, 0, e.num_envs, out.ctypes.data))
        return out

    def by_strategy(self, strategy=None, n_strategies=None) -> "StrategyStats":
        """These records folded into one record per strategy, on the device (`gte_reduce_backtest_stats`):
        a `StrategyStats`.  The defaults are the map and the S of the `backtest_signals()` call that
        produced this object; for the result of `backtest()` pass `n_strategies` (env e then belongs to
        strategy ``(env_id_base + e) % S``) or `strategy` (int32 [N], host or CUDA) with `n_strategies`.
        The sums are taken in the fixed order include/gte.h states: the same records give the same bits.

        This object is a live VIEW of the env's records: what is folded is what they hold when `by_strategy()`
        runs, so after a later `backtest()` / `backtest_signals()` it folds that call's records — while the
        default map and S stay those captured when this object was made.  Fold first, or pass the later
        call's `strategy` / `n_strategies`.  The launch is enqueued on the env's stream (see `StrategyStats`)."""
        strategy, n_strategies = resolve_strategy_map(self._map, strategy, n_strategies)
        return StrategyStats._reduce(self._env, None, strategy, n_strategies)


def _metric_code(metric) -> int:
    return metric_code(metric, _abi.STRATEGY_METRICS, "METRIC")


class StrategyStats(StrategyRecords):
    """Per-strategy statistics of a backtest: the env records of a `BacktestStats` folded over the
    members of each strategy by one device launch (struct gte_strategy_stats, include/gte.h), and the
    ranking of the strategies by a score, also on the device (`gte_rank_strategies`).

    Every field of the record is an attribute (``steps``, ``reward_sum``, ``reward_sq_sum``,
    ``ep_return_sum``, ``ep_return_sq_sum``, ``max_drawdown``, ``best_reward_sum``,
    ``worst_reward_sum``, ``trades``, ``episodes``, ``terminations``, ``envs``, ``envs_stepped``): a
    torch tensor [S] that is a strided view of the result records, which this object owns.

    Like `signal_actions()`, every call here enqueues its launches on the env's stream — torch's current
    stream when the env was made — and returns without waiting for the device: torch work on that stream is
    ordered with them, and the object keeps the records, the member lists and the result alive meanwhile.  An
    env moved to another stream (`gte_set_stream`) is the caller's to order.  `top()` alone waits: it trims
    its result to the number of ranked strategies, which it reads back (`numpy()` is a transfer)."""

    DTYPE, RECORD_FIELDS = _abi.STRATEGY_DTYPE, _abi.STRATEGY_FIELDS
    FIELDS = tuple(n for n, _ in RECORD_FIELDS)
    METRICS, METRIC_PREFIX = _abi.STRATEGY_METRICS, "METRIC"
    REDUCE, RANK = "gte_reduce_backtest_stats", "gte_rank_strategies"

    def __init__(self, env, records, inputs=()):
        super().__init__(env, records, inputs, (int(records.shape[0]),))  # records: uint8 [S, 128], CUDA

    # -- construction ---------------------------------------------------------------------------
    @classmethod
    def _reduce(cls, env, records, strategy, n_strategies):
        return cls(env, *cls._fold(env, records, strategy, n_strategies))

    @classmethod
    def from_records(cls, env, records, strategy=None, n_strategies=None) -> "StrategyStats":
        """Fold caller-held env records — a `BACKTEST_DTYPE` array [N] (e.g. `BacktestStats.numpy()` saved
        from an earlier chunk) or a contiguous CUDA uint8 [N, 128] tensor — over the strategies of `env`'s
        N envs.  `strategy` / `n_strategies` as in `BacktestStats.by_strategy`; `n_strategies` is required."""
        torch = env._torch
        if torch is None:
            raise ValueError("strategy statistics need output='torch'")
        if n_strategies is None:
            raise ValueError("from_records needs n_strategies")
        N = env.num_envs
        if isinstance(records, torch.Tensor):
            if not records.is_cuda:
                raise ValueError("a records tensor must live on the device (pass a BACKTEST_DTYPE array from the host)")
            if records.dtype != torch.uint8:
                raise TypeError(f"a records tensor is uint8 [N, 128], not {records.dtype}")
            if tuple(records.shape) != (N, 128) or not records.is_contiguous():
                raise ValueError(f"expected a contiguous records tensor of shape ({N}, 128)")
            if records.data_ptr() % 16:
                raise ValueError("records must be 16-byte aligned")
            dev_records = records
        else:
            a = np.asarray(records)
            if a.dtype != np.dtype(_abi.BACKTEST_DTYPE):
                raise TypeError("records must be a BACKTEST_DTYPE array (BacktestStats.numpy()) or a CUDA uint8 tensor")
            if a.shape != (N,):
                raise ValueError(f"expected records of shape ({N},)")
            raw = np.ascontiguousarray(a).view(np.uint8).reshape(N, 128)
            dev_records = torch.from_numpy(raw.copy()).to(env._t["obs"].device)
        return cls._reduce(env, dev_records, strategy, n_strategies)

    # -- figures ---------------------------------------------------------------------------------
    @property
    def mean_reward(self):
        """Mean step reward over all transitions of the strategy's envs."""
        return self._lazy("mean_reward", lambda: self.reward_sum / self.steps)

    @property
    def reward_std(self):
        """Population standard deviation of the pooled step rewards."""
        def make():
            var = self.reward_sq_sum / self.steps - self.mean_reward ** 2
            return var.clamp_min(0.0).sqrt()
        return self._lazy("reward_std", make)

    def sharpe(self, periods_per_year=None):
        """mean_reward / reward_std of the pooled step rewards, annualised by sqrt(periods_per_year)."""
        s = self.score("sharpe")
        return s if periods_per_year is None else s * float(periods_per_year) ** 0.5

    @property
    def mean_episode_return(self):
        """Mean return of the finished episodes of the strategy's envs (NaN where none finished)."""
        return self._lazy("mean_episode_return", lambda: self.ep_return_sum / self.episodes)

    @property
    def episode_return_std(self):
        """Population standard deviation of the finished episodes' returns."""
        def make():
            var = self.ep_return_sq_sum / self.episodes - self.mean_episode_return ** 2
            return var.clamp_min(0.0).sqrt()
        return self._lazy("episode_return_std", make)

    def score(self, metric):
        """The score of every strategy under `metric` (a name of `METRICS` or a `METRIC_*` constant), f64
        [S] on the device, as `gte_rank_strategies` computes it — NaN included."""
        code = self._code(metric)
        return self._lazy(("score", code), lambda: self._rank(code, 0, 1, True)[2])

    def top(self, k, metric="mean_episode_return", min_episodes=1):
        """The k best strategies: ``(index int32 [r], score f64 [r])`` on the device, best first, r = min(k,
        ranked strategies).  Ranked are those with at least one transition, at least `min_episodes`
        finished episodes and a score that is not NaN; equal scores order by index.  Waits for the device: the
        ranked count is read back to trim the result (`gte_rank_strategies` itself does not wait and pads with
        -1 / NaN)."""
        return self._top(metric, min_episodes, k)
