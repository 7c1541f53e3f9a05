"""BacktestStats — what `BatchedTradingEnv.backtest` returns: the per-env statistics records of
libgte (struct gte_backtest_stats, include/gte.h) as torch views of device memory, and the few
figures a backtest is read for, derived from them on the device when first asked for."""
from __future__ import annotations

import numpy as np

from . import _abi


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
        from .batched import _device_view
        self._env = env
        self._derived = {}
        dev = env._t["obs"].device
        stride = np.dtype(_abi.BACKTEST_DTYPE).itemsize
        offsets = np.dtype(_abi.BACKTEST_DTYPE).fields
        for name, typestr in _abi.BACKTEST_FIELDS:
            setattr(self, name, _device_view(ptr + offsets[name][1], (env.num_envs,), typestr, dev, (stride,)))

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

    def numpy(self) -> np.ndarray:
        """The whole record array on the host, one transfer: a structured array [N] with the
        record's field names (`gte_read_backtest_stats`)."""
        e = self._env
        out = np.empty(e.num_envs, dtype=np.dtype(_abi.BACKTEST_DTYPE))
        _abi.check(e._lib, e._lib.gte_read_backtest_stats(e._h, 0, e.num_envs, out.ctypes.data))
        return out
