"""What the record families of a backtest share — the per-env records (`BacktestStats`, `TradeStats`,
`PeriodStats`, `ExitState`) and their per-strategy folds (`StrategyStats`, `StrategyTradeStats`,
`StrategyPeriodStats`): metric names, the default strategy map, the member lists of an explicit map, the field
views, the period mask's two words, and `StrategyRecords`, the base of the three folds.  And what the analyses of
a leaderboard share (reality_check.py, overfit.py, diversify.py): the staging of their arguments and outputs and
`LeaderboardResult`, the base of their results."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi


def metric_code(metric, names, prefix) -> int:
    """`metric`, a name of `names` in either case or its index (the `<prefix>_*` constants), as the index."""
    if isinstance(metric, str):
        if metric.lower() not in names:
            raise ValueError(f"unknown metric {metric!r}: one of {', '.join(names)}")
        return names.index(metric.lower())
    if isinstance(metric, (bool, float)) or int(metric) != metric:
        raise TypeError(f"metric must be a name or a {prefix}_* constant")
    if not 0 <= int(metric) < len(names):
        raise ValueError(f"unknown metric {metric}: 0 .. {len(names) - 1}")
    return int(metric)


def resolve_strategy_map(captured_map, strategy, n_strategies):
    """`by_strategy()`'s arguments against the (strategy, S) of the `backtest_signals()` call that made the
    records, None after a `backtest()`: the (strategy, n_strategies) to fold with."""
    if strategy is None and n_strategies is None:
        if captured_map is None:
            raise ValueError("by_strategy() of a backtest() result needs n_strategies (and strategy=, unless "
                             "env e follows strategy (env_id_base + e) % S)")
        return captured_map
    if n_strategies is None:
        if captured_map is None:
            raise ValueError("by_strategy(strategy=...) needs n_strategies")
        n_strategies = captured_map[1]
    return strategy, n_strategies


def strategy_groups(env, strategy, S):
    """An explicit map int32 [N] -> the CSR lists of the gte_reduce_* calls, built on the device:
    members by increasing env id (a stable sort of the map), offsets by searchsorted."""
    torch = env._torch
    dev = env._t["obs"].device
    if isinstance(strategy, torch.Tensor) and strategy.is_cuda:
        if strategy.dtype not in (torch.int32, torch.int64):
            raise TypeError("strategy must be integers")
        m = strategy
    else:
        a = np.asarray(strategy.numpy() if isinstance(strategy, torch.Tensor) else strategy)
        if a.dtype.kind not in "iu":
            raise TypeError("strategy must be integers")
        if a.size and (a.min() < 0 or a.max() >= S):
            raise IndexError(f"strategy outside [0, {S})")
        m = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64))).to(dev)
    if tuple(m.shape) != (env.num_envs,):
        raise ValueError(f"expected strategy of shape ({env.num_envs},)")
    m = m.to(torch.int64)
    order = torch.sort(m, stable=True).indices
    sorted_map = m[order]
    # envs whose strategy lies outside [0, S) belong to nobody: offsets[0] skips the negative ones,
    # offsets[S] stops before those >= S
    bounds = torch.arange(S + 1, dtype=torch.int64, device=dev)
    offsets = torch.searchsorted(sorted_map, bounds).to(torch.int32).contiguous()
    return offsets, order.to(torch.int32).contiguous()


def field_views(ptr, fields, dtype, shape, device) -> dict:
    """name -> torch view of that field over the contiguous record array of `shape` at device address `ptr`
    (`fields`: (name, typestr) pairs of the structured `dtype`)."""
    from .batched import _device_view
    dt = np.dtype(dtype)
    strides = tuple(dt.itemsize * int(np.prod(shape[i + 1:])) for i in range(len(shape)))
    return {name: _device_view(ptr + dt.fields[name][1], tuple(shape), typestr, device, strides)
            for name, typestr in fields}


def mask_words(mask):
    """A bool mask over the periods as the two words of the libgte calls: bit b & 63 of word b >> 6 = period b."""
    words = (C.c_uint64 * 2)(0, 0)
    for b in np.flatnonzero(mask):
        words[int(b) >> 6] |= 1 << (int(b) & 63)
    return words


def _ptr(tensor):
    return None if tensor is None else C.c_void_p(tensor.data_ptr())


def is_int_in(value, lo, hi, floats=True) -> bool:
    """Is `value` an integer in [lo, hi]?  A bool is none, nor a float with a fraction — nor any float, unless
    `floats`.  What to raise, and in which words, is the caller's."""
    if isinstance(value, bool) or (isinstance(value, float) and not floats):
        return False
    return int(value) == value and lo <= int(value) <= hi


def f64_on(torch, dev, values, fits, expected):
    """`values`, NumPy or torch, as a contiguous f64 tensor on `dev`.  `fits(shape)` says whether its shape will
    do; one that will not is refused as "`expected`, not (shape)"."""
    if not hasattr(values, "is_cuda"):
        values = torch.from_numpy(np.ascontiguousarray(np.asarray(values, dtype=np.float64)))
    values = values.to(device=dev, dtype=torch.float64).contiguous()
    if not fits(tuple(values.shape)):
        raise ValueError(f"{expected}, not {tuple(values.shape)}")
    return values


def make_outputs(torch, dev, spec, out_struct, summary_struct):
    """What a leaderboard analysis writes: a tensor on `dev` for every (name, dtype, length) of `spec` and the bytes
    of its summary record, by name, and the `out_struct` of their addresses the libgte call takes."""
    with torch.cuda.device(dev):
        out = {name: torch.empty((length,), dtype=dtype, device=dev) for name, dtype, length in spec}
        out["summary"] = torch.empty((C.sizeof(summary_struct),), dtype=torch.uint8, device=dev)
    return out, out_struct(**{name: t.data_ptr() for name, t in out.items()})


class LeaderboardResult:
    """Base of what the analyses of a leaderboard give (`RealityCheck`, `OverfitCheck`, `Diversified`): the tensors
    the launches read, kept alive with the result, and the device's summary record, read once and only when a scalar
    is asked for.  A result states SUMMARY_DTYPE (its summary record), ARRAYS (the tensor attributes `numpy()`
    brings to the host) and `_scalars()` (what `numpy()` adds to them)."""

    def __init__(self, env, out, keep):
        self._env, self._keep = env, keep   # every tensor the launches read, alive with the result
        self._summary_dev, self._summary = out["summary"], None

    def _read(self):
        if self._summary is None:
            raw = self._summary_dev.cpu().numpy()
            self._summary = raw.view(np.dtype(self.SUMMARY_DTYPE))[0]
        return self._summary

    def numpy(self) -> dict:
        """Everything on the host: the arrays above by name, and the summary's scalars."""
        out = {name: getattr(self, name).cpu().numpy() for name in self.ARRAYS}
        out.update(self._scalars())
        return out


class StrategyRecords:
    """Result records of a per-strategy fold, owned by the object, and their ranking on the device.  A family
    states DTYPE and RECORD_FIELDS (its record), METRICS and METRIC_PREFIX, and REDUCE and RANK (its libgte
    calls); its constructor passes the shape of the record array, (S,) or (S, B)."""

    def __init__(self, env, records, inputs, shape):
        self._env = env
        self._records = records  # uint8 [records, record bytes], CUDA
        self._keep = inputs      # what the reduction reads: alive while the launch may be in flight
        self._derived = {}
        self._shape = shape
        self.num_strategies = shape[0]
        vars(self).update(field_views(records.data_ptr(), self.RECORD_FIELDS, self.DTYPE, shape, records.device))

    @classmethod
    def _fold(cls, env, records, strategy, n_strategies, per_strategy=1, extra=()):
        """The family's reduce call over `records` (None: the env's own): the result array, `per_strategy`
        records for each strategy, and what it reads.  `extra`: the call's arguments between the records and S."""
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
            offsets, members = strategy_groups(env, strategy, S)
        with torch.cuda.device(dev):
            out = torch.empty((S * per_strategy, np.dtype(cls.DTYPE).itemsize), dtype=torch.uint8, device=dev)
        _abi.check(env._lib, getattr(env._lib, cls.REDUCE)(env._h, _ptr(records), *extra, S, _ptr(offsets),
                                                           _ptr(members), _ptr(out)))
        return out, (records, offsets, members)

    def _lazy(self, key, make):
        if key not in self._derived:
            self._derived[key] = make()
        return self._derived[key]

    def _code(self, metric) -> int:
        return metric_code(metric, self.METRICS, self.METRIC_PREFIX)

    def _rank(self, metric, minimum, k, want_scores, extra=tuple):
        """The family's rank call: (index int32 [k], score f64 [k], scores f64 [S] or None).  `extra()`, made once
        metric and k have passed: the call's arguments between S and the metric."""
        env, torch = self._env, self._env._torch
        code = self._code(metric)
        if not is_int_in(k, 1, _abi.GTE_RANK_MAX):
            raise ValueError(f"k must lie in [1, {_abi.GTE_RANK_MAX}]")
        between = extra()
        dev = self._records.device
        with torch.cuda.device(dev):
            index = torch.empty((int(k),), dtype=torch.int32, device=dev)
            top = torch.empty((int(k),), dtype=torch.float64, device=dev)
            scores = torch.empty((self.num_strategies,), dtype=torch.float64, device=dev) if want_scores else None
        _abi.check(env._lib, getattr(env._lib, self.RANK)(
            env._h, _ptr(self._records), self.num_strategies, *between, code, int(minimum), int(k), _ptr(index),
            _ptr(top), _ptr(scores)))
        return index, top, scores

    def _top(self, metric, minimum, k, extra=tuple):
        """`top()`: the ranking trimmed to the ranked strategies, whose count is read back."""
        index, top, _ = self._rank(metric, minimum, k, False, extra)
        r = int((index >= 0).sum().item())
        return index[:r], top[:r]

    def numpy(self) -> np.ndarray:
        """The records on the host, one transfer: a structured array of the family's record dtype, [S] or
        [S, B]."""
        raw = self._records.cpu().numpy()
        return raw.view(np.dtype(self.DTYPE)).reshape(self._shape).copy()
