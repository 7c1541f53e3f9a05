"""TradeList — the per-trade list of a backtest (`TradeStats.trades`, kept while
`BatchedTradingEnv.track_trades(list_capacity=...)` is on): the records of libgte (struct gte_trade, include/gte.h)
of the requested envs, gathered on the device into one dense block and read in one transfer
(`gte_read_trade_list`), with the env, the strategy, the return and the dates of every trade next to them."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi

_RECORD = np.dtype(_abi.TRADE_LIST_DTYPE)


def _host_ids(env, ids, what, bound):
    torch = env._torch
    if torch is not None and isinstance(ids, torch.Tensor):
        ids = ids.detach().cpu().numpy()
    a = np.atleast_1d(np.asarray(ids))
    if a.size and a.dtype.kind not in "iu":
        raise TypeError(f"{what} must be integers")
    a = a.astype(np.int64).reshape(-1)
    if a.size and (a.min() < 0 or a.max() >= bound):
        raise IndexError(f"{what} outside [0, {bound})")
    return a


def strategy_of_envs(env, captured_map):
    """int64 [N]: the strategy every env followed under the (strategy, S) of a `backtest_signals()` call."""
    strategy, S = captured_map
    if strategy is None:
        return (int(env.cfg.env_id_base) + np.arange(env.num_envs, dtype=np.int64)) % int(S)
    torch = env._torch
    if torch is not None and isinstance(strategy, torch.Tensor):
        strategy = strategy.detach().cpu().numpy()
    return np.asarray(strategy).astype(np.int64).reshape(env.num_envs)


class TradeList:
    """The closed trades of the requested envs, in request order and, per env, in close order.

    Per trade (arrays [len(self)]): ``env``; ``strategy`` (None without a strategy map); every field of the record —
    ``open_value``, ``close_value``, ``position``, ``entry_row``, ``exit_row``, ``hold``, ``dataset``, ``kind`` (0
    left to flat, 1 reversal / resize, 2 forced by the episode's end), ``flags`` —; ``ret``, the trade's return
    ``close_value / open_value - 1`` (the bits the trade statistics summed); ``entry_date`` / ``exit_date``, the
    dataset's index at the two rows (None unless every dataset was staged with an index).

    Per request (arrays [n requests]): ``env_ids``, ``closed`` (the env's closed trades since the records were
    cleared), ``first`` ([n + 1]: the trades of request j are ``[first[j], first[j + 1])``) and ``truncated`` —
    the env closed more trades than the list's ``capacity``, which kept the first ones."""

    FIELDS = tuple(n for n, _ in _abi.TRADE_LIST_FIELDS)

    def __init__(self, env, env_ids, first, closed, records, capacity, strategy_of_env=None):
        self.env_ids, self.first, self.closed, self.capacity = env_ids, first, closed, int(capacity)
        self.truncated = closed > self.capacity
        self._records = records
        counts = np.diff(first)
        self.env = np.repeat(env_ids, counts)
        self.strategy = None if strategy_of_env is None else strategy_of_env[self.env]
        for name in self.FIELDS:
            setattr(self, name, np.ascontiguousarray(records[name]))
        with np.errstate(all="ignore"):
            self.ret = self.close_value / self.open_value - np.float64(1.0)
        self.entry_date, self.exit_date = self._dates(env)

    def _dates(self, env):
        datasets = getattr(env, "datasets", None)
        if not datasets or any(getattr(ds, "index", None) is None for ds in datasets):
            return None, None
        index = [np.asarray(ds.index) for ds in datasets]
        if len({i.dtype for i in index}) != 1:
            index = [i.astype(object) for i in index]
        out = []
        for rows in (self.entry_row, self.exit_row):
            col = np.empty(len(rows), dtype=index[0].dtype)
            for d, idx in enumerate(index):
                m = self.dataset == d
                col[m] = idx[np.clip(rows[m], 0, len(idx) - 1)]
            out.append(col)
        # (entry_row lies in the dataset the trade was CLOSED in: an episode never changes its dataset)
        return out[0], out[1]

    @classmethod
    def _read(cls, env, captured_map, env_ids=None, strategy=None):
        if not getattr(env, "_trade_list_capacity", 0):
            raise ValueError("no trade list is kept: track_trades(list_capacity=...) first")
        N = env.num_envs
        of_env = None if captured_map is None else strategy_of_envs(env, captured_map)
        if strategy is not None:
            if env_ids is not None:
                raise ValueError("trades() takes env_ids or strategy, not both")
            if of_env is None:
                raise ValueError("trades(strategy=...) needs the strategy map of a backtest_signals() call")
            wanted = _host_ids(env, strategy, "strategy", int(captured_map[1]))
            parts = [np.flatnonzero(of_env == s) for s in wanted]
            env_ids = np.concatenate(parts) if parts else np.zeros(0, np.int64)
        ids = None if env_ids is None else np.ascontiguousarray(_host_ids(env, env_ids, "env_ids", N).astype(np.int32))
        batch = _abi.GteTradeBatch()
        buf = ids if ids is None or len(ids) else np.zeros(1, np.int32)  # (NULL means all envs: never for no id)
        _abi.check(env._lib, env._lib.gte_read_trade_list(
            env._h, None if ids is None else buf.ctypes.data, 0 if ids is None else len(ids), C.byref(batch)))
        n, total = int(batch.n_ids), int(batch.n_trades)
        # (the library's memory is valid until the next call: copy)
        first = np.ctypeslib.as_array(batch.first, (n + 1,)).copy()
        closed = np.ctypeslib.as_array(batch.closed, (n,)).copy() if n else np.zeros(0, np.int32)
        records = np.zeros(total, dtype=_RECORD)
        if total:
            C.memmove(records.ctypes.data, batch.trades, total * _RECORD.itemsize)
        req = np.arange(N, dtype=np.int64) if ids is None else ids.astype(np.int64)
        return cls(env, req, first, closed, records, batch.capacity, of_env)

    def __len__(self):
        return len(self._records)

    def of(self, env) -> np.ndarray:
        """The trades of env `env` as `numpy()` gives them (its first request, if it was requested twice)."""
        where = np.flatnonzero(self.env_ids == int(env))
        if not len(where):
            raise KeyError(f"env {env} was not requested")
        j = int(where[0])
        return self.numpy()[int(self.first[j]):int(self.first[j + 1])]

    def numpy(self) -> np.ndarray:
        """A structured array [len(self)]: ``env``, ``strategy`` (-1 without a map), the record's fields, ``ret``."""
        dt = [("env", "<i8"), ("strategy", "<i8")] + list(_abi.TRADE_LIST_DTYPE) + [("ret", "<f8")]
        out = np.zeros(len(self), dtype=dt)
        out["env"], out["ret"] = self.env, self.ret
        out["strategy"] = -1 if self.strategy is None else self.strategy
        for name in self.FIELDS:
            out[name] = self._records[name]
        return out


def pack_trades(env, env_ids=None, max_trades=None):
    """The gather of `TradeList` with its results left ON THE DEVICE (`gte_pack_trade_list`), for torch users:
    ``(first int64 [n + 1], closed int32 [n], trades uint8 [n_trades, 48])`` — `trades` holds `gte_trade` records
    (`TRADE_LIST_DTYPE`); `env_ids`: an int32 CUDA tensor or None for all envs.  With `max_trades` the block has
    that many records and nothing is read back or waited for: one scan and one pack are enqueued, records past
    `max_trades` are not written, and ``first[n]`` says how many there were.  Without it the total is read back once
    to size the block (a scan, a wait, then scan and pack)."""
    torch = env._torch
    if torch is None:
        raise ValueError("pack_trades needs output='torch'")
    if not getattr(env, "_trade_list_capacity", 0):
        raise ValueError("no trade list is kept: track_trades(list_capacity=...) first")
    dev = env._t["obs"].device
    if env_ids is not None:
        if not (isinstance(env_ids, torch.Tensor) and env_ids.is_cuda and env_ids.dtype == torch.int32):
            raise TypeError("env_ids must be an int32 CUDA tensor")
        env_ids = env_ids.contiguous().reshape(-1)
    if max_trades is not None and (isinstance(max_trades, bool) or int(max_trades) != max_trades or max_trades < 0):
        raise ValueError("max_trades must be a non-negative integer")
    n = env.num_envs if env_ids is None else int(env_ids.numel())
    ptr = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
    if n == 0:  # (a NULL id pointer means all envs: nothing to ask the library)
        with torch.cuda.device(dev):
            return (torch.zeros((1,), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev),
                    torch.zeros((0, _RECORD.itemsize), dtype=torch.uint8, device=dev))
    with torch.cuda.device(dev):
        first = torch.empty((n + 1,), dtype=torch.int64, device=dev)
        closed = torch.empty((n,), dtype=torch.int32, device=dev)
    call = env._lib.gte_pack_trade_list
    if max_trades is None:
        _abi.check(env._lib, call(env._h, ptr(env_ids), n, ptr(first), ptr(closed), None, 0))
        env.synchronize()
        total = int(first[n].item())
    else:
        total = int(max_trades)
    with torch.cuda.device(dev):
        trades = torch.empty((total, _RECORD.itemsize), dtype=torch.uint8, device=dev)
    if total or max_trades is not None:
        _abi.check(env._lib, call(env._h, ptr(env_ids), n, ptr(first), ptr(closed), ptr(trades), total))
    return first, closed, trades
