"""TradeMonteCarlo — what `StrategyTradeStats.monte_carlo()` gives: a Monte Carlo over the closed trades of each
requested strategy, on the device (`gte_pool_trades`, `gte_trade_monte_carlo`, include/gte.h).  Trades are drawn
with replacement from the strategy's trade list and compounded; the distribution of final equity, maximum drawdown,
lowest equity and longest losing streak says how bad the strategy can get under another ordering of its trades.
`resample()` does the same for a caller's own pools of trade factors."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .strategy_records import LeaderboardResult, _ptr, f64_on, field_views, is_int_in

COLUMNS = ("final", "max_drawdown", "low", "max_loss_streak")


class TradeMonteCarlo(LeaderboardResult):
    """The result of `StrategyTradeStats.monte_carlo()` and `resample()`, Q pools and R resamples.

    Per path, device tensors [Q, R] for the columns that were kept (None otherwise): ``final`` (the equity after the
    path, 1.0 at its start), ``max_drawdown``, ``low`` (the lowest equity) — f64 — and ``max_loss_streak`` (int32).

    Per pool, device tensors [Q], none of which waits: ``pool_size`` (its trades), ``path_len`` (the trades of a path),
    ``truncated`` (member envs whose list had dropped trades; zeros for own pools), ``mean_final`` / ``std_final``,
    ``mean_drawdown`` / ``std_drawdown``, ``prob_loss`` (the share of paths that end below 1.0), ``risk_of_ruin`` (the
    share whose equity touches ``ruin``) and ``prob_drawdown`` [Q, D] (the share whose maximum drawdown reaches
    ``drawdown_levels[k]``).  Every share is count / R to the bit.  ``final_sum``, ``final_sq_sum``, ``mdd_sum``,
    ``mdd_sq_sum``, ``count_loss``, ``count_ruin`` and ``dd_count`` are the raw sums and counts of the library.  A path
    over an empty pool stays at 1.0 / 0.0 / 1.0 / 0.

    ``strategies`` (int32 [Q], the ids that were asked for, None for own pools), ``factors`` / ``first`` (the pools),
    ``num_resamples``, ``ruin``, ``drawdown_levels`` and ``seed`` describe the call."""

    SUMMARY_DTYPE = _abi.MC_POOL_DTYPE
    ARRAYS = ("pool_size", "path_len", "truncated", "mean_final", "std_final", "mean_drawdown", "std_drawdown",
              "prob_loss", "risk_of_ruin", "prob_drawdown", "final_sum", "final_sq_sum", "mdd_sum", "mdd_sq_sum",
              "count_loss", "count_ruin", "dd_count")

    def __init__(self, env, out, keep, Q, R, levels, ruin, seed, strategies, factors, first, truncated):
        super().__init__(env, out, keep)
        torch = env._torch
        dev = out["summary"].device
        self.num_pools, self.num_resamples = Q, R
        self.drawdown_levels, self.ruin, self.seed = tuple(levels), float(ruin), int(seed)
        self.strategies, self.factors, self.first = strategies, factors, first
        for name in COLUMNS:
            col = out.get(name)
            setattr(self, name, None if col is None else col.view(Q, R))
        vars(self).update(field_views(out["summary"].data_ptr(), [(n, t) for n, t in _abi.MC_POOL_DTYPE],
                                      _abi.MC_POOL_DTYPE, (Q,), dev))
        self.dd_count = out["dd_count"].view(Q, len(levels))
        self.truncated = truncated if truncated is not None else torch.zeros((Q,), dtype=torch.int32, device=dev)
        # (divided by a DEVICE scalar: torch turns a division by a host scalar into a multiplication by its
        # reciprocal, which is not count / R to the last bit)
        Rt = torch.full((), float(R), dtype=torch.float64, device=dev)
        self.mean_final = self.final_sum / Rt
        self.std_final = torch.sqrt(torch.clamp(self.final_sq_sum / Rt - self.mean_final * self.mean_final, min=0.0))
        self.mean_drawdown = self.mdd_sum / Rt
        self.std_drawdown = torch.sqrt(torch.clamp(self.mdd_sq_sum / Rt - self.mean_drawdown * self.mean_drawdown,
                                                   min=0.0))
        self.prob_loss = self.count_loss.to(torch.float64) / Rt
        self.risk_of_ruin = self.count_ruin.to(torch.float64) / Rt
        self.prob_drawdown = self.dd_count.to(torch.float64) / Rt
        self._sorted = {}

    def quantile(self, column, q):
        """The `q` quantile(s) of a kept column over the resamples of every pool, on the device: the value at place
        ``ceil(q * R) - 1`` (at least 0) of the pool's sorted paths — [Q] for a number, [Q, len(q)] for a sequence.
        The column is sorted once (`torch.sort`, NaN last) and the sorted copy kept."""
        if column not in COLUMNS:
            raise ValueError(f"unknown column {column!r}: one of {', '.join(COLUMNS)}")
        values = getattr(self, column)
        if values is None:
            raise ValueError(f"column {column!r} was not kept: monte_carlo(keep=(..., {column!r}))")
        qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
        if qs.ndim != 1 or not ((qs >= 0.0) & (qs <= 1.0)).all():
            raise ValueError("q must lie in [0, 1]")
        if column not in self._sorted:
            self._sorted[column] = self._env._torch.sort(values, dim=1).values
        places = [max(int(np.ceil(v * self.num_resamples)) - 1, 0) for v in qs]
        picked = self._sorted[column][:, places]
        return picked[:, 0] if np.ndim(q) == 0 else picked

    def _scalars(self) -> dict:
        return dict(num_pools=self.num_pools, num_resamples=self.num_resamples, ruin=self.ruin, seed=self.seed,
                    drawdown_levels=self.drawdown_levels)

    def numpy(self) -> dict:
        """Everything on the host: the per-pool arrays by name, the kept columns, `strategies` and the call."""
        out = super().numpy()
        for name in COLUMNS:
            col = getattr(self, name)
            if col is not None:
                out[name] = col.cpu().numpy()
        out["strategies"] = None if self.strategies is None else self.strategies.cpu().numpy()
        return out


def _checked(n_resamples, n_trades, seed, ruin, drawdown_levels, keep):
    """the scalar arguments of a resampling, refused in the words of the sibling analyses"""
    for name, v in (("n_resamples", n_resamples), ("seed", seed)) + ((("n_trades", n_trades),) if n_trades is not None else ()):
        if not is_int_in(v, -float("inf"), float("inf"), floats=False):
            raise TypeError(f"{name} must be an integer")
    if not 1 <= int(n_resamples) <= _abi.GTE_MC_MAX_RESAMPLES:
        raise ValueError(f"n_resamples must lie in [1, {_abi.GTE_MC_MAX_RESAMPLES}]")
    if n_trades is not None and not 1 <= int(n_trades) <= _abi.GTE_MC_MAX_PATH:
        raise ValueError(f"n_trades must lie in [1, {_abi.GTE_MC_MAX_PATH}] (None: as many as the pool holds)")
    if not float(ruin) == float(ruin):
        raise ValueError("ruin must not be NaN")
    levels = tuple(float(v) for v in drawdown_levels)
    if len(levels) > _abi.GTE_MC_MAX_LEVELS or any(v != v for v in levels):
        raise ValueError(f"drawdown_levels: at most {_abi.GTE_MC_MAX_LEVELS} levels, none of them NaN")
    keep = (keep,) if isinstance(keep, str) else tuple(keep)
    for name in keep:
        if name not in COLUMNS:
            raise ValueError(f"unknown column {name!r}: one of {', '.join(COLUMNS)}")
    return int(n_resamples), 0 if n_trades is None else int(n_trades), int(seed) & (2 ** 64 - 1), float(ruin), levels, keep


def resample(env, factors, first, n_resamples=1000, n_trades=None, seed=0, ruin=0.5,
             drawdown_levels=(0.1, 0.2, 0.3, 0.5), keep=("final", "max_drawdown"), streams=None, _of=None):
    """A Monte Carlo over a caller's own pools: `factors` (f64, NumPy or torch) holds the trade factors
    ``close_value / open_value`` of all pools one after the other and `first` (int64 [Q + 1]) where each begins, pool q
    being ``factors[first[q]:first[q + 1]]``.  `n_trades`: the trades of a path (None: as many as the pool holds);
    `ruin`: the equity level whose touch counts as ruin; `keep`: the per-path columns to keep.  `streams` (uint32 or
    int32 [Q], None: q) names the random stream of each pool: the rows of a pool depend on its stream, the seed and
    the pool alone.  Enqueued on the env's stream; nothing waits.  Returns a `TradeMonteCarlo`."""
    torch = env._torch
    if torch is None:
        raise ValueError("a trade Monte Carlo needs output='torch'")
    R, L, seed, ruin, levels, keep = _checked(n_resamples, n_trades, seed, ruin, drawdown_levels, keep)
    dev = env._t["obs"].device
    factors = f64_on(torch, dev, factors, lambda s: len(s) == 1, "factors must have shape [n]")
    if not hasattr(first, "is_cuda"):
        first = torch.from_numpy(np.ascontiguousarray(np.asarray(first, dtype=np.int64)))
    first = first.to(device=dev, dtype=torch.int64).contiguous()
    Q = int(first.numel()) - 1
    if first.dim() != 1 or not 1 <= Q <= _abi.GTE_MC_MAX_POOLS:
        raise ValueError(f"first must have shape [Q + 1] with 1 <= Q <= {_abi.GTE_MC_MAX_POOLS}")
    if streams is not None:
        if not hasattr(streams, "is_cuda"):
            streams = torch.from_numpy(np.ascontiguousarray(np.asarray(streams).astype(np.int64).astype(np.uint32)
                                                            .view(np.int32)))
        streams = streams.to(device=dev).contiguous()
        if streams.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or tuple(streams.shape) != (Q,):
            raise ValueError(f"streams must be 32-bit integers of shape ({Q},)")
    f64, i32 = torch.float64, torch.int32
    with torch.cuda.device(dev):
        out = {name: torch.empty((Q * R,), dtype=i32 if name == "max_loss_streak" else f64, device=dev)
               for name in COLUMNS if name in keep}
        out["summary"] = torch.empty((Q * C.sizeof(_abi.GteMcPool),), dtype=torch.uint8, device=dev)
        out["dd_count"] = torch.empty((Q * len(levels),), dtype=i32, device=dev)
        if factors.numel() == 0:  # (the call wants a pointer; no pool reads it)
            factors = torch.zeros((1,), dtype=f64, device=dev)
    ptrs = _abi.GteMcOut(pool=out["summary"].data_ptr(), dd_count=out["dd_count"].data_ptr() if levels else None,
                         **{name: out[name].data_ptr() for name in COLUMNS if name in keep})
    host_levels = (C.c_double * max(len(levels), 1))(*levels)
    _abi.check(env._lib, env._lib.gte_trade_monte_carlo(
        env._h, _ptr(factors), _ptr(first), _ptr(streams), Q, R, L, seed, ruin, host_levels, len(levels),
        C.byref(ptrs)))
    strategies, truncated = _of if _of is not None else (None, None)
    return TradeMonteCarlo(env, out, (factors, first, streams), Q, R, levels, ruin, seed, strategies, factors, first,
                           truncated)


def run(owner, strategies, n_resamples=1000, n_trades=None, seed=0, ruin=0.5, drawdown_levels=(0.1, 0.2, 0.3, 0.5),
        keep=("final", "max_drawdown")) -> TradeMonteCarlo:
    """`StrategyTradeStats.monte_carlo`: pool the trade lists of the requested strategies with the fold's own member
    lists (one count pass, ONE read of the total to size the block, one pack), then resample with stream = strategy
    id, so that a strategy's rows do not depend on who else was asked for."""
    env, torch = owner._env, owner._env._torch
    if not getattr(env, "_trade_list_capacity", 0):
        raise ValueError("no trade list is kept: track_trades(list_capacity=...) first")
    _checked(n_resamples, n_trades, seed, ruin, drawdown_levels, keep)   # (refused before anything is launched)
    dev = owner._records.device
    if isinstance(strategies, torch.Tensor) and strategies.is_cuda:
        if strategies.dtype != torch.int32:
            raise TypeError("strategies must be an int32 CUDA tensor or ids on the host")
        ids = strategies.contiguous().reshape(-1)
    else:
        a = np.atleast_1d(np.asarray(strategies.numpy() if isinstance(strategies, torch.Tensor) else strategies))
        if a.size and a.dtype.kind not in "iu":
            raise TypeError("strategies must be integers")
        ids = torch.from_numpy(np.ascontiguousarray(a.reshape(-1).astype(np.int32))).to(dev)
    Q = int(ids.numel())
    if not 1 <= Q <= _abi.GTE_MC_MAX_POOLS:
        raise ValueError(f"between 1 and {_abi.GTE_MC_MAX_POOLS} strategies can be asked for, not {Q}")
    _, offsets, members = owner._keep
    with torch.cuda.device(dev):
        first = torch.empty((Q + 1,), dtype=torch.int64, device=dev)
        truncated = torch.empty((Q,), dtype=torch.int32, device=dev)
    call = env._lib.gte_pool_trades
    head = (env._h, owner.num_strategies, _ptr(offsets), _ptr(members), _ptr(ids), Q, _ptr(first), _ptr(truncated))
    _abi.check(env._lib, call(*head, None, 0))
    env.synchronize()
    total = int(first[Q].item())
    with torch.cuda.device(dev):
        factors = torch.empty((max(total, 1),), dtype=torch.float64, device=dev)
    if total:
        _abi.check(env._lib, call(*head, _ptr(factors), total))
    return resample(env, factors, first, n_resamples, n_trades, seed, ruin, drawdown_levels, keep, streams=ids,
                    _of=(ids, truncated))
