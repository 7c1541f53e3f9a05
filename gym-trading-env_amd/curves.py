"""Curves — what `BatchedTradingEnv.backtest_curves` returns: the per-step rows of a backtest (struct
gte_curve_bufs, include/gte.h) as [R, N] device tensors next to the `BacktestStats` of the same steps.  The rows
are written by the launch that holds the step in registers (csrc/gte_curves.hip); nothing here computes one."""
from __future__ import annotations

import numpy as np

from . import _abi

#: column name -> torch dtype name, in the order of struct gte_curve_bufs
COLUMNS = dict(_abi.CURVE_COLUMNS)


def n_rows(steps: int, stride: int) -> int:
    """R = ceil(steps / stride): the rows a call of `steps` steps writes."""
    return -(-int(steps) // int(stride))


def column_shapes(torch, keep, steps, stride, num_envs):
    """{column: (shape, dtype)} of the kept columns, in the struct's order."""
    R = n_rows(steps, stride)
    return {c: ((R, num_envs), getattr(torch, t)) for c, t in COLUMNS.items() if keep.get(c)}


def take_out(torch, out, want, dev):
    """The tensors of a previous result (`out`: a Curves or a dict) for this call's columns, checked; or new ones."""
    if out is None:
        with torch.cuda.device(dev):
            return {c: torch.empty(shape, dtype=dt, device=dev) for c, (shape, dt) in want.items()}
    cols = out.columns if isinstance(out, Curves) else out
    got = {c: cols[c] for c in want}  # KeyError: not the result of a matching call
    for c, (shape, dt) in want.items():
        t = got[c]
        if tuple(t.shape) != tuple(shape) or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError(f"out[{c!r}] does not match this backtest_curves call")
    return got


class Curves:
    """The rows of one `backtest_curves` call.

    The kept columns are attributes and entries of ``columns`` — ``valuation``, ``drawdown``, ``reward`` f64,
    ``position`` (the position INDEX), ``row`` i32, ``flags`` u8, each a device tensor [R, N] with
    R = ceil(steps / stride); a column that was not asked for is None.  Row j closes the window of steps
    ``j * stride .. min((j + 1) * stride, steps) - 1``: `valuation`, `position` and `row` are those of the
    window's last step, `reward` the window's sum, `drawdown` its deepest, `flags` its OR (include/gte.h states
    each exactly).  ``stats`` is the `BacktestStats` of the same steps."""

    def __init__(self, env, columns, stats, steps, stride):
        self.columns = dict(columns)
        self.stats = stats
        self.steps = int(steps)
        self.stride = int(stride)
        self.num_envs = env.num_envs
        for c in COLUMNS:
            setattr(self, c, self.columns.get(c))

    @property
    def rows(self) -> int:
        return n_rows(self.steps, self.stride)

    @property
    def step_index(self):
        """The step of the call each row closes, int64 [R] on the host: stride - 1, 2 * stride - 1, ..., steps - 1."""
        last = np.arange(1, self.rows + 1, dtype=np.int64) * self.stride - 1
        return np.minimum(last, self.steps - 1)

    def _flag(self, bit):
        if self.flags is None:
            raise ValueError("the flags column was not kept (backtest_curves(flags=True))")
        return (self.flags & bit) != 0

    @property
    def terminated(self):
        """bool [R, N]: a transition of the window raised `terminated`."""
        return self._flag(_abi.CURVE_TERMINATED)

    @property
    def truncated(self):
        return self._flag(_abi.CURVE_TRUNCATED)

    @property
    def reset(self):
        """bool [R, N]: a reset happened in a step of the window (a next-step reset row, or after a same-step
        episode end)."""
        return self._flag(_abi.CURVE_RESET)

    @property
    def frozen(self):
        """bool [R, N]: a step of the window found the env finished and not reset (auto-reset off)."""
        return self._flag(_abi.CURVE_FROZEN)

    def dates(self, env):
        """The `row` column through the dataset's index: an array [R, N] of what the reference calls `date`.
        Single dataset only: a row number alone does not say which dataset it belongs to."""
        if self.row is None:
            raise ValueError("the row column was not kept (backtest_curves(row=True))")
        if len(env.datasets) != 1:
            raise ValueError("dates() needs a single dataset: the rows carry no dataset column "
                             f"(this env has {len(env.datasets)})")
        ds = env.datasets[0]
        index = np.asarray(ds.index) if ds.index is not None else np.arange(ds.T)
        return index[self.row.cpu().numpy()]

    def numpy(self):
        """{column: host array [R, N]} of the kept columns; waits for the env's stream."""
        return {c: t.cpu().numpy() for c, t in self.columns.items()}

    def __repr__(self):
        return (f"Curves(steps={self.steps}, stride={self.stride}, rows={self.rows}, num_envs={self.num_envs}, "
                f"columns={list(self.columns)})")
