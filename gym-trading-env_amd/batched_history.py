"""BatchedHistory — what a batch hands to `reward_function(history)`,
`dynamic_feature_functions` and metrics instead of the reference's per-env `History`
(src/gym_trading_env/utils/history.py:3-76, docs/source/history.rst:18-46).

Same access patterns, one value PER ENV:

    h["portfolio_valuation", -1]   [N]     the newest row of every env     (history.py:55-59)
    h["portfolio_valuation", -2]   [N]     the row before
    h["position", 0]               [N]     the first row of every env's CURRENT episode
    h["position"]                  [R, N]  the last R = len(h) rows of every env, oldest first
    h[["idx", "reward"]]           [R, N, 2]
    h[-1]                          dict of [N] arrays (the `info` of the step)
    h["reward", -1] = x            overwrite the newest reward (environments.py:267)

Backed by the device trajectory log (`log_steps` rows per env, gte_config.log_steps, what
`History.add` records each step, environments.py:253-264).  With `output="torch"` values
are `DeviceArray`s — torch tensors in HBM that NumPy formulas such as
`np.log(h[..., -1] / h[..., -2])` compute with unchanged (device_array.py); with
`output="numpy"` they are ndarrays copied from the device on access.

Differences from one env's History, inherent to a batch: `h[col]` is a sliding window of the
last `log_steps` steps of every env (episodes of different envs start at different rows;
`h.episode_mask()` marks the rows of each env's current episode), and non-numeric columns
(`date`, object-valued `data_*`) are host arrays.

Inside a graph capture (`capture_steps`, torch.cuda.is_current_stream_capturing()) the rows are
picked on the device from the log's row count there (gte_log_view.cursor), so that every replay
reads the rows of its own step: `h[col, -k]`, `h[col]`, `h[[cols]]`, `h[-1]` (entries computed
when read), `episode_mask()` and `h["reward", -1] = x` give the values of the eager views.  The
log must be full (`len(h)` is then `log_steps` in every replay).  What needs the host cannot be
captured and is refused: `h[col, t >= 0]` (its bounds check reads the device), host-valued
columns (`date`, object-valued `data_*`) and assigning a host value.
"""
from __future__ import annotations

from collections.abc import Mapping

import numpy as np

from . import _abi

_DIST = ("asset", "fiat", "borrowed_asset", "borrowed_fiat", "interest_asset", "interest_fiat")
# History columns that are raw per-env fields as they are
_RAW = ("idx", "step", "position_index", "dataset_index", "real_position", "portfolio_valuation", "reward")


def history_columns(env) -> list:
    """Flattened column names in the reference's order (environments.py:186-197, 253-264;
    history.py:20-33 flattening of the `data` and `portfolio_distribution` dicts)."""
    info = env.datasets[0].info_columns or ["close"]
    return (["idx", "step", "date", "position_index", "position", "real_position"]
            + [f"data_{c}" for c in info] + ["portfolio_valuation"]
            + [f"portfolio_distribution_{k}" for k in _DIST] + ["reward"])


def history_column(name, raw, positions, env, captured=False):
    """History column `name` (or dataset_index) derived from the raw per-env fields by the
    reference's rules (environments.py:186-197, 253-264; portfolio.py:49-57), whatever they come
    from: a state snapshot, the terminal records, the device log or a `read_log_envs` batch.

    raw(field) -> that field (idx, step, position_index, dataset_index, real_position,
    portfolio_valuation, asset, fiat, interest_asset, interest_fiat, reward); `positions`: the
    table `position` indexes.  Torch tensors are computed on the device, ndarrays on the host.
    captured: inside a graph capture, where `date` / `data_*` must already be on the device."""
    if name in _RAW:
        return raw(name)
    if name == "position":
        i = raw("position_index")
        return positions[i] if isinstance(i, np.ndarray) else positions[i.long()]
    if name.startswith("portfolio_distribution_"):
        k = name[len("portfolio_distribution_"):]
        if k in ("interest_asset", "interest_fiat"):
            return raw(k)
        if k in _DIST:  # Portfolio.get_portfolio_distribution, portfolio.py:49-57
            src = raw("asset" if k.endswith("asset") else "fiat")
            src = -src if k.startswith("borrowed") else src
            return np.maximum(0.0, src) if isinstance(src, np.ndarray) else src.clamp_min(0.0)
    if name == "date" or name.startswith("data_"):
        if captured:
            env._require_device_column(name)
        return env._dataset_column(name, raw("dataset_index"), raw("idx"))
    raise ValueError(f"Feature {name} does not exist ... Check the available features : {env.info_keys}")


class BatchedHistory:
    def __init__(self, env, terminal: bool = False):
        """terminal=True (same-step auto-reset): for the envs whose episode ended in the last
        step the NEWEST row is the terminal row `TradingEnv.step` logged (environments.py:253-264)
        — taken from the terminal records, because the log row of that step already holds the
        state after the in-launch reset; every other row and env reads the log as usual."""
        if not env.cfg.log_steps:
            raise ValueError("BatchedHistory needs log_steps > 0 (it reads the device trajectory log)")
        self._env = env
        self._terminal = bool(terminal)
        self.columns = history_columns(env) + ["dataset_index"]
        view = env._log_view()
        self._rows, self._L = int(view.rows), int(view.L)
        self._have = min(self._rows, self._L)
        # auto-reset disabled: a frozen env (ended on its dataset's last row) logs a copy of its last
        # row every step until it is reset; those copies are no rows of its episode
        self._frozen_runs = env.cfg.autoreset == _abi.AUTORESET_DISABLED
        # in a capture: the physical rows of the window, oldest first, as a device tensor [L]
        self._dev = None
        if env._capturing():
            if self._rows < self._L:
                raise ValueError(f"a BatchedHistory inside a graph capture needs a full log: take "
                                 f"log_steps = {self._L} eager steps (reset included) before capturing, "
                                 f"{self._rows} rows are logged")
            self._dev = env._log_order_on_device(view)

    def __len__(self):
        """Rows available per env: min(steps logged so far, log_steps)."""
        return self._have

    # -- row selection -------------------------------------------------------------------------
    def _phys(self, t):
        """Physical log row (scalar) of relative row t < 0, or per-env rows [N] of episode row
        t >= 0 (row t of every env's current episode).  In a capture: a device tensor [1]."""
        if t < 0:
            if -t > self._have:
                raise IndexError(f"index {t} is out of bounds: {self._have} rows are logged")
            if self._dev is not None:
                return self._dev[self._L + t:self._L + t + 1]
            return (self._rows + t) % self._L
        if self._dev is not None:
            raise ValueError(f"h[column, {t}] cannot be captured into a graph: its bounds check reads "
                             "the device (use negative indices, or h[column] with episode_mask())")
        step = self._env._log_rows("step", (self._rows - 1) % self._L, None)
        if self._terminal:
            step = self._env._overlay(step, "step")
        back = step - t  # rows between the wanted row and the newest one
        if self._frozen_runs:
            back = back + self._frozen_copies(self._env._log_rows("step", None, self._order()))
        if bool((back < 0).any()) or bool((back >= self._have).any()):
            raise IndexError(f"index {t} is outside the current episode / the {self._L} logged rows "
                             "of some env")
        return (self._rows - 1 - back) % self._L

    def _column(self, name, phys, t=None):
        """Values of column `name` at physical row(s) `phys`: a scalar row, a per-env row vector
        [N] or None for every logged row, oldest first ([R, N]).  t: the relative row `phys`
        stands for (when it is one)."""
        v = self._log_column(name, phys)
        if not self._terminal:
            return v
        e, newest = self._env, (self._rows - 1) % self._L
        if phys is None:      # the last row of the window is the newest one
            v = v.clone() if hasattr(v, "clone") else v.copy()
            v[-1] = e._overlay(v[-1], name)
            return v
        if self._dev is not None:  # a full log: relative row -1 is the newest one
            return e._overlay(v, name) if t == -1 else v
        if np.ndim(phys) == 0:
            return e._overlay(v, name) if int(phys) == newest else v
        return e._overlay(v, name, only=(phys == newest))

    def _log_column(self, name, phys):
        if self._dev is not None and phys is not None:  # one row, picked on the device: [1, N] -> [N]
            return self._log_column_rows(name, None, phys)[0]
        return self._log_column_rows(name, phys, self._order())

    def _log_column_rows(self, name, phys, order):
        e = self._env
        return history_column(name, lambda f: e._log_rows(f, phys, order), e._pos_table, e,
                              captured=self._dev is not None)

    def _order(self):
        """Physical rows of the logged window, oldest first."""
        if self._dev is not None:
            return self._dev
        return (np.arange(self._have) + self._rows - self._have) % self._L

    # -- the History protocol --------------------------------------------------------------------
    def __getitem__(self, arg):
        e = self._env
        if isinstance(arg, tuple):
            column, t = arg
            if isinstance(t, slice):
                return self[column][t]
            return e._wrap(self._column(column, self._phys(int(t)), int(t)))
        if isinstance(arg, (int, np.integer)):
            phys = self._phys(int(arg))
            if self._dev is not None:  # host-valued columns cannot be captured: read when asked for
                return _CapturedRow(self, phys, int(arg))
            return {c: e._wrap(self._column(c, phys)) for c in self.columns}
        if isinstance(arg, str):
            return e._wrap(self._column(arg, None))
        if isinstance(arg, list):
            return e._wrap(e._stack([self._column(c, None) for c in arg]))
        raise TypeError(f"unsupported History index {arg!r}")

    def __setitem__(self, arg, value):
        column, t = arg
        if column != "reward" or int(t) != -1:
            raise ValueError("only h['reward', -1] can be assigned (environments.py:267)")
        self._env._set_log_reward(value)

    def _frozen_copies(self, steps):
        """[N]: rows after the first of the run of equal `step` > 0 that ends each env's column of
        `steps` [R, N] (oldest first) — the copies a frozen env logged, 0 for every other env."""
        same = (steps == steps[-1:]) & (steps[-1:] > 0)
        if self._env._torch is not None:
            return (same.flip(0).to(self._env._torch.int32).cumprod(0).sum(0) - 1).clamp_min(0)
        return np.maximum(np.cumprod(same[::-1], axis=0).sum(0) - 1, 0)

    def episode_mask(self):
        """bool [R, N]: True where the logged row belongs to the env's CURRENT episode: its newest
        `step + 1` rows (with auto-reset disabled, a frozen env's copies at the end count as one)."""
        e = self._env
        if self._dev is not None:
            order = self._dev if self._frozen_runs else self._dev[-1:]
        else:
            order = self._order() if self._frozen_runs else self._order()[-1:]
        steps = e._log_rows("step", None, order)
        step_now = steps[-1]
        back = (self._have - 1 - e._arange_rows(self._have))[:, None]  # rows behind the newest one
        if self._frozen_runs:
            back = back - self._frozen_copies(steps)[None, :]
        return e._wrap((back >= 0) & (back <= step_now[None, :]))


class _CapturedRow(Mapping):
    """h[t] inside a graph capture: the columns of relative row t, each computed when read."""

    def __init__(self, h, phys, t):
        self._h, self._phys, self._t = h, phys, t

    def __getitem__(self, column):
        if column not in self._h.columns:
            raise KeyError(column)
        return self._h._env._wrap(self._h._column(column, self._phys, self._t))

    def __iter__(self):
        return iter(self._h.columns)

    def __len__(self):
        return len(self._h.columns)
