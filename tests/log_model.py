"""An independent model of the device trajectory log, built from the C oracle's state and the
reference's `History` (environments.py:186-197 reset rows, :253-264 one row per step), not from
the kernels.  Test infrastructure: tests/test_log_model_cpu.py pins it against
oracle/py_loop.PyEnv, whose per-env `log` list restates History; the GPU tests compare the
device log and every reader of it with it.

Drive it beside an `OracleEnv`: call `reset(mask)` after `ora.reset(mask, ...)` and `step()`
after every `ora.step(...)` (one call per step of a rollout too).

Two things it keeps:
* `ring` — what the device log holds: `L` physical rows of N envs (zero before first written)
  and `count`, the rows appended so far.  A step appends one row for every env.  A full reset,
  or the first one, appends one row for every env; a masked reset rewrites only the masked envs'
  slot of the newest row.  A frozen env (auto-reset disabled, ended on its dataset's last row)
  still takes a slot per step: a copy of its state with reward 0.
* the reference's History of every env's current episode (and, in same-step mode, of the
  episode that ended in the last step, whose terminal row comes from the oracle's terminal
  record).  A frozen env adds nothing to its episode.
"""
from __future__ import annotations

import numpy as np

COLUMNS = {"idx": np.int32, "step": np.int32, "position_index": np.int32, "dataset_index": np.int32,
           "portfolio_valuation": np.float64, "real_position": np.float64, "reward": np.float64,
           "flags": np.uint8, "asset": np.float64, "fiat": np.float64,
           "interest_asset": np.float64, "interest_fiat": np.float64}
_STATE = ("idx", "step", "position_index", "dataset_index", "portfolio_valuation", "real_position",
          "asset", "fiat", "interest_asset", "interest_fiat")


class LogModel:
    def __init__(self, ora, L, autoreset, dataset_lengths):
        """autoreset: None / "disabled", "next_step" or "same_step"; dataset_lengths: T per dataset."""
        self.ora, self.L, self.N = ora, int(L), ora.N
        self.mode = autoreset or "disabled"
        self.T = np.asarray(dataset_lengths, np.int64)
        self.count = 0
        self.ring = {k: np.zeros((self.L, self.N), dt) for k, dt in COLUMNS.items()}
        self.episodes = [[] for _ in range(self.N)]  # [(row number, row dict)] per env
        self.finished_rows = [None] * self.N          # same-step mode: the episode that just ended
        self.frozen = np.zeros(self.N, bool)          # a step now leaves the env where it is
        self.just_ended = np.zeros(self.N, bool)

    # -- what one launch logs ------------------------------------------------------------------
    def _rows(self):
        """The row of every env from the oracle state after the launch: {column: [N]}."""
        o = self.ora
        st = o.state()
        rows = {k: np.array(st[k], dtype=COLUMNS[k]) for k in _STATE}
        rows["reward"] = np.where(rows["step"] == 0, 0.0, o.reward64).astype(np.float64)
        rows["flags"] = (o.terminated.astype(np.uint8) | (o.truncated.astype(np.uint8) << 1))
        return rows

    def _write(self, number, rows, envs):
        phys = number % self.L
        for k, v in rows.items():
            self.ring[k][phys, envs] = v[envs]

    @staticmethod
    def _row(rows, e):
        return {k: v[e].item() for k, v in rows.items()}

    def _after(self):
        st = self.ora.state()
        self.just_ended = (self.ora.terminated | self.ora.truncated).astype(bool)
        T_now = self.T[st["dataset_index"]]
        self.frozen = ((self.mode == "disabled") & (st["needs_reset"] != 0)
                       & (st["idx"] >= T_now - 1))

    def reset(self, mask=None):
        rows = self._rows()
        envs = np.arange(self.N) if mask is None else np.flatnonzero(np.asarray(mask))
        if mask is None or self.count == 0:
            self._write(self.count, rows, np.arange(self.N))
            number = self.count
            self.count += 1
        else:
            number = self.count - 1
            self._write(number, rows, envs)
        for e in envs:
            self.episodes[e] = [(number, self._row(rows, e))]
            self.finished_rows[e] = None
        self._after()

    def step(self):
        frozen = self.frozen.copy()
        rows = self._rows()
        number = self.count
        self._write(number, rows, np.arange(self.N))
        self.count += 1
        ended = (self.ora.terminated | self.ora.truncated).astype(bool)
        fin = self.ora.final_state() if self.mode == "same_step" else None
        for e in range(self.N):
            if frozen[e]:
                continue
            row = self._row(rows, e)
            if self.mode == "same_step" and ended[e]:
                term = {k: fin[k][e].item() for k in _STATE}
                term["reward"] = float(self.ora.reward64[e])
                term["flags"] = row["flags"]
                self.finished_rows[e] = self.episodes[e] + [(number, term)]
                self.episodes[e] = [(number, row)]
            elif row["step"] == 0:  # next-step mode: this launch reset the env
                self.episodes[e] = [(number, row)]
            else:
                self.episodes[e].append((number, row))
        self._after()

    # -- what the readers should return --------------------------------------------------------
    def episode(self, e, finished=False):
        """The reference's History rows (dicts) of env e's current episode; finished=True (same-step
        mode, right after the step in which e ended): the episode that ended, terminal row last."""
        rows = self.finished_rows[e] if finished else self.episodes[e]
        assert rows is not None, f"env {e} has no finished episode"
        return [r for _, r in rows]

    def logged(self, e, finished=False):
        """The part of `episode(e, finished)` still in the log: rows older than the last L row
        numbers are gone (a frozen env's slots count too).  When the frozen time alone fills the
        log, what is left is one frozen copy: the episode's last state with reward 0."""
        rows = self.finished_rows[e] if finished else self.episodes[e]
        oldest = self.count - min(self.count, self.L)
        keep = [r for n, r in rows if n >= oldest]
        if not keep and self.frozen[e]:
            keep = [dict(rows[-1][1], reward=0.0)]
        return keep

    def window_rows(self):
        """Physical rows of the logged window, oldest first."""
        have = min(self.count, self.L)
        return (np.arange(have) + self.count - have) % self.L

    def episode_mask(self):
        """bool [have, N]: True where a row of the window belongs to the env's current episode."""
        have = min(self.count, self.L)
        oldest = self.count - have
        mask = np.zeros((have, self.N), bool)
        for e in range(self.N):
            numbers = [n for n, _ in self.episodes[e] if n >= oldest]
            if not numbers and self.frozen[e]:
                numbers = [oldest]
            mask[np.asarray(numbers, np.int64) - oldest, e] = True
        return mask
