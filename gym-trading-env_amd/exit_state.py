"""ExitState — what `BatchedTradingEnv.exit_state` returns: the per-env exit state of libgte (struct
gte_exit_state, include/gte.h) as torch views of device memory, in the manner of `BacktestStats`."""
from __future__ import annotations

import numpy as np

from . import _abi
from .strategy_records import field_views


class ExitState:
    """Per-env state of the bound exit rules, one value per env and field.

    ``entry``, ``peak`` (f64), ``held``, ``latched`` and the bookkeeping fields are torch tensors [N],
    ``exits`` is int32 [N, 4] — the exits fired so far in the order of `signals.EXIT_KINDS` (stop,
    trail, target, time).  All are strided VIEWS of the env's states: they show later steps as well —
    clone what has to outlive them — and are up to date with the env's stream once it has run what
    was enqueued (`env.synchronize()`, or any torch operation ordered after it)."""

    FIELDS = tuple(n for n, _ in _abi.EXIT_STATE_FIELDS) + ("exits",)

    def __init__(self, env, ptr: int):
        from .batched import _device_view
        self._env = env
        dev = env._t["obs"].device
        dt = np.dtype(_abi.EXIT_STATE_DTYPE)
        vars(self).update(field_views(ptr, _abi.EXIT_STATE_FIELDS, dt, (env.num_envs,), dev))
        self.exits = _device_view(ptr + dt.fields["exits"][1], (env.num_envs, 4), "<i4", dev, (dt.itemsize, 4))

    def numpy(self) -> np.ndarray:
        """The whole state array on the host, one transfer: a structured array [N] with the state's
        field names (`gte_read_exit_state`)."""
        e = self._env
        out = np.empty(e.num_envs, dtype=np.dtype(_abi.EXIT_STATE_DTYPE))
        _abi.check(e._lib, e._lib.gte_read_exit_state(e._h, 0, e.num_envs, out.ctypes.data))
        return out
