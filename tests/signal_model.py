"""The lookup rule of signal tables (include/gte.h, gte_bind_signals) in NumPy, for the tests: the
action of an env's next step is the entry of its strategy's row at the market row the env stands
on, in the table of its current dataset — `a = signals[strategy[e]][env._idx]`,
`env.step(a if 0 <= a < P else None)` — with -1 standing for None (hold)."""
from __future__ import annotations

import numpy as np


def default_strategy(n_envs, n_strategies, env_id_base=0):
    """strategy=None: env e follows strategy (env_id_base + e) % S."""
    return ((int(env_id_base) + np.arange(int(n_envs), dtype=np.int64)) % int(n_strategies)).astype(np.int32)


def as_tables(signals):
    """One [S, T] integer array per dataset (a single array is the only dataset's)."""
    if isinstance(signals, np.ndarray) and signals.ndim == 2:
        signals = [signals]
    tables = [np.asarray(t) for t in signals]
    assert all(t.ndim == 2 and t.dtype.kind in "iu" for t in tables)
    assert len({t.shape[0] for t in tables}) == 1, "one number of strategies for all datasets"
    return tables


def lookup(signals, strategy, idx, dataset, n_positions):
    """int32 [N]: the action each env's table gives it on row idx[e] of dataset dataset[e]; any
    table value outside [0, n_positions) is -1 (hold)."""
    tables = as_tables(signals)
    idx, dataset = np.asarray(idx), np.asarray(dataset)
    S = tables[0].shape[0]
    strategy = default_strategy(len(idx), S) if strategy is None else np.asarray(strategy)
    assert strategy.shape == idx.shape == dataset.shape
    assert ((0 <= strategy) & (strategy < S)).all()
    out = np.empty(len(idx), np.int32)
    for e in range(len(idx)):
        t = tables[int(dataset[e])]
        assert 0 <= idx[e] < t.shape[1], (e, idx[e], t.shape)
        a = int(t[int(strategy[e]), int(idx[e])])
        out[e] = a if 0 <= a < n_positions else -1
    return out


def trace_tables(g):
    """The signal tables of a fixture written by tests/golden/make_signal_golden.py."""
    tables, d = [], 0
    while f"signals_{d}" in g:
        tables.append(np.asarray(g[f"signals_{d}"]))
        d += 1
    return tables


def trace_actions(g):
    """What the rule gives for every step call of a signal trace: int32 [K, E], -1 where call k of
    env e is a reset.  The action of call k is looked up on the row the env stood on after call
    k - 1."""
    tables = trace_tables(g)
    P = len(g["cfg"]["positions"])
    K, E = g["op"].shape
    out = np.full((K, E), -1, np.int32)
    for k in range(1, K):
        a = lookup(tables, g["strategy"], g["idx"][k - 1], g["dataset"][k - 1], P)
        out[k] = np.where(g["op"][k] == 1, a, -1)
    return out
