"""The statement of what the rows of a backtest hold (struct gte_curve_bufs, include/gte.h): a plain per-env
Python loop over the step dicts of backtest_model, every floating operation one np.float64 operation in the order
of the header's table.  No dependence on the library.

A step dict of backtest_model is extended by the market row and the position INDEX that belong to its valuation:
    a transition (stepped)         v, i, pi — in same-step mode at an episode end the terminal ones —; with
                                   `reset` also true the new episode's v0 / p0 follow as backtest_model reads them
    a reset row (reset, not stepped)   v0, i0, pi0: the new episode's start valuation, the row the env landed on,
                                   the reset position index
    a frozen step (neither)        v, i, pi: the env as it stands
"""
from __future__ import annotations

import numpy as np

import backtest_model as bm

TERMINATED, TRUNCATED, RESET, FROZEN = 1, 2, 4, 8
COLUMNS = ("valuation", "drawdown", "reward", "position", "row", "flags")
DTYPES = dict(valuation=np.float64, drawdown=np.float64, reward=np.float64, position=np.int32, row=np.int32,
              flags=np.uint8)


def n_rows(K, stride):
    return -(-K // stride)


def rows(rec, steps, stride=1):
    """The rows of ONE env over one call: `rec` is its record before the call (backtest_model.new_record, or a
    record carried over) and is advanced exactly as backtest_model.run advances it; -> {column: array [R]}."""
    K = len(steps)
    out = {c: np.zeros(n_rows(K, stride), DTYPES[c]) for c in COLUMNS}
    m_r = m_d = np.float64(0.0)
    fl = 0
    with np.errstate(all="ignore"):
        for k, s in enumerate(steps):
            if k % stride == 0:
                m_r, m_d, fl = np.float64(0.0), np.float64(0.0), 0
            if s["stepped"]:
                v, i, pi = np.float64(s["v"]), s["i"], s["pi"]
                peak = v if v > rec["peak"] else rec["peak"]  # the record's peak after this transition
                d = np.float64(1.0) - v / peak
                if d > m_d:
                    m_d = d
                m_r = m_r + np.float64(s["r"])
                fl |= (TERMINATED if s["terminated"] else 0) | (TRUNCATED if s["truncated"] else 0)
                bm.transition(rec, s["v"], s["p"], s["r"], s["terminated"], s["truncated"])
                if s.get("reset"):
                    fl |= RESET
                    bm.reset(rec, s["v0"], s["p0"])
            elif s.get("reset"):
                v, i, pi = np.float64(s["v0"]), s["i0"], s["pi0"]
                fl |= RESET
                bm.reset(rec, s["v0"], s["p0"])
            else:
                v, i, pi = np.float64(s["v"]), s["i"], s["pi"]
                fl |= FROZEN
            if (k + 1) % stride == 0 or k == K - 1:
                j = k // stride
                out["valuation"][j], out["position"][j], out["row"][j] = v, pi, i
                out["reward"][j], out["drawdown"][j], out["flags"][j] = m_r, m_d, fl
    return out


def restride(one, K, stride):
    """The rows at `stride` derived from the stride-1 rows `one` of the same K steps: the last value, the OR,
    the running `d > m`, the sequential sum."""
    out = {c: np.zeros(n_rows(K, stride), DTYPES[c]) for c in COLUMNS}
    with np.errstate(all="ignore"):
        for j in range(n_rows(K, stride)):
            lo, hi = j * stride, min((j + 1) * stride, K)
            m_r = m_d = np.float64(0.0)
            fl = 0
            for k in range(lo, hi):
                # (a stride-1 row without a transition holds reward +0.0: m + 0.0 == m for every m but -0.0,
                # which a sum that started from +0.0 never is)
                m_r = m_r + one["reward"][k]
                if one["drawdown"][k] > m_d:
                    m_d = one["drawdown"][k]
                fl |= int(one["flags"][k])
            for c in ("valuation", "position", "row"):
                out[c][j] = one[c][hi - 1]
            out["reward"][j], out["drawdown"][j], out["flags"][j] = m_r, m_d, fl
    return out


def trace_steps(g, e):
    """backtest_model.trace_steps of env e of a golden trace, extended by the row and the position index the
    reference was on after every call (the traces have no same-step reset)."""
    out = []
    for k, s in enumerate(bm.trace_steps(g, e), start=1):
        i, pi = int(g["idx"][k, e]), int(g["pos_index"][k, e])
        if s.get("reset"):
            s.update(i0=i, pi0=pi)
        else:
            s.update(i=i, pi=pi)
            s.setdefault("v", g["portfolio_valuation"][k, e])  # (a frozen row)
        out.append(s)
    return out


def stack(per_env):
    """[R, N] arrays per column from the rows of every env."""
    return {c: np.stack([r[c] for r in per_env], axis=1) for c in COLUMNS}
