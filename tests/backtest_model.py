"""The statement of what a backtest statistics record holds (struct gte_backtest_stats,
include/gte.h): a plain per-env Python loop over per-step columns, every floating operation one
np.float64 operation in the order of the header's table.  No dependence on the library.

An env's timeline is a list of steps; each step is a dict of
    stepped     the env really advanced (a next-step auto-reset step and a frozen step did not)
    v, p, r     valuation the step computed, position VALUE after it, f64 reward (read if stepped)
    terminated, truncated   the step's flags (read if stepped)
    reset       the env was reset in this step: instead of a transition (next-step mode), or
                after it (same-step mode, stepped and reset both true)
    v0, p0      valuation and position value of that reset row (read if reset)
"""
from __future__ import annotations

import numpy as np

F64_FIELDS = ("reward_sum", "reward_sq_sum", "peak", "max_drawdown", "cur_return", "ep_return_sum",
              "ep_return_sq_sum", "valuation_last", "prev_position")
INT_FIELDS = ("steps", "trades", "episodes", "terminations")
FIELDS = INT_FIELDS + F64_FIELDS


def new_record(v, p, ended=False):
    """A cleared record of an env whose current valuation is v and position value p; `ended`: its
    episode has already ended and it has not been reset (needs_reset)."""
    rec = {f: 0 for f in INT_FIELDS}
    rec.update({f: np.float64(0.0) for f in F64_FIELDS})
    rec["peak"] = rec["valuation_last"] = np.float64(v)
    rec["prev_position"] = np.float64(p)
    rec["ended"] = bool(ended)
    return rec


def reset(rec, v0, p0):
    """A reset of any kind: next-step, same-step inside a launch, reset() between two calls."""
    rec["peak"] = np.float64(v0)
    rec["prev_position"] = np.float64(p0)
    rec["ended"] = False


def transition(rec, v, p, r, terminated, truncated):
    v, p, r = np.float64(v), np.float64(p), np.float64(r)
    with np.errstate(all="ignore"):
        rec["steps"] += 1
        rec["reward_sum"] = rec["reward_sum"] + r
        rec["reward_sq_sum"] = rec["reward_sq_sum"] + r * r
        if p != rec["prev_position"]:
            rec["trades"] += 1
        rec["prev_position"] = p
        if v > rec["peak"]:
            rec["peak"] = v
        d = np.float64(1.0) - v / rec["peak"]
        if d > rec["max_drawdown"]:
            rec["max_drawdown"] = d
        rec["cur_return"] = rec["cur_return"] + r
        if (terminated or truncated) and not rec["ended"]:
            rec["episodes"] += 1
            rec["terminations"] += int(bool(terminated))
            rec["ep_return_sum"] = rec["ep_return_sum"] + rec["cur_return"]
            rec["ep_return_sq_sum"] = rec["ep_return_sq_sum"] + rec["cur_return"] * rec["cur_return"]
            rec["cur_return"] = np.float64(0.0)
        if terminated or truncated:
            rec["ended"] = True
        rec["valuation_last"] = v
    return rec


def run(rec, steps):
    """Apply a list of step dicts (module docstring) to one env's record, in order."""
    for s in steps:
        if s["stepped"]:
            transition(rec, s["v"], s["p"], s["r"], s["terminated"], s["truncated"])
        if s.get("reset"):
            reset(rec, s["v0"], s["p0"])
    return rec


def trace_steps(g, e):
    """The step dicts of env e of a golden trace (replay.load), calls 1 .. K-1; call 0 is the reset
    the record is cleared at.  op == 0: the reference called reset() instead of step(); a call
    that left `step` where it was is a frozen row."""
    K = g["op"].shape[0]
    out = []
    for k in range(1, K):
        if g["op"][k, e] == 0:
            out.append(dict(stepped=False, reset=True, v0=g["portfolio_valuation"][k, e], p0=g["position"][k, e]))
        else:
            out.append(dict(stepped=bool(g["step"][k, e] != g["step"][k - 1, e]), reset=False,
                            v=g["portfolio_valuation"][k, e], p=g["position"][k, e], r=g["reward"][k, e],
                            terminated=bool(g["done"][k, e]), truncated=bool(g["truncated"][k, e])))
    return out


def trace_record(g, e):
    """The record of env e after the whole trace, cleared at its first reset."""
    return run(new_record(g["portfolio_valuation"][0, e], g["position"][0, e]), trace_steps(g, e))


def as_arrays(records):
    """[N] arrays per field from a list of records."""
    out = {f: np.array([r[f] for r in records], dtype=np.int64) for f in INT_FIELDS}
    out.update({f: np.array([r[f] for r in records], dtype=np.float64) for f in F64_FIELDS})
    return out
