"""The statement of what a trade statistics record holds (struct gte_trade_stats, include/gte.h,
gte_track_trades): a plain per-env Python loop over the step dicts of backtest_model.trace_steps, every
floating operation one np.float64 operation in the order of the header's text.  Plus the fold into one record
per strategy (gte_reduce_trade_stats) and the six scores and the ranking (gte_rank_trade_stats).  No
dependence on the library.

A trade record has no bookkeeping of its own: `ended` — the episode has ended and no reset followed — is that
of the env's statistics record BEFORE the step, which `run` keeps itself the way backtest_model does."""
from __future__ import annotations

import math

import numpy as np

import strategy_model as sm
from gym_trading_env_amd import _abi

TRADE = np.dtype(_abi.TRADE_DTYPE)
STRATEGY_TRADE = np.dtype(_abi.STRATEGY_TRADE_DTYPE)
F64_FIELDS = tuple(n for n, t in _abi.TRADE_FIELDS if t == "<f8")
INT_FIELDS = tuple(n for n, t in _abi.TRADE_FIELDS if t != "<f8")
FIELDS = F64_FIELDS + INT_FIELDS
SUMS = ("gross_profit", "gross_loss", "ret_sq_sum")
METRICS = _abi.TRADE_METRICS
INF = float("inf")


def new_record(v, p, ended=False):
    """A cleared record of an env whose current valuation is v and position value p; `ended`: its episode
    has already ended and it has not been reset."""
    rec = {f: 0 for f in INT_FIELDS}
    rec.update({f: np.float64(0.0) for f in F64_FIELDS})
    rec["best_trade"], rec["worst_trade"] = np.float64(-INF), np.float64(INF)
    rec["open_position"] = np.float64(p)
    rec["open_value"] = rec["last_valuation"] = np.float64(v)
    rec["ended"] = bool(ended)  # (the statistics record's, not a field of the trade record)
    return rec


def close(rec, vc):
    with np.errstate(all="ignore"):
        ret = np.float64(vc) / rec["open_value"] - np.float64(1.0)
        rec["closed"] += 1
        rec["hold_sum"] += rec["open_len"]
        if rec["open_len"] > rec["max_len"]:
            rec["max_len"] = rec["open_len"]
        if ret > 0.0:
            rec["wins"] += 1
            rec["gross_profit"] = rec["gross_profit"] + ret
            rec["ret_sq_sum"] = rec["ret_sq_sum"] + ret * ret
            rec["loss_streak"] = 0
        elif ret < 0.0:
            rec["losses"] += 1
            rec["gross_loss"] = rec["gross_loss"] + ret
            rec["ret_sq_sum"] = rec["ret_sq_sum"] + ret * ret
            rec["loss_streak"] += 1
            if rec["loss_streak"] > rec["max_loss_streak"]:
                rec["max_loss_streak"] = rec["loss_streak"]
        if ret > rec["best_trade"]:
            rec["best_trade"] = ret
        if ret < rec["worst_trade"]:
            rec["worst_trade"] = ret
    if "returns" in rec:  # (a test's own list of every closed trade's return, in close order)
        rec["returns"].append(ret)
    return ret


def reset(rec, v0, p0):
    """A reset row of any kind."""
    if rec["open_position"] != 0.0:
        rec["dropped"] += 1
    rec["open_position"] = np.float64(p0)
    rec["open_value"] = rec["last_valuation"] = np.float64(v0)
    rec["open_len"] = 0
    rec["ended"] = False


def transition(rec, v, p, terminated, truncated):
    v, p = np.float64(v), np.float64(p)
    flags = bool(terminated) or bool(truncated)
    if not rec["ended"]:
        if p != rec["open_position"]:
            if rec["open_position"] != 0.0:
                if p == 0.0:
                    close(rec, v)
                else:
                    close(rec, rec["last_valuation"])
                    rec["reversals"] += 1
            rec["open_position"] = p
            rec["open_value"] = rec["last_valuation"]
            rec["open_len"] = 0
        if rec["open_position"] != 0.0:
            rec["open_len"] += 1
            rec["exposure"] += 1
        if flags and rec["open_position"] != 0.0:
            close(rec, v)
            rec["forced"] += 1
            rec["open_position"] = np.float64(0.0)
        rec["last_valuation"] = v
    if flags:
        rec["ended"] = True
    return rec


def run(rec, steps):
    """Apply a list of step dicts (backtest_model's module docstring) to one env's record, in order."""
    for s in steps:
        if s["stepped"]:
            transition(rec, s["v"], s["p"], s["terminated"], s["truncated"])
        if s.get("reset"):
            reset(rec, s["v0"], s["p0"])
    return rec


def as_array(records):
    """TRADE_DTYPE [N] from a list of records (reserved zero, as the library writes it)."""
    out = np.zeros(len(records), dtype=TRADE)
    for f in FIELDS:
        out[f] = [r[f] for r in records]
    return out


def same_records(got, want):
    """{field: envs that differ}: integer fields exactly, f64 fields by value (every NaN the same value)."""
    bad = {}
    for f in INT_FIELDS:
        d = np.flatnonzero(np.asarray(got[f]) != np.asarray(want[f]))
        if len(d):
            bad[f] = d.tolist()
    for f in F64_FIELDS:
        a, b = np.asarray(got[f], np.float64), np.asarray(want[f], np.float64)
        d = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))
        if len(d):
            bad[f] = d.tolist()
    return bad


# ---- per strategy ---------------------------------------------------------------------------------------

COUNTERS = ("closed", "wins", "losses", "forced", "reversals", "exposure", "hold_sum")


def reduce_loop(records, groups):
    """STRATEGY_TRADE_DTYPE [S] from TRADE_DTYPE [N] and the member lists (ids outside [0, N) are skipped)"""
    N = len(records)
    out = np.zeros(len(groups), dtype=STRATEGY_TRADE)
    for s, g in enumerate(groups):
        members = [records[e] if 0 <= e < N else None for e in g]
        o = out[s]
        for name in SUMS:
            o[name] = sm.fixed_order_sum([None if r is None else float(r[name]) for r in members])
        tot = {c: 0 for c in COUNTERS}
        envs = traded = max_len = max_streak = 0
        best, worst = -INF, INF
        for r in members:
            if r is None:
                continue
            envs += 1
            traded += int(r["closed"]) > 0
            for c in COUNTERS:
                tot[c] += int(r[c])
            max_len = max(max_len, int(r["max_len"]))
            max_streak = max(max_streak, int(r["max_loss_streak"]))
            if float(r["best_trade"]) > best:
                best = float(r["best_trade"])
            if float(r["worst_trade"]) < worst:
                worst = float(r["worst_trade"])
        for c in COUNTERS:
            o[c] = tot[c]
        o["envs"], o["envs_traded"], o["max_len"], o["max_loss_streak"] = envs, traded, max_len, max_streak
        o["best_trade"], o["worst_trade"] = best, worst
    return out


def canonical(records):
    """a copy with every NaN of the three sums replaced by one bit pattern (their payloads are unspecified)"""
    out = records.copy()
    for name in SUMS:
        out[name] = np.where(np.isnan(out[name]), np.nan, out[name])
    return out


def same_bytes(a, b):
    return canonical(a).tobytes() == canonical(b).tobytes()


def scores_loop(stats, metric):
    metric = METRICS[metric] if not isinstance(metric, str) else metric
    out = np.empty(len(stats))
    for s, r in enumerate(stats):
        closed = float(int(r["closed"]))
        gp, gl = float(r["gross_profit"]), float(r["gross_loss"])
        if metric == "win_rate":
            out[s] = sm._div(float(int(r["wins"])), closed)
        elif metric == "profit_factor":
            out[s] = sm._div(gp, 0.0 - gl)
        elif metric == "worst_trade":
            out[s] = float(r["worst_trade"])
        elif metric == "neg_max_loss_streak":
            out[s] = -float(int(r["max_loss_streak"]))
        else:
            m = sm._div(gp + gl, closed)
            if metric == "expectancy":
                out[s] = m
            else:
                assert metric == "trade_sharpe"
                q = sm._div(float(r["ret_sq_sum"]), closed)
                v = q - m * m
                if not v > 0.0:
                    v = 0.0
                out[s] = sm._div(m, math.sqrt(v))
    return out


def rank_loop(stats, scores, min_trades, k):
    """(top_index int32 [k], top_score f64 [k]): repeated selection of the best remaining strategy"""
    need = max(1, int(min_trades))
    left = [s for s in range(len(stats)) if int(stats["closed"][s]) >= need and scores[s] == scores[s]]
    index, top = np.full(k, -1, dtype=np.int32), np.full(k, np.nan)
    for place in range(min(k, len(left))):
        best = left[0]
        for s in left[1:]:
            if scores[s] > scores[best]:  # (equal scores: the lower index, met first, stays)
                best = s
        left.remove(best)
        index[place], top[place] = best, scores[best]
    return index, top


def craft_records(N, seed=0):
    """TRADE_DTYPE [N] for the fold: returns of mixed magnitude, members without a closed trade, +-inf and NaN
    sums, equal extremes"""
    rng = np.random.default_rng(seed)
    r = np.zeros(N, dtype=TRADE)
    r["closed"] = rng.integers(0, 60, N)
    r["wins"] = rng.integers(0, 30, N)
    r["losses"] = rng.integers(0, 30, N)
    r["forced"], r["reversals"], r["dropped"] = rng.integers(0, 9, N), rng.integers(0, 50, N), rng.integers(0, 3, N)
    r["exposure"], r["hold_sum"] = rng.integers(0, 10 ** 6, N), rng.integers(0, 10 ** 6, N)
    r["open_len"], r["max_len"] = rng.integers(0, 99, N), rng.integers(0, 500, N)
    r["loss_streak"], r["max_loss_streak"] = rng.integers(0, 9, N), rng.integers(0, 12, N)
    r["gross_profit"] = 10.0 ** rng.uniform(-9, 2, N)
    r["gross_loss"] = -(10.0 ** rng.uniform(-9, 2, N))
    r["ret_sq_sum"] = 10.0 ** rng.uniform(-12, 3, N)
    r["best_trade"] = rng.integers(0, 6, N) * 0.25          # few distinct values: equal extremes
    r["worst_trade"] = -rng.integers(0, 6, N) * 0.125
    r["open_value"], r["open_position"], r["last_valuation"] = rng.normal(1000, 9, N), rng.integers(-1, 2, N), rng.normal(1000, 9, N)
    idle = rng.choice(N, max(1, N // 7), replace=False)  # envs that closed no trade
    for f in ("closed", "wins", "losses", "forced", "max_len", "max_loss_streak"):
        r[f][idle] = 0
    for f in SUMS:
        r[f][idle] = 0.0
    r["best_trade"][idle], r["worst_trade"][idle] = -INF, INF
    if N >= 64:
        pick = rng.choice(np.setdiff1d(np.arange(N), idle), 8, replace=False)
        r["gross_profit"][pick[0]], r["gross_profit"][pick[1]] = INF, np.nan
        r["gross_loss"][pick[2]], r["ret_sq_sum"][pick[3]] = -INF, INF
        r["best_trade"][pick[4]], r["worst_trade"][pick[5]] = INF, -INF
        r["closed"][pick[6]] = 2 ** 31 - 1
        r["exposure"][pick[7]] = 2 ** 40
    return r


def craft_stats(S, seed=0):
    """STRATEGY_TRADE_DTYPE [S] for the scores and the ranking: duplicates, +-0.0, +-inf, NaN, strategies
    with no or few closed trades"""
    rng = np.random.default_rng(seed)
    t = np.zeros(S, dtype=STRATEGY_TRADE)
    t["closed"] = rng.integers(1, 400, S)
    t["wins"] = (t["closed"] * rng.integers(0, 5, S)) // 4          # few distinct win rates
    t["losses"] = t["closed"] - t["wins"]
    t["gross_profit"] = rng.integers(0, 12, S) * 0.25
    t["gross_loss"] = -rng.integers(0, 6, S) * 0.5                  # zeros among them: inf and NaN profit factors
    t["ret_sq_sum"] = np.abs(rng.normal(0, 2, S))
    t["worst_trade"] = -rng.integers(0, 6, S) * 0.125
    t["best_trade"] = t["worst_trade"] + 1.0
    t["max_loss_streak"] = rng.integers(0, 7, S)
    t["envs"] = t["envs_traded"] = 4
    if S >= 16:
        pick = rng.choice(S, 12, replace=False)
        t["closed"][pick[0]] = 0                                    # no closed trade: not ranked
        t["closed"][pick[1]] = 1
        t["gross_profit"][pick[2]], t["gross_loss"][pick[2]] = 0.0, -0.0        # 0 / 0
        t["gross_profit"][pick[3]], t["worst_trade"][pick[3]] = INF, -INF
        t["gross_loss"][pick[4]], t["worst_trade"][pick[4]] = -INF, INF
        t["gross_profit"][pick[5]], t["worst_trade"][pick[5]] = np.nan, np.nan
        t["worst_trade"][pick[6]], t["worst_trade"][pick[7]] = 0.0, -0.0
        m = (t["gross_profit"][pick[8]] + t["gross_loss"][pick[8]]) / t["closed"][pick[8]]
        t["ret_sq_sum"][pick[8]] = m * m * t["closed"][pick[8]]                 # zero variance
    return t
