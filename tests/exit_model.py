"""The exit rules of include/gte.h (gte_bind_exit_rules) in NumPy / Python, for the tests: per env a
small state (entry, peak, held, latch, counters and the bookkeeping of the step-by-step path), brought
up to date from the env's record and asked for the action of the next step.  Every floating operation
is one IEEE f64 operation, written as in the header.

`ExitModel` holds the state of N envs as a structured array of the device's layout
(`_abi.EXIT_STATE_DTYPE`), so a test compares it with `ExitState.numpy()` field by field.  It also
records, for every comparison it evaluates, how far the valuation is from the threshold (`margins`),
which the fixture generator uses to keep every decision well away from a rounding."""
from __future__ import annotations

import numpy as np

STOP, TRAIL, TARGET, TIME = range(4)
KINDS = ("stop", "trail", "target", "time")
INT32_MAX = 2 ** 31 - 1

STATE_DTYPE = np.dtype([("entry", "<f8"), ("peak", "<f8"), ("v_seen", "<f8"), ("held", "<i4"), ("latched", "<i4"),
                        ("latched_raw", "<i4"), ("i_seen", "<i4"), ("episode_seen", "<i4"), ("step_seen", "<i4"),
                        ("decided", "<i4"), ("decided_action", "<i4"), ("reserved", "<i4", (2,)),
                        ("exits", "<i4", (4,))])
RULE_DTYPE = np.dtype([("stop_loss", "<f4"), ("take_profit", "<f4"), ("trailing", "<f4"), ("max_hold", "<i4"),
                       ("exit_position", "i1"), ("reserved0", "i1", (3,)), ("reserved", "<i4", (3,))])


def make_rules(stop_loss=0.0, take_profit=0.0, trailing=0.0, max_hold=0, exit_position=0):
    """RULE_DTYPE [R], the arguments broadcast (what signals.exit_rules builds, without its checks)."""
    arrays = [np.asarray(v) for v in (stop_loss, take_profit, trailing, max_hold, exit_position)]
    shape = np.broadcast_shapes(*(a.shape for a in arrays))
    out = np.zeros(int(np.prod(shape, dtype=np.int64)) if shape else 1, RULE_DTYPE)
    for name, a in zip(("stop_loss", "take_profit", "trailing", "max_hold", "exit_position"), arrays):
        out[name] = np.broadcast_to(a, shape).reshape(-1)
    return out


def new_state(n):
    """What a bind leaves: all zero, episode_seen = -1 (the next decision sees a reset row)."""
    s = np.zeros(int(n), STATE_DTYPE)
    s["episode_seen"] = -1
    return s


def rule_of(n_envs, n_rules, strategy, n_strategies, rule_of_env=None, env_id_base=0):
    """Rule index of every env: rule_of_env, or strategy_of(e) % n_rules."""
    if rule_of_env is not None:
        return np.asarray(rule_of_env, np.int64)
    if strategy is None:
        strategy = (int(env_id_base) + np.arange(int(n_envs), dtype=np.int64)) % int(n_strategies)
    return np.asarray(strategy, np.int64) % int(n_rules)


def reset_row(s, e, v0):
    s["entry"][e] = v0
    s["peak"][e] = v0
    s["held"][e] = 0
    s["latched"][e] = 0


def transition(s, e, v_prev, i_prev, v, i, d=1):
    """d >= 1 steps seen as one transition from (v_prev, i_prev) to (v, i)."""
    if i != i_prev:
        s["entry"][e] = v_prev
        s["peak"][e] = v_prev
        s["held"][e] = d
    else:
        s["held"][e] = min(int(s["held"][e]) + int(d), INT32_MAX)
    if v > s["peak"][e]:
        s["peak"][e] = v


def sync(s, e, episode, step, pv, pos):
    """The state of env e brought up to date with the row it stands on."""
    if episode != s["episode_seen"][e]:
        reset_row(s, e, pv)
    elif step != s["step_seen"][e]:
        transition(s, e, s["v_seen"][e], int(s["i_seen"][e]), pv, pos, max(1, int(step) - int(s["step_seen"][e])))
    s["v_seen"][e] = pv
    s["i_seen"][e] = pos
    s["episode_seen"][e] = episode
    s["step_seen"][e] = step


def conditions(s, e, R, v, margins=None):
    """[STOP, TRAIL, TARGET, TIME] as booleans for env e on valuation v under rule R (one record).
    margins: a list that receives |v - threshold| / |threshold| of every f64 comparison evaluated."""
    v = np.float64(v)
    one = np.float64(1.0)
    out = [False] * 4
    for k, name, base, sign in ((STOP, "stop_loss", "entry", -1), (TRAIL, "trailing", "peak", -1),
                                (TARGET, "take_profit", "entry", +1)):
        f = R[name]
        if not f > 0:  # <= 0 or NaN: off
            continue
        fd = np.float64(f)
        thr = np.float64(s[base][e]) * ((one - fd) if sign < 0 else (one + fd))
        out[k] = bool(v <= thr) if sign < 0 else bool(v >= thr)
        if margins is not None:
            with np.errstate(all="ignore"):
                margins.append(float(abs(v - thr) / abs(thr)))
    out[TIME] = bool(R["max_hold"] > 0 and s["held"][e] >= R["max_hold"])
    return out


def decide(s, e, R, raw, v, i, needs_reset, P, margins=None):
    """The action of env e's next step: a position index or -1 (hold)."""
    raw = int(raw)
    if needs_reset:
        return -1
    if s["latched"][e] and raw != s["latched_raw"][e]:
        s["latched"][e] = 0
    if s["latched"][e]:
        return -1
    xp = int(R["exit_position"])
    if 0 <= xp < P and i != xp:
        c = conditions(s, e, R, v, margins)
        if any(c):
            k = c.index(True)
            s["latched"][e] = 1
            s["latched_raw"][e] = raw
            s["exits"][e, k] += 1
            return xp
    return raw if 0 <= raw < P else -1


class ExitModel:
    """N envs' exit states and the step-by-step path of gte_signal_actions with rules bound."""

    def __init__(self, n_envs, rules, n_positions, rule_index):
        self.state = new_state(n_envs)
        self.rules = np.asarray(rules)
        self.P = int(n_positions)
        self.rule_index = np.asarray(rule_index, np.int64)
        assert self.rule_index.shape == (int(n_envs),)
        assert ((0 <= self.rule_index) & (self.rule_index < len(self.rules))).all()
        self.margins = []

    def rebind(self):
        self.state = new_state(len(self.state))

    def actions(self, raw, episode, step, pv, pos, needs_reset):
        """int32 [N] from the envs' records (arrays [N]) and their sign-extended table bytes `raw`."""
        s = self.state
        out = np.empty(len(s), np.int32)
        for e in range(len(s)):
            if s["decided"][e] and episode[e] == s["episode_seen"][e] and step[e] == s["step_seen"][e]:
                out[e] = s["decided_action"][e]
                continue
            sync(s, e, int(episode[e]), int(step[e]), np.float64(pv[e]), int(pos[e]))
            a = decide(s, e, self.rules[self.rule_index[e]], raw[e], np.float64(pv[e]), int(pos[e]),
                       bool(needs_reset[e]), self.P, self.margins)
            s["decided"][e] = 1
            s["decided_action"][e] = a
            out[e] = a
        return out


def raw_bytes(tables, strategy, idx, dataset):
    """The sign-extended table byte of every env: tables[dataset[e]][strategy[e], idx[e]]."""
    if isinstance(tables, np.ndarray) and tables.ndim == 2:
        tables = [tables]
    S = np.asarray(tables[0]).shape[0]
    n = len(idx)
    strategy = (np.arange(n) % S) if strategy is None else np.asarray(strategy)
    return np.array([int(np.asarray(tables[int(dataset[e])])[int(strategy[e]), int(idx[e])]) for e in range(n)],
                    np.int32)


def trace_tables(g):
    """The signal tables of a fixture written by tests/golden/make_exit_golden.py."""
    tables, d = [], 0
    while f"signals_{d}" in g:
        tables.append(np.asarray(g[f"signals_{d}"]))
        d += 1
    return tables


def trace_rules(g):
    """(RULE_DTYPE [R], rule_of_env [E]) of such a fixture (the rules travel as their bytes)."""
    return np.ascontiguousarray(g["exit_rules"]).view(RULE_DTYPE).reshape(-1), np.asarray(g["rule_of_env"])


def trace_actions(g):
    """What the model gives for every call of an exit trace, from the trace's own rows ->
    (int32 [K, E] actions, -1 where call k of env e is a reset; the smallest margin of every
    comparison evaluated; exits per kind [4]; the model, whose state is that after the last row).
    The action of call k is decided on the row the env stood on after call k - 1; an env whose
    episode ended there has needs_reset (the trace's next-step convention) and gets hold."""
    tables = trace_tables(g)
    rules, rule_of_env = trace_rules(g)
    P = len(g["cfg"]["positions"])
    K, E = g["op"].shape
    m = ExitModel(E, rules, P, rule_of_env)
    episode = np.cumsum(g["op"] == 0, axis=0)
    ended = (g["done"] | g["truncated"]).astype(bool)
    out = np.full((K, E), -1, np.int32)
    for k in range(1, K):
        raw = raw_bytes(tables, g["strategy"], g["idx"][k - 1], g["dataset"][k - 1])
        out[k] = m.actions(raw, episode[k - 1], g["step"][k - 1], g["portfolio_valuation"][k - 1],
                           g["pos_index"][k - 1], ended[k - 1])
        assert (out[k][g["op"][k] == 0] == -1).all()
    return out, (min(m.margins) if m.margins else np.inf), m.state["exits"].sum(axis=0), m
