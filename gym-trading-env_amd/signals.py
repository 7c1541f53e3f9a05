"""Signal tables of `BatchedTradingEnv.bind_signals` on the host: the layout `gte_bind_signals`
(include/gte.h) asks for — int8 [S, stride] with stride a multiple of 16 bytes and at least T
rounded up to 16, so that an aligned 16-byte load anywhere in a row stays inside it — and the
checks a table passes before it goes to the device.  Pure NumPy: no device is touched here."""
from __future__ import annotations

import numpy as np

#: bytes the fused kernel loads at once: rows are padded to a multiple of it, the base is aligned to it
PIECE = 16


def row_stride(T: int) -> int:
    """Bytes from one strategy's row to the next: T rounded up to a multiple of 16."""
    T = int(T)
    if T < 1:
        raise ValueError("a signal table needs at least one column")
    return (T + PIECE - 1) // PIECE * PIECE


def as_int8_table(signals) -> np.ndarray:
    """`signals` as an int8 [S, T] array; refuses anything but two-dimensional integers that fit."""
    a = np.asarray(signals)
    if a.dtype == np.bool_:
        a = a.astype(np.int8)
    if a.dtype.kind not in "iu":
        raise TypeError(f"signal tables hold integers (position indices), not {a.dtype}")
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"expected a signal table of shape (S, T), got {a.shape}")
    if a.size and (a.min() < -128 or a.max() > 127):
        raise ValueError("signal table values must fit int8")
    return a.astype(np.int8)


def pad_rows(table: np.ndarray, fill: int = -1) -> np.ndarray:
    """int8 [S, T] -> C-contiguous int8 [S, row_stride(T)]; the padding holds `fill` (hold) and is
    never looked up: an env's row index stays below T."""
    S, T = table.shape
    out = np.full((S, row_stride(T)), fill, dtype=np.int8)
    out[:, :T] = table
    return out


# ---- signal tables built on the device from indicator rules (gte_build_signals, include/gte.h) ----

#: `gte_signal_rule` of include/gte.h, 32 bytes
RULE_DTYPE = np.dtype({
    "names": ["a", "b", "hi", "lo", "warmup", "pos_up", "pos_down", "pos_neutral", "latch", "reserved"],
    "formats": [np.int32, np.int32, np.float32, np.float32, np.int32, np.int8, np.int8, np.int8, np.uint8,
                (np.int32, (2,))],
    "offsets": [0, 4, 8, 12, 16, 20, 21, 22, 23, 24],
    "itemsize": 32,
})


def rules(a, b=-1, hi=0.0, lo=0.0, warmup=0, pos_up=1, pos_down=0, pos_neutral=-1, latch=False) -> np.ndarray:
    """One `RULE_DTYPE` record per strategy, the arguments broadcast against each other (the result is
    one-dimensional): row t of strategy s is `pos_up` where ``x[a][t] - x[b][t] > hi`` (``x[a][t]``
    alone with ``b == -1``), `pos_down` where it is below `lo`, `pos_neutral` in between — or, with
    `latch`, whatever the last row outside the band gave — and -1 (hold) for ``t < warmup``.  The
    rule itself is stated in include/gte.h.  `pos_*` are table bytes: position indices, or anything
    outside ``[0, len(positions))`` for hold."""
    fields = dict(a=a, b=b, hi=hi, lo=lo, warmup=warmup, pos_up=pos_up, pos_down=pos_down,
                  pos_neutral=pos_neutral, latch=latch)
    arrays = {k: np.asarray(v) for k, v in fields.items()}
    for k in ("a", "b", "warmup", "pos_up", "pos_down", "pos_neutral"):
        if arrays[k].dtype.kind not in "iub":
            raise TypeError(f"{k} must be integers, not {arrays[k].dtype}")
        lo_, hi_ = (-128, 127) if k.startswith("pos_") else (-2 ** 31, 2 ** 31 - 1)
        if arrays[k].size and (arrays[k].min() < lo_ or arrays[k].max() > hi_):
            raise ValueError(f"{k} does not fit its field")
    shape = np.broadcast_shapes(*(v.shape for v in arrays.values()))
    out = np.zeros(int(np.prod(shape, dtype=np.int64)) if shape else 1, dtype=RULE_DTYPE)
    for k, v in arrays.items():
        v = v != 0 if k == "latch" else v
        out[k] = np.broadcast_to(v, shape).reshape(-1)
    return out


def check_rules(rules: np.ndarray, n_indicators: int, d: int) -> None:
    """`RULE_DTYPE` records against the bank of dataset d they read: `a` names one of its rows, `b` one
    or none (-1)."""
    C = int(n_indicators)
    if ((rules["a"] < 0) | (rules["a"] >= C) | (rules["b"] < -1) | (rules["b"] >= C)).any():
        raise IndexError(f"rules name indicators outside the {C} rows of dataset {d}'s bank "
                         "(a in [0, C), b in [-1, C))")


# ---- signal tables composed on the device from clause rows and a truth table (gte_compose_signals) ----

from ._abi import COMPOSE_DTYPE as _COMPOSE_FIELDS  # noqa: E402
from ._abi import COMPOSE_KEEP as KEEP  # noqa: E402

#: `gte_signal_compose` of include/gte.h, 128 bytes
COMPOSE_DTYPE = np.dtype(_COMPOSE_FIELDS)
#: the zone codes of a clause row: what `clauses(...)` makes `build_signals` write
DOWN, NEUTRAL, UP = 0, 1, 2


def clauses(a, b=-1, hi=0.0, lo=0.0, warmup=0, latch=False) -> np.ndarray:
    """`rules(...)` whose table bytes are the zone codes: `DOWN` (0) below `lo`, `NEUTRAL` (1) in
    between, `UP` (2) above `hi`, and -1 inside the warm-up — the rows `compose` specs read."""
    return rules(a, b, hi, lo, warmup, pos_up=UP, pos_down=DOWN, pos_neutral=NEUTRAL, latch=latch)


def compose(inputs, lut, initial=-1, invalid=-1) -> np.ndarray:
    """One `COMPOSE_DTYPE` record per strategy: row t of strategy s is ``lut[c0, c1, ...]`` with
    ``c_k`` the code (0 / 1 / 2) that clause row ``inputs[s, k]`` holds at t — or, where that entry is
    `KEEP`, what the row before gave (`initial` before the first decision) — and `invalid` where some
    input holds no code (a clause's warm-up), which leaves the state alone.  The rule itself is
    stated in include/gte.h.

    inputs: integers ``[S, n]``, or ``[n]`` for every strategy, ``1 <= n <= 4``.  lut: an array of
    shape ``(3,) * n`` indexed ``[c0, c1, ...]``; one per strategy as ``[S, 3, ...]``; or a callable
    ``f(c0, ..., c_{n-1}) -> byte | KEEP``, evaluated here over the 3**n tuples.  `initial` and
    `invalid` are bytes, or one per strategy.  The entries of the 81 that only a fifth, sixth ...
    code could reach repeat the others, so that missing inputs count as code 0."""
    idx = np.asarray(inputs)
    if idx.dtype.kind not in "iu":
        raise TypeError(f"inputs must be integers (clause rows), not {idx.dtype}")
    if idx.ndim not in (1, 2) or not 1 <= idx.shape[-1] <= 4:
        raise ValueError(f"inputs: [S, n] or [n] with 1 <= n <= 4, got shape {idx.shape}")
    if idx.size and (idx.min() < -2 ** 31 or idx.max() > 2 ** 31 - 1):
        raise ValueError("inputs do not fit their field")
    n = idx.shape[-1]
    if callable(lut):
        codes = np.indices((3,) * n).reshape(n, -1)
        small = np.array([lut(*(int(c) for c in tup)) for tup in codes.T]).reshape((3,) * n)
    else:
        small = np.asarray(lut)
    if small.dtype == np.bool_:
        small = small.astype(np.int64)
    if small.dtype.kind not in "iu":
        raise TypeError(f"truth-table entries must be integers (table bytes or KEEP), not {small.dtype}")
    if small.shape == (3,) * n:
        small = small[None]
    elif small.ndim != n + 1 or small.shape[1:] != (3,) * n or small.shape[0] < 1:
        raise ValueError(f"lut: shape {(3,) * n} or (S,) + {(3,) * n} for {n} inputs, got {small.shape}")
    extra = {"initial": np.asarray(initial), "invalid": np.asarray(invalid)}
    for name, v in list(extra.items()) + [("lut", small)]:
        if v.dtype.kind not in "iub":
            raise TypeError(f"{name} must be integers, not {v.dtype}")
        if v.size and (v.min() < -128 or v.max() > 127):
            raise ValueError(f"{name} does not fit a byte")
        if name != "lut" and v.ndim > 1:
            raise ValueError(f"{name}: a byte, or one per strategy")
    sizes = {int(v.shape[0]) for v in (idx[None] if idx.ndim == 1 else idx, small, *(v.reshape(-1) for v in extra.values()))}
    sizes.discard(1)
    if len(sizes) > 1:
        raise ValueError(f"inputs, lut, initial and invalid disagree about the number of strategies: {sorted(sizes)}")
    S = sizes.pop() if sizes else 1
    out = np.zeros(S, dtype=COMPOSE_DTYPE)
    out["in"][:, :n] = np.broadcast_to(idx if idx.ndim == 2 else idx[None], (S, n))
    out["n_in"] = n
    out["initial"] = np.broadcast_to(extra["initial"].reshape(-1), (S,))
    out["pos_invalid"] = np.broadcast_to(extra["invalid"].reshape(-1), (S,))
    # entry c0 + 3 c1 + ...: c0 runs fastest, so the axes are reversed before flattening; codes of missing
    # inputs are 0, and the entries a non-zero one would reach repeat those
    flat = small.transpose((0,) + tuple(range(n, 0, -1))).reshape(small.shape[0], 3 ** n)
    out["lut"] = np.broadcast_to(np.tile(flat, (1, 81 // 3 ** n)), (S, 81))
    return out


def check_compose(specs: np.ndarray, n_clause_rows: int, d: int) -> None:
    """`COMPOSE_DTYPE` records against the clause table of dataset d they read: one to four inputs,
    each of those one of its rows."""
    R = int(n_clause_rows)
    n_in = specs["n_in"].astype(np.int64)
    if ((n_in < 1) | (n_in > 4)).any():
        raise ValueError("specs hold an n_in outside [1, 4]")
    used = np.arange(4)[None, :] < n_in[:, None]
    if (used & ((specs["in"] < 0) | (specs["in"] >= R))).any():
        raise IndexError(f"specs name clause rows outside the {R} rows of dataset {d}'s clause table")


def bank_stride(T: int) -> int:
    """Floats from one indicator row to the next: T rounded up to a multiple of 16."""
    return row_stride(T)


def pad_bank(x) -> np.ndarray:
    """Indicators [C, T] (or one of [T]) -> C-contiguous f32 [C, bank_stride(T)], the layout
    `gte_build_signals` asks for; the padding is 0 and reaches no table byte."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None, :]
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1 or x.dtype.kind not in "fiu":
        raise ValueError(f"expected numeric indicators of shape (C, T), got {x.dtype} {x.shape}")
    out = np.zeros((x.shape[0], bank_stride(x.shape[1])), dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


def sma_bank(close, windows) -> np.ndarray:
    """f32 [len(windows), T]: row i is the simple moving average of `close` over the last
    ``windows[i]`` rows, row t included, from f64 prefix sums; NaN while the window has no history
    (``t < windows[i] - 1``), so a rule on it is neutral there."""
    close = np.asarray(close, dtype=np.float64).reshape(-1)
    T = close.shape[0]
    csum = np.concatenate([[0.0], np.cumsum(close)])
    out = np.full((len(windows), T), np.nan, dtype=np.float32)
    for i, n in enumerate(windows):
        n = int(n)
        if n < 1:
            raise ValueError("an SMA window has at least one row")
        if n <= T:
            out[i, n - 1:] = ((csum[n:] - csum[:-n]) / n).astype(np.float32)
    return out


# ---- indicator banks built on the device from the resident market data (gte_build_indicators) ----

from ._abi import IND_KINDS, IND_MAX_WINDOW, IND_SOURCES  # noqa: E402
from ._abi import INDICATOR_DTYPE as _INDICATOR_FIELDS  # noqa: E402

#: `gte_indicator_spec` of include/gte.h, 16 bytes
INDICATOR_DTYPE = np.dtype(_INDICATOR_FIELDS)

#: enum gte_indicator_kind
IND_VALUE, IND_SMA, IND_STD, IND_ZSCORE, IND_MAX, IND_MIN, IND_DIFF, IND_ROC, IND_EMA, IND_RSI = range(10)
#: enum gte_indicator_source
SRC_CLOSE, SRC_HIGH, SRC_LOW, SRC_FEATURE, SRC_INPUT = range(5)


def _codes(values, names, what):
    """names or constants of an enumeration -> an int array of the same shape"""
    a = np.asarray(values)
    if a.dtype.kind in "US":
        flat = [str(v).lower() for v in a.reshape(-1)]
        bad = sorted({v for v in flat if v not in names})
        if bad:
            raise ValueError(f"unknown {what} {bad[0]!r}: one of {', '.join(names)}")
        return np.array([names.index(v) for v in flat], dtype=np.int64).reshape(a.shape)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{what} must be names or integers, not {a.dtype}")
    if a.size and (a.min() < 0 or a.max() >= len(names)):
        raise ValueError(f"unknown {what}: expected 0 .. {len(names) - 1} ({', '.join(names)})")
    return a.astype(np.int64)


def indicators(kind, n=1, source="close", column=0) -> np.ndarray:
    """One `INDICATOR_DTYPE` record per bank row, the arguments broadcast against each other (the
    result is one-dimensional): `kind` over `n` rows of `source` — names (``"sma"``, ``"rsi"``, ...;
    ``"close"``, ``"high"``, ``"low"``, ``"feature"``, ``"input"``) or the `IND_*` / `SRC_*`
    constants; `column` is the static feature column of ``"feature"`` or the row of the input bank of
    ``"input"``.  What each kind computes, to the rounding, is stated in include/gte.h.  `n` must lie
    in ``[1, 4096]`` (``"value"`` ignores it)."""
    k, s = _codes(kind, IND_KINDS, "indicator kind"), _codes(source, IND_SOURCES, "source")
    arrays = {"kind": k, "source": s, "column": np.asarray(column), "n": np.asarray(n)}
    for name in ("column", "n"):
        v = arrays[name]
        if v.dtype.kind not in "iub":
            raise TypeError(f"{name} must be integers, not {v.dtype}")
        if v.size and (v.min() < -2 ** 31 or v.max() > 2 ** 31 - 1):
            raise ValueError(f"{name} does not fit its field")
    shape = np.broadcast_shapes(*(v.shape for v in arrays.values()))
    full = {name: np.broadcast_to(v, shape).reshape(-1) for name, v in arrays.items()}
    windowed = full["kind"] != IND_VALUE
    if ((full["n"][windowed] < 1) | (full["n"][windowed] > IND_MAX_WINDOW)).any():
        raise ValueError(f"n must lie in [1, {IND_MAX_WINDOW}]")
    if (full["column"] < 0).any():
        raise ValueError("column must not be negative")
    out = np.zeros(int(np.prod(shape, dtype=np.int64)) if shape else 1, dtype=INDICATOR_DTYPE)
    for name, v in full.items():
        out[name] = v
    return out


def check_indicators(specs: np.ndarray, n_static: int, n_inputs: int, has_high: bool, has_low: bool, d: int) -> None:
    """`INDICATOR_DTYPE` records against what dataset d can serve: known kinds and sources, windows in
    range, feature columns among its `n_static` static ones, input rows among the `n_inputs` of its
    input bank, and high / low only where the dataset has them."""
    kind, src, col, n = specs["kind"], specs["source"], specs["column"], specs["n"]
    if ((kind < 0) | (kind >= len(IND_KINDS)) | (src < 0) | (src >= len(IND_SOURCES))).any():
        raise ValueError("specs hold an unknown kind or source")
    if ((kind != IND_VALUE) & ((n < 1) | (n > IND_MAX_WINDOW))).any():
        raise ValueError(f"specs hold a window outside [1, {IND_MAX_WINDOW}]")
    if ((src == SRC_FEATURE) & ((col < 0) | (col >= n_static))).any():
        raise ValueError(f"specs name feature columns outside the {n_static} static ones")
    if ((src == SRC_INPUT) & ((col < 0) | (col >= n_inputs))).any():
        raise ValueError(f"specs name input rows outside the {n_inputs} rows of dataset {d}'s input bank")
    for name, code, has in (("high", SRC_HIGH, has_high), ("low", SRC_LOW, has_low)):
        if (src == code).any() and not has:
            raise ValueError(f"specs read {name}, which dataset {d} does not have")


# ---- exit rules: stop-loss, trailing stop, take-profit and time exits (gte_bind_exit_rules) ----

from ._abi import EXIT_KINDS  # noqa: E402,F401
from ._abi import EXIT_RULE_DTYPE as _EXIT_FIELDS  # noqa: E402

#: `gte_exit_rule` of include/gte.h, 32 bytes
EXIT_DTYPE = np.dtype(_EXIT_FIELDS)


def exit_rules(stop_loss=0.0, take_profit=0.0, trailing=0.0, max_hold=0, exit_position=0) -> np.ndarray:
    """One `EXIT_DTYPE` record per exit rule, the arguments broadcast against each other (the result is
    one-dimensional): leave for position index `exit_position` when the env's valuation has fallen
    `stop_loss` (a fraction) under the valuation it entered at, `trailing` under its best valuation
    since, has risen `take_profit` over the entry valuation, or when the position has been held
    `max_hold` transitions.  0 (or a NaN fraction) switches that exit off; the rule itself, with the
    order of the four and the latch that follows an exit, is stated in include/gte.h.  `exit_position`
    is checked against the env's `positions` by `bind_exits`; the kernels take one outside them as
    "this rule is off"."""
    arrays = {"stop_loss": np.asarray(stop_loss), "take_profit": np.asarray(take_profit),
              "trailing": np.asarray(trailing), "max_hold": np.asarray(max_hold),
              "exit_position": np.asarray(exit_position)}
    for k in ("stop_loss", "take_profit", "trailing"):
        if arrays[k].dtype.kind not in "fiu":
            raise TypeError(f"{k} must be numbers, not {arrays[k].dtype}")
    for k, (lo_, hi_) in (("max_hold", (-2 ** 31, 2 ** 31 - 1)), ("exit_position", (-128, 127))):
        if arrays[k].dtype.kind not in "iu":
            raise TypeError(f"{k} must be integers, not {arrays[k].dtype}")
        if arrays[k].size and (arrays[k].min() < lo_ or arrays[k].max() > hi_):
            raise ValueError(f"{k} does not fit its field")
    shape = np.broadcast_shapes(*(v.shape for v in arrays.values()))
    out = np.zeros(int(np.prod(shape, dtype=np.int64)) if shape else 1, dtype=EXIT_DTYPE)
    for k, v in arrays.items():
        out[k] = np.broadcast_to(v, shape).reshape(-1)
    return out


def check_exit_rules(rules: np.ndarray, n_positions: int) -> None:
    """`EXIT_DTYPE` records against the env they are bound to: `exit_position` names one of its positions."""
    P = int(n_positions)
    if ((rules["exit_position"] < 0) | (rules["exit_position"] >= P)).any():
        raise IndexError(f"exit rules name an exit_position outside the env's {P} positions")
