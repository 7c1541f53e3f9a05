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
