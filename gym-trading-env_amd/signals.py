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
