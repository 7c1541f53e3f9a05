"""Period rows for `BatchedTradingEnv.track_periods`: one small integer per market row that says which period
the row belongs to — equal blocks, train / embargo / test splits, calendar periods of a DatetimeIndex.  Host-side
NumPy; the first three functions return an int8 array [T] with ids 0 .. B-1 and -1 for rows that count nowhere.
`bootstrap_weights` makes the resampling table of a bootstrap over periods, on the device; `cscv_groups` and
`cscv_splits` make the group and split tables of `StrategyPeriodStats.cscv`."""
from __future__ import annotations

import numpy as np

#: what libgte keeps per env (GTE_MAX_PERIODS, include/gte.h)
MAX_PERIODS = 128
#: the most groups and splits of one `gte_cscv` call (GTE_CSCV_MAX_GROUPS, GTE_CSCV_MAX_SPLITS)
CSCV_MAX_GROUPS = 32
CSCV_MAX_SPLITS = 65536


def _checked(ids: np.ndarray) -> np.ndarray:
    if ids.size and int(ids.max()) >= MAX_PERIODS:
        raise ValueError(f"{int(ids.max()) + 1} periods: at most {MAX_PERIODS} are kept per env")
    return ids.astype(np.int8)


def blocks(T: int, n: int) -> np.ndarray:
    """n consecutive blocks of (almost) equal length over T rows: row t is in block ``t * n // T`` (walk-forward
    folds; block sizes differ by at most one row)."""
    T, n = int(T), int(n)
    if T < 1 or not 1 <= n <= min(T, MAX_PERIODS):
        raise ValueError(f"blocks(T={T}, n={n}): 1 <= n <= min(T, {MAX_PERIODS}) required")
    return _checked(np.arange(T, dtype=np.int64) * n // T)


def split(T: int, fractions, embargo: int = 0) -> np.ndarray:
    """Consecutive segments with the given fractions of T rows (they must sum to 1), e.g. ``(0.6, 0.4)`` for
    train / test: segment j ends at ``round(T * sum(fractions[:j + 1]))``, the last at T.  The first `embargo`
    rows of every segment but the first get -1: they count in no period, so an indicator's memory of the
    previous segment does not leak into the next one's figures."""
    T, embargo = int(T), int(embargo)
    f = np.asarray(fractions, dtype=np.float64)
    if f.ndim != 1 or not 1 <= len(f) <= MAX_PERIODS or (f <= 0).any() or abs(float(f.sum()) - 1.0) > 1e-9:
        raise ValueError("fractions: 1 .. 128 positive numbers that sum to 1")
    if T < len(f) or embargo < 0:
        raise ValueError("T >= len(fractions) and embargo >= 0 required")
    edges = np.rint(np.cumsum(f) * T).astype(np.int64)
    edges[-1] = T
    starts = np.concatenate(([0], edges[:-1]))
    if (edges <= starts).any():
        raise ValueError(f"split(T={T}): a segment would be empty")
    out = np.full(T, -1, dtype=np.int64)
    for j, (a, b) in enumerate(zip(starts, edges)):
        out[min(b, a + (embargo if j else 0)):b] = j
    return _checked(out)


def from_index(index, freq: str = "M") -> np.ndarray:
    """Calendar periods of a pandas DatetimeIndex (or anything ``pandas.DatetimeIndex`` accepts): rows of the
    same calendar period `freq` (a pandas period alias: "D", "W", "M", "Q", "Y") share an id, ids count from 0
    at the earliest period PRESENT in the index, in time order (a calendar period without rows takes no id)."""
    import pandas as pd
    idx = pd.DatetimeIndex(index)
    if getattr(idx, "tz", None) is not None:
        idx = idx.tz_localize(None)
    ordinals = np.asarray(idx.to_period(freq).asi8)
    uniq, ids = np.unique(ordinals, return_inverse=True)
    if len(uniq) > MAX_PERIODS:
        raise ValueError(f"{len(uniq)} periods of frequency {freq!r}: at most {MAX_PERIODS} are kept per env")
    return _checked(ids.astype(np.int64))


def bootstrap_weights(env, n, n_resamples, block=1.0, seed=0):
    """The stationary bootstrap's resampling weights over `n` selected periods, made on the env's device
    (`gte_bootstrap_weights`): a torch f64 tensor [n_resamples, n], entry [r, i] the number of times position i is
    drawn in resample r.  `block` >= 1 is the mean block length (1: every draw independent).  What
    `StrategyPeriodStats.reality_check` uses unless it is given `weights=`."""
    from .reality_check import bootstrap_weights as make
    return make(env, n, n_resamples, block, seed)


def cscv_groups(ids, n_groups) -> np.ndarray:
    """The period ids, taken in ascending order, cut into `n_groups` contiguous groups of (almost) equal size, the
    first ``len(ids) % n_groups`` one longer: a uint64 table [n_groups, 2], row g the mask of group g (bit b % 64 of
    word b // 64 = period b), as `gte_cscv` takes it."""
    ids = sorted({int(b) for b in ids})
    G = int(n_groups)
    if ids and not 0 <= ids[0] <= ids[-1] < MAX_PERIODS:
        raise ValueError(f"period ids must lie in [0, {MAX_PERIODS})")
    if not 2 <= G <= min(len(ids), CSCV_MAX_GROUPS):
        raise ValueError(f"cscv_groups: {G} groups of {len(ids)} periods: 2 <= n_groups <= min(periods, "
                         f"{CSCV_MAX_GROUPS}) required")
    size, longer = divmod(len(ids), G)
    words = [[0, 0] for _ in range(G)]
    at = 0
    for g in range(G):
        for b in ids[at:at + size + (g < longer)]:
            words[g][b >> 6] |= 1 << (b & 63)
        at += size + (g < longer)
    return np.array(words, dtype=np.uint64)


def cscv_splits(n_groups):
    """Every way of taking half of `n_groups` groups as in-sample, in lexicographic order of the chosen groups, the
    other half out-of-sample: ``(is_groups, oos_groups)``, two uint32 arrays [C], C = C(G, G/2), bit g = group g.
    Split c and split C - 1 - c are mirror images.  G must be even; G >= 20 has more than 65 536 splits and is
    refused."""
    from itertools import combinations
    from math import comb
    G = int(n_groups)
    if G < 2 or G % 2 or G > CSCV_MAX_GROUPS:
        raise ValueError(f"cscv_splits: n_groups must be even and lie in [2, {CSCV_MAX_GROUPS}], not {n_groups}")
    if comb(G, G // 2) > CSCV_MAX_SPLITS:
        raise ValueError(f"cscv_splits: {G} groups have {comb(G, G // 2)} splits, more than {CSCV_MAX_SPLITS}")
    every = (1 << G) - 1
    is_groups = np.array([sum(1 << g for g in pick) for pick in combinations(range(G), G // 2)], dtype=np.uint32)
    return is_groups, (np.uint32(every) & ~is_groups).astype(np.uint32)
