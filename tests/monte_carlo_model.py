"""A NumPy restatement of the trade Monte Carlo (gte_pool_trades, gte_trade_monte_carlo, include/gte.h), in exactly
the stated order: a plain loop over the trades i of a path, vector operations across the resamples only, the slab
tree level by level.  Used by test_monte_carlo_model_cpu.py (the model alone, and include/gte_mc.h compiled for the
host) and test_gpu_monte_carlo.py (the device, bit for bit).  The Philox is the oracle's."""
from __future__ import annotations

import numpy as np

from oracle import oracle

SLAB = 256                 # GTE_MC_SLAB
MAX_RESAMPLES = 65536      # GTE_MC_MAX_RESAMPLES
MAX_POOLS = 65536          # GTE_MC_MAX_POOLS
MAX_PATH = 1 << 20         # GTE_MC_MAX_PATH
MAX_LEVELS = 8             # GTE_MC_MAX_LEVELS
LDS_POOL = 8192            # GTE_MC_LDS_POOL
TRMC = 0x54524D43          # 'TRMC': word 3 of the counter
POOL = np.dtype([("final_sum", "<f8"), ("final_sq_sum", "<f8"), ("mdd_sum", "<f8"), ("mdd_sq_sum", "<f8"),
                 ("count_loss", "<i4"), ("count_ruin", "<i4"), ("pool_size", "<i4"), ("path_len", "<i4")])
COLUMNS = ("final", "max_drawdown", "low", "max_loss_streak")

# NaN, +-inf, +-0.0, a negative, subnormals, a huge and a tiny factor, and ordinary ones on either side of 1.0
SPECIAL = np.array([1.25, 0.8, np.nan, 1.0, np.inf, 0.5, -np.inf, 2.0, 0.0, 1.5, -0.0, 0.75, -1.5, 5e-324, 2.2e-308,
                    1e300, 1e-300, 0.999999999, 1.000000001], np.float64)


def special_pools():
    """(factors, first): one pool per special value mixed with ordinary factors, one of all of them, one of ordinary
    factors alone — a path that meets a NaN or a zero never recovers, so each gets a pool where it is rare"""
    rng = np.random.default_rng(11)
    ordinary = np.exp(rng.normal(0.0, 0.05, 24))
    pools = [np.concatenate([ordinary[:6], [v]]) for v in SPECIAL] + [SPECIAL.copy(), ordinary]
    first = np.concatenate([[0], np.cumsum([len(p) for p in pools])]).astype(np.int64)
    return np.concatenate(pools), first


_blocks = {}   # (seed, stream) -> uint32 [R, blocks, 4], grown on demand: a block depends on (seed, stream, r, i >> 2)


def blocks(seed: int, stream: int, R: int, n_blocks: int):
    """philox4x32_10(counter = {b, r, stream, 'TRMC'}, key = {seed low, seed high}) for r < R, b < n_blocks"""
    have = _blocks.get((seed, stream))
    if have is None or have.shape[0] < R or have.shape[1] < n_blocks:
        R2 = max(R, have.shape[0] if have is not None else 0)
        n2 = max(n_blocks, have.shape[1] if have is not None else 0)
        o = np.zeros((R2, n2, 4), np.uint32)
        key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        for r in range(R2):
            for b in range(n2):
                if have is not None and r < have.shape[0] and b < have.shape[1]:
                    o[r, b] = have[r, b]
                else:
                    o[r, b] = oracle.philox((b, r, stream & 0xFFFFFFFF, TRMC), key)
        _blocks[(seed, stream)] = have = o
    return have[:R, :n_blocks]


def words(seed, stream, R, L, repeat_word0=False):
    """uint32 [R, L]: the word draw i of resample r takes, o[i & 3] of block i >> 2 (`repeat_word0`: o[0] of that
    block instead — the mistake that repeats every draw four times, for the test of the uniformity check)"""
    o = blocks(seed, stream, R, (L + 3) // 4)
    if repeat_word0:
        return np.repeat(o[:, :, 0], 4, axis=1)[:, :L]
    return o.reshape(R, -1)[:, :L]


def indices(seed, stream, R, L, P, repeat_word0=False):
    """int64 [R, L]: j = mulhi32(word, P)"""
    w = words(seed, stream, R, L, repeat_word0)
    return ((w.astype(np.uint64) * np.uint64(P)) >> np.uint64(32)).astype(np.int64)


def pool_size(first, q) -> int:
    """P of pool q: 0 for a reversed pool, one of 2^31 factors or more, one outside [first[0], first[n_pools])"""
    lo, hi = int(first[q]), int(first[q + 1])
    if hi < lo or lo < int(first[0]) or hi > int(first[-1]) or hi - lo >= 1 << 31:
        return 0
    return hi - lo


def path_len(P, requested) -> int:
    if P == 0:
        return 0
    return requested if requested > 0 else min(P, MAX_PATH)


def walk(pool, R, L, seed, stream):
    """the R paths of L trades over `pool` (f64 [P]) -> final, max_drawdown, low (f64 [R]), max_loss_streak (i32 [R])"""
    P = len(pool)
    e, peak, mdd, low = np.ones(R), np.ones(R), np.zeros(R), np.ones(R)
    streak, max_streak = np.zeros(R, np.int32), np.zeros(R, np.int32)
    if L:
        j = indices(seed, stream, R, L, P)
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        for i in range(L):
            f = pool[j[:, i]]
            e = e * f
            peak = np.where(e > peak, e, peak)
            d = one - e / peak
            mdd = np.where(d > mdd, d, mdd)
            low = np.where(e < low, e, low)
            lose = f < one
            streak = np.where(lose, streak + 1, 0).astype(np.int32)
            max_streak = np.where(lose & (streak > max_streak), streak, max_streak).astype(np.int32)
    return dict(final=e, max_drawdown=mdd, low=low, max_loss_streak=max_streak)


def slab_sum(x):
    """the sum of x[r] over the resamples in the stated order: slabs of 256 places, a place past R holds 0.0, the
    tree h = 128 .. 1 within a slab, the slabs' results added from 0.0 in ascending order"""
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for lo in range(0, len(x), SLAB):
            a = np.zeros(SLAB)
            part = x[lo:lo + SLAB]
            a[:len(part)] = part
            h = SLAB // 2
            while h:
                a[:h] = a[:h] + a[h:2 * h]
                h //= 2
            total = total + a[0]
    return total


def monte_carlo(factors, first, streams, R, requested_len, seed, ruin, levels):
    """every output of gte_trade_monte_carlo: the four columns [Q, R], pool (structured [Q]) and dd_count [Q, D]"""
    Q = len(first) - 1
    out = dict(final=np.zeros((Q, R)), max_drawdown=np.zeros((Q, R)), low=np.zeros((Q, R)),
               max_loss_streak=np.zeros((Q, R), np.int32), pool=np.zeros(Q, POOL),
               dd_count=np.zeros((Q, len(levels)), np.int32))
    for q in range(Q):
        P = pool_size(first, q)
        L = path_len(P, requested_len)
        lo = int(first[q])
        w = walk(np.asarray(factors[lo:lo + P], dtype=np.float64), R, L, seed, q if streams is None else int(streams[q]))
        for name in COLUMNS:
            out[name][q] = w[name]
        rec = out["pool"][q]
        with np.errstate(all="ignore"):
            rec["final_sum"], rec["final_sq_sum"] = slab_sum(w["final"]), slab_sum(w["final"] * w["final"])
            rec["mdd_sum"] = slab_sum(w["max_drawdown"])
            rec["mdd_sq_sum"] = slab_sum(w["max_drawdown"] * w["max_drawdown"])
            rec["count_loss"] = int((w["final"] < 1.0).sum())
            rec["count_ruin"] = int((w["low"] <= np.float64(ruin)).sum())
            rec["pool_size"], rec["path_len"] = P, L
            for k, level in enumerate(levels):
                out["dd_count"][q, k] = int((w["max_drawdown"] >= np.float64(level)).sum())
    return out


def trade_pools(strategies, member_lists, first, closed, capacity, open_value, close_value):
    """what gte_pool_trades gives: `member_lists[s]` the envs of strategy s in member order (an entry outside
    [0, N) names no env); first / closed / open_value / close_value: the trade list of ALL envs as `TradeList` reads
    it -> (first int64 [Q + 1], truncated int32 [Q], factors f64)"""
    N = len(closed)
    parts, sizes, trunc = [], [], []
    with np.errstate(all="ignore"):
        for s in strategies:
            mine, t = [], 0
            if 0 <= s < len(member_lists):
                for e in member_lists[s]:
                    if not 0 <= e < N:
                        continue
                    lo, hi = int(first[e]), int(first[e + 1])
                    mine.append(close_value[lo:hi] / open_value[lo:hi])
                    t += int(closed[e] > capacity)
            parts.append(np.concatenate(mine) if mine else np.zeros(0))
            sizes.append(len(parts[-1]))
            trunc.append(t)
    return (np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), np.asarray(trunc, np.int32),
            np.concatenate(parts) if parts else np.zeros(0))
