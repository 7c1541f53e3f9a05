"""A NumPy restatement of the bootstrap reality check (gte_bootstrap_weights, gte_reality_check, include/gte.h), in
exactly the stated order: plain loops over the periods i and the resamples r, vector operations across the
strategies only (NumPy does not fuse a + w * d).  Used by test_bootstrap_model_cpu.py (the model alone) and
test_gpu_bootstrap.py (the device, bit for bit).  The Philox is the oracle's."""
from __future__ import annotations

import numpy as np

from oracle import oracle

SLAB = 256               # GTE_BOOT_SLAB
MAX_RESAMPLES = 65536    # GTE_BOOT_MAX_RESAMPLES
BOOT = 0x424F4F54        # 'BOOT': word 3 of the counter
SUMMARY = np.dtype([("best_mean", "<f8"), ("best", "<i4"), ("count_rc", "<i4"), ("eligible", "<i4"),
                    ("reserved", "<i4")])
STRATEGY_PERIOD = np.dtype([("reward_sum", "<f8"), ("reward_sq_sum", "<f8"), ("steps", "<i8"), ("trades", "<i8"),
                            ("episodes", "<i8"), ("envs_stepped", "<i4"), ("reserved", "<i4")])

_draws = {}   # seed -> (o0, o1) uint32 [R, n], grown on demand: the draws depend on (r, j, seed) alone


def draws(seed: int, R: int, n: int):
    """words 0 and 1 of philox4x32_10(counter = {r, j, 0, 'BOOT'}, key = {seed low, seed high}) for r < R, j < n"""
    have = _draws.get(seed)
    if have is None or have[0].shape[0] < R or have[0].shape[1] < n:
        R2 = max(R, have[0].shape[0] if have else 0)
        n2 = max(n, have[0].shape[1] if have else 0)
        o0, o1 = np.zeros((R2, n2), np.uint32), np.zeros((R2, n2), np.uint32)
        key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        for r in range(R2):
            for j in range(n2):
                if have is not None and r < have[0].shape[0] and j < have[0].shape[1]:
                    o0[r, j], o1[r, j] = have[0][r, j], have[1][r, j]
                else:
                    o = oracle.philox((r, j, 0, BOOT), key)
                    o0[r, j], o1[r, j] = o[0], o[1]
        _draws[seed] = have = (o0, o1)
    return have[0][:R, :n], have[1][:R, :n]


def threshold(block: float) -> int:
    return int(min(np.floor(np.float64(4294967296.0) / np.float64(block)), 4294967295.0))


def restarts(n, R, block, seed):
    """bool [R, n]: draw j of resample r starts a new block"""
    o0, _ = draws(seed, R, n)
    new = o0.astype(np.int64) < threshold(block)
    if block == 1.0:
        new[:] = True
    new[:, 0] = True
    return new


def positions(n, R, block, seed):
    """int64 [R, n]: the position draw j of resample r takes"""
    _, o1 = draws(seed, R, n)
    new = restarts(n, R, block, seed)
    pos = np.zeros((R, n), np.int64)
    cur = np.zeros(R, np.int64)
    for j in range(n):
        cur = np.where(new[:, j], (o1[:, j].astype(np.uint64) * np.uint64(n) >> np.uint64(32)).astype(np.int64),
                       (cur + 1) % n)
        pos[:, j] = cur
    return pos


def weights(n, R, block, seed):
    """f64 [R, n]: w[r][i] = how many of the n draws of resample r take position i"""
    pos = positions(n, R, block, seed)
    w = np.zeros((R, n), np.float64)
    rows = np.arange(R)
    for j in range(n):
        w[rows, pos[:, j]] = w[rows, pos[:, j]] + 1.0   # (one draw per row and j: no index repeats within a call)
    return w


def reality_check(stats, mask, benchmark, w):
    """stats: structured [S, B] with steps and reward_sum; mask: bool [B]; benchmark: f64 [B] or None; w: f64 [R, n]
    -> dict of every output of gte_reality_check"""
    S, B = stats.shape
    P = [int(b) for b in np.flatnonzero(mask)]
    n, R = len(P), w.shape[0]
    assert n >= 2 and w.shape == (R, n)
    x = np.ascontiguousarray(stats["reward_sum"]).astype(np.float64)
    elig = np.ones(S, bool)
    for b in P:
        elig &= (stats["steps"][:, b] > 0) & np.isfinite(x[:, b])
    NaN, dn = np.float64("nan"), np.float64(n)
    with np.errstate(all="ignore"):
        d = [x[:, b].copy() if benchmark is None else x[:, b] - np.float64(benchmark[b]) for b in P]
        t = np.zeros(S)
        for i in range(n):
            t = t + d[i]
        mean = t / dn
        max_stat, max_index = np.full(R, -np.inf), np.full(R, -1, np.int32)
        boot_sum, boot_sq, count_ge = np.zeros(S), np.zeros(S), np.zeros(S, np.int32)
        q1, q2, ge = np.zeros(S), np.zeros(S), np.zeros(S, np.int32)
        for r in range(R):
            a = np.zeros(S)
            for i in range(n):
                p = w[r, i] * d[i]
                a = a + p
            c = a / dn - mean
            # m = -inf; over eligible s ascending: if (c > m) m = c, index = s
            cand = np.where(elig & ~np.isnan(c), c, -np.inf)
            if S and cand.max() > -np.inf:
                max_stat[r], max_index[r] = cand.max(), int(np.argmax(cand))
            q1 = q1 + c
            q2 = q2 + c * c
            ge = ge + (c >= mean)
            if (r + 1) % SLAB == 0 or r + 1 == R:   # the slab is closed: added in ascending slab order
                boot_sum, boot_sq, count_ge = boot_sum + q1, boot_sq + q2, count_ge + ge
                q1, q2, ge = np.zeros(S), np.zeros(S), np.zeros(S, np.int32)
        count_adj = np.array([(max_stat >= m).sum() for m in mean], np.int32)
    out = dict(mean=np.where(elig, mean, NaN), boot_sum=np.where(elig, boot_sum, NaN),
               boot_sq_sum=np.where(elig, boot_sq, NaN), count_ge=np.where(elig, count_ge, 0).astype(np.int32),
               count_adj=np.where(elig, count_adj, 0).astype(np.int32), max_stat=max_stat, max_index=max_index,
               eligible=elig)
    summary = np.zeros(1, SUMMARY)
    cand = np.where(elig & ~np.isnan(mean), mean, -np.inf)
    best = int(np.argmax(cand)) if S and cand.max() > -np.inf else -1
    summary["best"], summary["best_mean"] = best, mean[best] if best >= 0 else NaN
    summary["count_rc"] = out["count_adj"][best] if best >= 0 else 0
    summary["eligible"] = int(elig.sum())
    out["summary"] = summary
    return out


def p_values(out, R):
    """(the Reality Check p-value, naive p-values [S], adjusted p-values [S])"""
    s = out["summary"][0]
    rc = float(s["count_rc"]) / R if s["best"] >= 0 else float("nan")
    return rc, out["count_ge"] / R, out["count_adj"] / R


def records(reward_sum, steps=None):
    """[S, B] strategy period records around a matrix of period returns (steps 1 unless given)"""
    t = np.zeros(reward_sum.shape, STRATEGY_PERIOD)
    t["reward_sum"] = reward_sum
    with np.errstate(all="ignore"):
        t["reward_sq_sum"] = np.square(reward_sum)
    t["steps"] = 1 if steps is None else steps
    t["envs_stepped"] = 1
    return t


def same_f64(a, b):
    """two f64 arrays bit for bit, every NaN counting as the same value"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fix = lambda v: np.where(np.isnan(v), np.nan, v).view(np.uint64)
    return a.shape == b.shape and bool((fix(a) == fix(b)).all())
