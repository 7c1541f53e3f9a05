"""A NumPy restatement of the decorrelated leaderboard (gte_diversify, include/gte.h), in exactly the stated order:
plain loops over the selected periods and over the rounds, vector operations across the strategies only (NumPy does
not fuse q + e * e).  Used by test_diversify_model_cpu.py (the model alone) and test_gpu_diversify.py (the device,
bit for bit)."""
from __future__ import annotations

import numpy as np

MAX_PERIODS = 128        # GTE_MAX_PERIODS
RANK_MAX = 256           # GTE_RANK_MAX
SUMMARY = np.dtype([(n, "<i4") for n in ("picked", "candidates", "eligible", "remaining", "reserved")])
STRATEGY_PERIOD = np.dtype([("reward_sum", "<f8"), ("reward_sq_sum", "<f8"), ("steps", "<i8"), ("trades", "<i8"),
                            ("episodes", "<i8"), ("envs_stepped", "<i4"), ("reserved", "<i4")])


def periods_of(mask):
    """the selected periods, ascending, from a bool mask [B], a list of ids or the two uint64 words"""
    mask = np.asarray(mask)
    if mask.dtype == bool:
        return [int(b) for b in np.flatnonzero(mask)]
    if mask.dtype == np.uint64 and mask.shape == (2,):
        return [b for b in range(128) if (int(mask[b >> 6]) >> (b & 63)) & 1]
    return sorted(int(b) for b in mask)


def words_of(periods):
    """the two uint64 words of a set of period ids: bit b % 64 of word b // 64"""
    w = [0, 0]
    for b in periods:
        w[int(b) >> 6] |= 1 << (int(b) & 63)
    return np.array(w, np.uint64)


def standardise(stats, periods):
    """(u: list of n f64 [S], eligible bool [S]) — u as computed for every strategy, eligible or not"""
    S, n = stats.shape[0], len(periods)
    with np.errstate(all="ignore"):
        x = [stats["reward_sum"][:, b].astype(np.float64) for b in periods]
        ok = np.ones(S, bool)
        for b, xi in zip(periods, x):
            ok &= (stats["steps"][:, b] > 0) & np.isfinite(xi)
        t = np.zeros(S)
        for xi in x:
            t = t + xi
        m = t / np.float64(n)
        e = [xi - m for xi in x]
        q = np.zeros(S)
        for ei in e:
            q = q + ei * ei
        norm = np.sqrt(q)
        u = [ei / norm for ei in e]
    return u, ok & np.isfinite(q) & (q > 0.0)


def corr(u, s, j):
    """the correlation of every strategy of `s` (an index array, or slice(None)) with strategy j"""
    with np.errstate(all="ignore"):
        c = np.zeros(len(u[0][s]))
        for ui in u:
            c = c + ui[s] * ui[j]
    return c


def diversify(stats, periods, scores, max_corr, k):
    """stats: structured [S, B]; periods: ids, a bool mask or the two words; scores: f64 [S]
    -> dict of every output of gte_diversify (and `eligible`, `candidate`, bool [S])"""
    periods = periods_of(periods)
    assert len(periods) >= 3 and 1 <= k <= RANK_MAX and max_corr == max_corr
    S = stats.shape[0]
    scores = np.asarray(scores, np.float64)
    u, elig = standardise(stats, periods)
    cand = elig & ~np.isnan(scores)
    live = cand.copy()
    NaN = np.float64("nan")
    pick, pick_score, size = np.full(k, -1, np.int32), np.full(k, NaN), np.zeros(k, np.int32)
    owner = np.where(cand, -1, -2).astype(np.int32)
    owner_corr = np.full(S, NaN)
    for r in range(k):
        idx = np.flatnonzero(live)
        if not len(idx):
            break
        p = int(idx[np.argmax(scores[idx])])        # (the first of equal maxima: the lowest index; -0.0 == 0.0)
        pick[r], pick_score[r] = p, scores[p]
        c = corr(u, idx, p)
        with np.errstate(invalid="ignore"):
            leaves = (idx == p) | (c > max_corr)
        gone = idx[leaves]
        live[gone] = False
        owner[gone] = r
        owner_corr[gone] = c[leaves]
        size[r] = len(gone)
    pick_corr = np.full((k, k), NaN)
    taken = np.flatnonzero(pick >= 0)
    for a in taken:
        pick_corr[a, taken] = corr(u, pick[taken], int(pick[a]))
    summary = np.zeros(1, SUMMARY)
    summary["picked"], summary["candidates"] = len(taken), int(cand.sum())
    summary["eligible"], summary["remaining"] = int(elig.sum()), int(live.sum())
    return dict(pick=pick, pick_score=pick_score, cluster_size=size, owner=owner, owner_corr=owner_corr,
                pick_corr=pick_corr, summary=summary, eligible=elig, candidate=cand)


def records(reward_sum, steps=None):
    """[S, B] strategy period records around a matrix of period returns (squares of the returns, steps 1 unless
    given)"""
    t = np.zeros(reward_sum.shape, STRATEGY_PERIOD)
    t["reward_sum"] = reward_sum
    with np.errstate(all="ignore"):
        t["reward_sq_sum"] = np.square(reward_sum)
    t["steps"] = 1 if steps is None else steps
    t["envs_stepped"] = 1
    return t


def planted(seed, S=257, F=6, n=24, noise=0.05, scale=1e-3):
    """(x f64 [S, n], family int [S]): F factor rows of n normals, every strategy one factor plus noise * normals,
    all times `scale`"""
    rng = np.random.default_rng(seed)
    factors = rng.normal(0, 1, (F, n))
    family = rng.integers(0, F, S)
    family[:F] = np.arange(F)                       # every family has a member
    x = (factors[family] + noise * rng.normal(0, 1, (S, n))) * scale
    return x, family


def same_f64(a, b):
    """two f64 arrays bit for bit, every NaN counting as the same value"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fix = lambda v: np.where(np.isnan(v), np.nan, v).view(np.uint64)
    return a.shape == b.shape and bool((fix(a) == fix(b)).all())
