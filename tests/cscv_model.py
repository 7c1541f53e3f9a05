"""A NumPy restatement of the probability of backtest overfitting by combinatorially symmetric cross-validation
(gte_cscv, include/gte.h), in exactly the stated order: plain loops over the groups and the splits, vector
operations across the strategies only (NumPy does not fuse q - m * m).  Used by test_cscv_model_cpu.py (the model
alone) and test_gpu_cscv.py (the device, bit for bit)."""
from __future__ import annotations

import numpy as np

MAX_GROUPS = 32          # GTE_CSCV_MAX_GROUPS
MAX_SPLITS = 65536       # GTE_CSCV_MAX_SPLITS
CHUNK = 256              # GTE_CSCV_CHUNK
MEAN_REWARD, SHARPE, REWARD_SUM = 0, 1, 2      # the three of gte_period_metric that gte_cscv scores by
SUMMARY = np.dtype([(n, "<i4") for n in ("splits", "valid", "overfit", "loss", "eligible", "reserved")])
STRATEGY_PERIOD = np.dtype([("reward_sum", "<f8"), ("reward_sq_sum", "<f8"), ("steps", "<i8"), ("trades", "<i8"),
                            ("episodes", "<i8"), ("envs_stepped", "<i4"), ("reserved", "<i4")])


def periods_of(words):
    """the periods of a group mask (two uint64 words), ascending"""
    return [b for b in range(128) if (int(words[b >> 6]) >> (b & 63)) & 1]


def groups_of(word, G):
    """the groups of a split side (one uint32 word), ascending"""
    return [g for g in range(G) if (int(word) >> g) & 1]


def group_sums(stats, group_masks):
    """(a1 f64 [G][S], a2 f64 [G][S], n int64 [G][S], eligible bool [S])"""
    S = stats.shape[0]
    a1, a2, n = [], [], []
    elig = np.ones(S, bool)
    with np.errstate(all="ignore"):
        for words in group_masks:
            t1, t2, tn = np.zeros(S), np.zeros(S), np.zeros(S, np.int64)
            for b in periods_of(words):
                t1 = t1 + stats["reward_sum"][:, b]
                t2 = t2 + stats["reward_sq_sum"][:, b]
                tn = tn + stats["steps"][:, b]
            elig &= (tn > 0) & np.isfinite(t1) & np.isfinite(t2)
            a1.append(t1), a2.append(t2), n.append(tn)
    return a1, a2, n, elig


def score(metric, s1, s2, n):
    """the MEAN_REWARD, SHARPE and REWARD_SUM formulas of gte_rank_period_stats on (s1, s2, n), across strategies"""
    if metric == REWARD_SUM:
        return s1
    with np.errstate(all="ignore"):
        count = n.astype(np.float64)
        m = s1 / count
        if metric == MEAN_REWARD:
            return m
        assert metric == SHARPE
        q = s2 / count
        v = q - m * m
        v = np.where(v > 0.0, v, 0.0)
        return m / np.sqrt(v)


def side_score(metric, a1, a2, n, groups):
    S = a1[0].shape[0]
    s1, s2, c = np.zeros(S), np.zeros(S), np.zeros(S, np.int64)
    with np.errstate(all="ignore"):
        for g in groups:
            s1 = s1 + a1[g]
            s2 = s2 + a2[g]
            c = c + n[g]
    return score(metric, s1, s2, c)


def cscv(stats, group_masks, is_groups, oos_groups, metric):
    """stats: structured [S, B]; group_masks: uint64 [G, 2]; is_groups, oos_groups: uint32 [C]
    -> dict of every output of gte_cscv (and `eligible`, bool [S])"""
    S, G, C = stats.shape[0], len(group_masks), len(is_groups)
    a1, a2, n, elig = group_sums(stats, group_masks)
    NaN = np.float64("nan")
    best = np.full(C, -1, np.int32)
    is_score, oos_score = np.full(C, NaN), np.full(C, NaN)
    below, equal, ranked = np.zeros(C, np.int32), np.zeros(C, np.int32), np.zeros(C, np.int32)
    summary = np.zeros(1, SUMMARY)
    with np.errstate(all="ignore"):
        for c in range(C):
            IS = side_score(metric, a1, a2, n, groups_of(is_groups[c], G))
            OOS = side_score(metric, a1, a2, n, groups_of(oos_groups[c], G))
            # m = -inf; over eligible s ascending: if (IS > m) { m = IS; best = s; }
            cand = np.where(elig & ~np.isnan(IS), IS, -np.inf)
            if cand.max() > -np.inf:
                best[c] = int(np.argmax(cand))             # (the first of equal maxima: the lowest index)
                is_score[c], oos_score[c] = cand[best[c]], OOS[best[c]]
            counted = elig & ~np.isnan(OOS)
            ranked[c] = int(counted.sum())
            if best[c] >= 0 and not np.isnan(oos_score[c]):
                below[c] = int((counted & (OOS < oos_score[c])).sum())
                equal[c] = int((counted & (OOS == oos_score[c])).sum())
                summary["valid"] += 1
                summary["overfit"] += int(2 * int(below[c]) + int(equal[c]) <= int(ranked[c]))
                summary["loss"] += int(oos_score[c] < 0.0)
    summary["splits"], summary["eligible"] = C, int(elig.sum())
    return dict(best=best, is_score=is_score, oos_score=oos_score, below=below, equal=equal, ranked=ranked,
                summary=summary, eligible=elig)


def pbo(out):
    s = out["summary"][0]
    return float(s["overfit"]) / float(s["valid"]) if s["valid"] > 0 else float("nan")


def prob_loss(out):
    s = out["summary"][0]
    return float(s["loss"]) / float(s["valid"]) if s["valid"] > 0 else float("nan")


def derived(out):
    """(valid bool [C], rel_rank f64 [C], logit f64 [C], (slope, intercept)) from the counts, as OverfitCheck states
    them"""
    valid = (out["best"] >= 0) & ~np.isnan(out["oos_score"])
    with np.errstate(all="ignore"):
        w = (out["below"].astype(np.float64) + (out["equal"].astype(np.float64) + 1.0) / 2.0) / \
            (out["ranked"].astype(np.float64) + 1.0)
        w = np.where(valid, w, np.nan)
        logit = np.log(w / (1.0 - w))
        use = valid & np.isfinite(out["is_score"]) & np.isfinite(out["oos_score"])
        x, y = out["is_score"][use], out["oos_score"][use]
        if len(x) >= 2:
            slope = ((x - x.mean()) * (y - y.mean())).sum() / ((x - x.mean()) ** 2).sum()
            line = (float(slope), float(y.mean() - slope * x.mean()))
        else:
            line = (float("nan"), float("nan"))
    return valid, w, logit, line


def records(reward_sum, reward_sq_sum=None, steps=None):
    """[S, B] strategy period records around a matrix of period returns (squares of the returns and steps 1 unless
    given)"""
    t = np.zeros(reward_sum.shape, STRATEGY_PERIOD)
    t["reward_sum"] = reward_sum
    with np.errstate(all="ignore"):
        t["reward_sq_sum"] = np.square(reward_sum) if reward_sq_sum is None else reward_sq_sum
    t["steps"] = 1 if steps is None else steps
    t["envs_stepped"] = 1
    return t


def from_step_rewards(r, periods):
    """[S, B] records from step rewards r [S, T] and the period of every step (int [T], ids 0 .. B-1)"""
    S, B = r.shape[0], int(periods.max()) + 1
    t = np.zeros((S, B), STRATEGY_PERIOD)
    for b in range(B):
        col = r[:, periods == b]
        t["reward_sum"][:, b] = col.sum(axis=1)
        t["reward_sq_sum"][:, b] = (col * col).sum(axis=1)
        t["steps"][:, b] = col.shape[1]
    t["envs_stepped"] = 1
    return t


def same_f64(a, b):
    """two f64 arrays bit for bit, every NaN counting as the same value"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fix = lambda v: np.where(np.isnan(v), np.nan, v).view(np.uint64)
    return a.shape == b.shape and bool((fix(a) == fix(b)).all())
