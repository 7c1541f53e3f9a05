"""A NumPy restatement of the test for superior predictive ability and its step-down (gte_spa_test, include/gte.h), in
exactly the stated order: pass 1 is `bootstrap_model.reality_check`, then plain loops over the periods i and the
resamples r, vector operations across the strategies only (NumPy does not fuse a + w * d, and 1.0 / se, sqrt and the
multiplication by the reciprocal are each one correctly rounded operation, as on the device).  The model may keep the
[R, S] matrix of q_rs between the rounds; the device never writes it.  Used by test_spa_model_cpu.py (the model alone)
and test_gpu_spa.py (the device, bit for bit)."""
from __future__ import annotations

import math

import numpy as np

import bootstrap_model as bm

MAX_ROUNDS = 64          # GTE_SPA_MAX_ROUNDS
SUMMARY = np.dtype([("statistic", "<f8"), ("best", "<i4"), ("count_lower", "<i4"), ("count_consistent", "<i4"),
                    ("count_upper", "<i4"), ("rounds_run", "<i4"), ("num_rejected", "<i4"), ("studentised", "<i4"),
                    ("reserved", "<i4")])


def crit_rank(alpha: float, R: int) -> int:
    """the rank (0-based, ascending) of the 1 - alpha quantile among R maxima, as `StrategyPeriodStats.spa` takes it"""
    return min(R - 1, max(0, math.ceil((1.0 - alpha) * R) - 1))


def default_threshold(n: int) -> float:
    """Hansen's sqrt(2 log log n), for n >= 3"""
    return math.sqrt(2.0 * math.log(math.log(n)))


def _maxima(q, live, g, rse):
    """q: f64 [R, S]; one recentring g over the live strategies -> (M f64 [R], I int32 [R])"""
    R, S = q.shape
    M, I = np.zeros(R), np.full(R, -1, np.int32)
    for r in range(R):
        z = (q[r] - g) * rse
        # m = -inf; over live s ascending: if (z > m) m = z, index = s
        cand = np.where(live & ~np.isnan(z), z, -np.inf)
        if S and cand.max() > -np.inf:
            m = cand.max()
            I[r] = int(np.argmax(cand))
            M[r] = m if m > 0.0 else 0.0
    return M, I


def spa_test(stats, mask, benchmark, w, threshold, rank, max_rounds):
    """stats: structured [S, B] with steps and reward_sum; mask: bool [B]; benchmark: f64 [B] or None; w: f64 [R, n]
    -> dict of every output of gte_spa_test; "rc" is the dict of the nested reality check"""
    S, B = stats.shape
    P = [int(b) for b in np.flatnonzero(mask)]
    n, R = len(P), w.shape[0]
    assert n >= 2 and w.shape == (R, n) and threshold >= 0.0 and 0 <= rank < R and 1 <= max_rounds <= MAX_ROUNDS
    rc = bm.reality_check(stats, mask, benchmark, w)
    x = np.ascontiguousarray(stats["reward_sum"]).astype(np.float64)
    elig, mean = rc["eligible"], rc["mean"]
    NaN, dn, dR = np.float64("nan"), np.float64(n), np.float64(R)
    with np.errstate(all="ignore"):
        d = [x[:, b].copy() if benchmark is None else x[:, b] - np.float64(benchmark[b]) for b in P]
        m1 = rc["boot_sum"] / dR
        v = rc["boot_sq_sum"] / dR - m1 * m1
        se = np.sqrt(np.where(v > 0, v, 0.0))
        rse = 1.0 / se
        stud = elig & np.isfinite(mean) & np.isfinite(se) & (se > 0)
        t = mean * rse
        keep = stud & (t >= -np.float64(threshold))
        g = [np.where(stud & (mean > 0), mean, 0.0), np.where(keep, mean, 0.0), np.where(stud, mean, 0.0)]
        rse = np.where(stud, rse, 0.0)
        q = np.zeros((R, S))
        for r in range(R):
            a = np.zeros(S)
            for i in range(n):
                p = w[r, i] * d[i]
                a = a + p
            q[r] = a / dn
        max_stat, max_index = np.zeros((3, R)), np.full((3, R), -1, np.int32)
        for j in range(3):
            max_stat[j], max_index[j] = _maxima(q, stud, g[j], rse)
        cand = np.where(stud & ~np.isnan(t), t, -np.inf)
        best = int(np.argmax(cand)) if S and cand.max() > -np.inf else -1
        statistic = cand[best] if best >= 0 and cand[best] > 0.0 else 0.0
        summary = np.zeros(1, SUMMARY)
        summary["statistic"], summary["best"], summary["studentised"] = statistic, best, int(stud.sum())
        if stud.any():
            for j, name in enumerate(("count_lower", "count_consistent", "count_upper")):
                summary[name] = int((max_stat[j] >= statistic).sum())
        count_adj = np.array([(max_stat[1] >= ts).sum() if ok else 0 for ts, ok in zip(t, stud)], np.int32)
        # the step-down on the consistent recentring
        crit, round_rejected = np.full(max_rounds, NaN), np.zeros(max_rounds, np.int32)
        rejected_round = np.full(S, -1, np.int32)
        live, k = stud.copy(), 0
        while live.any() and k < max_rounds:
            M = max_stat[1] if k == 0 else _maxima(q, live, g[1], rse)[0]
            crit[k] = np.sort(M)[rank]
            out = live & (t > crit[k])
            round_rejected[k] = int(out.sum())
            rejected_round[out] = k
            live = live & ~out
            k += 1
            if not out.any():
                break
        summary["rounds_run"], summary["num_rejected"] = k, int(round_rejected.sum())
    return dict(t_stat=np.where(stud, t, NaN), std_error=np.where(elig, se, NaN), recentred=keep.astype(np.uint8),
                count_adj=count_adj, rejected_round=rejected_round, max_stat=max_stat.reshape(-1),
                max_index=max_index.reshape(-1), crit=crit, round_rejected=round_rejected, summary=summary,
                studentised=stud, rc=rc)


def two_round_board(seed):
    """S = 20, n = 12: six noisy losers, three mild losers, seven winners shifted by 0.6e-3 .. 2.4e-3 at noise 1e-3,
    four neutral rows.  The weakest winners fall only once the strongest have left the maximum."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1e-3, (20, 12))
    x[:6] = rng.normal(-2e-3, 2e-2, (6, 12))
    x[6:9] = rng.normal(-1e-3, 1e-3, (3, 12))
    x[9:16] += np.linspace(0.6e-3, 2.4e-3, 7)[:, None]
    return bm.records(x)


def near_null_board(seed):
    """S = 40, n = 24 at noise 1e-3, 15 rows shifted by -0.5e-3: the three recentrings disagree"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1e-3, (40, 24))
    x[:15] -= 0.5e-3
    return bm.records(x)


def p_values(out, R):
    """(p_lower, p_consistent, p_upper), NaN when no strategy has a statistic"""
    s = out["summary"][0]
    if s["best"] < 0:
        return (float("nan"),) * 3
    return tuple(float(s[k]) / R for k in ("count_lower", "count_consistent", "count_upper"))
