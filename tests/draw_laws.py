"""The laws of the reset draws, as the reference states them (environments.py:167,173-177,383-388),
and numpy-only statistics to hold a sample to them.  Used by test_draw_laws_cpu.py (the oracle) and
test_gpu_draw_laws.py (the device).

  start rows   np.random.randint(low, high): uniform on [W-1, T - max_dur - (W-1))
  positions    np.random.choice(positions): uniform over the P positions
  datasets     "uniform among the least-used datasets": every round of D picks of an env is a
               uniformly random permutation of range(D), whatever came before

Every sample comes from a fixed seed, so every p-value below is a fixed number; a law fails when
p < ALPHA.  The p-values come from the regularized upper incomplete gamma function (series plus
continued fraction, Numerical Recipes 6.2), so the suite needs no scipy.
"""
from __future__ import annotations

import math
from itertools import permutations

import numpy as np

ALPHA = 1e-6
MIN_EXPECTED = 5.0  # the chi-square approximation needs about 5 expected counts per cell


# ---------------------------------------------------------------------------------------------
# p-values

def _gamma_p_series(a: float, x: float) -> float:
    """Regularized lower incomplete gamma P(a, x) by its series (converges fast for x < a + 1)."""
    term = total = 1.0 / a
    ap = a
    for _ in range(100_000):
        ap += 1.0
        term *= x / ap
        total += term
        if abs(term) < abs(total) * 1e-16:
            break
    return total * math.exp(-x + a * math.log(x) - math.lgamma(a))


def _gamma_q_fraction(a: float, x: float) -> float:
    """Regularized upper incomplete gamma Q(a, x) by its continued fraction (modified Lentz;
    converges fast for x >= a + 1)."""
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 100_000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return math.exp(-x + a * math.log(x) - math.lgamma(a)) * h


def gamma_q(a: float, x: float) -> float:
    """Q(a, x) = Gamma(a, x) / Gamma(a), a > 0, x >= 0."""
    if a <= 0:
        raise ValueError("a must be > 0")
    if x <= 0:
        return 1.0
    if x < a + 1.0:
        return max(0.0, 1.0 - _gamma_p_series(a, x))
    return _gamma_q_fraction(a, x)


def chi2_sf(stat: float, dof: int) -> float:
    """P(X >= stat) for X ~ chi-square with `dof` degrees of freedom."""
    return gamma_q(0.5 * dof, 0.5 * stat)


def chisquare(counts, expected) -> float:
    """Goodness-of-fit p-value of observed `counts` against `expected` counts (same total)."""
    counts = np.asarray(counts, np.float64).ravel()
    expected = np.asarray(expected, np.float64).ravel()
    assert counts.shape == expected.shape and counts.size >= 2
    assert abs(counts.sum() - expected.sum()) <= 1e-6 * counts.sum(), "totals differ"
    assert expected.min() >= MIN_EXPECTED, f"{expected.min():.2f} expected in a cell: sample too small"
    stat = float(((counts - expected) ** 2 / expected).sum())
    return chi2_sf(stat, counts.size - 1)


def uniform_p(values, k: int) -> float:
    """p-value of `values` (integers, each in [0, k)) being uniform on range(k)."""
    v = np.asarray(values).ravel()
    assert v.min() >= 0 and v.max() < k, (int(v.min()), int(v.max()), k)
    counts = np.bincount(v.astype(np.int64), minlength=k)
    return chisquare(counts, np.full(k, v.size / k))


def independence_p(a, b, ka: int, kb: int) -> float:
    """Contingency-table p-value of the pairs (a[i], b[i]) (a in [0, ka), b in [0, kb)) having
    independent coordinates.  Both are meant to be uniform, so the expected count of a cell is
    n / (ka * kb); a table that would leave fewer than MIN_EXPECTED per cell is an error."""
    a = np.asarray(a).ravel().astype(np.int64)
    b = np.asarray(b).ravel().astype(np.int64)
    assert a.shape == b.shape
    assert a.min() >= 0 and a.max() < ka and b.min() >= 0 and b.max() < kb
    table = np.bincount(a * kb + b, minlength=ka * kb).reshape(ka, kb).astype(np.float64)
    rows, cols = table.sum(1), table.sum(0)
    rows, cols, table = rows[rows > 0], cols[cols > 0], table[rows > 0][:, cols > 0]
    expected = np.outer(rows, cols) / a.size
    assert expected.min() >= MIN_EXPECTED, f"{expected.min():.2f} expected in a cell: sample too small"
    stat = float(((table - expected) ** 2 / expected).sum())
    return chi2_sf(stat, (rows.size - 1) * (cols.size - 1))


def coarse(values, k: int, g: int):
    """values in [0, k) -> g nearly equal classes (floor(v * g / k)); identity when k <= g."""
    v = np.asarray(values).astype(np.int64)
    return (v, k) if k <= g else (v * g // k, g)


def uniform_range_p(values, low: int, high: int, bins: int = 256, moduli=(2, 3, 64)) -> dict:
    """p-values of integers `values` being uniform on [low, high): every value, or `bins` nearly
    equal bins of the range when it is wider (expected counts exact per bin width), plus the
    residues modulo each m < span (the fine structure a coarse binning cannot see: a rounding
    that skips odd rows or the last one).  Out-of-range values raise."""
    v = np.asarray(values).ravel().astype(np.int64) - low
    span = high - low
    assert span >= 1 and v.min() >= 0 and v.max() < span, (int(v.min()) + low, int(v.max()) + low,
                                                            low, high)
    if span == 1:
        return {}
    out = {}
    if span <= bins:
        out["value"] = uniform_p(v, span)
    else:
        edges = (np.arange(bins + 1) * span) // bins
        counts = np.bincount(np.searchsorted(edges, v, side="right") - 1, minlength=bins)
        out["bin"] = chisquare(counts, np.diff(edges) * (v.size / span))
    for m in moduli:
        if m < span and span > bins:
            width = np.array([(span - c + m - 1) // m for c in range(m)], np.float64)
            out[f"mod{m}"] = chisquare(np.bincount(v % m, minlength=m), width * (v.size / span))
    return out


# ---------------------------------------------------------------------------------------------
# collecting draws

FIELDS = ("start_idx", "position_index", "dataset_index")


def read_state(env, names=FIELDS) -> dict:
    """The named per-env state arrays of an oracle (OracleEnv.state() -> dict) or a device
    (BatchedTradingEnv.state(name)) env, as copies."""
    if getattr(env, "_l", None) is not None and hasattr(env, "_view"):  # oracle.OracleEnv
        st = env.state()
        return {n: np.array(st[n]) for n in names}
    return {n: np.array(env.state(n)) for n in names}


def collect_resets(env, R: int, mask=None, fields=FIELDS) -> dict:
    """R resets of `env` (all envs, or those in `mask`): {field: i32 [R, N]} after each."""
    out = {n: [] for n in fields}
    for _ in range(R):
        env.reset(mask=mask)
        for n, a in read_state(env, fields).items():
            out[n].append(a)
    return {n: np.stack(a) for n, a in out.items()}


def picks_from_resets(ds, switch_every: int, D: int):
    """The dataset picks an env made, in order, from the dataset_index [R, N] its resets showed.

    The constructor makes pick 0 (environments.py:378) and reset number t (t = 0, 1, ...) makes
    one more when (t + 1) % switch_every == 0 (:394-398, the episode counter restarts at every
    pick).  With switch_every == 1 reset 0 already shows pick 1 and pick 0 is never seen: it is
    returned as -1.  Returns [n_picks, N], pick m at row m."""
    ds = np.asarray(ds)
    R = ds.shape[0]
    rows = []
    if switch_every == 1:
        rows.append(np.full(ds.shape[1], -1, ds.dtype))
    else:
        rows.append(ds[0])
    for t in range(R):
        if (t + 1) % switch_every == 0:
            rows.append(ds[t])
    return np.stack(rows)


def full_rounds(picks, D: int):
    """[N, n_rounds, D] of the complete rounds (picks kD .. kD+D-1) among picks [n, N], round 0
    dropped when its pick 0 was not seen."""
    picks = np.asarray(picks)
    n = picks.shape[0] // D
    r = picks[: n * D].reshape(n, D, -1).transpose(2, 0, 1)
    if n and (r[:, 0] < 0).any():
        r = r[:, 1:]
    return r


# ---------------------------------------------------------------------------------------------
# the laws of a round of dataset picks

def assert_rounds_are_permutations(rounds, D: int, tag=""):
    """Every round (last axis, D picks) visits each dataset once."""
    r = np.asarray(rounds).reshape(-1, D)
    bad = (np.sort(r, axis=1) != np.arange(D)).any(axis=1)
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {len(r)} rounds are not permutations, e.g. {r[bad][0]}"


def round_laws(rounds, D: int, group: int = 16) -> dict:
    """p-values of the laws of uniformly random rounds, for rounds [E, R, D] (env, round, pick):

      first      the first pick of a round is uniform
      order      the full order is uniform over all D! orders (D <= 6)
      gap        (pick1 - pick0) mod D is uniform on [1, D)
      where0     the place of dataset 0 within the round is uniform
      carry      the first pick of round r+1 is independent of the last pick of round r (the two
                 coarsened to `group` classes when D is larger)
    """
    r = np.asarray(rounds).astype(np.int64)
    assert r.ndim == 3 and r.shape[2] == D
    flat = r.reshape(-1, D)
    out = {"first": uniform_p(flat[:, 0], D)}
    if D <= 6:
        code = {p: i for i, p in enumerate(permutations(range(D)))}
        keys = (flat * (D ** np.arange(D))).sum(1)
        lut = {sum(c * D ** i for i, c in enumerate(p)): k for p, k in code.items()}
        out["order"] = uniform_p(np.vectorize(lut.__getitem__)(keys), len(code))
    if D > 2:  # two different picks: the gap is never 0
        out["gap"] = uniform_p((flat[:, 1] - flat[:, 0]) % D - 1, D - 1)
    out["where0"] = uniform_p(np.argmax(flat == 0, axis=1), D)
    if r.shape[1] >= 2:
        last, kl = coarse(r[:, :-1, -1], D, group)
        first, kf = coarse(r[:, 1:, 0], D, group)
        out["carry"] = independence_p(last, first, kl, kf)
    return out


def failing(ps: dict) -> dict:
    return {k: v for k, v in ps.items() if v < ALPHA}


def rejects(ps: dict) -> bool:
    return bool(failing(ps))
