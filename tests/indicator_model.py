"""The indicators of `gte_build_indicators` (include/gte.h, struct gte_indicator_spec) on the host, stated
twice: `LOOP` is the header's table as plain loops over t and k on IEEE doubles (Python floats: one
rounding per operation, nothing fused), `VECTOR` an independently written NumPy statement of each kind,
vectorised over t with the terms still added in k order, so the two agree bit for bit.
tests/test_indicators_cpu.py holds them equal; the GPU tests compare the device's banks with
`build_bank`.  Plus the fixture both use."""
import functools
import math

import numpy as np

from gym_trading_env_amd import signals

NAN = float("nan")
KINDS = signals.IND_KINDS
WINDOWED = ("sma", "std", "zscore", "max", "min")


def _div(a, b):
    """a / b as IEEE does it (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _f32(y):
    with np.errstate(all="ignore"):
        return np.asarray(y, dtype=np.float64).astype(np.float32)


# ---- the header's table, line by line: x is a tuple of Python floats, the result a list of floats ----

def loop_value(x, n):
    return list(x)


@functools.lru_cache(maxsize=128)
def loop_sma(x, n):
    y = [NAN] * len(x)
    for t in range(n - 1, len(x)):
        s = 0.0
        for k in range(n):
            s += x[t - n + 1 + k]
        y[t] = s / n
    return y


@functools.lru_cache(maxsize=128)
def _loop_mean_sd(x, n):
    m, sd = loop_sma(x, n), [NAN] * len(x)
    for t in range(n - 1, len(x)):
        q, mt = 0.0, m[t]
        for k in range(n):
            d = x[t - n + 1 + k] - mt
            q += d * d
        v = q / n
        sd[t] = v if v != v else math.sqrt(v)
    return m, sd


def loop_std(x, n):
    return _loop_mean_sd(x, n)[1]


def loop_zscore(x, n):
    m, sd = _loop_mean_sd(x, n)
    return [NAN if t < n - 1 else _div(x[t] - m[t], sd[t]) for t in range(len(x))]


def _loop_extreme(x, n, greater):
    y = [NAN] * len(x)
    for t in range(n - 1, len(x)):
        m, bad = x[t - n + 1], x[t - n + 1] != x[t - n + 1]
        for k in range(1, n):
            v = x[t - n + 1 + k]
            bad = bad or v != v
            if (v > m) if greater else (v < m):
                m = v
        y[t] = NAN if bad else m
    return y


def loop_max(x, n):
    return _loop_extreme(x, n, True)


def loop_min(x, n):
    return _loop_extreme(x, n, False)


def loop_diff(x, n):
    return [NAN if t < n else x[t] - x[t - n] for t in range(len(x))]


def loop_roc(x, n):
    return [NAN if t < n else _div(x[t], x[t - n]) - 1.0 for t in range(len(x))]


def loop_ema(x, n):
    a = 2.0 / (n + 1.0)
    y = [x[0]] * len(x)
    for t in range(1, len(x)):
        d = x[t] - y[t - 1]
        y[t] = y[t - 1] + a * d
    return y


def loop_rsi(x, n):
    y = [NAN] * len(x)
    su = sd = au = ad = 0.0
    for t in range(1, len(x)):
        c = x[t] - x[t - 1]
        g = c if c > 0 else 0.0
        l = -c if c < 0 else 0.0
        if t <= n:
            su += g
            sd += l
            if t < n:
                continue
            au, ad = su / n, sd / n
        else:
            au, ad = (au * (n - 1) + g) / n, (ad * (n - 1) + l) / n
        y[t] = 100.0 - _div(100.0, 1.0 + _div(au, ad))
    return y


LOOP = dict(value=loop_value, sma=loop_sma, std=loop_std, zscore=loop_zscore, max=loop_max, min=loop_min,
            diff=loop_diff, roc=loop_roc, ema=loop_ema, rsi=loop_rsi)


# ---- the second statement: NumPy over t; sums still run over k in order ----

def _windows(x, n):
    """L = T - n + 1 windows; term k of all of them is x[k : k + L]"""
    return max(len(x) - n + 1, 0)


def _tail(T, n_nan, values):
    y = np.full(T, np.nan)
    if n_nan < T:
        y[n_nan:] = values
    return y


def vec_value(x, n):
    return x.copy()


def _vec_mean(x, n):
    L = _windows(x, n)
    s = np.zeros(L)
    for k in range(n if L else 0):
        s = s + x[k:k + L]
    return s / n


def vec_sma(x, n):
    return _tail(len(x), n - 1, _vec_mean(x, n))


def _vec_sd(x, n, m):
    L = _windows(x, n)
    q = np.zeros(L)
    for k in range(n if L else 0):
        d = x[k:k + L] - m
        q = q + d * d
    return np.sqrt(q / n)


def vec_std(x, n):
    return _tail(len(x), n - 1, _vec_sd(x, n, _vec_mean(x, n)))


def vec_zscore(x, n):
    m = _vec_mean(x, n)
    return _tail(len(x), n - 1, (x[n - 1:] - m) / _vec_sd(x, n, m))


def _vec_extreme(x, n, greater):
    L = _windows(x, n)
    if not L:
        return np.full(len(x), np.nan)
    m, bad = x[:L].copy(), np.isnan(x[:L])
    for k in range(1, n):
        v = x[k:k + L]
        bad |= np.isnan(v)
        m = np.where((v > m) if greater else (v < m), v, m)
    return _tail(len(x), n - 1, np.where(bad, np.nan, m))


def vec_max(x, n):
    return _vec_extreme(x, n, True)


def vec_min(x, n):
    return _vec_extreme(x, n, False)


def vec_diff(x, n):
    return _tail(len(x), n, x[n:] - x[:len(x) - n] if n < len(x) else 0)


def vec_roc(x, n):
    return _tail(len(x), n, x[n:] / x[:len(x) - n] - 1.0 if n < len(x) else 0)


def vec_ema(x, n):
    """(a recurrence has no second order of evaluation: NumPy scalars instead of Python floats, and
    pandas' ewm within a bound in the CPU test)"""
    a, y = np.float64(2.0) / np.float64(n + 1.0), x.copy()
    for t in range(1, len(x)):
        y[t] = y[t - 1] + a * (x[t] - y[t - 1])
    return y


def vec_rsi(x, n):
    T = len(x)
    c = np.diff(x)                                   # c[j - 1] = x[j] - x[j - 1]
    g, l = np.where(c > 0, c, 0.0), np.where(c < 0, -c, 0.0)
    y = np.full(T, np.nan)
    if n >= T:
        return y
    nn = np.float64(n)
    au, ad = np.add.accumulate(g[:n])[-1] / nn, np.add.accumulate(l[:n])[-1] / nn   # (in order, unlike sum())
    for t in range(n, T):
        if t > n:
            au, ad = (au * np.float64(n - 1) + g[t - 1]) / nn, (ad * np.float64(n - 1) + l[t - 1]) / nn
        y[t] = 100.0 - 100.0 / (1.0 + au / ad)
    return y


VECTOR = dict(value=vec_value, sma=vec_sma, std=vec_std, zscore=vec_zscore, max=vec_max, min=vec_min,
              diff=vec_diff, roc=vec_roc, ema=vec_ema, rsi=vec_rsi)


def row(kind, x, n, statement="vector"):
    """f32 [T] of one kind over the f64 series x"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        if statement == "loop":
            return _f32(LOOP[kind](tuple(float(v) for v in x), int(n)))  # (a tuple: SMA, STD, ZSCORE share loops)
        return _f32(VECTOR[kind](x, int(n)))


# ---- a bank from specs, as the kernel serves them ----

def source_of(spec, data):
    """The f64 series a spec reads, or None where the header calls the spec invalid.  data: dict with
    close / high / low f64 [T] (high / low may be None), features f32 [T, F] (the static columns),
    inputs f32 [C_in, T] or None."""
    kind, src, col, n = (int(spec[f]) for f in ("kind", "source", "column", "n"))
    if not 0 <= kind < len(KINDS) or (KINDS[kind] != "value" and not 1 <= n <= signals.IND_MAX_WINDOW):
        return None
    if src in (signals.SRC_CLOSE, signals.SRC_HIGH, signals.SRC_LOW):
        x = data[("close", "high", "low")[src]]
        return None if x is None else np.asarray(x, np.float64)
    if src == signals.SRC_FEATURE:
        f = data["features"]
        return f[:, col].astype(np.float64) if 0 <= col < f.shape[1] else None
    if src == signals.SRC_INPUT:
        i = data.get("inputs")
        return i[col].astype(np.float64) if i is not None and 0 <= col < i.shape[0] else None
    return None


def build_bank(specs, data, T=None, statement="vector"):
    """f32 [len(specs), T]: row s is spec s over the first T rows of `data` (equal specs are computed
    once)."""
    T = len(data["close"]) if T is None else T
    out, seen = np.full((len(specs), T), np.nan, np.float32), {}
    for s, spec in enumerate(specs):
        x = source_of(spec, data)
        if x is None:
            continue
        kind = KINDS[int(spec["kind"])]
        key = (kind, int(spec["source"]), int(spec["column"]), 1 if kind == "value" else int(spec["n"]))
        if key not in seen:
            seen[key] = row(kind, x[:T], key[3], statement)
        out[s] = seen[key]
    return out


T_FIX = 2500
N_FIX = (1, 2, 15, 16, 17, 63, 64, 65, 200, 1025, 4096)
SPECIAL = 2   # the feature column with the planted values
FLAT = (1200, 1260)


@functools.lru_cache(maxsize=None)
def fixture():
    """(data, specs): close a random walk near 100 with high / low around it; three static feature
    columns, column 2 with NaN, +-inf, -0.0 beside +0.0, subnormals and 60 equal values planted; a
    two-row input bank; every kind x every source x N_FIX (feature columns and input rows in turn),
    then seven specs the header calls invalid."""
    rng = np.random.default_rng(17)
    T = T_FIX
    close = 100.0 * np.exp(np.cumsum(rng.normal(0, 1e-2, T)))
    high = close * (1.0 + 5e-3 * np.abs(rng.normal(0, 1, T)))
    low = close * (1.0 - 5e-3 * np.abs(rng.normal(0, 1, T)))
    feat = np.stack([rng.normal(0, 1, T), np.cumsum(rng.normal(0, 1, T)), rng.normal(0, 1, T)], 1).astype(np.float32)
    f = feat[:, SPECIAL]
    f[300] = np.nan
    f[600], f[620] = np.inf, -np.inf
    f[900:904] = [0.0, -0.0, -0.0, 0.0]
    f[1000:1010] = np.float32(1.4e-45) * np.arange(1, 11, dtype=np.float32) * np.float32(-1) ** np.arange(10)
    f[FLAT[0]:FLAT[1]] = np.float32(3.25)
    f[2000:2070] = 0.0   # (and a flat stretch of zeros: ROC divides by it)
    inputs = np.stack([np.exp(rng.normal(8, 1, T)), np.cumsum(rng.normal(0, 1, T))]).astype(np.float32)
    data = dict(close=close, high=high, low=low, features=feat, inputs=inputs)
    for v in data.values():
        v.setflags(write=False)
    kind, src, col, n = [], [], [], []
    for k in range(len(KINDS)):
        for s in range(len(signals.IND_SOURCES)):
            for i, w in enumerate(N_FIX):
                kind.append(k), src.append(s), n.append(w)
                col.append((SPECIAL + i) % 3 if s == signals.SRC_FEATURE else i % 2 if s == signals.SRC_INPUT else 0)
    specs = signals.indicators(np.array(kind), np.array(n), np.array(src), np.array(col))
    bad = np.zeros(7, dtype=signals.INDICATOR_DTYPE)
    bad["kind"] = [99, signals.IND_SMA, signals.IND_EMA, signals.IND_SMA, signals.IND_RSI, signals.IND_MAX, -1]
    bad["n"] = [5, 0, 4097, 5, 5, 5, 5]
    bad["source"] = [0, 0, 0, signals.SRC_FEATURE, signals.SRC_INPUT, 7, 0]
    bad["column"] = [0, 0, 0, 3, 2, 0, 0]
    specs = np.concatenate([specs, bad])
    specs.setflags(write=False)
    return data, specs
