"""The table that holds `DeviceArray` (gym-trading-env_amd/device_array.py) to NumPy: formulas a
user writes with `np.` and operators, the operands they run over, the bound of each class and the
checks, shared by tests/test_device_array_cpu.py (CPU and meta tensors) and
tests/test_gpu_device_array.py (HBM tensors).  DESIGN.md "DeviceArray and NumPy" states the rule.

A row is (name, formula over a namespace `n`, class, capturable).  The namespace of one operand
kind (`host_namespace`) holds

    x, y      columns [N] of the kind, with the planted values below
    u, v, d   the same for floats; for int32 `u` stays below 2**25 and `v`, `d` are small and nonzero
              (sums, differences, products and quotients of them stay inside int32 and divide by no
              zero: NumPy's result is platform-dependent there); for bool `d` is all True
    M, W      windows [R, N] with planted values;  F, f, P, Q, q: finite windows / columns for the
              reductions (P positive, Q and q near 1 so that products stay in range)
    c, C      a bool column / window;  step: an int32 column (the env's `step`)
    s         the scalar of the scalar kind;  a: a host ndarray [N]

Classes and what a device result is held to (a `host` row must come back as a host value, equal
to NumPy's in dtype and bits; where NumPy raises, DeviceArray must raise):

    exact           the bits of NumPy's result (NaNs: the same places, payload open)
    transcendental  ulp error against mpmath at 110 digits; on CPU tensors at most NumPy's own
                    worst error on the same inputs + 1 ulp, on the GPU GPU_ULP[...] + 1 ulp
    reduction       against math.fsum / mpmath: `reduction_bound` below; integers exactly

GPU_ULP: the worst ulp error measured on an MI355X (ROCm 7.0, torch 2.10) per row and result
dtype over these fixed inputs (rounded up to 0.001); the test allows one ulp more (a driver library
update).  The worst of all is 1.62 ulp (float32 log of a quotient); float64 stays below 1.2 ulp.
Nothing comes near the 4 ulp at which a function would have to leave the device.
"""
import math
import operator
import warnings
from types import SimpleNamespace

import numpy as np

try:
    import mpmath
except ImportError:  # no mpmath: np.longdouble (64-bit mantissa on x86) is the reference then
    mpmath = None

N, R = 257, 7
CARRIED = ("bool", "int32", "int64", "float32", "float64")

# (row name, result dtype) -> worst ulp error measured on the GPU; see the module docstring
GPU_ULP = {
    ("call_rolling_reward", "float32"): 1.614, ("call_rolling_reward", "float64"): 1.032,
    ("doc_log_return", "float32"): 1.536, ("doc_log_return", "float64"): 0.598,
    ("doc_log_return_planted", "float32"): 1.488, ("doc_log_return_planted", "float64"): 0.574,
    ("op_pow", "float32"): 1.128, ("op_pow", "float64"): 1.067,
    ("op_pow_float", "float32"): 0.885, ("op_pow_float", "float64"): 0.987,
    ("op_pow_ndarray", "float32"): 0.899, ("op_pow_ndarray", "float64"): 1.088,
    ("op_pow_scalar", "float32"): 0.500, ("op_pow_scalar", "float64"): 0.565,
    ("rop_pow_ndarray", "float32"): 0.813, ("rop_pow_ndarray", "float64"): 1.021,
    ("rop_pow_scalar", "float32"): 1.005, ("rop_pow_scalar", "float64"): 0.999,
    ("ufunc_arctan", "float32"): 1.554, ("ufunc_arctan", "float64"): 1.162,
    ("ufunc_cos", "float32"): 0.918, ("ufunc_cos", "float64"): 0.693,
    ("ufunc_cosh", "float32"): 0.532, ("ufunc_cosh", "float64"): 0.525,
    ("ufunc_exp", "float32"): 0.577, ("ufunc_exp", "float64"): 0.737,
    ("ufunc_exp2", "float32"): 0.621, ("ufunc_exp2", "float64"): 0.660,
    ("ufunc_expm1", "float32"): 0.970, ("ufunc_expm1", "float64"): 1.193,
    ("ufunc_log", "float32"): 1.522, ("ufunc_log", "float64"): 0.565,
    ("ufunc_log10", "float32"): 1.554, ("ufunc_log10", "float64"): 0.606,
    ("ufunc_log1p", "float32"): 0.500, ("ufunc_log1p", "float64"): 1.000,
    ("ufunc_log2", "float32"): 0.948, ("ufunc_log2", "float64"): 0.512,
    ("ufunc_power", "float32"): 1.128, ("ufunc_power", "float64"): 1.067,
    ("ufunc_power_scalar", "float32"): 1.024, ("ufunc_power_scalar", "float64"): 1.198,
    ("ufunc_sin", "float32"): 0.853, ("ufunc_sin", "float64"): 0.688,
    ("ufunc_sinh", "float32"): 0.594, ("ufunc_sinh", "float64"): 0.588,
    ("ufunc_tan", "float32"): 1.445, ("ufunc_tan", "float64"): 0.772,
    ("ufunc_tanh", "float32"): 0.932, ("ufunc_tanh", "float64"): 0.584,
}

COLUMN_KINDS = ("f64", "f32", "i32", "bool")
SCALARS = {"pyfloat": 0.5, "pyint": 2, "pybool": True, "npf64": np.float64(0.5),
           "npf32": np.float32(0.5), "npi64": np.int64(2)}
NDARRAYS = {"f64": np.float64, "f32": np.float32}
DEVICE_NAMES = ("x", "y", "u", "v", "d", "M", "W", "F", "f", "P", "Q", "q", "c", "C", "step")


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
def _float_operands(dt, rng):
    tiny = np.finfo(dt).smallest_subnormal
    big = 1e300 if dt == np.float64 else 3e38
    planted = [0.0, -0.0, np.nan, np.inf, -np.inf, tiny, big, 2.5, -2.5, 0.5, -0.5, 1.5, -1.5, -big, -tiny]

    def column(first):
        v = rng.uniform(-3, 3, N)
        v[20:30] = -np.abs(v[20:30])  # a negative run
        v[first:first + len(planted)] = planted
        return v
    x, y = column(0), column(40)
    y[0], y[3], y[4] = 0.0, np.inf, np.inf  # 0/0, inf-inf, -inf+inf; never +0 against -0 (max / min)
    M, W = rng.uniform(-3, 3, (R, N)), rng.uniform(-3, 3, (R, N))
    M[2, 5:5 + len(planted)] = planted
    M[5, 100:100 + len(planted)] = planted[::-1]
    W[4, 60:60 + len(planted)] = planted
    F, P = rng.uniform(-2, 2, (R, N)), rng.uniform(0.5, 2, (R, N))
    Q = rng.uniform(0.9, 1.1, (R, N)) * np.where(rng.uniform(size=(R, N)) < 0.05, -1, 1)
    o = dict(x=x, y=y, M=M, W=W, F=F, f=rng.uniform(-2, 2, N), P=P, Q=Q, q=Q[3].copy())
    o = {k: v.astype(dt) for k, v in o.items()}
    o.update(u=o["x"], v=o["y"], d=o["y"])
    return o


def _int_operands(rng):
    planted = [0, -1, 2 ** 24 + 1, 2 ** 31 - 1, -(2 ** 24 + 1), -(2 ** 31 - 1), 7, -7, 1]
    small = lambda shape: rng.choice([-9, -5, -3, -2, -1, 1, 2, 3, 4, 7], shape)  # noqa: E731
    x = rng.integers(-1000, 1000, N)
    x[:len(planted)] = planted
    u = np.where(np.abs(x) > 2 ** 24 + 1, 2 ** 24 - 3, x)
    M = rng.integers(-1000, 1000, (R, N))
    M[2, 5:5 + len(planted)] = planted
    Q = np.ones((R, N), np.int64)
    Q.reshape(-1)[rng.choice(R * N, 40, replace=False)] = [2] * 30 + [-1] * 7 + [3] * 3
    q = np.ones(N, np.int64)
    q[rng.choice(N, 20, replace=False)] = [2] * 12 + [-1] * 5 + [3] * 3
    o = dict(x=x, y=small(N), u=u, M=M, W=small((R, N)), F=rng.integers(-1000, 1000, (R, N)),
             f=rng.integers(-1000, 1000, N), P=rng.integers(1, 50, (R, N)), Q=Q, q=q)
    o = {k: v.astype(np.int32) for k, v in o.items()}
    o.update(v=o["y"], d=o["y"])
    return o


def _bool_operands(rng):
    o = {k: rng.uniform(size=(N,) if k in "xyfq" else (R, N)) < 0.5 for k in "xyMWFfPQq"}
    o.update(u=o["x"], v=o["y"], d=np.ones(N, bool))
    return o


_NS, _DEVICE = {}, {}


def host_namespace(col, scalar="pyfloat", nd="f64"):
    """The operands of one kind as host values (built once, never written to)."""
    key = (col, scalar, nd)
    if key not in _NS:
        if (col,) not in _NS:
            rng = np.random.default_rng(COLUMN_KINDS.index(col) + 20240)
            o = (_float_operands(np.float64 if col == "f64" else np.float32, rng) if col[0] == "f"
                 else _int_operands(rng) if col == "i32" else _bool_operands(rng))
            o.update(c=rng.uniform(size=N) < 0.5, C=rng.uniform(size=(R, N)) < 0.6,
                     step=rng.integers(0, 6, N).astype(np.int32))
            for v in o.values():
                v.setflags(write=False)
            _NS[(col,)] = o
        a = np.random.default_rng(7).uniform(0.5, 2.0, N).astype(NDARRAYS[nd])
        a.setflags(write=False)
        _NS[key] = SimpleNamespace(**_NS[(col,)], s=SCALARS[scalar], a=a, kind=key)
    return _NS[key]


def device_namespace(host, device):
    """The same operands with every column a DeviceArray on `device` (`s` and `a` stay host values:
    they are what a caller passes from the host)."""
    import torch
    from gym_trading_env_amd.device_array import DeviceArray
    key = (host.kind[0], str(device))
    if key not in _DEVICE:  # (the formulas never write to an operand: one copy per column kind)
        _DEVICE[key] = {k: DeviceArray(torch.from_numpy(getattr(host, k).copy()).to(device)) for k in DEVICE_NAMES}
    return SimpleNamespace(**{**vars(host), **_DEVICE[key]})


# ------------------------------------------------------------------------------------------------
# the high-precision reference
# ------------------------------------------------------------------------------------------------
class _Mp:
    """The transcendental functions at 110 digits."""
    def __init__(self):
        self.m = mpmath.mp.clone()
        self.m.dps = 110

    def num(self, v):
        return self.m.mpf(int(v)) if isinstance(v, (int, np.integer, bool, np.bool_)) else self.m.mpf(float(v))

    def __getattr__(self, name):
        m = self.m
        special = {"arctan": m.atan, "log2": lambda t: m.log(t) / m.log(2), "exp2": lambda t: m.power(2, t)}
        return special[name] if name in special else getattr(m, name)

    def value(self, r):
        """-> (float64 nearest the reference, the reference) or None where it is not a real number"""
        if isinstance(r, self.m.mpc):
            if r.imag != 0:
                return None
            r = r.real
        return None if not self.m.isfinite(r) else r

    def err_ulps(self, got, r, spacing):
        return float(abs(self.m.mpf(float(got)) - r) / self.m.mpf(float(spacing)))


class _LongDouble:
    """The fallback without mpmath: np.longdouble (about 3 more digits than float64)."""
    def num(self, v):
        return np.longdouble(v)

    def __getattr__(self, name):
        return getattr(np, name)

    def value(self, r):
        return r if np.isfinite(r) else None

    def err_ulps(self, got, r, spacing):
        return float(abs(np.longdouble(got) - r) / np.longdouble(spacing))


REF = _Mp() if mpmath is not None else _LongDouble()


def worst_ulp(values, ref_fn, args):
    """The worst error of the finite `values` (float array) in units of the spacing of their dtype at
    the reference, `ref_fn(REF, *args elementwise)`; entries whose reference is no finite real number
    are left to the NaN / inf placement check."""
    values = np.asarray(values)
    args = np.broadcast_arrays(*[np.asarray(a) for a in args], np.empty(values.shape))[:-1]
    fi = np.finfo(values.dtype)
    worst = 0.0
    with np.errstate(all="ignore"):
        for i in np.ndindex(values.shape):
            if not np.isfinite(values[i]):
                continue
            try:
                r = REF.value(ref_fn(REF, *[REF.num(a[i]) for a in args]))
            except (ValueError, ZeroDivisionError, OverflowError):
                r = None
            if r is None:
                continue
            at = min(abs(float(r)), float(fi.max))  # the spacing of the dtype at the reference's size
            spacing = np.spacing(values.dtype.type(at))
            if not np.isfinite(spacing):
                spacing = np.spacing(fi.max)
            worst = max(worst, REF.err_ulps(values[i], r, spacing))
    return worst


def _unit_roundoff(dtype):
    return float(np.finfo(dtype).eps) / 2


def reduction_bound(kind, x, axis, dtype, ddof=0):
    """(reference, bound) of reduction `kind` over float data `x` along `axis` (None: all of it) for a
    result of float `dtype`; |computed - reference| <= bound must hold for ANY order of the
    operations, with u the unit roundoff of `dtype` and n the number of values reduced:

      sum      n u sum|x|           (each of the n-1 additions errs by u of a partial sum <= sum|x|)
      mean     the sum's bound / n + u |mean|                      (one more rounding: the division)
      cumsum   the sum's bound of every prefix
      prod     (n-1) u |prod|, cumprod the same per prefix          (n-1 roundings, each relative u)
      var      two passes.  The mean m^ is off by e = n u mean|x| + u |m| (above).  Each deviation
               d^_i = fl(x_i - m^) is off by e + u |d_i|, its square by 2 |d_i| (e + u |d_i|) + e^2 and
               one rounding u d_i^2; the n squares are summed (n u S with S = sum d_i^2) and divided
               (u S).  Together, to first order in u:  ((n + 4) u S + 2 e sum|d_i| + n e^2) / (n - ddof),
               taken twice to cover the second-order terms.  Updating formulas (Welford, pairwise
               merges) err by n u sqrt(1 + m^2 / var) var <= n u (S + n |m| sigma) / n, which the
               e sum|d_i| term covers (Chan, Golub, LeVeque 1983).
      std      sqrt: |s^ - s| <= the variance's bound / s (s^ + s >= s), + u s for the root's rounding
    """
    u = _unit_roundoff(dtype)
    x = np.asarray(x)
    if axis is None:
        x, axis = x.reshape(-1), 0
    x = np.moveaxis(x, axis, 0)
    n = x.shape[0]
    ref = np.empty(x.shape[1:] if kind not in ("cumsum", "cumprod") else x.shape, dtype=object)
    bound = np.empty(ref.shape, dtype=object)
    m = REF.m if mpmath is not None else None
    num = (lambda v: m.mpf(float(v))) if m is not None else np.longdouble
    for i in np.ndindex(x.shape[1:]):
        col = [float(v) for v in x[(slice(None),) + i]]
        if kind in ("sum", "mean"):
            s, sa = math.fsum(col), math.fsum(abs(v) for v in col)
            if kind == "sum":
                ref[i], bound[i] = num(s), n * u * sa
            else:  # (fsum's sum is the exact one correctly rounded: its error is far below the bound)
                ref[i], bound[i] = num(s) / n, u * sa + u * abs(s) / n
        elif kind == "cumsum":
            for k in range(n):
                ref[(k,) + i] = num(math.fsum(col[:k + 1]))
                bound[(k,) + i] = (k + 1) * u * math.fsum(abs(v) for v in col[:k + 1])
        elif kind in ("prod", "cumprod"):
            p = num(1)
            for k in range(n):
                p = p * num(col[k])
                if kind == "cumprod":
                    ref[(k,) + i], bound[(k,) + i] = p, k * u * abs(p)
            if kind == "prod":
                ref[i], bound[i] = p, (n - 1) * u * abs(p)
        else:  # var, std
            vals = [num(v) for v in col]
            mean = sum(vals, num(0)) / n
            dev = [v - mean for v in vals]
            S, D = sum((t * t for t in dev), num(0)), sum((abs(t) for t in dev), num(0))
            e = n * u * sum((abs(v) for v in vals), num(0)) / n + u * abs(mean)
            var = S / (n - ddof)
            bvar = 2 * ((n + 4) * u * S + 2 * e * D + n * e * e) / (n - ddof)
            if kind == "var":
                ref[i], bound[i] = var, bvar
            else:
                s = var ** 0.5 if m is None else m.sqrt(var)
                ref[i] = s  # (a constant column: |s^ - 0| = sqrt(var^) <= sqrt(the variance's bound))
                bound[i] = (bvar / s if s > 0 else (bvar ** 0.5 if m is None else m.sqrt(bvar))) + u * s
    return ref, bound


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, name, f, cls, capturable=None, ref=None, args=None, red=None, sync=False, host_on=(),
                 cpu_host=False):
        """ref / args (transcendental): the reference `ref(REF, *values)` over the elements of the host
        arrays `args(n)` — the exact-class intermediates of the formula, computed by NumPy.
        red (reduction): (kind, the host array reduced as a function of n, axis, ddof).
        sync: the result stays on the device but its SHAPE is data (boolean indexing): not capturable
        and not evaluable on meta tensors.  host_on: column kinds (or a predicate of the operand kind) for
        which this device row is computed on the host although NumPy's result has a carried dtype.
        cpu_host: a float result is NumPy's own over CPU tensors (device_array._CPU_INEXACT: torch's CPU
        sqrt and fmod are not the IEEE operations); on the GPU and on meta tensors it is a device row."""
        assert cls in ("exact", "transcendental", "reduction", "host")
        self.name, self.f, self.cls = name, f, cls
        self.capturable = (cls != "host" and not sync) if capturable is None else capturable
        self.ref, self.args, self.red, self.sync, self.cpu_host = ref, args, red, sync, cpu_host
        self.host_on = host_on if callable(host_on) else (lambda kind: kind[0] in host_on)

    def __repr__(self):
        return self.name


ROWS = []


def row(*a, **k):
    ROWS.append(Row(*a, **k))


# -- documented reward and metric formulas -------------------------------------------------------
_LOG = dict(ref=lambda m, t: m.log(t))
# docs/source/customization.rst:13-14, examples/example_vectorized_environment.py:39-40 (also
# tests/test_gpu_vector_api.py `reward_function`, custom_callables.reward_log_return_example)
row("doc_log_return", lambda n: np.log(n.P[-1] / n.P[-2]), "transcendental", args=lambda n: (n.P[-1] / n.P[-2],), **_LOG)
row("doc_log_return_planted", lambda n: np.log(n.x / n.y), "transcendental", args=lambda n: (n.x / n.y,), **_LOG)
# docs/source/customization.rst:39: the position-changes metric, of one env and of every env
row("doc_position_changes", lambda n: np.sum(np.diff(n.x) != 0), "exact")
row("doc_position_changes_batch", lambda n: np.sum(np.diff(n.M, axis=0) != 0, axis=0), "exact")
# the callables of tests/test_gpu_vector_api.py and tests/test_gpu_graph_log.py
row("call_valuation_ratio", lambda n: n.x / 1000.0, "exact")
row("call_exposure_change", lambda n: np.where(n.step == 0, 0.0, n.u - n.v), "exact")
row("call_return_minus_turnover", lambda n: n.x / n.y - 1 - 1e-4 * abs(n.u - n.v), "exact")
# _rolling_reward, in its two parts (the error of the mean would count many times over in ulps of
# the logarithm): the reference value over the episode mask, and the reward from it
row("call_rolling_reference", lambda n: np.where(n.C, n.P, n.P[-1]).mean(axis=0), "reduction",
    red=("mean", lambda n: np.where(n.C, n.P, n.P[-1]), 0, 0))
# (the turnover term stays far below the logarithm, as position changes do below returns: where the
# two cancel, the rounding of the logarithm counts many times over in ulps of the difference)
row("call_rolling_reward", lambda n: np.log(n.P[-1] / n.P[0]) - 1e-4 * abs(n.q * 1), "transcendental",
    ref=lambda m, t, w: m.log(t) - w, args=lambda n: (n.P[-1] / n.P[0], 1e-4 * abs(n.q * 1)))
# an int32 column with a Python float, and np.where over two scalars (the env-level test uses these)
row("mix_step_times_half", lambda n: n.step * 0.5, "exact")
row("mix_int_times_half", lambda n: n.x * 0.5, "exact")
row("mix_where_two_scalars", lambda n: np.where(n.x > 0, 1, 0.5), "exact")

# -- every entry of _UFUNCS ----------------------------------------------------------------------
for _n, _arg in (("negative", "x"), ("positive", "x"), ("absolute", "x"), ("fabs", "x"), ("sign", "x"),
                 ("sqrt", "x"), ("square", "v"), ("floor", "x"), ("ceil", "x"), ("rint", "x"), ("trunc", "x"),
                 ("reciprocal", "v"), ("isnan", "x"), ("isfinite", "x"), ("isinf", "x"), ("logical_not", "x"),
                 ("invert", "x")):
    row(f"ufunc_{_n}", (lambda n, _f=getattr(np, _n), _a=_arg: _f(getattr(n, _a))), "exact",
        # (torch has no integer reciprocal and no abs / floor / ceil / trunc of bools)
        host_on=("i32",) if _n == "reciprocal" else ("bool",) if _n in ("absolute", "floor", "ceil", "trunc") else (),
        cpu_host=_n == "sqrt")
for _n in ("exp", "expm1", "exp2", "log", "log2", "log10", "log1p", "sin", "cos", "tan", "tanh", "sinh",
           "cosh", "arctan"):
    row(f"ufunc_{_n}", (lambda n, _f=getattr(np, _n): _f(n.x)), "transcendental",
        ref=(lambda m, t, _n=_n: getattr(m, _n)(t)), args=lambda n: (n.x,))
for _n, _ab in (("add", "uv"), ("subtract", "uv"), ("multiply", "uv"), ("divide", "xy"), ("true_divide", "xy"),
                ("floor_divide", "ud"), ("remainder", "ud"), ("maximum", "xy"), ("minimum", "xy"),
                ("fmax", "xy"), ("fmin", "xy"), ("greater", "xy"), ("greater_equal", "xy"), ("less", "xy"),
                ("less_equal", "xy"), ("equal", "xy"), ("not_equal", "xy"), ("logical_and", "xy"),
                ("logical_or", "xy"), ("bitwise_and", "xy"), ("bitwise_or", "xy")):
    row(f"ufunc_{_n}", (lambda n, _f=getattr(np, _n), _ab=_ab: _f(getattr(n, _ab[0]), getattr(n, _ab[1]))), "exact",
        cpu_host=_n in ("floor_divide", "remainder"))
    if _n in ("add", "maximum", "minimum", "fmax", "greater", "logical_and"):
        row(f"ufunc_{_n}_scalar", (lambda n, _f=getattr(np, _n): _f(n.u, n.s)), "exact")
        row(f"ufunc_{_n}_ndarray", (lambda n, _f=getattr(np, _n): _f(n.a, n.u)), "exact", capturable=False)
_POW = dict(ref=lambda m, b, e: m.power(b, e))
row("ufunc_power", lambda n: np.power(n.x, n.y), "transcendental", args=lambda n: (n.x, n.y), **_POW)
row("ufunc_power_scalar", lambda n: np.power(n.v, n.s), "transcendental", args=lambda n: (n.v, n.s), **_POW)
row("ufunc_clip", lambda n: np.clip(n.x, -0.5, 1.5), "exact")

# -- every name of _FUNCTIONS --------------------------------------------------------------------
row("func_where", lambda n: np.where(n.c, n.x, n.y), "exact")
row("func_where_scalar_right", lambda n: np.where(n.c, n.x, n.s), "exact")
row("func_where_scalar_left", lambda n: np.where(n.c, n.s, n.x), "exact")
row("func_where_scalar_and_float", lambda n: np.where(n.x > n.y, n.s, 0.25), "exact")
row("func_where_two_ints", lambda n: np.where(n.c, 1, 0), "exact")
row("func_where_ndarray", lambda n: np.where(n.c, n.x, n.a), "exact", capturable=False)
row("func_where_window", lambda n: np.where(n.C, n.M, n.M[-1]), "exact")
row("func_where_one_argument", lambda n: np.where(n.c), "host")
row("func_clip_scalar_kinds", lambda n: np.clip(n.x, -n.s, n.s), "exact")
row("func_clip_no_lower", lambda n: np.clip(n.x, None, 1.5), "exact")
row("func_clip_no_upper", lambda n: np.clip(n.x, -1.5, None), "exact")
row("func_clip_array_bounds", lambda n: np.clip(n.M, n.f, n.P[0]), "exact", host_on=("bool",))
row("func_clip_a_min_a_max", lambda n: np.clip(n.x, a_min=-1.5, a_max=1.5), "exact")
row("func_clip_min_max", lambda n: np.clip(n.x, min=-1.5, max=1.5), "exact")
row("func_clip_ndarray_bound", lambda n: np.clip(n.x, -1.5, n.a), "exact", capturable=False)
row("func_clip_out", lambda n: np.clip(n.x, -1.5, 1.5, out=np.empty(N)), "host")

_FORMS = (("all", "F", {}), ("axis0", "F", dict(axis=0)), ("axis1_keepdims", "F", dict(axis=1, keepdims=True)),
          ("all_keepdims", "F", dict(keepdims=True)), ("column", "f", {}))
for _n in ("sum", "prod", "mean", "std", "var"):
    for _form, _arg, _kw in _FORMS:
        _arg = {"F": "Q", "f": "q"}[_arg] if _n == "prod" else _arg
        row(f"func_{_n}_{_form}", (lambda n, _f=getattr(np, _n), _a=_arg, _kw=_kw: _f(getattr(n, _a), **_kw)),
            "reduction", red=(_n, (lambda n, _a=_arg: getattr(n, _a)), _kw.get("axis"), 0))
for _n in ("std", "var"):
    row(f"func_{_n}_ddof1", (lambda n, _f=getattr(np, _n): _f(n.F, axis=0, ddof=1)), "reduction",
        red=(_n, lambda n: n.F, 0, 1))
for _n in ("max", "min", "amax", "amin", "any", "all"):
    for _form, _arg, _kw in _FORMS:
        _arg = _arg.replace("F", "M")  # (the planted NaN and infinities are in)
        row(f"func_{_n}_{_form}", (lambda n, _f=getattr(np, _n), _a=_arg, _kw=_kw: _f(getattr(n, _a), **_kw)), "exact")
row("func_sum_tuple_axis", lambda n: np.sum(n.F, axis=(0, 1)), "reduction", red=("sum", lambda n: n.F, None, 0))
row("func_sum_positional_axis", lambda n: np.sum(n.F, 0), "reduction", red=("sum", lambda n: n.F, 0, 0))
row("func_sum_dtype", lambda n: np.sum(n.F, axis=0, dtype=np.float64), "host")
row("func_sum_initial", lambda n: np.sum(n.F, axis=0, initial=1), "host")
row("func_sum_where", lambda n: np.sum(n.F, axis=0, where=n.C), "host")
row("func_sum_out", lambda n: np.sum(n.F, axis=0, out=np.empty(N)), "host")
row("func_sum_ddof", lambda n: np.sum(n.F, ddof=1), "host")  # (NumPy raises: so must DeviceArray)
row("func_mean_dtype", lambda n: np.mean(n.F, axis=0, dtype=np.float64), "host")
row("func_max_initial", lambda n: np.max(n.F, axis=0, initial=0), "host")
row("func_std_dtype", lambda n: np.std(n.F, axis=0, dtype=np.float64), "host")
row("func_var_correction", lambda n: np.var(n.F, axis=0, correction=1), "host")
row("reduce_add", lambda n: np.add.reduce(n.F), "reduction", red=("sum", lambda n: n.F, 0, 0))
row("reduce_add_axis1", lambda n: np.add.reduce(n.F, axis=1, keepdims=True), "reduction", red=("sum", lambda n: n.F, 1, 0))
row("reduce_multiply", lambda n: np.multiply.reduce(n.Q), "reduction", red=("prod", lambda n: n.Q, 0, 0))
row("reduce_maximum", lambda n: np.maximum.reduce(n.M), "exact")
row("reduce_minimum", lambda n: np.minimum.reduce(n.M, axis=1), "exact")
row("reduce_add_dtype", lambda n: np.add.reduce(n.F, dtype=np.float64), "host")
row("reduce_add_initial", lambda n: np.add.reduce(n.F, initial=1), "host")
row("accumulate_add", lambda n: np.add.accumulate(n.F), "host")
row("ufunc_out", lambda n: np.add(n.u, n.v, out=np.empty(N)), "host")
row("ufunc_where", lambda n: np.add(n.f, n.f, out=np.zeros(N), where=n.c), "host")
row("ufunc_dtype", lambda n: np.add(n.f, n.f, dtype=np.float64), "host")

row("func_diff", lambda n: np.diff(n.u), "exact")
row("func_diff_axis0", lambda n: np.diff(n.F, axis=0), "exact")
row("func_diff_twice", lambda n: np.diff(n.F, n=2, axis=0), "exact")
row("func_diff_prepend", lambda n: np.diff(n.F, axis=0, prepend=0), "host")
row("func_diff_append", lambda n: np.diff(n.f, append=1), "host")
row("func_cumsum_axis0", lambda n: np.cumsum(n.F, axis=0), "reduction", red=("cumsum", lambda n: n.F, 0, 0))
row("func_cumsum_column", lambda n: np.cumsum(n.f), "reduction", red=("cumsum", lambda n: n.f, 0, 0))
row("func_cumsum_flat", lambda n: np.cumsum(n.F), "reduction", red=("cumsum", lambda n: n.F, None, 0))
row("func_cumprod_axis0", lambda n: np.cumprod(n.Q, axis=0), "reduction", red=("cumprod", lambda n: n.Q, 0, 0))
row("func_cumprod_column", lambda n: np.cumprod(n.q), "reduction", red=("cumprod", lambda n: n.q, 0, 0))
row("func_cumsum_dtype", lambda n: np.cumsum(n.F, axis=0, dtype=np.float64), "host")
row("func_cumprod_out", lambda n: np.cumprod(n.Q, axis=0, out=np.empty((R, N))), "host")
row("func_round", lambda n: np.round(n.x), "exact")
row("func_around", lambda n: np.around(n.M), "exact")
row("func_round_decimals", lambda n: np.round(n.x, 2), "host")
row("func_round_negative_decimals", lambda n: np.round(n.F, decimals=-1), "host")
row("func_nan_to_num", lambda n: np.nan_to_num(n.x), "exact")
row("func_nan_to_num_nan", lambda n: np.nan_to_num(n.x, nan=7.0), "exact")
row("func_nan_to_num_all", lambda n: np.nan_to_num(n.M, nan=7.0, posinf=1e9, neginf=-1e9), "exact")
row("func_stack", lambda n: np.stack([n.x, n.y]), "exact")
row("func_stack_last_axis", lambda n: np.stack([n.x, n.y, n.u], axis=-1), "exact")
row("func_stack_mixed", lambda n: np.stack([n.x, n.step]), "exact")
row("func_stack_ndarray", lambda n: np.stack([n.x, n.a]), "exact", capturable=False)
row("func_concatenate", lambda n: np.concatenate([n.x, n.y]), "exact")
row("func_concatenate_axis1", lambda n: np.concatenate([n.M, n.W], axis=1), "exact")
row("func_concatenate_flat", lambda n: np.concatenate([n.M, n.W], axis=None), "exact")
row("func_stack_dtype", lambda n: np.stack([n.x, n.y], dtype=np.float64), "host")
row("func_concatenate_out", lambda n: np.concatenate([n.f, n.f], out=np.empty(2 * N)), "host")
row("func_zeros_like", lambda n: np.zeros_like(n.x), "exact")
row("func_ones_like", lambda n: np.ones_like(n.M), "exact")
row("func_full_like", lambda n: np.full_like(n.x, 3), "exact")
row("func_full_like_scalar_kinds", lambda n: np.full_like(n.x, n.s), "exact",  # (a float into integers: C's cast)
    host_on=lambda kind: kind[0] in ("i32", "bool") and kind[1] in ("pyfloat", "npf64", "npf32"))
row("func_zeros_like_dtype", lambda n: np.zeros_like(n.x, dtype=float), "exact")
row("func_ones_like_dtype", lambda n: np.ones_like(n.x, dtype=np.float32), "exact")
row("func_full_like_dtype", lambda n: np.full_like(n.x, 1.5, dtype=np.float64), "exact")
row("func_zeros_like_shape", lambda n: np.zeros_like(n.x, shape=(3,)), "host")

# -- methods, casts, indexing --------------------------------------------------------------------
row("method_mean", lambda n: n.F.mean(), "reduction", red=("mean", lambda n: n.F, None, 0))
row("method_mean_axis0", lambda n: n.F.mean(axis=0), "reduction", red=("mean", lambda n: n.F, 0, 0))
row("method_mean_positional_keepdims", lambda n: n.F.mean(1, keepdims=True), "reduction", red=("mean", lambda n: n.F, 1, 0))
row("method_sum_axis0", lambda n: n.F.sum(axis=0), "reduction", red=("sum", lambda n: n.F, 0, 0))
row("method_max_axis0", lambda n: n.M.max(axis=0), "exact")
row("method_max", lambda n: n.M.max(), "exact")
row("method_min", lambda n: n.M.min(), "exact")
row("method_min_axis1", lambda n: n.M.min(axis=1), "exact")
row("method_sum_dtype", lambda n: n.F.sum(axis=0, dtype=np.float64), "host")
row("astype_float32", lambda n: n.x.astype(np.float32), "exact")
row("astype_float64", lambda n: n.x.astype(np.float64), "exact")
row("astype_python_float", lambda n: n.M.astype(float), "exact")
row("astype_mask_to_int32", lambda n: (n.x > 0).astype(np.int32), "exact")
row("astype_step_to_int64", lambda n: n.step.astype(np.int64), "exact")
row("astype_float16", lambda n: n.f.astype(np.float16), "host")
row("astype_int16", lambda n: n.step.astype(np.int16), "host")
row("index_int", lambda n: n.M[-1], "exact")
row("index_element", lambda n: n.x[3], "exact")
row("index_slice", lambda n: n.M[2:5], "exact")
row("index_strided", lambda n: n.x[::2], "exact")
row("index_two_slices", lambda n: n.M[1:, ::3], "exact")
row("index_bool", lambda n: n.x[n.c], "exact", sync=True)
row("index_bool_computed", lambda n: n.x[n.y > 0], "exact", sync=True)
row("index_bool_columns", lambda n: n.M[:, n.c], "exact", sync=True)

# -- operators, both orientations ----------------------------------------------------------------
for _n, _ab in (("add", "uv"), ("sub", "uv"), ("mul", "uv"), ("truediv", "xy"), ("floordiv", "ud"), ("mod", "ud")):
    _op, _div = getattr(operator, _n), _n in ("floordiv", "mod")
    row(f"op_{_n}", (lambda n, _op=_op, _ab=_ab: _op(getattr(n, _ab[0]), getattr(n, _ab[1]))), "exact", cpu_host=_div)
    row(f"op_{_n}_scalar", (lambda n, _op=_op, _a=_ab[0]: _op(getattr(n, _a), n.s)), "exact", cpu_host=_div)
    row(f"rop_{_n}_scalar", (lambda n, _op=_op, _b=_ab[1]: _op(n.s, getattr(n, _b))), "exact", cpu_host=_div)
    row(f"op_{_n}_ndarray", (lambda n, _op=_op, _a=_ab[0]: _op(getattr(n, _a), n.a)), "exact", capturable=False, cpu_host=_div)
    row(f"rop_{_n}_ndarray", (lambda n, _op=_op, _b=_ab[1]: _op(n.a, getattr(n, _b))), "exact", capturable=False, cpu_host=_div)
row("op_pow_two", lambda n: n.v ** 2, "exact")
# (NumPy's `**` takes the root of floating-point arrays only: an integer column ** 0.5 is a power, below)
row("op_pow_half", lambda n: n.x.astype(np.float64) ** 0.5, "exact", cpu_host=True)
row("op_pow_half_f32", lambda n: n.x.astype(np.float32) ** 0.5, "exact", cpu_host=True)
row("op_pow_scalar", lambda n: n.v ** n.s, "transcendental", args=lambda n: (n.v, n.s),
    cpu_host=lambda kind: kind[0][0] == "f" and kind[1] in ("pyfloat", "npf64", "npf32"), **_POW)  # (0.5: the root)
row("op_pow_minus_one", lambda n: n.v ** -1, "exact", host_on=("i32",))
row("op_pow", lambda n: n.x ** n.y, "transcendental", args=lambda n: (n.x, n.y), **_POW)
row("op_pow_float", lambda n: n.x ** 2.5, "transcendental", args=lambda n: (n.x, 2.5), **_POW)
row("rop_pow_scalar", lambda n: n.s ** n.f, "transcendental", args=lambda n: (n.s, n.f),
    # (an integer power with an array of exponents: NumPy raises for a negative one, by value)
    host_on=lambda kind: kind[0] in ("i32", "bool") and kind[1] in ("pyint", "pybool", "npi64"), **_POW)
row("op_pow_ndarray", lambda n: n.P[0] ** n.a, "transcendental", args=lambda n: (n.P[0], n.a), capturable=False, **_POW)
row("rop_pow_ndarray", lambda n: n.a ** n.f, "transcendental", args=lambda n: (n.a, n.f), capturable=False, **_POW)
for _n in ("lt", "le", "gt", "ge", "eq", "ne"):
    _op = getattr(operator, _n)
    row(f"op_{_n}", (lambda n, _op=_op: _op(n.x, n.y)), "exact")
    row(f"op_{_n}_scalar", (lambda n, _op=_op: _op(n.x, n.s)), "exact")
    row(f"rop_{_n}_scalar", (lambda n, _op=_op: _op(n.s, n.x)), "exact")
    row(f"op_{_n}_ndarray", (lambda n, _op=_op: _op(n.x, n.a)), "exact", capturable=False)
    row(f"rop_{_n}_ndarray", (lambda n, _op=_op: _op(n.a, n.x)), "exact", capturable=False)
row("op_and", lambda n: (n.x > 0) & (n.y > 0), "exact")
row("op_or", lambda n: (n.x > 0) | n.c, "exact")
row("op_and_scalar", lambda n: (n.x > 0) & True, "exact")
row("rop_and_scalar", lambda n: False & (n.x > 0), "exact")
row("op_or_scalar", lambda n: (n.x > 0) | False, "exact")
row("rop_or_scalar", lambda n: True | (n.x > 0), "exact")
row("op_and_columns", lambda n: n.x & n.y, "exact")
row("op_or_columns", lambda n: n.x | n.step, "exact")
row("op_invert_mask", lambda n: ~(n.x > 0), "exact")
row("op_invert", lambda n: ~n.x, "exact")
row("op_neg", lambda n: -n.x, "exact")
row("op_pos", lambda n: +n.x, "exact")
row("op_abs", lambda n: abs(n.x), "exact", host_on=("bool",))

# -- functions that are not mapped ---------------------------------------------------------------
row("unmapped_percentile", lambda n: np.percentile(n.f, 30), "host")
row("unmapped_arctan2", lambda n: np.arctan2(n.x, 2.0), "host")

BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


# ------------------------------------------------------------------------------------------------
# the checks
# ------------------------------------------------------------------------------------------------
class _Spy:
    """A namespace that notes which operands a formula reads."""
    def __init__(self, ns):
        self._ns, self.used = ns, set()

    def __getattr__(self, k):
        self.used.add(k)
        return getattr(self._ns, k)


_USES = {}


def kinds_of(r):
    """The operand kinds row `r` runs over: every column kind, times every scalar kind if it reads
    `s`, times both ndarray kinds if it reads `a`."""
    if r.name not in _USES:
        spy = _Spy(host_namespace("f64"))
        _, _ = evaluate(r, spy)
        _USES[r.name] = spy.used
    used = _USES[r.name]
    return [(c, s, a) for c in COLUMN_KINDS for s in (SCALARS if "s" in used else ("pyfloat",))
            for a in (NDARRAYS if "a" in used else ("f64",))]


def evaluate(r, ns):
    """-> ("value", result) or ("raises", exception)"""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        try:
            return "value", r.f(ns)
        except Exception as e:  # noqa: BLE001 (whatever NumPy raises is the reference)
            return "raises", e


def same_bits(got, want):
    """dtype, shape and bits equal; NaNs in the same places (payload open)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        if not np.array_equal(np.isnan(got), nan):
            return False
        bits = f"u{got.dtype.itemsize}"
        return np.array_equal(got[~nan].view(bits), want[~nan].view(bits))
    return np.array_equal(got, want)


def _describe(a):
    a = np.asarray(a)
    return f"{a.dtype}{list(a.shape)} {a.reshape(-1)[:6]}"


_WANT = {}


def check_case(r, kind, device, where, record=None):
    """Row `r` over the operands of `kind` on torch device `device`, against the rule.  where: "cpu",
    "gpu" (the class bounds differ) or "meta" (dtype and shape only; host rows must raise).
    Returns None, or the sentence that says what is wrong.  record: dict that takes the worst ulp
    error of transcendental device results, {(row name, dtype name): ulps}."""
    from gym_trading_env_amd.device_array import DeviceArray
    import torch
    host = host_namespace(*kind)
    if (r.name, kind) not in _WANT:
        _WANT[(r.name, kind)] = evaluate(r, host)
    how, want = _WANT[(r.name, kind)]
    ghow, got = evaluate(r, device_namespace(host, device))
    tag = f"row {r.name} over {'/'.join(kind)} on {where}: "
    if how == "raises":
        return None if ghow == "raises" else tag + f"NumPy raises {type(want).__name__}, DeviceArray returned {type(got).__name__}"
    wdt = np.asarray(want[0] if isinstance(want, tuple) else want).dtype
    expect_host = (r.cls == "host" or r.host_on(kind) or wdt.name not in CARRIED
                   or (where == "cpu" and wdt.kind == "f" and (r.cpu_host(kind) if callable(r.cpu_host) else r.cpu_host)))
    if where == "meta":
        if expect_host or r.sync:
            return None if ghow == "raises" else tag + f"must need the host, but ran on meta tensors: {type(got).__name__}"
        if ghow == "raises":
            return tag + f"reads the device or leaves it: {type(got).__name__}: {got}"
        if not isinstance(got, DeviceArray) or got.device.type != "meta":
            return tag + f"returned {type(got).__name__}, not a DeviceArray on meta"
        if got.dtype != wdt or got.shape != np.shape(want):
            return tag + f"{got.dtype}{list(got.shape)}, NumPy gives {wdt}{list(np.shape(want))}"
        return None
    if ghow == "raises":
        return tag + f"raised {type(got).__name__}: {got}; NumPy gives {_describe(want)}"
    if expect_host:
        parts = zip(got, want) if isinstance(want, tuple) and isinstance(got, tuple) else [(got, want)]
        for g, w in parts:
            if isinstance(g, (DeviceArray, torch.Tensor)) or not isinstance(g, (np.ndarray, np.generic)):
                return tag + f"must be a host value, got {type(g).__name__}"
            if not same_bits(g, w):
                return tag + f"host value {_describe(g)} differs from NumPy's {_describe(w)}"
        return None
    if not isinstance(got, DeviceArray):
        return tag + f"returned a host {type(got).__name__}: a {r.cls} row must stay on the device"
    if got.dtype != wdt or got.shape != np.shape(want):
        return tag + f"{got.dtype}{list(got.shape)}, NumPy gives {wdt}{list(np.shape(want))}"
    g, want = got.numpy(), np.asarray(want)
    if r.cls == "exact" or wdt.kind != "f":
        if not same_bits(g, want):
            same = (g == want) | (np.isnan(g) & np.isnan(want)) if wdt.kind == "f" else g == want
            bad = np.flatnonzero(~same.reshape(-1))
            bad = bad if len(bad) else np.flatnonzero(np.signbit(g) != np.signbit(want))  # the sign of a zero
            return tag + (f"{len(bad)} values differ from NumPy's bits, first at {bad[:1]}: "
                          f"{g.reshape(-1)[bad[:4]]} for {want.reshape(-1)[bad[:4]]}")
        return None
    # NaN and infinities sit where NumPy puts them
    fin = np.isfinite(want)
    if not (np.array_equal(np.isnan(g), np.isnan(want)) and np.array_equal(g[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])):
        return tag + "NaN / inf are not where NumPy puts them"
    if r.cls == "transcendental":
        with np.errstate(all="ignore"):
            args = r.args(host)
        key = (r.name, kind, "numpy")
        if key not in _WANT:
            _WANT[key] = worst_ulp(want, r.ref, args)
        mine, numpys = worst_ulp(g, r.ref, args), _WANT[key]
        if record is not None:
            k = (r.name, wdt.name)
            record[k] = max(record.get(k, 0.0), mine)
        bound = numpys + 1 if where == "cpu" else GPU_ULP.get((r.name, wdt.name), 0.0) + 1
        if not mine <= bound:
            return tag + f"{mine:.3f} ulp from the reference, bound {bound:.3f} (NumPy itself: {numpys:.3f})"
        return None
    red, arg, axis, ddof = r.red
    key = (r.name, kind, "bound")
    if key not in _WANT:
        _WANT[key] = reduction_bound(red, arg(host), axis, wdt, ddof)
    ref, bound = (np.asarray(v).reshape(want.shape) for v in _WANT[key])
    for what, val in (("NumPy's own result", want), ("the result", g)):
        for i in np.ndindex(want.shape):
            if not fin[i]:
                continue
            err = abs(REF.num(val[i]) - ref[i])
            if not err <= bound[i]:
                return tag + f"{what} at {i}: {val[i]!r} is {float(err):.3e} from the reference, bound {float(bound[i]):.3e}"
    return None


def check_row(r, device, where, record=None):
    """Every operand kind of row `r`: the list of what is wrong."""
    return [m for m in (check_case(r, k, device, where, record) for k in kinds_of(r)) if m]
