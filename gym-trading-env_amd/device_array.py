"""DeviceArray — a per-env column living in HBM that NumPy code can compute with.

`BatchedHistory` hands user callables (`reward_function(history)`,
`dynamic_feature_functions`, metrics) values like `history["portfolio_valuation", -1]`.  In
the reference those are Python floats; for a batch they are arrays with one entry per env,
resident on the device.  The reference's documented formulas are written with NumPy
(`np.log(h[..., -1] / h[..., -2])`, docs/source/customization.rst:13-20,
luckymodel/envs/env.py:16-18 `np.clip(...)`): DeviceArray implements NumPy's
`__array_ufunc__` / `__array_function__` protocols and the arithmetic operators by
forwarding to torch on the device, so such formulas run UNCHANGED and vectorised, without a
device->host copy.

The rule (DESIGN.md "DeviceArray and NumPy", held by tests/device_array_cases.py): a formula
over DeviceArrays gives one of

  device   a DeviceArray with the dtype and shape the installed NumPy gives for host copies of
           the same operands (Python scalars are weak, NumPy scalars and ndarrays keep their
           dtype: `_plan` asks NumPy's own `ufunc.resolve_dtypes` / `np.result_type`),
           computed without reading a device value; scalars reach the device through
           `torch.full` there, so the formula can be captured into a graph;
  host     a plain ndarray / NumPy scalar computed by NumPy on host copies (`__array__`), which
           the env accepts as well;
  raises   only where NumPy raises on the host copies too.

What runs on the device: the ufuncs of `_UFUNCS` (called, or `.reduce`d for add / multiply /
maximum / minimum), the functions of `_FUNCTIONS`, the operators, `astype`, indexing and the
`.mean/.sum/.max/.min` methods, for bool / int32 / int64 / float32 / float64 data.  What goes
to the host: every other NumPy function, every argument form that is not mapped (`out=`,
`where=`, `dtype=` of a reduction, `initial=`, `ddof` outside std / var, `decimals`,
`prepend` / `append`, `shape=`...), results NumPy gives in a dtype the device path does not
carry (float16 from bool inputs, int8 from bool // bool), and integer powers whose exponent
could be negative (NumPy raises by value there).
"""
from __future__ import annotations

import operator

import numpy as np

_NV = np._NoValue
# the dtypes the device path carries (what the env hands out and what NumPy promotes them to)
_CARRIED = ("bool", "int32", "int64", "float32", "float64")


_TORCH = None


def _torch():
    global _TORCH
    if _TORCH is None:  # (imported at first use: the package imports without torch)
        import torch
        _TORCH = torch
    return _TORCH


class _Host(Exception):
    """This call is not mapped to the device: compute it with NumPy on host copies."""


_NP_OF, _TORCH_OF = {}, {}  # torch dtype <-> NumPy dtype of the carried types (filled at first use)


def _np_dtype(t):
    if not _NP_OF:
        torch = _torch()
        for name in _CARRIED:
            _NP_OF[getattr(torch, name)], _TORCH_OF[np.dtype(name)] = np.dtype(name), getattr(torch, name)
    dt = _NP_OF.get(t.dtype)
    return dt if dt is not None else np.dtype(str(t.dtype)[6:])  # "torch.float16" -> float16


def _tdt(dt):
    """torch dtype of a NumPy dtype the device path carries."""
    tdt = _TORCH_OF.get(dt)
    if tdt is None:
        if not _TORCH_OF and np.dtype(dt).name in _CARRIED:
            _np_dtype(_torch().empty(0))
        tdt = _TORCH_OF.get(np.dtype(dt))
        if tdt is None:
            raise _Host
    return tdt


_WEAK = {float: float, int: int, bool: np.dtype(bool)}


def _spec(x):
    """What NumPy's promotion sees of an operand: a dtype (tensors, ndarrays, NumPy scalars and
    Python bools are strong) or the Python type of a weak scalar."""
    if type(x) is DeviceArray:
        return _NP_OF.get(x.t.dtype) or _np_dtype(x.t)
    weak = _WEAK.get(type(x))
    if weak is not None:
        return weak
    if isinstance(x, (np.ndarray, np.generic)):
        return x.dtype
    if isinstance(x, _torch().Tensor):
        return _np_dtype(x)
    if isinstance(x, (list, tuple)):
        return np.asarray(x).dtype
    raise _Host


def _promote(inputs):
    """NumPy's plain promotion of operands that meet outside a ufunc (where, stack, concatenate):
    weak Python scalars count by value."""
    try:
        return np.result_type(*[x if type(x) in (int, float) else _spec(x) for x in inputs])
    except TypeError:
        raise _Host from None


def _operand(x, dt, like, tdt=None):
    """Operand `x` as a tensor of NumPy dtype `dt` on `like`'s device.  Scalars are filled in on
    the device (no host->device copy: the value can be part of a captured graph); only host
    arrays the caller passed are copied."""
    tdt = tdt or _tdt(dt)
    if type(x) is DeviceArray:
        x = x.t
        return x if x.dtype is tdt else x.to(tdt)
    torch = _torch()
    if isinstance(x, torch.Tensor):
        return x if x.dtype == tdt else x.to(tdt)
    if isinstance(x, (np.ndarray, list, tuple)):
        return torch.as_tensor(np.asarray(x), device=like.device).to(tdt)
    if isinstance(x, np.generic):
        x = x.item()
    if dt.kind in "iu" and not isinstance(x, bool):
        if isinstance(x, float) or not np.iinfo(dt).min <= x <= np.iinfo(dt).max:
            raise _Host  # NumPy raises OverflowError for a Python int that does not fit
    return torch.full((), x, dtype=tdt, device=like.device)


def _first_tensor(args):
    for a in args:
        if type(a) is DeviceArray:
            return a.t
        if isinstance(a, (list, tuple)):
            t = _first_tensor(a)
            if t is not None:
                return t
    return None


def _wrap(x):
    torch = _torch()
    if isinstance(x, torch.Tensor):
        return DeviceArray(x)
    if isinstance(x, tuple):
        return tuple(_wrap(v) for v in x)
    return x


def _host(v):
    """Host copies of every DeviceArray in (possibly nested) `v`."""
    if isinstance(v, DeviceArray):
        return v.numpy()
    if isinstance(v, (list, tuple)):
        return type(v)(_host(w) for w in v)
    if isinstance(v, dict):
        return {k: _host(w) for k, w in v.items()}
    return v


# numpy ufunc name -> torch function name (same argument order)
_UFUNCS = {
    "add": "add", "subtract": "sub", "multiply": "mul", "true_divide": "true_divide",
    "divide": "true_divide", "floor_divide": "floor_divide", "power": "pow", "negative": "neg",
    "positive": "positive", "absolute": "abs", "fabs": "abs", "sign": "sign", "sqrt": "sqrt",
    "square": "square", "exp": "exp", "expm1": "expm1", "exp2": "exp2", "log": "log",
    "log2": "log2", "log10": "log10", "log1p": "log1p", "sin": "sin", "cos": "cos", "tan": "tan",
    "tanh": "tanh", "sinh": "sinh", "cosh": "cosh", "arctan": "atan", "maximum": "maximum",
    "minimum": "minimum", "fmax": "fmax", "fmin": "fmin", "greater": "gt", "greater_equal": "ge",
    "less": "lt", "less_equal": "le", "equal": "eq", "not_equal": "ne",
    "logical_and": "logical_and", "logical_or": "logical_or", "logical_not": "logical_not",
    "isnan": "isnan", "isfinite": "isfinite", "isinf": "isinf", "floor": "floor", "ceil": "ceil",
    "rint": "round", "trunc": "trunc", "remainder": "remainder", "reciprocal": "reciprocal",
    "clip": "clamp", "bitwise_and": "bitwise_and", "bitwise_or": "bitwise_or",
    "invert": "bitwise_not",
}
_REDUCE = {"add": "sum", "multiply": "prod", "maximum": "max", "minimum": "min"}
# Over CPU tensors (tests; the env hands out HBM tensors) these are left to NumPy for floats: torch's
# CPU kernels are not the IEEE operations there (its sqrt is a vector library's, 1 ulp off for 0.5,
# and its fmod gives NaN for a quotient beyond the exponent range), the device's are.
_CPU_INEXACT = ("sqrt", "remainder", "floor_divide")
_NO_BOOL = ("absolute", "floor", "ceil", "trunc", "clip")  # NumPy has bool loops for these, torch has not


_PLANS = {}  # (ufunc, operand specs) -> how to run it: a formula asks the same question every step


def _plan(key):
    """(NumPy dtypes, torch dtypes, torch function, name when the call needs a look at its operands)
    of ufunc key[0] over operands of specs key[1:], or _Host."""
    torch = _torch()
    ufunc, name = key[0], key[0].__name__
    try:
        if name not in _UFUNCS:
            raise _Host
        try:  # the dtypes NumPy computes in: (input dtypes..., output dtype)
            dts = ufunc.resolve_dtypes(key[1:] + (None,) * ufunc.nout)
        except TypeError:
            raise _Host from None  # NumPy has no loop for these types: it raises on the host too
        if name in _NO_BOOL and dts[0].kind == "b":
            raise _Host
        tdts = tuple(_tdt(dt) for dt in dts)
        if name == "sign" and dts[0].kind == "f":  # NumPy: sign(NaN) is NaN
            fn = lambda x: torch.where(x != x, x, torch.sign(x))  # noqa: E731
        elif name in ("remainder", "floor_divide") and dts[0].kind == "f":
            fn = (lambda a, b: _float_divmod(a, b)[1]) if name == "remainder" else (lambda a, b: _float_divmod(a, b)[0])
        else:
            fn = getattr(torch, _UFUNCS[name])
        look = name if (name == "power" and dts[-1].kind in "iu") or (name in _CPU_INEXACT and dts[0].kind == "f") else None
        plan = (dts, tdts, fn, look)
    except _Host:
        plan = _Host
    _PLANS[key] = plan
    return plan


def _ufunc_call(ufunc, inputs):
    """`ufunc(*inputs)` on the device, in the dtypes NumPy resolves for these operands."""
    key = (ufunc, *[_spec(x) for x in inputs])
    plan = _PLANS.get(key) or _plan(key)
    if plan is _Host:
        raise _Host
    dts, tdts, fn, look = plan
    like = _first_tensor(inputs)
    if look == "power":
        # NumPy raises for a negative integer exponent, by value: only a host scalar can be checked
        e = inputs[1]
        if isinstance(e, (DeviceArray, np.ndarray, list, tuple)) or e < 0:
            raise _Host
    elif look is not None and like.device.type == "cpu":
        raise _Host  # _CPU_INEXACT
    r = fn(*[_operand(x, dt, like, tdt) for x, dt, tdt in zip(inputs, dts, tdts)])
    if r.dtype is not tdts[-1]:
        raise _Host  # torch computes this one in another type than NumPy
    return r


def _float_divmod(a, b):
    """NumPy's floor division and remainder of floats (npy_divmod: built on the exact fmod, where
    torch's are a - b * floor(a / b)): the same values, signs of zero and NaNs."""
    torch = _torch()
    mod = torch.fmod(a, b)
    div = (a - mod) / b
    wrap = (mod != 0) & ((b < 0) != (mod < 0))  # the remainder takes the divisor's sign
    div = torch.where(wrap, div - 1, div)
    mod = torch.where(wrap, mod + b, torch.where(mod != 0, mod, torch.copysign(torch.zeros_like(mod), b)))
    floor = torch.floor(div)
    floor = torch.where(div - floor > 0.5, floor + 1, floor)
    floor = torch.where(div != 0, floor, torch.copysign(torch.zeros_like(div), a / b))
    zero = b == 0  # x // 0 is x / 0, x % 0 is fmod's NaN
    return torch.where(zero, a / b, floor), torch.where(zero, torch.fmod(a, b), mod)


def _axis_kw(axis, keepdims):
    """numpy's axis= / keepdims= -> torch's dim= / keepdim= (None = all)."""
    out = {}
    if axis is not None:
        out["dim"] = axis
    if keepdims is not _NV and keepdims:
        out["keepdim"] = True
    return out


def _array(a):
    """The array argument of a mapped function as a tensor (DeviceArrays only: a function called
    on a host array with a DeviceArray among its other arguments is left to NumPy)."""
    if not isinstance(a, DeviceArray):
        raise _Host
    if a.dtype.name not in _CARRIED:
        raise _Host
    return a.t


def _reduction(name):
    def f(a, axis=None, dtype=None, out=None, keepdims=_NV, **rest):
        torch = _torch()
        x = _array(a)
        ddof = rest.pop("ddof", 0) if name in ("std", "var") else 0
        if dtype is not None or out is not None or rest or not isinstance(ddof, int):
            raise _Host  # dtype=, out=, initial=, where=, ddof on something else, correction=...
        kind = _np_dtype(x).kind
        if axis is None and keepdims is not _NV and keepdims:
            axis = tuple(range(x.dim()))
        if name in ("sum", "prod"):
            if kind in "bi":
                x = x.to(torch.int64)  # NumPy adds and multiplies bools and small ints as C longs
            if name == "prod" and (axis is None or isinstance(axis, tuple)):  # (torch.prod takes one dim)
                if isinstance(axis, tuple) and sorted(a % x.dim() for a in axis) != list(range(x.dim())):
                    raise _Host
                r = torch.prod(x.reshape(-1), dim=0)
                return r.reshape((1,) * x.dim()) if axis is not None else r
            return getattr(torch, name)(x, **_axis_kw(axis, keepdims))
        if name in ("mean", "std", "var"):
            if kind in "bi":
                x = x.to(torch.float64)  # floats keep their own dtype, like NumPy's
            if name == "mean":
                return torch.mean(x, **_axis_kw(axis, keepdims))
            return getattr(torch, name)(x, correction=ddof, **_axis_kw(axis, keepdims))
        if name in ("max", "min"):
            return getattr(torch, "a" + name)(x, **_axis_kw(axis, keepdims))
        return getattr(torch, name)(x, **_axis_kw(axis, keepdims))  # any, all
    return f


def _f_where(condition, x=_NV, y=_NV):
    torch = _torch()
    if x is _NV or y is _NV:
        raise _Host  # np.where(c): index arrays, their size is data
    like = _first_tensor((condition, x, y))
    c = _operand(condition, np.dtype(bool), like)
    dt = _promote((x, y))  # the two branches promote like any binary operation
    return torch.where(c, _operand(x, dt, like), _operand(y, dt, like))


def _f_clip(a, a_min=_NV, a_max=_NV, out=None, *, min=_NV, max=_NV, **rest):
    if out is not None or rest:
        raise _Host
    lo = None if (a_min if min is _NV else min) is _NV else (a_min if min is _NV else min)
    hi = None if (a_max if max is _NV else max) is _NV else (a_max if max is _NV else max)
    _array(a)
    if lo is None and hi is None:
        raise _Host
    if lo is None:  # NumPy's own definition: one bound is a minimum / maximum
        return _ufunc_call(np.minimum, (a, hi))
    if hi is None:
        return _ufunc_call(np.maximum, (a, lo))
    return _ufunc_call(np._core.umath.clip, (a, lo, hi))


def _f_diff(a, n=1, axis=-1, prepend=_NV, append=_NV):
    if prepend is not _NV or append is not _NV or not isinstance(n, int) or n < 1:
        raise _Host
    return _torch().diff(_array(a), n=n, dim=axis)


def _cumulative(name):
    def f(a, axis=None, dtype=None, out=None):
        torch = _torch()
        x = _array(a)
        if dtype is not None or out is not None:
            raise _Host
        if _np_dtype(x).kind in "bi":
            x = x.to(torch.int64)
        if axis is None:
            x, axis = x.reshape(-1), 0
        return getattr(torch, name)(x, dim=axis)
    return f


def _f_round(a, decimals=0, out=None):
    x = _array(a)
    if decimals != 0 or out is not None:
        raise _Host
    if x.dtype == _torch().bool:
        raise _Host  # (NumPy rounds bools in float16)
    return _torch().round(x) if x.is_floating_point() else x.clone()


def _f_nan_to_num(x, copy=True, nan=0.0, posinf=None, neginf=None):
    t = _array(x)
    real = lambda v: v is None or (isinstance(v, (int, float, np.integer, np.floating))  # noqa: E731
                                   and not isinstance(v, bool))
    if not copy or not (real(nan) and real(posinf) and real(neginf)):
        raise _Host
    if not t.is_floating_point():
        return t.clone()
    f = lambda v: None if v is None else float(v)  # noqa: E731
    return _torch().nan_to_num(t, nan=float(nan), posinf=f(posinf), neginf=f(neginf))


def _join(name):
    def f(arrays, axis=0, out=None, **rest):
        torch = _torch()
        if out is not None or rest or not all(isinstance(v, (DeviceArray, np.ndarray)) for v in arrays):
            raise _Host
        like = _first_tensor(arrays)
        dt = _promote(arrays)
        seq = [_operand(v, dt, like) for v in arrays]
        if name == "concatenate" and axis is None:
            seq, axis = [v.reshape(-1) for v in seq], 0
        return (torch.stack if name == "stack" else torch.cat)(seq, dim=axis)
    return f


def _like(name):
    def f(a, *fill, dtype=None, order="K", subok=True, shape=None, device=None):
        torch = _torch()
        x = _array(a)
        if shape is not None or device is not None or len(fill) != (name == "full_like"):
            raise _Host
        tdt = x.dtype if dtype is None else _tdt(np.dtype(dtype))
        if name != "full_like":
            return getattr(torch, name)(x, dtype=tdt)
        v = fill[0].item() if isinstance(fill[0], np.generic) else fill[0]
        if not isinstance(v, (bool, int, float)) or (isinstance(v, float) and not tdt.is_floating_point):
            raise _Host  # NumPy casts the fill value to the array's type by C rules
        return torch.full_like(x, v, dtype=tdt)
    return f


# NumPy function name (`func.__name__`) -> the same call on tensors.  A handler raises _Host for
# an argument form it does not map; a TypeError (an argument it does not know) means the same.
_FUNCTIONS = {
    "where": _f_where, "clip": _f_clip, "diff": _f_diff, "round": _f_round, "around": _f_round,
    "nan_to_num": _f_nan_to_num, "cumsum": _cumulative("cumsum"), "cumprod": _cumulative("cumprod"),
    "stack": _join("stack"), "concatenate": _join("concatenate"),
    "zeros_like": _like("zeros_like"), "ones_like": _like("ones_like"), "full_like": _like("full_like"),
    "amax": _reduction("max"), "amin": _reduction("min"),
}
_FUNCTIONS.update({n: _reduction(n) for n in ("sum", "prod", "mean", "std", "var", "max", "min", "any", "all")})


class DeviceArray:
    """A torch tensor on the device with NumPy's calling conventions (see module docstring).
    `.t` / `.tensor` is the tensor; `np.asarray(x)` / `.numpy()` copy it to the host."""

    __array_priority__ = 1000
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t

    # -- basics ----------------------------------------------------------------------------
    tensor = property(lambda self: self.t)
    shape = property(lambda self: tuple(self.t.shape))
    ndim = property(lambda self: self.t.dim())
    size = property(lambda self: self.t.numel())
    dtype = property(lambda self: _np_dtype(self.t))
    device = property(lambda self: self.t.device)

    def __len__(self):
        return self.t.shape[0]

    def __repr__(self):
        return f"DeviceArray({self.t!r})"

    def numpy(self):
        a = self.t.detach().cpu().numpy()
        return a.copy() if self.t.device.type == "cpu" else a  # (never a view of the tensor)

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype)

    def astype(self, dtype):
        try:
            return DeviceArray(self.t.to(_tdt(dtype)))
        except _Host:
            return self.numpy().astype(dtype)

    def __getitem__(self, i):
        def index(i):
            if isinstance(i, DeviceArray):
                return i.t
            if isinstance(i, (np.ndarray, list)):
                return _torch().as_tensor(np.asarray(i), device=self.t.device)
            return i
        return DeviceArray(self.t[tuple(index(j) for j in i) if isinstance(i, tuple) else index(i)])

    def __float__(self):
        return float(self.t)

    def __bool__(self):
        return bool(self.t)

    def item(self):
        return self.t.item()

    # the methods are NumPy's functions of the same name (one set of rules: _FUNCTIONS)
    def mean(self, *args, **kw):
        return np.mean(self, *args, **kw)

    def sum(self, *args, **kw):
        return np.sum(self, *args, **kw)

    def max(self, *args, **kw):
        return np.max(self, *args, **kw)

    def min(self, *args, **kw):
        return np.min(self, *args, **kw)

    # -- NumPy protocols ---------------------------------------------------------------------
    def __array_ufunc__(self, ufunc, method, *inputs, out=None, **kw):
        try:
            if method == "__call__" and out is None and not kw:  # (the usual call, first)
                return DeviceArray(_ufunc_call(ufunc, inputs))
            if out is not None or kw.get("where", True) is not True:
                raise _Host
            rest = {k: v for k, v in kw.items() if k != "where"}
            if method == "__call__" and not rest:
                return _wrap(_ufunc_call(ufunc, inputs))
            if method == "reduce" and ufunc.__name__ in _REDUCE and set(rest) <= {"axis", "keepdims"}:
                rest.setdefault("axis", 0)  # ufunc.reduce's default axis
                return _wrap(_FUNCTIONS[_REDUCE[ufunc.__name__]](inputs[0], **rest))
        except (_Host, TypeError, RuntimeError):
            pass
        # not mapped: compute on the host; the result is a plain ndarray
        if out is not None:
            kw["out"] = out
        return getattr(ufunc, method)(*_host(inputs), **_host(kw))

    def __array_function__(self, func, types, args, kwargs):
        name = func.__name__
        if name in ("shape", "ndim", "size") and len(args) == 1 and not kwargs:
            return getattr(self, name)
        handler = _FUNCTIONS.get(name)
        if handler is not None:
            try:
                return _wrap(handler(*args, **kwargs))
            except (_Host, TypeError, RuntimeError):
                pass  # an argument form that is not mapped: host fallback below
        return func(*_host(args), **_host(kwargs))


# NumPy's `**` takes these scalar exponents (Python's or NumPy's) of a floating-point array, and the
# square of any array, as the exact operation: in the array's own dtype
_SCALARS = (int, float, np.integer, np.floating, np.bool_)
_FAST_POWERS = {2: np.square, 0.5: np.sqrt, 1: np.positive, -1: np.reciprocal}


def _binary(ufunc, pyop, reflected=False):
    def op(self, other):
        a, b = (other, self) if reflected else (self, other)
        try:
            if ufunc is np.power and not reflected and isinstance(other, _SCALARS) and other in _FAST_POWERS \
                    and (self.t.is_floating_point() or other == 2):
                return DeviceArray(_ufunc_call(_FAST_POWERS[other], (self,)))
            return DeviceArray(_ufunc_call(ufunc, (a, b)))
        except (_Host, TypeError, RuntimeError):
            return pyop(_host(a), _host(b))
    return op


def _unary(ufunc, pyop):
    def op(self):
        try:
            return DeviceArray(_ufunc_call(ufunc, (self,)))
        except (_Host, TypeError, RuntimeError):
            return pyop(self.numpy())
    return op


# operator -> the ufunc NumPy's ndarray uses for it
_OPERATORS = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "truediv": np.true_divide,
              "floordiv": np.floor_divide, "pow": np.power, "mod": np.remainder,
              "and": np.bitwise_and, "or": np.bitwise_or}
_COMPARISONS = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal,
                "eq": np.equal, "ne": np.not_equal}
_UNARY = {"neg": np.negative, "pos": np.positive, "abs": np.absolute, "invert": np.invert}
for _py, _u in _OPERATORS.items():
    _op = getattr(operator, _py + "_" if _py in ("and", "or") else _py)
    setattr(DeviceArray, f"__{_py}__", _binary(_u, _op))
    setattr(DeviceArray, f"__r{_py}__", _binary(_u, _op, reflected=True))
for _py, _u in _COMPARISONS.items():
    setattr(DeviceArray, f"__{_py}__", _binary(_u, getattr(operator, _py)))
for _py, _u in _UNARY.items():
    setattr(DeviceArray, f"__{_py}__", _unary(_u, getattr(operator, _py)))
DeviceArray.__hash__ = None


def to_tensor(x, device, dtype=None):
    """Whatever a user callable returned (DeviceArray, tensor, ndarray, list, scalar) ->
    torch tensor on `device`."""
    torch = _torch()
    if isinstance(x, DeviceArray):
        x = x.t
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x), device=device)
    x = x.to(device)
    return x if dtype is None else x.to(dtype)
