"""Indicator banks, no GPU needed: the table of `gte_build_indicators` (include/gte.h) as plain loops
against an independently written vectorised statement on the fixture the GPU tests use, pandas where it
offers the same indicator, prefixes, hand-written cases for the NaN rows and the tie rule, the 16-byte
layout of `gte_indicator_spec` against the C header, and the host helpers of signals.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import indicator_model as im
from gym_trading_env_amd import _abi, signals
from replay import same_value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def banks():
    data, specs = im.fixture()
    return data, specs, im.build_bank(specs, data), im.build_bank(specs, data, statement="loop")


def test_the_two_statements_agree_on_the_fixture(banks):
    data, specs, vec, loop = banks
    assert vec.shape == (10 * 5 * 11 + 7, im.T_FIX) and vec.dtype == np.float32
    ok = same_value(vec, loop)
    assert ok.all(), f"spec {specs[np.argwhere(~ok)[0][0]]} row {np.argwhere(~ok)[0][1]}"
    # the model against itself: no unequal value (the count the GPU test takes for STD and ZSCORE)
    assert int((~same_value(loop, loop)).sum()) == 0
    # the fixture exercises what it is there for
    valid = np.array([im.source_of(s, data) is not None for s in specs])
    assert (~valid).sum() == 7 and np.isnan(vec[~valid]).all()
    by_kind = {k: vec[valid & (specs["kind"] == i)] for i, k in enumerate(im.KINDS)}
    for k, rows in by_kind.items():
        assert np.isfinite(rows).mean() > 0.5, k
    special = vec[valid & (specs["source"] == signals.SRC_FEATURE) & (specs["column"] == im.SPECIAL)]
    assert np.isinf(special).any() and np.isnan(special[:, 2400:]).any() and (special == 0).any()
    tiny = np.finfo(np.float32).tiny
    assert ((special != 0) & (np.abs(special) < tiny)).any(), "no subnormal output"
    assert np.signbit(special[special == 0]).any() and not np.signbit(special[special == 0]).all()


def test_invalid_specs_and_long_windows_give_rows_of_nan(banks):
    data, specs, vec, _ = banks
    assert np.isnan(vec[-7:]).all()
    long = (specs["n"] == 4096) & (specs["kind"] != signals.IND_VALUE) & (specs["kind"] != signals.IND_EMA)
    assert long.sum() == 8 * 5 and np.isnan(vec[long]).all()
    ema = (specs["n"] == 4096) & (specs["kind"] == signals.IND_EMA) & (specs["source"] == signals.SRC_CLOSE)
    assert np.isfinite(vec[ema]).all()   # (an EMA has no NaN rows: its warm-up is the rule's)
    no_hl = dict(data, high=None, low=None)
    got = im.build_bank(specs, no_hl, 100)
    hl = (specs["source"] == signals.SRC_HIGH) | (specs["source"] == signals.SRC_LOW)
    assert np.isnan(got[hl]).all() and same_value(got[~hl], vec[~hl, :100]).all()
    no_in = dict(data, inputs=None)
    assert np.isnan(im.build_bank(specs, no_in, 100)[specs["source"] == signals.SRC_INPUT]).all()


@pytest.mark.parametrize("T", [2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_a_prefix_of_the_source_gives_a_prefix_of_every_row(T, banks):
    data, specs, vec, _ = banks
    pick = np.r_[np.arange(0, len(specs), 7), np.arange(len(specs) - 7, len(specs))]
    assert same_value(im.build_bank(specs[pick], data, T), vec[pick, :T]).all()


def test_rows_that_are_nan(banks):
    data, specs, vec, _ = banks
    for s in np.flatnonzero(specs["source"][:-7] == signals.SRC_CLOSE):
        kind, n = im.KINDS[specs["kind"][s]], int(specs["n"][s])
        first = 0 if kind in ("value", "ema") else n if kind in ("diff", "roc", "rsi") else n - 1
        if kind == "zscore" and n == 1:
            first = im.T_FIX   # (x - x) / 0
        assert np.isnan(vec[s, :first]).all() and np.isfinite(vec[s, first:]).all(), (kind, n)


def test_hand_written_cases():
    x = [1.0, 2.0, 4.0, 8.0, 16.0]
    r = lambda kind, n, x=x, **kw: im.row(kind, np.array(x), n, **kw).tolist()
    for st in ("loop", "vector"):
        assert r("value", 3, statement=st) == x
        assert r("sma", 2, statement=st)[1:] == [1.5, 3.0, 6.0, 12.0] and np.isnan(r("sma", 2, statement=st)[0])
        assert r("std", 2, statement=st)[1:] == [0.5, 1.0, 2.0, 4.0]
        assert r("zscore", 2, statement=st)[1:] == [1.0, 1.0, 1.0, 1.0]
        assert r("max", 3, statement=st)[2:] == [4.0, 8.0, 16.0] and r("min", 3, statement=st)[2:] == [1.0, 2.0, 4.0]
        assert r("diff", 2, statement=st)[2:] == [3.0, 6.0, 12.0] and np.isnan(r("diff", 2, statement=st)[:2]).all()
        assert r("roc", 1, statement=st)[1:] == [1.0, 1.0, 1.0, 1.0]
        assert r("ema", 1, statement=st) == x                       # a = 1: the series itself
        assert r("ema", 3, statement=st) == [1.0, 1.5, 2.75, 5.375, 10.6875]
        assert r("rsi", 2, statement=st)[2:] == [100.0, 100.0, 100.0]   # no losses: au / 0 = inf
        down = r("rsi", 2, x=[4.0, 3.0, 4.0, 2.0], statement=st)
        assert np.isnan(down[:2]).all() and down[2:] == [50.0, float(np.float32(100.0 - 100.0 / (1.0 + 0.25 / 1.25)))]
        # a flat window: 0 / 0; a window longer than the series: nothing but NaN
        assert np.isnan(r("zscore", 3, x=[2.0] * 5, statement=st)).all()
        assert r("std", 3, x=[2.0] * 5, statement=st)[2:] == [0.0] * 3
        assert np.isnan(r("sma", 6, statement=st)).all() and np.isnan(r("rsi", 5, statement=st)).all()
        # one NaN in the window poisons MAX and MIN (a comparison alone would skip it)
        assert np.isnan(r("max", 2, x=[1.0, np.nan, 3.0, 2.0], statement=st)[:3]).all()
        assert r("max", 2, x=[1.0, np.nan, 3.0, 2.0], statement=st)[3] == 3.0
        # a NaN change counts as neither gain nor loss
        assert r("rsi", 2, x=[1.0, np.nan, 1.0, 3.0, 2.0], statement=st)[3:] == [100.0, 50.0]


def test_the_oldest_of_equal_values_stays():
    """[+0.0, -0.0]: MAX and MIN both keep the first one, whatever its sign"""
    for st in ("loop", "vector"):
        for x, neg in (([0.0, -0.0], False), ([-0.0, 0.0], True)):
            for kind in ("max", "min"):
                y = im.row(kind, np.array(x), 2, statement=st)
                assert y[1] == 0 and bool(np.signbit(y[1])) == neg, (st, x, kind)


@pytest.mark.parametrize("kind", ["sma", "std", "ema"])
def test_pandas_agrees_within_the_bound_of_another_order_of_summation(kind, banks):
    """pandas `rolling(n)` over close / high / low, every n of the fixture that fits: the mean and the
    standard deviation (ddof = 0) of each window equal the model's within n * 2^-52 * max|x| in f64, and
    `ewm(adjust=False)` the EMA within (n + 1) * 2^-52 * max|x| (pandas multiplies where the header
    subtracts; the rounding of one step, 3 * 2^-53 * max|x|, summed over a geometric series of ratio
    1 - 2 / (n + 1)).

    The bound is that of the same n terms added in another order, so the windows are reduced one by one:
    `rolling(n).apply(np.mean / np.std, raw=True)`, a pairwise sum of each window.  The shortcuts
    `rolling(n).mean()` and `.std(ddof=0)` are not such a sum: they update a running sum and a running
    sum of squares ONLINE (add the new row, remove the oldest), so their error grows with t instead of n.
    Against them the model measured, on this fixture with pandas 2.3.3: SMA high n = 2: 8.5e-14 against a
    bound of 6.9e-14; STD n = 2: 3.4e-9 .. 3.1e-8 against 6.9e-14, n = 15 .. 17: 0.8 .. 2.8e-11 against
    5.1 .. 5.9e-13, n = 63 .. 65: 0.3 .. 1.5e-11 against 2.2e-12 — the drift of an online variance, which
    says nothing about a window's sum.  Every figure is printed before it is asserted."""
    pd = pytest.importorskip("pandas")
    data = banks[0]
    worst = []
    for name in ("close", "high", "low"):
        x = np.asarray(data[name])
        s, top = pd.Series(x), np.abs(x).max()
        for n in (w for w in im.N_FIX if w <= im.T_FIX):
            other = {"sma": lambda: s.rolling(n).apply(np.mean, raw=True),
                     "std": lambda: s.rolling(n).apply(np.std, raw=True),   # (np.std: ddof = 0)
                     "ema": lambda: s.ewm(alpha=2.0 / (n + 1.0), adjust=False).mean()}[kind]().to_numpy()
            ours = im.VECTOR[kind](x, n)
            assert (np.isnan(ours) == np.isnan(other)).all(), (name, kind, n)
            bound = (n + 1 if kind == "ema" else n) * 2.0 ** -52 * top
            err = np.nanmax(np.abs(ours - other))
            print(f"{kind} {name} n={n}: {err:.3g} (bound {bound:.3g})")
            if err > bound:
                worst.append((name, n, float(err), float(bound)))
    assert not worst, worst


def test_sums_in_another_order_agree_within_the_bound(banks):
    """Without pandas: the same n terms added pairwise (np.sum over a window view) instead of oldest
    first: the mean within n * 2^-52 * max|x|, and the variance q / n within n * 2^-52 * (2 max|x|)^2 — its terms are
    squares of deviations of at most 2 max|x| (the deviation of the two means enters squared)."""
    from numpy.lib.stride_tricks import sliding_window_view
    data = banks[0]
    for name in ("close", "high", "low"):
        x = np.asarray(data[name])
        top = np.abs(x).max()
        for n in (w for w in im.N_FIX if w <= im.T_FIX):
            win = sliding_window_view(x, n)
            mean = win.sum(axis=1) / n
            var = ((win - mean[:, None]) ** 2).sum(axis=1) / n
            assert np.abs(im.vec_sma(x, n)[n - 1:] - mean).max() <= n * 2.0 ** -52 * top, (name, n)
            assert np.abs(im.vec_std(x, n)[n - 1:] ** 2 - var).max() <= n * 2.0 ** -52 * (2 * top) ** 2, (name, n)


def test_indicator_dtype_is_the_c_struct(tmp_path):
    assert signals.INDICATOR_DTYPE.itemsize == 16 and signals.INDICATOR_DTYPE == np.dtype(_abi.INDICATOR_DTYPE)
    fields = signals.INDICATOR_DTYPE.names
    assert fields == tuple(n for n, _ in _abi.INDICATOR_FIELDS) == ("kind", "source", "column", "n")
    probe = "#include <stddef.h>\n#include <stdio.h>\n#include \"gte.h\"\n" + \
        "_Static_assert(sizeof(gte_indicator_spec) == 16, \"16 bytes\");\nint main(void) {\n" + \
        "".join(f'  printf("{f} %zu %zu\\n", offsetof(gte_indicator_spec, {f}), sizeof(((gte_indicator_spec*)0)->{f}));\n'
                for f in fields) + \
        '  printf("%d %d %d %d\\n", GTE_IND_VALUE, GTE_IND_RSI, GTE_SRC_INPUT, GTE_IND_MAX_WINDOW);\n  return 0;\n}\n'
    src = tmp_path / "probe.c"
    src.write_text(probe)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = [ln for ln in subprocess.check_output([exe], text=True).split("\n") if ln]
    c_fields = [(n, int(o), int(s)) for n, o, s in (ln.split() for ln in lines[:-1])]
    dt = signals.INDICATOR_DTYPE
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in fields] == c_fields
    assert sum(s for _, _, s in c_fields) == 16
    assert lines[-1].split() == ["0", "9", "4", "4096"]
    # the names of the header are those of signals.py, in the header's order
    hdr = open(os.path.join(ROOT, "include", "gte.h")).read()
    kinds = re.search(r"enum gte_indicator_kind \{(.*?)\}", hdr, re.S).group(1)
    assert [k.lower() for k in re.findall(r"GTE_IND_(\w+) =", kinds)] == list(signals.IND_KINDS)
    assert [getattr(signals, "IND_" + k.upper()) for k in signals.IND_KINDS] == list(range(10))
    srcs = re.search(r"enum gte_indicator_source \{(.*?)\}", hdr, re.S).group(1)
    assert [k.lower() for k in re.findall(r"GTE_SRC_(\w+) =", srcs)] == list(signals.IND_SOURCES)
    assert [getattr(signals, "SRC_" + k.upper()) for k in signals.IND_SOURCES] == list(range(5))
    # the kernel's own static_assert
    hip = open(os.path.join(ROOT, "gym-trading-env_amd", "csrc", "gte_indicators.hip")).read()
    assert "static_assert(sizeof(gte_indicator_spec) == 16" in hip


def test_header_and_ctypes_table_declare_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "gte.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint gte_build_indicators\s*\(([^)]*)\)\s*;", code)
    assert m, "include/gte.h does not declare gte_build_indicators"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["gte_env* env", "int32_t ds", "const gte_indicator_spec* specs_device", "int32_t n_specs",
                    "const float* input_device", "int32_t n_inputs", "int64_t input_stride",
                    "float* bank_device", "int64_t ind_stride"]
    res, argtypes = _abi.SYMBOLS["gte_build_indicators"]
    assert len(argtypes) == len(args)
    import ctypes as C
    assert [t for t in argtypes] == [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64,
                                     C.c_void_p, C.c_int64]
    lib = _abi.load_library()
    assert lib.gte_build_indicators(None, 0, None, 1, None, 0, 0, None, 16) == _abi.GTE_ERR_INVALID


def test_indicators_broadcasts_and_checks_its_arguments():
    s = signals.indicators("sma", [5, 10, 20])
    assert s.dtype == signals.INDICATOR_DTYPE and s.shape == (3,)
    assert s["kind"].tolist() == [1, 1, 1] and s["n"].tolist() == [5, 10, 20] and s["source"].tolist() == [0] * 3
    s = signals.indicators(["EMA", "rsi"], 14, source=["feature", "input"], column=[2, 0])
    assert s["kind"].tolist() == [signals.IND_EMA, signals.IND_RSI] and s["source"].tolist() == [3, 4]
    assert s["column"].tolist() == [2, 0] and s["n"].tolist() == [14, 14]
    s = signals.indicators(signals.IND_ZSCORE, np.arange(1, 4)[:, None], source=[signals.SRC_HIGH, signals.SRC_LOW])
    assert s.shape == (6,) and s["n"].tolist() == [1, 1, 2, 2, 3, 3] and s["source"].tolist() == [1, 2] * 3
    assert signals.indicators("value").tolist() == [(0, 0, 0, 1)]
    assert signals.indicators("value", n=0)["n"].tolist() == [0]   # VALUE ignores n
    assert signals.indicators("sma", 4096)["n"].tolist() == [4096]
    for bad in (dict(kind="wma"), dict(kind=10), dict(kind=-1), dict(kind="sma", source="open"),
                dict(kind="sma", source=5), dict(kind="sma", n=0), dict(kind="sma", n=4097),
                dict(kind=["value", "ema"], n=0), dict(kind="sma", n=5, column=-1),
                dict(kind="sma", n=5, column=2 ** 31)):
        with pytest.raises(ValueError):
            signals.indicators(**bad)
    for bad in (dict(kind=1.0), dict(kind="sma", n=5.0), dict(kind="sma", n=5, column=0.5),
                dict(kind="sma", source=0.0)):
        with pytest.raises(TypeError):
            signals.indicators(**bad)
