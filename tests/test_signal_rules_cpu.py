"""Signal tables from indicator rules, no GPU needed: the rule of `gte_build_signals` (include/gte.h) as
a plain loop against an independently written vectorised statement on the fixture the GPU tests use,
hand-written cases for each line of the rule, the 32-byte layout of `gte_signal_rule` against the C
header, the host helpers of signals.py, and the entry point's refusals that need no device."""
import os
import re
import subprocess

import numpy as np
import pytest

import signal_rule_model as rm
from gym_trading_env_amd import _abi, signals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fix():
    x, rules = rm.fixture()
    return x, rules, rm.build_table(x, rules, rm.T_FIX, row=rm.build_row)


def test_loop_and_vectorised_statement_agree_on_the_fixture(fix):
    x, rules, by_loop = fix
    assert x.shape == (rm.C_FIX, rm.T_FIX) and x.dtype == np.float32 and len(rules) == 132
    np.testing.assert_array_equal(by_loop, rm.build_table(x, rules, rm.T_FIX))
    for T in (1, 15, 16, 17, 1023, 1024, 1025):  # a prefix of the bank gives a prefix of the table
        np.testing.assert_array_equal(rm.build_table(x, rules, T), by_loop[:, :T])


def test_the_fixture_exercises_what_it_is_for(fix):
    x, rules, table = fix
    assert np.isnan(x[2]).sum() >= 30 and (x[4, 1000:2300] == x[3, 1000:2300]).all()
    assert set(np.unique(table)) == {-1, 0, 1, 2}
    for byte in (-1, 0, 1, 2):
        share = (table == byte).mean()
        print(f"byte {byte}: {share:.3f} of the table")
        assert share >= 0.02, byte
    assert set(rules["warmup"]) == {0, 1, 15, 16, 17, 100, 1023, 1024, 1030, 3000}
    assert set(rules["b"]) == set(range(-1, rm.C_FIX)) and set(rules["latch"]) == {0, 1}
    assert {round(float(h) - float(l), 1) for h, l in zip(rules["hi"][:130], rules["lo"][:130])} == {0.0, 0.3, 2.0}
    carried = [i for i, r in enumerate(rules) if rm.carries_through_silent_piece(x, r)]
    print("latch rows that carry a state through rows 1024-2047:", carried)
    assert carried, "no latch row carries its state through a silent 1 024-row piece"
    for i in carried:  # ... and the table shows it: one byte, not the neutral one, over the whole piece
        piece = table[i, rm.SILENT[0]:rm.SILENT[1]]
        assert (piece == piece[0]).all() and piece[0] in (0, 2)


def _row(x, **kw):
    x = np.asarray(x, np.float32)
    x = x[None, :] if x.ndim == 1 else x
    r = signals.rules(**{"a": 0, "pos_up": 2, "pos_down": 0, "pos_neutral": 1, **kw})[0]
    loop, vec = rm.build_row(x, r, x.shape[1]), rm.build_row_vectorised(x, r, x.shape[1])
    np.testing.assert_array_equal(loop, vec)
    return loop.tolist()


def test_each_line_of_the_rule_by_hand():
    inf, nan = np.inf, np.nan
    x = [3, -3, 0.5, 3, 0.2, -0.2, -3, 0]
    # no latch: the zone of the row itself; thresholds are strict
    assert _row(x, hi=1, lo=-1) == [2, 0, 1, 2, 1, 1, 0, 1]
    assert _row([1, -1, 0], hi=1, lo=-1) == [1, 1, 1]
    # latch: the last non-zero zone, neutral before the first
    assert _row([0.5] + x, hi=1, lo=-1, latch=True) == [1, 2, 0, 0, 2, 2, 2, 0, 0]
    # warm-up: -1, and the state is untouched (row 0 would have latched "up")
    assert _row(x, hi=1, lo=-1, latch=True, warmup=1) == [-1, 0, 0, 2, 2, 2, 0, 0]
    assert _row([3, 0.5, 0.5], hi=1, lo=-1, latch=True, warmup=1) == [-1, 1, 1]
    assert _row(x, hi=1, lo=-1, warmup=100) == [-1] * 8
    assert _row(x, hi=1, lo=-1, warmup=-5) == _row(x, hi=1, lo=-1)
    # b == -1 compares a alone; with b the difference
    two = [[5, 5, 5, 1], [1, 5, 9, 1]]
    assert _row(two, b=1, hi=0, lo=0) == [2, 1, 0, 1]
    assert _row(two, b=-1, hi=0, lo=0) == [2, 2, 2, 2]
    assert _row(two, a=1, b=0, hi=0, lo=0) == [0, 1, 2, 1]
    # hi < lo: both comparisons hold in between, "up" wins
    assert _row([0, 2, -2], hi=-1, lo=1) == [2, 2, 0]
    # NaN in the indicator or in a threshold: neutral, and a latch keeps its state over it
    assert _row([3, nan, -3, nan], hi=1, lo=-1) == [2, 1, 0, 1]
    assert _row([3, nan, -3, nan], hi=1, lo=-1, latch=True) == [2, 2, 0, 0]
    assert _row([3, -3], hi=nan, lo=-1) == [1, 0]
    assert _row([3, -3], hi=1, lo=nan) == [2, 1]
    # infinities compare as numbers; inf - inf is NaN
    assert _row([inf, -inf, 3], hi=1e30, lo=-1e30) == [2, 0, 1]
    assert _row([[inf, -inf, inf, 1], [inf, -inf, -inf, inf]], b=1, hi=0, lo=0, latch=True) == [1, 1, 2, 0]
    # a subnormal difference is a difference
    tiny = np.float32(1e-45)
    assert tiny > 0 and _row([[tiny * 3, tiny], [tiny, tiny * 3]], b=1, hi=0, lo=0) == [2, 0]
    # the bytes are written as given
    assert _row([3, -3, 0], hi=1, lo=-1, pos_up=-128, pos_down=127, pos_neutral=-1) == [-128, 127, -1]
    # an indicator outside the bank: a row of -1
    for bad in (dict(a=2), dict(a=-1), dict(b=2), dict(b=-2)):
        assert _row(two, hi=0, lo=0, **bad) == [-1] * 4


def test_rule_dtype_is_the_c_struct(tmp_path):
    assert signals.RULE_DTYPE.itemsize == 32
    fields = signals.RULE_DTYPE.names
    probe = "#include <stddef.h>\n#include <stdio.h>\n#include \"gte.h\"\nint main(void) {\n" + \
        '  printf("sizeof %zu\\n", sizeof(gte_signal_rule));\n' + \
        "".join(f'  printf("{f} %zu %zu\\n", offsetof(gte_signal_rule, {f}), sizeof(((gte_signal_rule*)0)->{f}));\n'
                for f in fields) + "  return 0;\n}\n"
    src = tmp_path / "probe.c"
    src.write_text(probe)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).split("\n")
    assert int(lines[0].split()[1]) == 32
    c_fields = [(n, int(o), int(s)) for n, o, s in (ln.split() for ln in lines[1:] if ln)]
    dt = signals.RULE_DTYPE
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in fields] == c_fields
    assert sum(s for _, _, s in c_fields) == 32  # no padding: the fields are the struct
    assert [dt.fields[n][0].kind for n in ("a", "hi", "pos_up", "latch")] == ["i", "f", "i", "u"]


def test_rules_broadcasts_and_checks_its_arguments():
    r = signals.rules(a=[0, 1, 2], b=7, hi=0.5, lo=[-1.0, -2.0, -3.0], warmup=20, pos_up=2, pos_down=0, latch=[1, 0, 5])
    assert r.dtype == signals.RULE_DTYPE and r.shape == (3,)
    assert r["a"].tolist() == [0, 1, 2] and r["b"].tolist() == [7] * 3 and r["lo"].tolist() == [-1, -2, -3]
    assert r["latch"].tolist() == [1, 0, 1] and r["pos_neutral"].tolist() == [-1] * 3 and (r["reserved"] == 0).all()
    assert r["hi"].dtype == np.float32 and r["warmup"].tolist() == [20] * 3
    one = signals.rules(3)
    assert one.shape == (1,) and (one["a"][0], one["b"][0], one["latch"][0]) == (3, -1, 0)
    grid = signals.rules(a=np.arange(4)[:, None], b=np.arange(5)[None, :])  # a grid, flattened in C order
    assert grid.shape == (20,) and grid["a"].tolist() == np.repeat(np.arange(4), 5).tolist()
    with pytest.raises(ValueError, match="pos_up"):
        signals.rules(0, pos_up=128)
    with pytest.raises(TypeError, match="a must be integers"):
        signals.rules(0.5)
    with pytest.raises(ValueError):
        signals.rules([0, 1], b=[0, 1, 2])


def test_pad_bank():
    x = np.arange(2 * 17, dtype=np.float64).reshape(2, 17)
    p = signals.pad_bank(x)
    assert p.dtype == np.float32 and p.shape == (2, 32) and p.flags.c_contiguous
    np.testing.assert_array_equal(p[:, :17], x)
    assert (p[:, 17:] == 0).all() and signals.bank_stride(17) == 32 and signals.bank_stride(16) == 16
    assert signals.pad_bank(np.ones(5)).shape == (1, 16)
    with pytest.raises(ValueError):
        signals.pad_bank(np.ones((2, 3, 4)))


def test_sma_bank_against_a_direct_windowed_mean():
    rng = np.random.default_rng(3)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 1e-2, 300)))
    windows = [1, 2, 7, 50, 300, 301]
    bank = signals.sma_bank(close, windows)
    assert bank.dtype == np.float32 and bank.shape == (6, 300)
    for i, n in enumerate(windows):
        assert np.isnan(bank[i, :n - 1]).all() and not np.isnan(bank[i, n - 1:]).any()
        for t in range(n - 1, 300):
            # f64 prefix sums against an f64 mean of the window: both within a few f64 ulp of the true
            # mean, far below half an f32 ulp almost everywhere — allow one f32 ulp for a tie
            direct = np.float32(close[t + 1 - n:t + 1].mean())
            assert abs(bank[i, t] - direct) <= np.spacing(direct), (n, t)
    np.testing.assert_array_equal(bank[0], close.astype(np.float32))
    with pytest.raises(ValueError):
        signals.sma_bank(close, [0])


def test_header_and_ctypes_table_declare_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "gte.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint gte_build_signals\s*\(([^)]*)\)\s*;", code)
    assert m, "include/gte.h does not declare gte_build_signals"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["gte_env* env", "int32_t ds", "const float* indicators_device", "int32_t n_indicators",
                    "int64_t ind_stride", "const gte_signal_rule* rules_device", "int32_t n_rules",
                    "int8_t* table_device", "int64_t row_stride"]
    restype, argtypes = _abi.SYMBOLS["gte_build_signals"]
    assert len(argtypes) == len(args)
    # the rule's text stands in the header
    comment = hdr[hdr.index("typedef struct gte_signal_rule"):hdr.index("int gte_build_signals(")]
    for line in ("if t < warmup: out[t] = -1; continue", "q = z if (z != 0 or not latch) else q",
                 "out[t] = pos_up if q > 0, pos_down if q < 0, else pos_neutral"):
        assert line in comment, line


def test_library_exports_the_entry_point_and_refuses_without_an_env():
    lib = _abi.load_library()
    assert hasattr(lib, "gte_build_signals")
    assert lib.gte_build_signals(None, 0, None, 1, 16, None, 1, None, 16) == _abi.GTE_ERR_INVALID
    assert "env is NULL" in lib.gte_last_error().decode()


def test_the_new_unit_is_built_like_the_others_and_uses_no_scratch():
    """gte_signals.hip: in the Makefile's SRCS (so under its flags: gfx950, -ffp-contract=off), no
    scratch memory, f32 subnormals kept."""
    import test_host_cpu as th
    assert "gte_signals.hip" in th._makefile_srcs()
    for k in th._resource_usage("gte_signals.hip"):
        print(k)
        assert k["scratch"] == 0, k
