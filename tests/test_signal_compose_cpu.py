"""Signal tables composed from clause rows, no GPU needed: the rule of `gte_compose_signals`
(include/gte.h) as a plain loop against an independently written vectorised statement on the fixture
the GPU tests use, hand-written cases for each line of the rule, the 128-byte layout of
`gte_signal_compose` against the C header, `signals.compose` / `signals.clauses`, and the entry point's
refusals that need no device."""
import os
import re
import subprocess

import numpy as np
import pytest

import signal_compose_model as cm
from gym_trading_env_amd import _abi, signals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP = signals.KEEP


@pytest.fixture(scope="module")
def fix():
    clauses, specs = cm.fixture()
    return clauses, specs, cm.compose_table(clauses, specs, cm.T_FIX, row=cm.compose_row)


def test_loop_and_vectorised_statement_agree_on_the_fixture(fix):
    clauses, specs, by_loop = fix
    assert clauses.shape == (cm.R_FIX, cm.T_FIX) and clauses.dtype == np.int8 and 90 <= len(specs) <= 130
    np.testing.assert_array_equal(by_loop, cm.compose_table(clauses, specs, cm.T_FIX))
    for T in (1, 15, 16, 17, 1023, 1024, 1025):  # a prefix of the clauses gives a prefix of the table
        np.testing.assert_array_equal(cm.compose_table(clauses, specs, T), by_loop[:, :T])
        np.testing.assert_array_equal(cm.compose_table(clauses, specs, T, row=cm.compose_row), by_loop[:, :T])


def test_the_fixture_exercises_what_it_is_for(fix):
    clauses, specs, table = fix
    for byte in (-1, 0, 1, 2):
        share = (table == byte).mean()
        print(f"byte {byte}: {share:.3f} of the table")
        assert share >= 0.02, byte
    assert {-128, 7} <= set(np.unique(table))
    for r, n in enumerate(cm.PREFIXES):  # the -1 prefixes, and codes behind them
        assert (clauses[r, :n] == -1).all() and clauses[r, n] in (0, 1, 2)
    assert set(cm.PREFIXES) == {0, 1, 15, 16, 17, 1023, 1024, 1030}
    stray = [r for r in range(cm.R_FIX) if np.isin(clauses[r], (3, 127, -128)).any()]
    assert stray == [3, 8] and {3, 127, -128} <= set(clauses[3]) and {3, 127, -128} <= set(clauses[8])
    runs = [np.diff(np.flatnonzero(np.diff(clauses[r].astype(int)) != 0)).mean() for r in range(cm.R_FIX)]
    assert min(runs) > 1.5 and max(runs) > 100  # runs, not noise
    assert set(specs["n_in"]) == {0, 1, 2, 3, 4, 5}
    assert set(specs["initial"]) == set(cm.INITIALS) and set(specs["pos_invalid"]) == set(cm.INVALIDS)
    assert (specs["lut"] == KEEP).all(axis=1).sum() >= 4 and (specs["lut"] == KEEP).any(axis=1).sum() >= 30
    twice = [s for s in specs if 2 <= s["n_in"] <= 4 and len(set(s["in"][:s["n_in"]])) < s["n_in"]]
    assert len(twice) >= 3
    invalid = [i for i, s in enumerate(specs) if not cm.names_clause_rows(clauses, s)]
    assert len(invalid) == 4 and all((table[i] == -1).all() for i in invalid)
    assert [int(specs[i]["n_in"]) for i in invalid] == [0, 5, 2, 2]
    assert specs[invalid[2]]["in"][0] == -1 and specs[invalid[3]]["in"][1] == cm.R_FIX
    carried = [i for i, s in enumerate(specs) if cm.carries_through_silent_piece(clauses, s)]
    print("rows that carry a state through rows 1024-2047:", carried)
    assert carried, "no row carries its state through a silent 1 024-row piece"
    shown = 0
    for i in carried:  # ... and the table shows it: one byte over the whole piece
        piece = table[i, cm.SILENT[0]:cm.SILENT[1]]
        assert (piece == piece[0]).all()
        shown += piece[0] != specs[i]["initial"]
    assert shown >= 1, "no carried state differs from its row's initial"


def _row(clauses, inputs, lut, T=None, **kw):
    x = np.asarray(clauses, np.int8)
    x = x[None, :] if x.ndim == 1 else x
    spec = signals.compose(inputs, lut, **kw)[0]
    T = x.shape[1] if T is None else T
    loop, vec = cm.compose_row(x, spec, T), cm.compose_row_vectorised(x, spec, T)
    np.testing.assert_array_equal(loop, vec)
    return loop.tolist()


def test_each_line_of_the_rule_by_hand():
    ident = [0, 1, 2]
    # one input, the table applied byte by byte
    assert _row([0, 1, 2, 2, 0], [0], ident) == [0, 1, 2, 2, 0]
    assert _row([0, 1, 2], [0], [5, -7, 127]) == [5, -7, 127]
    # KEEP before any decision gives `initial`, afterwards the last decided entry
    assert _row([1, 1, 2, 1, 0, 1], [0], [0, KEEP, 2]) == [-1, -1, 2, 2, 0, 0]
    assert _row([1, 1, 2, 1, 0, 1], [0], [0, KEEP, 2], initial=1) == [1, 1, 2, 2, 0, 0]
    assert _row([1, 1, 1], [0], [KEEP] * 3, initial=2) == [2, 2, 2]
    # initial == KEEP is a state like any other: written as -128 until an entry decides
    assert _row([1, 1, 2, 1], [0], [0, KEEP, 2], initial=KEEP) == [-128, -128, 2, 2]
    # an input that is no code: pos_invalid, and the state is left alone (row 1 would have decided 0)
    assert _row([2, -1, 1, 3, 1, -128, 127, 1], [0], [0, KEEP, 2]) == [2, -1, 2, -1, 2, -1, -1, 2]
    assert _row([2, -1, 1], [0], [0, KEEP, 2], invalid=7) == [2, 7, 2]
    assert _row([-1, -1, 1, 0], [0], [0, KEEP, 2], initial=1, invalid=0) == [0, 0, 1, 0]
    two = [[0, 1, 2, 0, 1, 2, 0, 1, 2, -1, 2], [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, -1]]
    # the strides of the index: entry c0 + 3 c1
    assert _row(two, [0, 1], np.arange(9).reshape(3, 3).T, invalid=-5) == [0, 1, 2, 3, 4, 5, 6, 7, 8, -5, -5]
    assert _row(two, [1, 0], np.arange(9).reshape(3, 3).T, invalid=-5) == [0, 3, 6, 1, 4, 7, 2, 5, 8, -5, -5]
    assert _row(two, [0, 1], lambda a, b: 10 * a + b)[:9] == [0, 10, 20, 1, 11, 21, 2, 12, 22]
    # ... + 9 c2 + 27 c3, on the record itself
    four = np.array([[1, 2, 0], [2, 0, 0], [0, 1, 0], [2, 2, 1]], np.int8)
    spec = signals.compose([0, 1, 2, 3], np.zeros((3, 3, 3, 3), int))[0]
    spec["lut"] = np.arange(81)
    for row in (cm.compose_row, cm.compose_row_vectorised):
        assert row(four, spec, 3).tolist() == [1 + 6 + 0 + 54, 2 + 0 + 9 + 54, 27]
    # missing inputs count as code 0: with n_in = 2 only entries 0 .. 8 are reached, whatever the rest holds
    spec = signals.compose([0, 1], np.zeros((3, 3), int))[0]
    spec["lut"] = np.arange(81)
    for row in (cm.compose_row, cm.compose_row_vectorised):
        assert row(four, spec, 3).tolist() == [1 + 6, 2, 0]
    # ... and in[k] beyond n_in is not looked at, not even when it names no row
    spec["in"][2:] = (-1, 99)
    assert cm.compose_row(four, spec, 3).tolist() == [7, 2, 0] == cm.compose_row_vectorised(four, spec, 3).tolist()
    # a spec that names no clause row, or has no n_in: a row of -1
    for field, value in (("n_in", 0), ("n_in", 5), ("n_in", -1)):
        bad = spec.copy()
        bad[field] = value
        assert cm.compose_row(four, bad, 3).tolist() == [-1] * 3 == cm.compose_row_vectorised(four, bad, 3).tolist()
    for k, value in ((0, -1), (1, 4), (0, 2 ** 31 - 1)):
        bad = spec.copy()
        bad["in"][k] = value
        assert cm.compose_row(four, bad, 3).tolist() == [-1] * 3 == cm.compose_row_vectorised(four, bad, 3).tolist()
    # asymmetric entry / exit: up on a, down only on b
    a = [1, 2, 1, 0, 0, 1, 2, 1]
    b = [1, 1, 1, 1, 0, 1, 1, 0]
    assert _row([a, b], [0, 1], cm._enter_exit, initial=0) == [0, 2, 2, 2, 0, 0, 2, 0]
    # the same row named twice
    assert _row([a], [0, 0], cm._and) == [0, 2, 0, 0, 0, 0, 2, 0]


def test_compose_dtype_is_the_c_struct(tmp_path):
    assert signals.COMPOSE_DTYPE.itemsize == 128 and signals.KEEP == -128
    assert (signals.DOWN, signals.NEUTRAL, signals.UP) == (0, 1, 2)
    fields = signals.COMPOSE_DTYPE.names
    assert fields == ("in", "n_in", "initial", "pos_invalid", "reserved0", "lut", "reserved")
    probe = "#include <stddef.h>\n#include <stdio.h>\n#include \"gte.h\"\nint main(void) {\n" + \
        '  printf("sizeof %zu %d\\n", sizeof(gte_signal_compose), GTE_COMPOSE_KEEP);\n' + \
        "".join(f'  printf("{f} %zu %zu\\n", offsetof(gte_signal_compose, {f}), sizeof(((gte_signal_compose*)0)->{f}));\n'
                for f in fields) + "  return 0;\n}\n"
    src = tmp_path / "probe.c"
    src.write_text(probe)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).split("\n")
    assert lines[0].split()[1:] == ["128", "-128"]
    c_fields = [(n, int(o), int(s)) for n, o, s in (ln.split() for ln in lines[1:] if ln)]
    dt = signals.COMPOSE_DTYPE
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in fields] == c_fields
    assert sum(s for _, _, s in c_fields) == 128  # no padding: the fields are the struct
    assert dt.fields["in"][0].base == np.dtype("<i4") and dt.fields["lut"][0].base == np.dtype("i1")
    assert dt.fields["lut"][0].shape == (81,) and dt.fields["in"][0].shape == (4,)


def test_clauses_are_rules_that_write_zone_codes():
    c = signals.clauses(a=[0, 1], b=2, hi=0.5, lo=-0.5, warmup=9, latch=[0, 1])
    r = signals.rules(a=[0, 1], b=2, hi=0.5, lo=-0.5, warmup=9, pos_up=2, pos_down=0, pos_neutral=1, latch=[0, 1])
    assert c.dtype == signals.RULE_DTYPE and c.tobytes() == r.tobytes()


def test_compose_from_a_callable_an_array_and_per_strategy_tables():
    rng = np.random.default_rng(4)
    for n in (1, 2, 3, 4):
        table = rng.integers(-128, 128, (3,) * n)
        inputs = rng.integers(0, 50, (6, n))
        by_array = signals.compose(inputs, table, initial=2, invalid=7)
        by_call = signals.compose(inputs, lambda *c: int(table[c]), initial=2, invalid=7)
        assert by_array.dtype == signals.COMPOSE_DTYPE and by_array.shape == (6,)
        assert by_array.tobytes() == by_call.tobytes()
        assert signals.compose(inputs, np.broadcast_to(table, (6,) + table.shape), initial=2, invalid=7).tobytes() \
            == by_array.tobytes()
        assert (by_array["n_in"] == n).all() and (by_array["in"][:, :n] == inputs).all()
        assert (by_array["in"][:, n:] == 0).all() and (by_array["reserved"] == 0).all() and (by_array["reserved0"] == 0).all()
        assert (by_array["initial"] == 2).all() and (by_array["pos_invalid"] == 7).all()
        # entry c0 + 3 c1 + 9 c2 + 27 c3, the codes of missing inputs free: they count as 0
        for e in range(81):
            c = [(e // 3 ** k) % 3 for k in range(4)]
            assert by_array["lut"][0, e] == table[tuple(c[:n])]
    # one table per strategy, inputs for all; bytes per strategy
    tables = rng.integers(-2, 3, (5, 3, 3))
    s = signals.compose([4, 9], tables, initial=[0, 1, 2, -1, KEEP], invalid=-1)
    assert s.shape == (5,) and (s["in"][:, :2] == [4, 9]).all() and s["initial"].tolist() == [0, 1, 2, -1, -128]
    for i in range(5):
        assert s[i].tobytes() == signals.compose([4, 9], tables[i], initial=s["initial"][i])[0].tobytes()
    one = signals.compose([3], [0, KEEP, 2])
    assert one.shape == (1,) and one["lut"][0, :3].tolist() == [0, -128, 2] and one["initial"][0] == -1 == one["pos_invalid"][0]
    assert signals.compose([[1, 2]], np.ones((3, 3), bool))["lut"][0].tolist() == [1] * 81


def test_compose_refuses_what_does_not_fit():
    ok = np.zeros((3, 3), int)
    with pytest.raises(ValueError, match="1 <= n <= 4"):
        signals.compose(np.zeros((2, 5), int), np.zeros((3,) * 5, int))
    with pytest.raises(ValueError, match="1 <= n <= 4"):
        signals.compose(np.zeros((2, 0), int), ok)
    with pytest.raises(ValueError, match="1 <= n <= 4"):
        signals.compose(3, [0, 1, 2])
    with pytest.raises(TypeError, match="inputs must be integers"):
        signals.compose([0.5, 1.0], ok)
    with pytest.raises(ValueError, match="lut does not fit a byte"):
        signals.compose([0, 1], ok + 128)
    with pytest.raises(ValueError, match="lut does not fit a byte"):
        signals.compose([0, 1], lambda a, b: -129)
    with pytest.raises(ValueError, match="initial does not fit a byte"):
        signals.compose([0, 1], ok, initial=200)
    with pytest.raises(ValueError, match="invalid does not fit a byte"):
        signals.compose([0, 1], ok, invalid=-200)
    with pytest.raises(TypeError, match="truth-table entries must be integers"):
        signals.compose([0, 1], ok + 0.5)
    with pytest.raises(ValueError, match="lut: shape"):
        signals.compose([0, 1], np.zeros((3, 3, 3, 3), int))
    with pytest.raises(ValueError, match="lut: shape"):
        signals.compose([0, 1], np.zeros((3, 2), int))
    with pytest.raises(ValueError, match="number of strategies"):
        signals.compose(np.zeros((4, 2), int), np.zeros((5, 3, 3), int))
    with pytest.raises(ValueError, match="number of strategies"):
        signals.compose(np.zeros((4, 2), int), ok, initial=[0, 1, 2])
    with pytest.raises(ValueError, match="inputs do not fit"):
        signals.compose([0, 2 ** 31], ok)


def test_header_and_ctypes_table_declare_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "gte.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint gte_compose_signals\s*\(([^)]*)\)\s*;", code)
    assert m, "include/gte.h does not declare gte_compose_signals"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["gte_env* env", "int32_t ds", "const int8_t* clauses_device", "int32_t n_clause_rows",
                    "int64_t clause_stride", "const gte_signal_compose* specs_device", "int32_t n_specs",
                    "int8_t* table_device", "int64_t row_stride"]
    restype, argtypes = _abi.SYMBOLS["gte_compose_signals"]
    assert len(argtypes) == len(args)
    assert re.search(r"#define GTE_ABI_VERSION\s+5\b", hdr) and _abi.GTE_ABI_VERSION == 5
    # the rule's text stands in the header
    comment = hdr[hdr.index("typedef struct gte_signal_compose"):hdr.index("int gte_compose_signals(")]
    for line in ("c_k = clauses[in[k]][t] for k < n_in;  c_k = 0 for k >= n_in",
                 "if any c_k (k < n_in) is outside {0, 1, 2}:   out[t] = pos_invalid; continue",
                 "e = lut[c_0 + 3 c_1 + 9 c_2 + 27 c_3]", "if e != GTE_COMPOSE_KEEP:  q = e", "out[t] = q"):
        assert line in comment, line


def test_library_exports_the_entry_point_and_refuses_without_an_env():
    lib = _abi.load_library()
    assert hasattr(lib, "gte_compose_signals")
    assert lib.gte_compose_signals(None, 0, None, 1, 16, None, 1, None, 16) == _abi.GTE_ERR_INVALID
    assert "env is NULL" in lib.gte_last_error().decode()


def test_the_new_unit_is_built_like_the_others_and_uses_no_scratch():
    """gte_compose.hip: in the Makefile's SRCS (so under its flags: gfx950), no scratch memory, and the
    launcher is the one gte_launch.h declares."""
    import test_host_cpu as th
    assert "gte_compose.hip" in th._makefile_srcs()
    kernels = th._resource_usage("gte_compose.hip")
    assert [k["name"] for k in kernels if "gte_compose_signals_kernel" in k["name"]]
    for k in kernels:
        print(k)
        assert k["scratch"] == 0, k
    src = th._csrc_sources()
    assert "launch_compose_signals" in th._signatures(src["gte_launch.h"])
    assert th._signatures(src["gte_compose.hip"])["launch_compose_signals"][1]
    assert "gte::launch_compose_signals(" in src["gte_api_backtest.hip"]
