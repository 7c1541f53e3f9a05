"""Per-strategy statistics and ranking, no GPU needed: the reduction, the scores and the ranking of
`gte_reduce_backtest_stats` / `gte_rank_strategies` (include/gte.h) as plain loops against an independently
written vectorised statement on the families the GPU tests use, the fixed summation order against
`math.fsum` and against a plain sequential sum, the ranking against a brute-force sort, the 128-byte layout
of `gte_strategy_stats` against the C header, and the declarations."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import strategy_model as sm
from gym_trading_env_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FIX = 2048


def families():
    """(name, records, member lists): what tests/test_gpu_strategy_stats.py sends through the device"""
    rec = sm.craft_records(N_FIX, seed=0)
    out = []
    for S in (1, 3, 64, 65, N_FIX, N_FIX + 5):
        for base in (0, 7):
            out.append((f"default S={S} base={base}", rec, sm.default_groups(N_FIX, S, base)))
    for extra in (0, 40):
        m, S = sm.skewed_map(extra_strategies=extra)
        out.append((f"skewed S={S}", sm.craft_records(len(m), seed=2), sm.map_groups(m, S)))
    # a CSR list that names envs outside [0, N): they keep their place and are skipped
    groups = sm.default_groups(200, 5)
    groups[1][3], groups[1][9], groups[4][0] = -1, 200, 2 ** 31 - 1
    out.append(("skipped ids", sm.craft_records(200, seed=3), groups))
    return out


FAMILIES = families()


@pytest.mark.parametrize("name,rec,groups", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_loop_and_vectorised_reduction_agree_byte_for_byte(name, rec, groups):
    by_loop, by_vector = sm.reduce_loop(rec, groups), sm.reduce_vector(rec, groups)
    assert by_loop.dtype == sm.STRATEGY and by_loop.dtype.itemsize == 128
    assert sm.same_bytes(by_loop, by_vector)
    assert not by_loop["reserved"].any()
    assert by_loop["envs"].sum() == sum(1 for g in groups for e in g if 0 <= e < len(rec))


def test_the_families_exercise_what_they_are_for():
    rec = sm.craft_records(N_FIX, seed=0)
    assert (rec["steps"] == 0).sum() > 100 and np.isnan(rec["reward_sum"]).sum() == 1
    assert np.isinf(rec["reward_sum"]).sum() == 2 and (rec["trades"] == 2 ** 30).sum() == 8
    mags = np.abs(rec["reward_sum"][np.isfinite(rec["reward_sum"]) & (rec["reward_sum"] != 0)])
    assert mags.min() < 1e-10 and mags.max() > 1e2 and (rec["reward_sum"] < 0).sum() > 500
    whole = sm.reduce_loop(rec, sm.default_groups(N_FIX, 1))[0]
    assert whole["trades"] > 2 ** 32 and whole["episodes"] > 2 ** 31 and whole["envs"] == N_FIX
    assert whole["envs_stepped"] == (rec["steps"] > 0).sum() and np.isnan(whole["reward_sum"])
    empty = sm.reduce_loop(rec, sm.default_groups(N_FIX, N_FIX + 5))[-1]
    assert empty["envs"] == 0 and empty["best_reward_sum"] == -np.inf and empty["worst_reward_sum"] == np.inf
    assert empty["max_drawdown"] == 0.0 and empty["reward_sum"] == 0.0 and empty["steps"] == 0
    m, S = sm.skewed_map()
    assert sorted(np.bincount(m, minlength=S).tolist()) == sorted(sm.SKEWED_COUNTS)
    assert {0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600} <= set(sm.SKEWED_COUNTS)


def test_extremes_follow_the_member_order():
    rec = np.zeros(4, dtype=sm.BACKTEST)
    rec["steps"] = [1, 1, 0, 1]
    rec["reward_sum"] = [-0.0, 0.0, 5.0, np.nan]
    rec["max_drawdown"] = [-0.0, np.nan, 0.25, 0.125]
    for groups, bits in (([[0, 1, 2, 3]], b"\x80"), ([[1, 0, 3, 2]], b"\x00")):
        for out in (sm.reduce_loop(rec, groups), sm.reduce_vector(rec, groups)):
            # of equal values the first stays: the sign of the zero says which; env 2 never stepped; NaN never wins
            assert out["best_reward_sum"].tobytes()[7:] == bits and out["worst_reward_sum"].tobytes()[7:] == bits
            assert out["best_reward_sum"][0] == 0.0 and out["max_drawdown"][0] == 0.25 and out["envs_stepped"][0] == 3


def _finite_family():
    """the GPU test's records without the NaN and the infinities, under every default map it uses"""
    rec = sm.craft_records(N_FIX, seed=0, specials=False)
    return rec, [sm.default_groups(N_FIX, S, base) for S in (1, 3, 64, 65, N_FIX, N_FIX + 5) for base in (0, 7)]


def test_fixed_order_sums_lie_within_the_sequential_rounding_bound_of_fsum():
    """|sum - exact| <= n * 2^-52 * sum|x| for n members (the bound the project holds pandas' rolling sums to,
    from one rounding per addition).  It covers the fixed order: the first addition into each accumulator is
    0.0 + x and joining an accumulator that is still 0.0 changes nothing, both exact, so of the additions into
    the eight accumulators and the seven that join them at most n - 1 round."""
    rec, maps = _finite_family()
    checked = 0
    for groups in maps:
        out = sm.reduce_loop(rec, groups)
        for s, g in enumerate(groups):
            for name in sm.SUMS:
                x = rec[name][g].tolist()
                bound = len(x) * 2.0 ** -52 * math.fsum(abs(v) for v in x)
                assert abs(float(out[name][s]) - math.fsum(x)) <= bound, (name, s, len(x))
                checked += 1
    assert checked == 4 * 2 * (1 + 3 + 64 + 65 + N_FIX + N_FIX + 5)


def test_the_fixed_order_differs_from_a_plain_sequential_sum_on_the_gpu_family():
    """so that bit equality with the device says something: at least one sum of every GPU family with
    strategies of more than eight members is not what adding the members one after the other gives (S = 1
    aside, where the NaN and the infinities of the family reach every sum)"""
    checked = 0
    for name, rec, groups in FAMILIES:
        if max(len(g) for g in groups) <= 8 or "skipped" in name:
            continue
        out = sm.reduce_loop(rec, groups)
        differ = finite = 0
        for s, g in enumerate(groups):
            for field in sm.SUMS:
                seq = functools.reduce(lambda a, b: a + b, rec[field][g].tolist(), 0.0)
                finite += math.isfinite(seq) and len(g) > 8
                differ += math.isfinite(seq) and seq != float(out[field][s])
        assert differ >= 1 or finite == 0, name
        checked += finite > 0
    assert checked >= 8


@pytest.mark.parametrize("S", [1, 5, 300, 3000])
def test_scores_loop_and_vector_agree(S):
    stats = sm.craft_stats(S, seed=S)
    for metric in sm.METRICS:
        assert sm.same_f64(sm.scores_loop(stats, metric), sm.scores_vector(stats, metric)), metric
    real = sm.reduce_loop(sm.craft_records(N_FIX), sm.default_groups(N_FIX, 65))
    for metric in range(len(sm.METRICS)):
        assert sm.same_f64(sm.scores_loop(real, metric), sm.scores_vector(real, metric)), metric


def test_sharpe_is_backtest_stats_sharpe_on_the_pooled_sums():
    stats = sm.craft_stats(300, seed=1)
    with np.errstate(all="ignore"):
        m = stats["reward_sum"] / stats["steps"]
        sd = np.sqrt(np.maximum(stats["reward_sq_sum"] / stats["steps"] - m ** 2, 0.0))
        ok = np.isfinite(m / sd)
        np.testing.assert_array_equal((m / sd)[ok], sm.scores_vector(stats, "sharpe")[ok])
    assert ok.sum() > 250


def _brute_force(stats, scores, min_episodes, k):
    keyed = []
    for s in range(len(stats)):
        if stats["steps"][s] >= 1 and stats["episodes"][s] >= min_episodes and not math.isnan(scores[s]):
            keyed.append((-(float(scores[s]) + 0.0), s))  # (-0.0 + 0.0 = 0.0: the zeros tie, the index decides)
    keyed.sort()
    index = [s for _, s in keyed[:k]] + [-1] * (k - min(k, len(keyed)))
    return index, [scores[s] if s >= 0 else float("nan") for s in index]


@pytest.mark.parametrize("S,k,min_episodes", [(1, 1, 0), (1, 256, 1), (16, 5, 1), (300, 1, 1), (300, 256, 0),
                                               (300, 256, 30), (3000, 256, 1), (300, 40, 10 ** 9)])
def test_ranking_against_a_brute_force_sort(S, k, min_episodes):
    stats = sm.craft_stats(S, seed=S + k)
    for metric in sm.METRICS:
        scores = sm.scores_vector(stats, metric)
        want_i, want_s = _brute_force(stats, scores, min_episodes, k)
        for index, top in (sm.rank_loop(stats, scores, min_episodes, k), sm.rank_vector(stats, scores, min_episodes, k)):
            assert index.dtype == np.int32 and index.tolist() == want_i, metric
            assert sm.same_f64(top, np.array(want_s, dtype=np.float64)), metric
    if min_episodes == 10 ** 9:
        assert set(want_i) == {-1}


def test_ranking_rules_by_hand():
    t = np.zeros(8, dtype=sm.STRATEGY)
    t["steps"], t["episodes"] = [5, 5, 0, 5, 5, 5, 5, 5], [2, 2, 2, 0, 2, 2, 2, 2]
    t["worst_reward_sum"] = [0.0, -0.0, 99.0, 98.0, np.nan, -np.inf, np.inf, 0.0]
    scores = sm.scores_vector(t, "worst_reward_sum")
    for rank in (sm.rank_loop, sm.rank_vector):
        index, top = rank(t, scores, 1, 8)
        # +inf first; the three zeros tie and keep index order (-0.0 == 0.0); -inf ranks like any value; never
        # stepped (2), too few episodes (3) and NaN (4) are not ranked
        assert index.tolist() == [6, 0, 1, 7, 5, -1, -1, -1]
        assert math.copysign(1, top[2]) == -1 and np.isnan(top[5:]).all() and top[4] == -np.inf
        assert rank(t, scores, 0, 2)[0].tolist() == [6, 3]


def test_strategy_dtype_is_the_c_struct(tmp_path):
    dt = np.dtype(_abi.STRATEGY_DTYPE)
    assert dt.itemsize == 128 == C.sizeof(_abi.GteStrategyStats)
    probe = "#include <stddef.h>\n#include <stdio.h>\n#include \"gte.h\"\nint main(void) {\n" + \
        '  printf("size %zu\\n", sizeof(gte_strategy_stats));\n' + \
        "".join(f'  printf("{f} %zu %zu\\n", offsetof(gte_strategy_stats, {f}), sizeof(((gte_strategy_stats*)0)->{f}));\n'
                for f in dt.names) + "  return 0;\n}\n"
    src = tmp_path / "probe.c"
    src.write_text(probe)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).split("\n")
    assert int(lines[0].split()[1]) == 128
    c_fields = [(n, int(o), int(s)) for n, o, s in (ln.split() for ln in lines[1:] if ln)]
    assert c_fields == [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names]
    assert [(n, getattr(_abi.GteStrategyStats, n).offset) for n in dt.names] == [(n, o) for n, o, _ in c_fields]
    # the 16-byte pieces the kernel stores: no field straddles one
    assert all(o // 16 == (o + min(s, 16) - 1) // 16 for _, o, s in c_fields)


def _prototype(code, name):
    m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", code)
    assert m, f"include/gte.h does not declare {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_prototypes_against_the_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "gte.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert _prototype(code, "gte_reduce_backtest_stats") == [
        "gte_env* env", "const gte_backtest_stats* records_device", "int32_t n_strategies",
        "const int32_t* group_offsets_device", "const int32_t* group_envs_device", "gte_strategy_stats* out_device"]
    assert _prototype(code, "gte_rank_strategies") == [
        "gte_env* env", "const gte_strategy_stats* stats_device", "int32_t n_strategies", "int32_t metric",
        "int64_t min_episodes", "int32_t k", "int32_t* top_index_device", "double* top_score_device",
        "double* scores_device"]
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in ("gte_reduce_backtest_stats", "gte_rank_strategies"):
        restype, argtypes = _abi.SYMBOLS[name]
        want = [C.c_void_p if "*" in a else ctype[a.split()[0]] for a in _prototype(code, name)]
        assert restype is C.c_int and argtypes == want, name
    assert re.search(r"#define GTE_ABI_VERSION 5\b", code) and _abi.GTE_ABI_VERSION == 5
    assert int(re.search(r"#define GTE_RANK_MAX (\d+)", code).group(1)) == _abi.GTE_RANK_MAX == 256
    # the order rule stands in the header
    text = " ".join(hdr.split())
    for line in ("eight interleaved accumulators", "((((((a_0 + a_1) + a_2) + a_3) + a_4) + a_5) + a_6) + a_7",
                 "if (x > m) m = x", "e = ((s - env_id_base) mod S) + j * S"):
        assert line in text, line


def test_metric_enum_against_its_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "gte.h")).read()
    body = re.search(r"typedef enum gte_strategy_metric \{(.*?)\} gte_strategy_metric;", hdr, re.S).group(1)
    enum = [(n, int(v)) for n, v in re.findall(r"GTE_METRIC_(\w+) = (\d+)", body)]
    assert len(enum) == 6 and [v for _, v in enum] == list(range(6))
    assert [n.lower() for n, _ in enum] == list(_abi.STRATEGY_METRICS)
    for n, v in enum:
        assert getattr(_abi, "METRIC_" + n) == v


def test_library_exports_the_entry_points_and_refuses_without_an_env():
    lib = _abi.load_library()
    assert lib.gte_reduce_backtest_stats(None, None, 1, None, None, None) == _abi.GTE_ERR_INVALID
    assert "env is NULL" in lib.gte_last_error().decode()
    assert lib.gte_rank_strategies(None, None, 1, 0, 1, 1, None, None, None) == _abi.GTE_ERR_INVALID
    assert "env is NULL" in lib.gte_last_error().decode()


def test_the_new_unit_is_built_like_the_others_and_uses_no_scratch():
    """gte_strategy.hip: in the Makefile's SRCS (so under its flags: gfx950, -ffp-contract=off), four kernels,
    none with scratch memory; only the selection uses LDS."""
    import test_host_cpu as th
    assert "gte_strategy.hip" in th._makefile_srcs()
    usage = th._resource_usage("gte_strategy.hip")
    assert len(usage) == 4
    for k in usage:
        print(k)
        assert k["scratch"] == 0, k


def test_python_layer_names():
    import gym_trading_env_amd as gte
    from gym_trading_env_amd.backtest_stats import BacktestStats, StrategyStats, _metric_code
    assert gte.StrategyStats is StrategyStats and hasattr(BacktestStats, "by_strategy")
    assert StrategyStats.FIELDS == tuple(n for n in np.dtype(_abi.STRATEGY_DTYPE).names if n != "reserved")
    assert [_metric_code(n) for n in _abi.STRATEGY_METRICS] == list(range(6)) and _metric_code("SHARPE") == 1
    assert _metric_code(_abi.METRIC_WORST_REWARD_SUM) == 5
    with pytest.raises(ValueError):
        _metric_code("median")
    with pytest.raises(ValueError):
        _metric_code(6)
    with pytest.raises(TypeError):
        _metric_code(1.5)
