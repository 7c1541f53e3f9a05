"""The model of the probability of backtest overfitting (tests/cscv_model.py, restating gte_cscv of include/gte.h):
the model against a per-strategy brute force in Python floats, the group and split tables of
gym_trading_env_amd.periods, what the figure is FOR (a leaderboard of noise overfits about half the time, a real edge
never), the constants and struct layouts against the C header, and the build of the new translation unit.  No GPU."""
import ctypes as C
import math
import os
import subprocess
from itertools import combinations

import numpy as np
import pytest

import cscv_model as cm
from gym_trading_env_amd import _abi, periods

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model against a brute force ---------------------------------------------------------------------------

def _brute(stats, group_masks, is_groups, oos_groups, metric):
    """strategy by strategy, Python floats and ints, no NumPy arithmetic"""
    S, G, C_ = stats.shape[0], len(group_masks), len(is_groups)
    inf, nan = float("inf"), float("nan")

    def div(a, b):
        if b == 0:
            return nan if a == 0 or a != a else math.copysign(inf, a) * math.copysign(1.0, b)
        return a / b

    sums, elig = [], []
    for s in range(S):
        row, ok = [], True
        for words in group_masks:
            a1, a2, n = 0.0, 0.0, 0
            for b in cm.periods_of(words):
                a1 = a1 + float(stats["reward_sum"][s, b])
                a2 = a2 + float(stats["reward_sq_sum"][s, b])
                n += int(stats["steps"][s, b])
            ok = ok and n > 0 and math.isfinite(a1) and math.isfinite(a2)
            row.append((a1, a2, n))
        sums.append(row), elig.append(ok)

    def score(s, word):
        s1, s2, n = 0.0, 0.0, 0
        for g in cm.groups_of(word, G):
            s1, s2, n = s1 + sums[s][g][0], s2 + sums[s][g][1], n + sums[s][g][2]
        if metric == cm.REWARD_SUM:
            return s1
        m = div(s1, float(n))
        if metric == cm.MEAN_REWARD:
            return m
        v = div(s2, float(n)) - m * m
        if not v > 0.0:
            v = 0.0
        return div(m, math.sqrt(v))

    out = dict(best=[], is_score=[], oos_score=[], below=[], equal=[], ranked=[])
    valid = overfit = loss = 0
    for c in range(C_):
        m, best = -inf, -1
        for s in range(S):
            if elig[s] and score(s, is_groups[c]) > m:
                m, best = score(s, is_groups[c]), s
        oos = [score(s, oos_groups[c]) for s in range(S)]
        w = oos[best] if best >= 0 else nan
        ranked = sum(1 for s in range(S) if elig[s] and oos[s] == oos[s])
        ok = best >= 0 and w == w
        below = sum(1 for s in range(S) if elig[s] and oos[s] < w) if ok else 0
        equal = sum(1 for s in range(S) if elig[s] and oos[s] == w) if ok else 0
        valid, overfit, loss = valid + ok, overfit + (ok and 2 * below + equal <= ranked), loss + (ok and w < 0.0)
        for k, v in zip(out, (best, m if best >= 0 else nan, w, below, equal, ranked)):
            out[k].append(v)
    out["summary"] = (C_, valid, overfit, loss, sum(elig), 0)
    return out


def _tiny(seed):
    rng = np.random.default_rng(seed)
    S, B = 9, 7
    x = rng.normal(0, 1, (S, B)) * 10.0 ** rng.integers(-3, 3, (S, 1))
    sq = x * x * rng.uniform(1.0, 3.0, (S, B))
    steps = rng.integers(1, 9, (S, B))
    x[2] = x[1]; sq[2] = sq[1]; steps[2] = steps[1]      # a duplicate: the lower index wins
    x[3] = 0.0; sq[3] = 0.0                               # never trades: Sharpe 0 / 0
    x[4] = 0.25; sq[4] = 0.0625; steps[4] = 1             # constant reward: Sharpe +inf
    x[5, 1] = np.nan                                      # not eligible
    steps[6, [4, 5]] = 0                                  # a group without steps: not eligible
    x[7, 0] = -0.0
    return cm.records(x, sq, steps)


@pytest.mark.parametrize("metric", [cm.MEAN_REWARD, cm.SHARPE, cm.REWARD_SUM])
def test_model_equals_a_brute_force(metric):
    for seed in range(4):
        stats = _tiny(seed)
        groups = periods.cscv_groups(range(7), 4)            # 2, 2, 2, 1 periods
        tables = [periods.cscv_splits(4),
                  (np.array([1, 2, 12], np.uint32), np.array([8, 9, 1], np.uint32))]     # purged, uneven sides
        for is_g, oos_g in tables:
            got = cm.cscv(stats, groups, is_g, oos_g, metric)
            want = _brute(stats, groups, is_g, oos_g, metric)
            for k in ("best", "below", "equal", "ranked"):
                assert got[k].tolist() == want[k], (seed, k)
            for k in ("is_score", "oos_score"):
                assert cm.same_f64(got[k], want[k]), (seed, k, got[k], want[k])
            assert tuple(int(v) for v in got["summary"][0]) == want["summary"]
            assert got["eligible"].tolist() == [True] * 5 + [False, False, True, True]
            if metric == cm.SHARPE:
                assert (got["best"] == 4).all() and (got["is_score"] == np.inf).all()     # the constant reward
                assert (got["ranked"] == 6).all()                                         # 7 eligible, one 0 / 0


def test_single_period_groups_score_like_the_ranking():
    """groups of one period each: the score over a side is the ranking's s1 / s2 / n chain over those periods"""
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (5, 6))
    stats = cm.records(x, x * x * 2.0, rng.integers(1, 20, (5, 6)))
    groups = periods.cscv_groups(range(6), 6)
    a1, a2, n, _ = cm.group_sums(stats, groups)
    side = [0, 2, 5]
    s1, s2, c = np.zeros(5), np.zeros(5), np.zeros(5, np.int64)
    for b in side:
        s1, s2, c = s1 + stats["reward_sum"][:, b], s2 + stats["reward_sq_sum"][:, b], c + stats["steps"][:, b]
    for metric in (cm.MEAN_REWARD, cm.SHARPE, cm.REWARD_SUM):
        assert cm.same_f64(cm.side_score(metric, a1, a2, n, side), cm.score(metric, s1, s2, c))


# ---- the tables -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [2, 4, 6, 8, 12, 16, 18])
def test_cscv_splits(G):
    is_g, oos_g = periods.cscv_splits(G)
    n = math.comb(G, G // 2)
    assert is_g.dtype == oos_g.dtype == np.uint32 and is_g.shape == oos_g.shape == (n,)
    every = (1 << G) - 1
    assert not (is_g & oos_g).any() and ((is_g | oos_g) == every).all()
    assert all(bin(int(w)).count("1") == G // 2 for w in is_g)
    picks = [tuple(g for g in range(G) if (int(w) >> g) & 1) for w in is_g]
    assert picks == sorted(picks) == list(combinations(range(G), G // 2))      # lexicographic, each once
    assert np.array_equal(is_g[::-1], oos_g)                                    # split c and C - 1 - c mirror


def test_cscv_splits_refusals():
    assert _abi.GTE_CSCV_MAX_SPLITS == periods.CSCV_MAX_SPLITS == 65536 < math.comb(20, 10)
    for bad in (20, 22, 32, 34, 3, 7, 0, -2):
        with pytest.raises(ValueError):
            periods.cscv_splits(bad)


@pytest.mark.parametrize("ids,G", [(range(16), 16), (range(7), 4), ([3, 70, 64, 9, 127, 5, 63], 3), (range(128), 32),
                                   (range(2), 2), (range(100), 7)])
def test_cscv_groups(ids, G):
    table = periods.cscv_groups(ids, G)
    assert table.dtype == np.uint64 and table.shape == (G, 2)
    got = [cm.periods_of(row) for row in table]
    want_ids = sorted(ids)
    assert [b for g in got for b in g] == want_ids                              # contiguous, disjoint, in order
    size, longer = divmod(len(want_ids), G)
    assert [len(g) for g in got] == [size + 1] * longer + [size] * (G - longer)


def test_cscv_groups_refusals():
    for ids, G in ((range(3), 4), (range(5), 1), (range(40), 33), ([0, 128], 2), ([-1, 4], 2)):
        with pytest.raises(ValueError):
            periods.cscv_groups(ids, G)


# ---- what it is for --------------------------------------------------------------------------------------------

def _noise(seed, edge):
    """256 strategies, 8 groups of one period of 50 steps each, step rewards N(0, 0.01^2)"""
    S, G, steps = 256, 8, 50
    r = np.random.default_rng(seed).normal(0, 0.01, (S, G * steps))
    if edge:
        r[0] += 0.005
    return cm.from_step_rewards(r, np.repeat(np.arange(G), steps))


def test_noise_overfits_half_the_time_and_an_edge_never():
    """Selecting the best Sharpe of 256 strategies of pure noise: the in-sample winner is as likely to land in the
    lower half out of sample as in the upper one, PBO about 1/2 — averaged over 20 seeds it lies in [0.4, 0.6] (one
    seed alone ranges widely: 70 splits that share their data).  With half a standard deviation per step added to
    strategy 0 it wins every split on both sides: PBO exactly 0 for every seed."""
    groups = periods.cscv_groups(range(8), 8)
    is_g, oos_g = periods.cscv_splits(8)
    values = []
    for seed in range(20):
        out = cm.cscv(_noise(seed, False), groups, is_g, oos_g, cm.SHARPE)
        assert out["summary"][0]["valid"] == 70 and out["summary"][0]["eligible"] == 256
        values.append(cm.pbo(out))
        edge = cm.cscv(_noise(seed, True), groups, is_g, oos_g, cm.SHARPE)
        assert cm.pbo(edge) == 0.0 and (edge["best"] == 0).all(), seed
    mean = float(np.mean(values))
    print(f"[cscv] noise: mean PBO over 20 seeds {mean:.3f}, per seed {min(values):.2f} .. {max(values):.2f}")
    assert 0.4 <= mean <= 0.6


# ---- layout ---------------------------------------------------------------------------------------------------

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gte.h"
#define F(t, f) printf(#t " " #f " %zu %zu\n", offsetof(t, f), sizeof(((t*)0)->f));
int main(void) {
  printf("consts %d %d %d %d %zu %zu\n", GTE_CSCV_MAX_GROUPS, GTE_CSCV_MAX_SPLITS, GTE_CSCV_CHUNK, GTE_ABI_VERSION,
         sizeof(gte_cscv_summary), sizeof(gte_cscv_out));
  F(gte_cscv_summary, splits) F(gte_cscv_summary, valid) F(gte_cscv_summary, overfit) F(gte_cscv_summary, loss)
  F(gte_cscv_summary, eligible) F(gte_cscv_summary, reserved)
  F(gte_cscv_out, best) F(gte_cscv_out, is_score) F(gte_cscv_out, oos_score) F(gte_cscv_out, below)
  F(gte_cscv_out, equal) F(gte_cscv_out, ranked) F(gte_cscv_out, summary)
  return 0;
}
"""


def test_constants_and_struct_layouts_match_the_c_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).split("\n")
    assert lines[0].split()[1:] == ["32", "65536", "256", str(_abi.GTE_ABI_VERSION), "24", "56"]
    assert (_abi.GTE_CSCV_MAX_GROUPS, _abi.GTE_CSCV_MAX_SPLITS, _abi.GTE_CSCV_CHUNK) == \
        (cm.MAX_GROUPS, cm.MAX_SPLITS, cm.CHUNK) == (32, 65536, 256)
    assert periods.CSCV_MAX_GROUPS == 32
    assert C.sizeof(_abi.GteCscvSummary) == cm.SUMMARY.itemsize == 24
    assert np.dtype(_abi.CSCV_SUMMARY_DTYPE) == cm.SUMMARY
    assert C.sizeof(_abi.GteCscvOut) == 56
    for struct, ct in (("gte_cscv_summary", _abi.GteCscvSummary), ("gte_cscv_out", _abi.GteCscvOut)):
        c_fields = [(n, int(o), int(s)) for t, n, o, s in (ln.split() for ln in lines[1:] if ln) if t == struct]
        assert c_fields == [(n, getattr(ct, n).offset, getattr(ct, n).size) for n, _ in ct._fields_]
    assert [(n, cm.SUMMARY.fields[n][1]) for n in cm.SUMMARY.names] == \
        [(n, getattr(_abi.GteCscvSummary, n).offset) for n, _ in _abi.GteCscvSummary._fields_]
    assert _abi.SYMBOLS["gte_cscv"][0] is C.c_int and len(_abi.SYMBOLS["gte_cscv"][1]) == 11
    assert np.dtype(_abi.STRATEGY_PERIOD_DTYPE) == cm.STRATEGY_PERIOD
    assert [_abi.PERIOD_METRICS[m] for m in (cm.MEAN_REWARD, cm.SHARPE, cm.REWARD_SUM)] == list(_abi.CSCV_METRICS)


# ---- build -----------------------------------------------------------------------------------------------------

def test_the_new_unit_is_built_like_the_others_and_uses_no_scratch():
    """gte_cscv.hip: in the Makefile's SRCS (so under its flags: gfx950, -ffp-contract=off); no kernel of it uses
    scratch memory — the two passes keep a lane's 8, 16 or 32 group triplets in registers — and its launcher is
    the one gte_launch.h declares."""
    import test_host_cpu as th
    assert "gte_cscv.hip" in th._makefile_srcs()
    kernels = th._resource_usage("gte_cscv.hip")
    assert len(kernels) == 10
    for k in kernels:
        assert k["scratch"] == 0, k
    for name, copies in (("gte_cscv_pass1_kernel", 3), ("gte_cscv_pass2_kernel", 3), ("gte_cscv_fold_kernel", 1),
                         ("gte_cscv_winner_kernel", 1), ("gte_cscv_close_kernel", 1), ("gte_cscv_summary_kernel", 1)):
        assert sum(name in k["name"] for k in kernels) == copies, name
    src = th._csrc_sources()
    declared = th._signatures(src["gte_launch.h"])
    assert "launch_cscv" in declared and "cscv_scratch_bytes" in declared
    assert "atomic" not in src["gte_cscv.hip"]
