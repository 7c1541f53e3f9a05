"""The model of the decorrelated leaderboard (tests/diversify_model.py, restating gte_diversify of include/gte.h):
what it is FOR (planted families come back as the clusters, one pick each), the threshold that drops nothing against
a plain sort, invariants on random inputs, the model against a per-strategy brute force in Python floats, the struct
layouts against the C header, and the build of the new translation unit.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import diversify_model as dm
from gym_trading_env_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- what it is for --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(5))
def test_planted_families_come_back_as_the_clusters(seed):
    """F = 6 factor rows of n = 24 normals, S = 257 strategies each a factor plus 0.05 x noise, all x 1e-3; score the
    row sum, max_corr 0.9, k = 16: exactly 6 picks, nothing remaining, each cluster exactly one family, the sizes sum
    to 257.  (Within a family the correlation is about 0.995, across families at most about 0.43 for these seeds.)"""
    x, family = dm.planted(seed)
    S = len(family)
    out = dm.diversify(dm.records(x), range(24), x.sum(axis=1), 0.9, 16)
    s = out["summary"][0]
    assert (s["picked"], s["candidates"], s["eligible"], s["remaining"], s["reserved"]) == (6, S, S, 0, 0)
    assert (out["pick"][:6] >= 0).all() and (out["pick"][6:] == -1).all() and np.isnan(out["pick_score"][6:]).all()
    assert int(out["cluster_size"].sum()) == S == 257 and not out["cluster_size"][6:].any()
    assert sorted(family[out["pick"][:6]].tolist()) == list(range(6))            # one pick per family
    for r in range(6):
        members = np.flatnonzero(out["owner"] == r)
        assert len(members) == out["cluster_size"][r]
        assert (family[members] == family[out["pick"][r]]).all()
        assert len(members) == int((family == family[out["pick"][r]]).sum())     # the whole family, nothing else
    assert (np.diff(out["pick_score"][:6]) <= 0).all()                            # best first
    off = out["pick_corr"][:6, :6][~np.eye(6, dtype=bool)]
    assert off.max() < 0.9 and np.isnan(out["pick_corr"][6:]).all() and np.isnan(out["pick_corr"][:, 6:]).all()
    assert np.abs(np.diag(out["pick_corr"])[:6] - 1.0).max() < 1e-14


def test_a_threshold_above_one_is_a_plain_sort():
    """max_corr = +inf drops only the picks: they are the first k candidates by (score descending, index ascending),
    every cluster_size is 1"""
    rng = np.random.default_rng(3)
    S, n, k = 90, 5, 40
    x = rng.normal(0, 1, (S, n))
    scores = np.round(rng.normal(0, 1, S), 1)            # many ties
    scores[[4, 50]] = np.nan
    scores[7], scores[8], scores[60] = np.inf, -np.inf, np.inf
    x[20] = 2.5                                           # constant: no candidate
    for max_corr in (np.inf, 1.5):
        out = dm.diversify(dm.records(x), range(n), scores, max_corr, k)
        cand = [s for s in range(S) if s not in (4, 50, 20)]
        order = sorted(cand, key=lambda s: (-scores[s], s))
        assert out["pick"].tolist() == order[:k] and (out["cluster_size"] == 1).all()
        assert dm.same_f64(out["pick_score"], scores[order[:k]])
        assert out["summary"][0]["remaining"] == len(cand) - k and out["summary"][0]["candidates"] == len(cand)
        assert (out["owner"][order[k:]] == -1).all() and (out["owner"][[4, 50, 20]] == -2).all()
    out = dm.diversify(dm.records(x), range(n), scores, np.inf, 256)     # k beyond the candidates
    assert out["pick"][:len(cand)].tolist() == order and (out["pick"][len(cand):] == -1).all()
    assert out["summary"][0]["picked"] == len(cand) and out["summary"][0]["remaining"] == 0


@pytest.mark.parametrize("seed", range(6))
def test_invariants_on_random_inputs(seed):
    rng = np.random.default_rng(100 + seed)
    S, B = int(rng.integers(5, 400)), int(rng.integers(3, 40))
    ids = np.sort(rng.choice(B, int(rng.integers(3, B + 1)), replace=False))
    base = rng.normal(0, 1, (int(rng.integers(1, 8)), B))
    x = base[rng.integers(0, len(base), S)] + rng.uniform(0.05, 1.0) * rng.normal(0, 1, (S, B))
    steps = rng.integers(0, 3, (S, B)) + (rng.random((S, 1)) < 0.9)
    x[rng.random(S) < 0.05, ids[0]] = np.nan
    scores = rng.normal(0, 1, S)
    scores[rng.random(S) < 0.1] = np.nan
    k = int(rng.integers(1, 30))
    max_corr = float(rng.choice([-0.3, 0.0, 0.5, 0.8, 0.95]))
    out = dm.diversify(dm.records(x, steps), ids, scores, max_corr, k)
    s = out["summary"][0]
    taken = out["pick"] >= 0
    assert taken[:int(taken.sum())].all() and s["picked"] == taken.sum()              # a -1 is never followed by a pick
    off = out["pick_corr"][np.ix_(taken, taken)][~np.eye(int(taken.sum()), dtype=bool)]
    assert not len(off) or off.max() <= max_corr                                      # the shortlist is decorrelated
    owned = out["owner"] >= 0
    not_pick = owned.copy()
    not_pick[out["pick"][taken]] = False
    assert (out["owner_corr"][not_pick] > max_corr).all()                             # what a pick took, it took for cause
    assert (out["owner"][out["pick"][taken]] == np.flatnonzero(taken)).all()          # a pick owns itself
    assert int(out["cluster_size"].sum()) + s["remaining"] == s["candidates"] <= s["eligible"] <= S
    assert np.array_equal(out["owner"] == -2, ~out["candidate"])
    assert np.array_equal(np.isnan(out["owner_corr"]), out["owner"] < 0)
    assert s["remaining"] == int((out["owner"] == -1).sum())
    assert np.array_equal(np.bincount(out["owner"][owned], minlength=k), out["cluster_size"])
    assert dm.same_f64(out["pick_corr"], out["pick_corr"].T)                          # symmetric to the bit
    assert np.array_equal(out["candidate"], out["eligible"] & ~np.isnan(scores))


# ---- the model against a brute force ---------------------------------------------------------------------------

def _brute(stats, periods, scores, max_corr, k):
    """strategy by strategy, Python floats, no NumPy arithmetic"""
    S, n = stats.shape[0], len(periods)
    nan = float("nan")
    u, elig = [], []
    for s in range(S):
        x = [float(stats["reward_sum"][s, b]) for b in periods]
        ok = all(int(stats["steps"][s, b]) > 0 and math.isfinite(v) for b, v in zip(periods, x))
        t = 0.0
        for v in x:
            t = t + v
        m = t / float(n)
        e = [v - m for v in x]
        q = 0.0
        for v in e:
            q = q + v * v
        ok = ok and math.isfinite(q) and q > 0.0
        u.append([v / math.sqrt(q) for v in e] if ok else None)
        elig.append(ok)

    def corr(s, j):
        c = 0.0
        for a, b in zip(u[s], u[j]):
            c = c + a * b
        return c
    live = [elig[s] and scores[s] == scores[s] for s in range(S)]
    cands = sum(live)
    owner = [-1 if v else -2 for v in live]
    owner_corr = [nan] * S
    pick, pick_score, size = [-1] * k, [nan] * k, [0] * k
    for r in range(k):
        p = -1
        for s in range(S):
            if live[s] and (p < 0 or scores[s] > scores[p]):
                p = s
        if p < 0:
            break
        pick[r], pick_score[r] = p, float(scores[p])
        for s in range(S):
            if live[s]:
                c = corr(s, p)
                if s == p or c > max_corr:
                    live[s], owner[s], owner_corr[s] = False, r, c
                    size[r] += 1
    pick_corr = [[corr(a, b) if a >= 0 and b >= 0 else nan for b in pick] for a in pick]
    return dict(pick=pick, pick_score=pick_score, cluster_size=size, owner=owner, owner_corr=owner_corr,
                pick_corr=pick_corr, summary=(sum(p >= 0 for p in pick), cands, sum(elig), sum(live), 0))


def test_model_equals_a_brute_force():
    for seed in range(6):
        rng = np.random.default_rng(seed)
        S, B = 23, 9
        base = rng.normal(0, 1, (4, B))
        x = (base[rng.integers(0, 4, S)] + 0.3 * rng.normal(0, 1, (S, B))) * 10.0 ** rng.integers(-6, 6, (S, 1))
        steps = np.ones((S, B), np.int64)
        x[2] = x[1]                                  # a duplicate of a row
        x[3] = -x[1]                                 # its mirror
        x[4] = 0.0                                   # all zero
        x[5] = -3.25                                 # constant
        x[6, 2] = np.nan
        x[7, 4] = np.inf
        steps[8, 7] = 0
        x[9, 0], steps[9, 8] = np.nan, 0             # poison outside the selection: does not matter
        scores = np.round(rng.normal(0, 1, S), 1)
        scores[10], scores[11], scores[12], scores[13], scores[14] = np.nan, np.inf, -np.inf, 0.0, -0.0
        periods = [1, 2, 3, 4, 5, 6, 7]
        stats = dm.records(x, steps)
        for max_corr, k in ((0.5, 4), (-np.inf, 3), (0.0, 23), (0.9, 30), (2.0, 5)):
            got = dm.diversify(stats, periods, scores, max_corr, k)
            want = _brute(stats, periods, scores, max_corr, k)
            for key in ("pick", "cluster_size", "owner"):
                assert got[key].tolist() == want[key], (seed, max_corr, key)
            for key in ("pick_score", "owner_corr", "pick_corr"):
                assert dm.same_f64(got[key], np.array(want[key], np.float64)), (seed, max_corr, key)
            assert tuple(int(v) for v in got["summary"][0]) == want["summary"]
            assert got["eligible"].tolist() == [s not in (4, 5, 6, 7, 8) for s in range(S)]
            if max_corr == -np.inf:
                assert got["cluster_size"].tolist() == [want["summary"][1], 0, 0]


def test_duplicates_and_a_mirror():
    rng = np.random.default_rng(8)
    x = rng.normal(0, 1, (12, 10))
    x[5], x[9] = x[2], x[2]                          # 5 and 9 duplicate 2
    x[7] = -x[2]                                     # 7 mirrors it
    scores = np.zeros(12)
    scores[[2, 5, 9]] = 3.0                          # the duplicates tie for the lead: the lowest index takes it
    scores[7] = 2.0
    out = dm.diversify(dm.records(x), range(10), scores, 0.99, 3)
    assert out["pick"][0] == 2 and (out["owner"][[2, 5, 9]] == 0).all()
    assert out["owner_corr"][5].tobytes() == out["owner_corr"][2].tobytes() == out["owner_corr"][9].tobytes()
    assert out["pick"][1] == 7 and out["pick_corr"][0, 1] == -out["pick_corr"][0, 0]   # the hedge stays, and is next


# ---- layout ---------------------------------------------------------------------------------------------------

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gte.h"
#define F(t, f) printf(#t " " #f " %zu %zu\n", offsetof(t, f), sizeof(((t*)0)->f));
int main(void) {
  printf("consts %d %d %d %zu %zu\n", GTE_RANK_MAX, GTE_MAX_PERIODS, GTE_ABI_VERSION, sizeof(gte_diversify_summary),
         sizeof(gte_diversify_out));
  F(gte_diversify_summary, picked) F(gte_diversify_summary, candidates) F(gte_diversify_summary, eligible)
  F(gte_diversify_summary, remaining) F(gte_diversify_summary, reserved)
  F(gte_diversify_out, pick) F(gte_diversify_out, pick_score) F(gte_diversify_out, cluster_size)
  F(gte_diversify_out, owner) F(gte_diversify_out, owner_corr) F(gte_diversify_out, pick_corr)
  F(gte_diversify_out, summary)
  return 0;
}
"""


def test_struct_layouts_match_the_c_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).split("\n")
    assert lines[0].split()[1:] == ["256", "128", str(_abi.GTE_ABI_VERSION), "20", "56"]
    assert (_abi.GTE_RANK_MAX, _abi.GTE_MAX_PERIODS) == (dm.RANK_MAX, dm.MAX_PERIODS) == (256, 128)
    assert C.sizeof(_abi.GteDiversifySummary) == dm.SUMMARY.itemsize == 20
    assert np.dtype(_abi.DIVERSIFY_SUMMARY_DTYPE) == dm.SUMMARY
    assert C.sizeof(_abi.GteDiversifyOut) == 56
    for struct, ct in (("gte_diversify_summary", _abi.GteDiversifySummary), ("gte_diversify_out", _abi.GteDiversifyOut)):
        c_fields = [(n, int(o), int(s)) for t, n, o, s in (ln.split() for ln in lines[1:] if ln) if t == struct]
        assert c_fields == [(n, getattr(ct, n).offset, getattr(ct, n).size) for n, _ in ct._fields_]
    assert [(n, dm.SUMMARY.fields[n][1]) for n in dm.SUMMARY.names] == \
        [(n, getattr(_abi.GteDiversifySummary, n).offset) for n, _ in _abi.GteDiversifySummary._fields_]
    assert _abi.SYMBOLS["gte_diversify"][0] is C.c_int and len(_abi.SYMBOLS["gte_diversify"][1]) == 9
    assert _abi.SYMBOLS["gte_diversify"][1][6] is C.c_double
    assert np.dtype(_abi.STRATEGY_PERIOD_DTYPE) == dm.STRATEGY_PERIOD


# ---- build -----------------------------------------------------------------------------------------------------

def test_the_new_unit_is_built_like_the_others_and_uses_no_scratch():
    """gte_diversify.hip: in the Makefile's SRCS (so under its flags: gfx950, -ffp-contract=off); none of its three
    kernels uses scratch memory; its launcher is the one gte_launch.h declares; the launch boundary is its only
    device-wide ordering."""
    import test_host_cpu as th
    assert "gte_diversify.hip" in th._makefile_srcs()
    kernels = th._resource_usage("gte_diversify.hip")
    assert len(kernels) == 3
    for k in kernels:
        assert k["scratch"] == 0, k
    for name in ("gte_div_prepare_kernel", "gte_div_round_kernel", "gte_div_close_kernel"):
        assert sum(name in k["name"] for k in kernels) == 1, name
    src = th._csrc_sources()
    declared = th._signatures(src["gte_launch.h"])
    assert "launch_diversify" in declared and "diversify_scratch_bytes" in declared
    assert "atomic" not in src["gte_diversify.hip"].lower()
    assert "cooperative" not in src["gte_diversify.hip"].lower()
