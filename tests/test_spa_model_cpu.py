"""The model of the test for superior predictive ability (tests/spa_model.py; gte_spa_test, include/gte.h) alone, no
GPU: the order of the three p-values, the two ends of the threshold, a step-down that stops at once and one that
rejects in two rounds, a board on which the three recentrings disagree, the leaderboard the Reality Check calls luck
and the studentised test does not, and the layout of the two structs against the C header and the ctypes table."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bootstrap_model as bm
import spa_model as sm
from gym_trading_env_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_ROUND_SEED = 1        # of seeds 0 .. 11 of two_round_board, 1, 4, 5 and 9 reject in rounds 0 and 1


@pytest.fixture(scope="module")
def w12():
    return bm.weights(12, 300, 2.0, 3)


@pytest.fixture(scope="module")
def w24():
    return bm.weights(24, 400, 2.0, 3)


def run(stats, w, threshold=None, alpha=0.1, max_rounds=8):
    n, R = w.shape[1], w.shape[0]
    thr = sm.default_threshold(n) if threshold is None else threshold
    return sm.spa_test(stats, np.ones(n, bool), None, w, thr, sm.crit_rank(alpha, R), max_rounds)


def test_crit_rank_and_threshold():
    assert sm.crit_rank(0.05, 1000) == 949 and sm.crit_rank(0.1, 300) == 269 and sm.crit_rank(0.05, 1) == 0
    assert sm.crit_rank(0.0, 300) == 299 and sm.crit_rank(1.0, 300) == 0
    assert sm.default_threshold(3) == math.sqrt(2 * math.log(math.log(3))) > 0
    with pytest.raises(ValueError):
        sm.default_threshold(2)       # log log 2 < 0


@pytest.mark.parametrize("seed", [0, 1, 4])
def test_p_values_are_ordered_and_the_threshold_has_two_ends(w24, seed):
    stats = sm.near_null_board(seed)
    mid = run(stats, w24)
    lo, co, up = sm.p_values(mid, 400)
    assert 0.0 <= lo <= co <= up <= 1.0
    assert (mid["max_stat"][:400] <= mid["max_stat"][400:800]).all()
    assert (mid["max_stat"][400:800] <= mid["max_stat"][800:]).all()
    # threshold = inf: nothing is recentred to zero, the consistent row IS the upper row
    inf = run(stats, w24, threshold=np.inf)
    assert inf["recentred"].all()
    assert inf["max_stat"][400:800].tobytes() == inf["max_stat"][800:].tobytes()
    assert inf["max_index"][400:800].tobytes() == inf["max_index"][800:].tobytes()
    assert inf["summary"]["count_consistent"] == inf["summary"]["count_upper"]
    # threshold = 0.0 and no mean at zero: g1 = mean exactly where mean > 0, the lower row
    zero = run(stats, w24, threshold=0.0)
    assert (zero["rc"]["mean"] != 0).all()
    assert zero["max_stat"][400:800].tobytes() == zero["max_stat"][:400].tobytes()
    assert zero["max_index"][400:800].tobytes() == zero["max_index"][:400].tobytes()
    assert zero["summary"]["count_consistent"] == zero["summary"]["count_lower"]
    # the lower and the upper row do not depend on the threshold
    for o in (inf, zero):
        assert o["max_stat"][:400].tobytes() == mid["max_stat"][:400].tobytes()
        assert o["max_stat"][800:].tobytes() == mid["max_stat"][800:].tobytes()


def test_the_three_p_values_differ_near_the_null(w24):
    out = run(sm.near_null_board(0), w24, alpha=0.05)
    lo, co, up = sm.p_values(out, 400)
    assert lo < co < up and (lo, co, up) == (0.085, 0.165, 0.2625)
    assert 0 < out["recentred"].sum() < 40


def test_a_round_that_rejects_nothing_is_the_last(w24):
    out = run(sm.near_null_board(0), w24, alpha=0.05)
    s = out["summary"][0]
    assert s["rounds_run"] == 1 and s["num_rejected"] == 0 and (out["rejected_round"] == -1).all()
    assert np.isfinite(out["crit"][0]) and np.isnan(out["crit"][1:]).all() and not out["round_rejected"].any()
    assert out["crit"][0] == np.sort(out["max_stat"][400:800])[sm.crit_rank(0.05, 400)]
    assert out["t_stat"].max() <= out["crit"][0]


def test_two_rounds_of_step_down(w12):
    """the crafted board of S = 20, n = 12, R = 300, block 2, alpha = 0.1: the fixed seed rejects in rounds 0 and 1 (the
    GPU test asks the device for the same board), a third round rejects nothing"""
    out = run(sm.two_round_board(TWO_ROUND_SEED), w12)
    s = out["summary"][0]
    assert out["round_rejected"][0] > 0 and out["round_rejected"][1] > 0 and out["round_rejected"][2] == 0
    assert s["rounds_run"] == 3 and s["num_rejected"] == out["round_rejected"].sum() == (out["rejected_round"] >= 0).sum()
    assert out["crit"][1] < out["crit"][0] and out["crit"][2] <= out["crit"][1] and np.isnan(out["crit"][3:]).all()
    late = np.flatnonzero(out["rejected_round"] == 1)
    assert (out["t_stat"][late] <= out["crit"][0]).all() and (out["t_stat"][late] > out["crit"][1]).all()
    assert set(np.flatnonzero(out["rejected_round"] >= 0)) <= set(range(9, 16))      # winners only
    # cut short: round max_rounds - 1 is the last whatever it rejects
    for rounds in (1, 2):
        cut = run(sm.two_round_board(TWO_ROUND_SEED), w12, max_rounds=rounds)
        assert cut["summary"][0]["rounds_run"] == rounds and len(cut["crit"]) == rounds
        assert cut["crit"].tobytes() == out["crit"][:rounds].tobytes()
        assert (cut["rejected_round"] == np.where(out["rejected_round"] < rounds, out["rejected_round"], -1)).all()
    seeds = [k for k in range(12) if (run(sm.two_round_board(k), w12)["round_rejected"][:2] > 0).all()]
    assert seeds == [1, 4, 5, 9]


def test_noisy_losers_blind_the_reality_check_not_the_studentised_test(w12):
    out = run(sm.two_round_board(TWO_ROUND_SEED), w12)
    p_rc = bm.p_values(out["rc"], 300)[0]
    assert p_rc >= 0.5 and sm.p_values(out, 300) == (0.0, 0.0, 0.0)
    assert out["summary"][0]["best"] in range(9, 16) and out["summary"][0]["statistic"] > 3
    adjusted = out["count_adj"] / 300
    assert (adjusted[out["rejected_round"] == 0] <= 0.1).all()         # round 0 is the single-step test


def test_nothing_studentised_and_everything_rejected(w12):
    # constant rows of few mantissa bits: every resampled mean is the mean exactly, se = 0
    flat = bm.records(np.repeat(np.arange(-10, 10)[:, None] / 1024.0, 12, axis=1))
    out = run(flat, w12)
    s = out["summary"][0]
    assert s["best"] == -1 and s["studentised"] == 0 and s["rounds_run"] == 0 and s["statistic"] == 0.0
    assert all(np.isnan(p) for p in sm.p_values(out, 300)) and np.isnan(out["t_stat"]).all() and np.isnan(out["crit"]).all()
    assert not out["max_stat"].any() and (out["max_index"] == -1).all() and not out["count_adj"].any()
    assert (out["std_error"] == 0).all()
    rng = np.random.default_rng(5)
    winners = bm.records(rng.normal(5e-3, 1e-3, (9, 12)))
    out = run(winners, w12)
    s = out["summary"][0]
    assert s["num_rejected"] == s["studentised"] == 9 and (out["rejected_round"] >= 0).all()
    assert s["rounds_run"] == int(out["rejected_round"].max()) + 1           # the round that empties the set is the last


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gte.h"
#define F(t, f) printf(#t " " #f " %zu %zu\n", offsetof(t, f), sizeof(((t*)0)->f));
int main(void) {
  printf("consts %d %zu %zu\n", GTE_SPA_MAX_ROUNDS, sizeof(gte_spa_summary), sizeof(gte_spa_out));
  F(gte_spa_summary, statistic) F(gte_spa_summary, best) F(gte_spa_summary, count_lower)
  F(gte_spa_summary, count_consistent) F(gte_spa_summary, count_upper) F(gte_spa_summary, rounds_run)
  F(gte_spa_summary, num_rejected) F(gte_spa_summary, studentised) F(gte_spa_summary, reserved)
  F(gte_spa_out, t_stat) F(gte_spa_out, std_error) F(gte_spa_out, recentred) F(gte_spa_out, count_adj)
  F(gte_spa_out, rejected_round) F(gte_spa_out, max_stat) F(gte_spa_out, max_index) F(gte_spa_out, crit)
  F(gte_spa_out, round_rejected) F(gte_spa_out, summary)
  return 0;
}
"""


def test_constants_and_struct_layouts_match_the_c_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).split("\n")
    assert lines[0].split()[1:] == ["64", "40", "80"] and _abi.GTE_SPA_MAX_ROUNDS == sm.MAX_ROUNDS == 64
    assert C.sizeof(_abi.GteSpaSummary) == sm.SUMMARY.itemsize == 40 and np.dtype(_abi.SPA_SUMMARY_DTYPE) == sm.SUMMARY
    assert C.sizeof(_abi.GteSpaOut) == 80
    for struct, ct in (("gte_spa_summary", _abi.GteSpaSummary), ("gte_spa_out", _abi.GteSpaOut)):
        c_fields = [(n, int(o), int(s)) for t, n, o, s in (ln.split() for ln in lines[1:] if ln) if t == struct]
        assert c_fields == [(n, getattr(ct, n).offset, getattr(ct, n).size) for n, _ in ct._fields_]
    assert _abi.SYMBOLS["gte_spa_test"][0] is C.c_int and len(_abi.SYMBOLS["gte_spa_test"][1]) == 13


def test_pass_kernel_keeps_its_registers():
    """csrc/gte_spa.hip for gfx950: no kernel of the unit uses scratch memory, and the four instantiations of the pass
    kernel (round 0 and later rounds, n a power of two or not) keep the 5 waves per SIMD their 32 KB of LDS allow"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-fno-fast-math", "-c", os.path.join(csrc, "gte_spa.hip"), "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    get = lambda block, key: int(re.search(key + r":\s*(\d+)", block).group(1))
    kernels = {b.split()[0]: b for b in r.stderr.split("Function Name:")[1:]}
    assert len(kernels) == 11, sorted(kernels)
    for name, block in kernels.items():
        assert get(block, r"ScratchSize \[bytes/lane\]") == 0, name
    passes = [b for name, b in kernels.items() if "gte_spa_pass_kernel" in name]
    assert len(passes) == 4
    for block in passes:
        assert get(block, r"Occupancy \[waves/SIMD\]") >= 5 and get(block, r"LDS Size \[bytes/block\]") == 32768


def test_python_arguments_are_checked_before_any_call():
    """`spa.arguments`: crit_rank from alpha and R, the default threshold and what is refused, without an env"""
    from gym_trading_env_amd import spa
    assert spa.arguments(12, 300, 0.1, 8, None) == (sm.default_threshold(12), 269, 8)
    assert spa.arguments(3, 1000, 0.05, 1, 0.0) == (0.0, 949, 1)
    assert spa.arguments(2, 10, 0.05, 64, float("inf")) == (float("inf"), 9, 64)
    with pytest.raises(ValueError, match="at least three"):
        spa.arguments(2, 10, 0.05, 8, None)
    for bad in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(max_rounds=0), dict(max_rounds=65),
                dict(threshold=-1.0), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            spa.arguments(**{**dict(n=12, R=300, alpha=0.1, max_rounds=8, threshold=None), **bad})
    with pytest.raises(TypeError):
        spa.arguments(12, 300, 0.1, 2.5, None)
