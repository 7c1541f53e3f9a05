"""The bootstrap reality check's model (tests/bootstrap_model.py, restating include/gte.h): the laws of its
resampling weights, hand-worked answers of the resample pass and the close, the constants and the struct layouts
against the C header, what the check is FOR (a leaderboard of pure noise is not significant, a real edge is), and
the register budget of the new translation unit.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bootstrap_model as bm
import draw_laws
from gym_trading_env_amd import _abi
from gym_trading_env_amd._abi import GTE_BOOT_MAX_RESAMPLES, GTE_BOOT_SLAB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (0xB007 << 32) | 12345   # the high word set


# ---- the weights ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,R,block", [(2, 300, 1.0), (3, 257, 1.5), (64, 256, 4.0), (127, 100, 2.5), (128, 64, 1e9)])
def test_every_weight_row_sums_to_n(n, R, block):
    w = bm.weights(n, R, block, SEED)
    assert w.shape == (R, n) and (w >= 0).all() and (w == np.floor(w)).all()
    assert (w.sum(axis=1) == n).all()


def test_threshold():
    assert bm.threshold(1.0) == 4294967295 and bm.threshold(2.0) == 2 ** 31 and bm.threshold(1.5) == 2863311530
    assert bm.threshold(4.0) == 2 ** 30 and bm.threshold(1e9) == 4 and bm.threshold(1e300) == 0


def test_block_one_draws_every_position_uniformly():
    """block = 1: every draw starts a new block at mulhi(o[1], n), so the 4096 * 64 positions are independent
    uniform draws on [0, 64): a chi-square goodness-of-fit p-value (63 degrees of freedom, 4096 expected per cell),
    which is a fixed number for the fixed seed and must not fall below draw_laws.ALPHA = 1e-6; likewise the
    position as a function of the draw's place j must stay uniform (no place favours a position)."""
    n, R = 64, 4096
    assert bm.restarts(n, R, 1.0, SEED).all()
    pos = bm.positions(n, R, 1.0, SEED)
    p = draw_laws.uniform_p(pos, n)
    p_first, p_last = draw_laws.uniform_p(pos[:, 0], n), draw_laws.uniform_p(pos[:, -1], n)
    print(f"[bootstrap-laws] block=1: p(all)={p:.4f} p(j=0)={p_first:.4f} p(j=n-1)={p_last:.4f}")
    assert min(p, p_first, p_last) >= draw_laws.ALPHA
    w = bm.weights(n, R, 1.0, SEED)
    assert np.array_equal(w.sum(axis=0), np.bincount(pos.ravel(), minlength=n))


def test_block_four_restarts_at_the_stated_rate():
    """block = 4, R * n = 4096 * 64 draws: draw 0 of a resample always restarts; each of the other 4096 * 63 restarts
    with probability q = thr / 2^32 independently, so their number is Binomial(N, q): within five standard deviations
    sqrt(N q (1 - q)) of N q.  A run that continues takes the next position on the circle."""
    n, R = 64, 4096
    new = bm.restarts(n, R, 4.0, SEED)
    assert new[:, 0].all()
    N, q = R * (n - 1), bm.threshold(4.0) / 2.0 ** 32
    assert q == 0.25
    k, sd = int(new[:, 1:].sum()), (N * q * (1 - q)) ** 0.5
    print(f"[bootstrap-laws] block=4: {k} restarts of {N}, expected {N * q:.0f} +- {sd:.1f}")
    assert abs(k - N * q) <= 5 * sd
    pos = bm.positions(n, R, 4.0, SEED)
    cont = ~new[:, 1:]
    assert ((pos[:, 1:] - pos[:, :-1]) % n == 1)[cont].all()
    assert draw_laws.uniform_p(pos[:, 1:][new[:, 1:]], n) >= draw_laws.ALPHA


def test_a_huge_block_gives_one_run_per_row():
    """block = 1e9: thr = 4, no draw after the first restarts, every row walks once round the circle from its start:
    a rotation of all ones."""
    n, R = 64, 4096
    new = bm.restarts(n, R, 1e9, SEED)
    assert new[:, 0].all() and not new[:, 1:].any()
    pos = bm.positions(n, R, 1e9, SEED)
    assert ((pos - pos[:, :1]) % n == np.arange(n)).all()
    assert (bm.weights(n, R, 1e9, SEED) == 1.0).all()
    assert draw_laws.uniform_p(pos[:, 0], n) >= draw_laws.ALPHA


# ---- the resample pass and the close, by hand ------------------------------------------------------------------

def test_hand_worked_pass():
    x = np.array([[1.0, 3.0, 100.0], [2.0, 2.0, np.nan], [0.0, 8.0, 5.0], [4.0, np.inf, 1.0], [2.0, 2.0, 7.0]])
    steps = np.ones((5, 3), np.int64)
    steps[2, 0] = 0                                     # strategy 2 never stepped in period 0
    mask = np.array([True, True, False])                # period 2 is not selected: its NaN does not matter
    w = np.array([[2.0, 0.0], [0.0, 2.0], [1.0, 1.0], [0.5, 1.5]])
    o = bm.reality_check(bm.records(x, steps), mask, None, w)
    assert o["eligible"].tolist() == [True, True, False, False, True]
    assert bm.same_f64(o["mean"], [2.0, 2.0, np.nan, np.nan, 2.0])
    # c of strategy 0: (2*1)/2 - 2 = -1, (2*3)/2 - 2 = 1, 0, (0.5 + 4.5)/2 - 2 = 0.5; strategies 1 and 4: 0 everywhere
    assert bm.same_f64(o["max_stat"], [0.0, 1.0, 0.0, 0.5]) and o["max_index"].tolist() == [1, 0, 0, 0]
    assert bm.same_f64(o["boot_sum"], [0.5, 0.0, np.nan, np.nan, 0.0])
    assert bm.same_f64(o["boot_sq_sum"], [2.25, 0.0, np.nan, np.nan, 0.0])
    assert o["count_ge"].tolist() == [0, 0, 0, 0, 0]
    assert o["count_adj"].tolist() == [0, 0, 0, 0, 0]
    s = o["summary"][0]
    assert (s["best"], s["best_mean"], s["count_rc"], s["eligible"]) == (0, 2.0, 0, 3)
    # with a benchmark that takes the means to zero the centred statistics reach them
    o = bm.reality_check(bm.records(x, steps), mask, np.array([1.0, 3.0, np.nan]), w)
    assert bm.same_f64(o["mean"], [0.0, 0.0, np.nan, np.nan, 0.0])
    assert o["count_ge"].tolist() == [4, 2, 0, 0, 2] and o["count_adj"].tolist() == [4, 4, 0, 0, 4]
    assert bm.p_values(o, 4)[0] == 1.0
    # nobody eligible
    steps[:] = 0
    o = bm.reality_check(bm.records(x, steps), mask, None, w)
    assert (o["max_index"] == -1).all() and (o["max_stat"] == -np.inf).all() and o["summary"][0]["best"] == -1
    assert np.isnan(o["summary"][0]["best_mean"]) and o["summary"][0]["eligible"] == 0


def test_slabs_fix_the_order_of_the_moment_sums():
    """R = 600: three slabs (256, 256, 88), each summed from zero over r ascending, then added in slab order"""
    assert bm.SLAB == GTE_BOOT_SLAB == 256 and bm.MAX_RESAMPLES == GTE_BOOT_MAX_RESAMPLES
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1, (7, 5)) * 10.0 ** rng.integers(-8, 8, (7, 5))
    w = bm.weights(5, 600, 2.0, 9)
    o = bm.reality_check(bm.records(x), np.ones(5, bool), None, w)
    d, mean = x, None
    t = np.zeros(7)
    for i in range(5):
        t = t + d[:, i]
    mean = t / 5.0
    c = np.empty((600, 7))
    for r in range(600):
        a = np.zeros(7)
        for i in range(5):
            a = a + w[r, i] * d[:, i]
        c[r] = a / 5.0 - mean
    want = np.zeros(7)
    for lo in range(0, 600, GTE_BOOT_SLAB):
        q = np.zeros(7)
        for r in range(lo, min(lo + GTE_BOOT_SLAB, 600)):
            q = q + c[r]
        want = want + q
    assert bm.same_f64(o["boot_sum"], want)
    straight = np.zeros(7)
    for r in range(600):
        straight = straight + c[r]
    assert not bm.same_f64(want, straight)   # (the slab order is a different rounding from the straight one)
    assert bm.same_f64(o["max_stat"], c.max(axis=1))


# ---- layout ---------------------------------------------------------------------------------------------------

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gte.h"
#define F(t, f) printf(#t " " #f " %zu %zu\n", offsetof(t, f), sizeof(((t*)0)->f));
int main(void) {
  printf("consts %d %d %d %d %zu %zu\n", GTE_BOOT_SLAB, GTE_BOOT_MAX_RESAMPLES, GTE_MAX_PERIODS, GTE_ABI_VERSION,
         sizeof(gte_reality_check_summary), sizeof(gte_reality_check_out));
  F(gte_reality_check_summary, best_mean) F(gte_reality_check_summary, best) F(gte_reality_check_summary, count_rc)
  F(gte_reality_check_summary, eligible) F(gte_reality_check_summary, reserved)
  F(gte_reality_check_out, mean) F(gte_reality_check_out, boot_sum) F(gte_reality_check_out, boot_sq_sum)
  F(gte_reality_check_out, count_ge) F(gte_reality_check_out, count_adj) F(gte_reality_check_out, max_stat)
  F(gte_reality_check_out, max_index) F(gte_reality_check_out, summary)
  return 0;
}
"""


def test_constants_and_struct_layouts_match_the_c_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).split("\n")
    assert lines[0].split()[1:] == ["256", "65536", "128", "5", "24", "64"] and _abi.GTE_ABI_VERSION == 5
    assert _abi.GTE_BOOT_SLAB == bm.SLAB == 256 and _abi.GTE_BOOT_MAX_RESAMPLES == bm.MAX_RESAMPLES == 65536
    assert C.sizeof(_abi.GteRealityCheckSummary) == bm.SUMMARY.itemsize == 24
    assert np.dtype(_abi.REALITY_CHECK_SUMMARY_DTYPE) == bm.SUMMARY
    assert C.sizeof(_abi.GteRealityCheckOut) == 64
    for struct, ct in (("gte_reality_check_summary", _abi.GteRealityCheckSummary),
                       ("gte_reality_check_out", _abi.GteRealityCheckOut)):
        c_fields = [(n, int(o), int(s)) for t, n, o, s in (ln.split() for ln in lines[1:] if ln) if t == struct]
        assert c_fields == [(n, getattr(ct, n).offset, getattr(ct, n).size) for n, _ in ct._fields_]
    assert [(n, bm.SUMMARY.fields[n][1]) for n in bm.SUMMARY.names] == \
        [(n, getattr(_abi.GteRealityCheckSummary, n).offset) for n, _ in _abi.GteRealityCheckSummary._fields_]
    for name in ("gte_bootstrap_weights", "gte_reality_check"):
        assert _abi.SYMBOLS[name][0] is C.c_int
    assert len(_abi.SYMBOLS["gte_bootstrap_weights"][1]) == 6 and len(_abi.SYMBOLS["gte_reality_check"][1]) == 9


# ---- what it is for --------------------------------------------------------------------------------------------

def test_noise_is_not_significant_and_an_edge_is():
    """512 strategies x 48 periods of seeded Gaussian noise: the best of 512 naive p-values is far below 0.05 — the
    leaderboard's winner looks significant on its own — while the Reality Check p-value, which knows that 512 were
    tried, is not.  With one strategy's mean shifted by one standard deviation per period, its adjusted p-value is
    at most 0.01.  Seed 1 (data and weights) satisfies both; fixed here."""
    S, n, R, seed = 512, 48, 1000, 1
    x = np.random.default_rng(seed).normal(0, 1, (S, n))
    w = bm.weights(n, R, 1.0, seed)
    every = np.ones(n, bool)
    rc, naive, _ = bm.p_values(bm.reality_check(bm.records(x), every, None, w), R)
    print(f"[reality-check] noise: best naive p {naive.min():.3f}, Reality Check p {rc:.3f}")
    assert naive.min() < 0.05 < rc
    x[137] += 1.0
    o = bm.reality_check(bm.records(x), every, None, w)
    rc, naive, adjusted = bm.p_values(o, R)
    print(f"[reality-check] edge: adjusted p of the shifted strategy {adjusted[137]:.3f}, Reality Check p {rc:.3f}")
    assert o["summary"][0]["best"] == 137 and adjusted[137] <= 0.01 and rc <= 0.01
    assert (np.delete(adjusted, 137) > 0.05).all()     # nobody else rides along


# ---- build -----------------------------------------------------------------------------------------------------

def test_bootstrap_kernel_register_budget():
    """gte_bootstrap.hip: no kernel uses scratch memory; the resample kernel keeps 16 accumulators per lane and
    still runs at least four waves per SIMD."""
    import test_host_cpu
    kernels = test_host_cpu._resource_usage("gte_bootstrap.hip")
    assert len(kernels) >= 7
    for k in kernels:
        assert k["scratch"] == 0, k
        assert k["occupancy"] >= 4, k
    assert sum("gte_boot_resample_kernel" in k["name"] for k in kernels) == 2
