"""The strata tables of the reference-generated fixture families: STRATA for the configuration
sweep (tests/golden/sweep_NN.npz), NUMERIC_STRATA further down for the numeric family
(numeric_NN.npz), SLIDE_STRATA at the end for the family at shapes whose window slides (slide_NN.npz).

Every row names one corner of the configuration space the HIP kernels branch on and a
predicate over a loaded trace (replay.load) that says whether the trace covers it.  The
predicates read only the trace's configuration, its data shapes and its recorded flags, so
tests/test_sweep_strata.py can assert that the committed fixtures still cover every row, and
make_golden.py can assert it before it writes them.
"""
from __future__ import annotations

import numpy as np

from gym_trading_env_amd import _abi

DEFAULT_DYN = ["last_position_taken", "real_position"]


def facts(g):
    """Derived shape / configuration facts of a loaded trace."""
    cfg = g["cfg"]
    kinds = cfg.get("dynamic_feature_functions", DEFAULT_DYN)
    nd = len(kinds)
    Fs = g["datasets"][0][0].shape[1]
    W = cfg["windows"]
    rf = cfg.get("reward_function", "basic_reward_function")
    reward = "basic" if isinstance(rf, str) else rf[0].split("_")[0]
    Ts = [len(ds[1]) for ds in g["datasets"]]
    op = g["op"]
    K, E = op.shape
    positions = cfg["positions"]
    dur = cfg["max_episode_duration"]
    ends = (g["done"] | g["truncated"]).astype(bool)
    last_row = np.array([[Ts[d] - 1 for d in row] for row in g["dataset"]])
    return dict(cfg=cfg, kinds=kinds, nd=nd, Fs=Fs, Fobs=Fs + nd, W=W, Wn=W or 1, reward=reward,
                Ts=Ts, D=len(Ts), K=K, E=E, positions=positions, dur=dur,
                autoreset=bool((op[1:] == 0).any()), persist=bool(cfg.get("dyn_persist", False)),
                switch=cfg.get("episodes_between_dataset_switch", 1),
                limit="lo_pos" in g, high_low=len(g["datasets"][0]) == 4,
                episodes=(op == 0).sum(axis=0), ends=ends,
                trunc_end=bool((g["truncated"].astype(bool) & (g["idx"] == last_row)).any()),
                trunc_dur=bool((g["truncated"].astype(bool) & (g["idx"] < last_row)).any()))


def _lean(f, nd):
    # the lean copy loop (gte_step.h): 16-byte vectors, raw rings staged in LDS (not
    # dyn_persist), a window of at least one wave instruction (256 floats)
    return (f["nd"] == nd and f["Fobs"] % 4 == 0 and f["W"] is not None and f["W"] * f["Fobs"] >= 256
            and not f["persist"])


def _tight(f):
    # randint(low, T - max_dur - low) (environments.py:173-177) leaves one or two start rows
    if f["dur"] == "max":
        return False
    low = f["Wn"] - 1
    return all(1 <= T - f["dur"] - 2 * low <= 2 for T in f["Ts"])


def _fill_with_market_action(g, f):
    # a step whose market action moved the position and whose final position is not the action's
    # target: a limit order filled after the market trade of the same step (environments.py:234-238)
    if not f["limit"]:
        return False
    op, a, pi = g["op"], g["action"], g["pos_index"]
    prev = pi[:-1]
    step = op[1:] == 1
    moved = (a[1:] >= 0) & (a[1:] != prev)
    return bool((step & moved & (pi[1:] != a[1:])).any())


def _several_orders(g, f):
    # at least two limit orders added to one env inside one episode
    if not f["limit"]:
        return False
    lo, op = g["lo_pos"], g["op"]
    for e in range(f["E"]):
        episode = np.cumsum(op[:, e] == 0)
        have = lo[:, e] >= 0
        if have.any() and np.bincount(episode[have]).max() >= 2:
            return True
    return False


def _steps_after_end(g, f):
    if f["autoreset"]:
        return False
    ended = np.maximum.accumulate(f["ends"], axis=0)
    return bool((ended[:-1] & (g["op"][1:] == 1)).any())


#: gte_rollout's paths by (kernel_variant, keep_obs) of the rollout() call
ROLLOUT_MODES = {"resident": (0, True), "gather": (_abi.KV_ROLLOUT_GATHER, True), "state": (0, False),
                 "per-step": (_abi.KV_ROLLOUT_PER_STEP, True)}


def hot_shape(f):
    """The shape the fused rollout kernels are written for (gte_plan.h, plan_create): 16-byte
    rows and dynamic columns staged raw in LDS (nd > 0, not dyn_persist), given a cooperative
    phase A (envs_per_wave <= 16)."""
    return f["Fobs"] % 4 == 0 and f["nd"] > 0 and not f["persist"]


def rollout_path(f, mode, n_steps=2):
    """The path gte_rollout takes for a trace in one of ROLLOUT_MODES: the window-resident kernel
    needs a window of 2 rows or more; a state-only call of one step is a plain step launch."""
    kv, keep = ROLLOUT_MODES[mode]
    if not hot_shape(f) or kv & _abi.KV_ROLLOUT_PER_STEP:
        return "per-step"
    if not keep:
        return "state-only" if n_steps > 1 else "per-step"
    return "resident" if (f["Wn"] >= 2 and not kv & _abi.KV_ROLLOUT_GATHER) else "gather"


def _fused(f, mode):
    return rollout_path(f, mode) == {"resident": "resident", "gather": "gather", "state": "state-only"}[mode]


STRATA = {
    "lean_nd1": lambda g, f: _lean(f, 1),
    "lean_nd2": lambda g, f: _lean(f, 2),
    "lean_nd3": lambda g, f: _lean(f, 3),
    "lean_nd4": lambda g, f: _lean(f, 4),
    "fobs_mod4_1": lambda g, f: f["Fobs"] % 4 == 1,
    "fobs_mod4_2": lambda g, f: f["Fobs"] % 4 == 2,
    "fobs_mod4_3": lambda g, f: f["Fobs"] % 4 == 3,
    "fobs_4byte_ge61": lambda g, f: f["Fobs"] % 4 != 0 and f["Fobs"] >= 61,
    "nd0": lambda g, f: f["nd"] == 0,
    "nd3_mixed": lambda g, f: f["nd"] == 3 and len(set(f["kinds"])) == 2,
    "nd4_mixed": lambda g, f: f["nd"] == 4 and len(set(f["kinds"])) == 2,
    "real_position_first": lambda g, f: f["nd"] >= 2 and f["kinds"][0] == "real_position",
    "window_none": lambda g, f: f["W"] is None,
    "window_1": lambda g, f: f["W"] == 1,
    "window_2": lambda g, f: f["W"] == 2,
    "window_ge64": lambda g, f: f["W"] is not None and f["W"] >= 64,
    "leverage_above_1": lambda g, f: max(f["positions"]) > 1,
    "leverage_below_m1": lambda g, f: min(f["positions"]) < -1,
    "fractional_positions": lambda g, f: any(p != int(p) for p in f["positions"]),
    "positions_ge16": lambda g, f: len(f["positions"]) >= 16,
    "fees_0": lambda g, f: f["cfg"]["trading_fees"] == 0,
    "fees_1e-2": lambda g, f: f["cfg"]["trading_fees"] == 1e-2,
    "borrow_0": lambda g, f: f["cfg"]["borrow_interest_rate"] == 0,
    "borrow_1e-3": lambda g, f: f["cfg"]["borrow_interest_rate"] == 1e-3,
    "initial_value_1": lambda g, f: f["cfg"]["portfolio_initial_value"] == 1,
    "initial_value_1e6_leverage": lambda g, f: (f["cfg"]["portfolio_initial_value"] == 1e6
                                                and (max(f["positions"]) > 1 or min(f["positions"]) < -1)),
    "fixed_initial_position_autoreset": lambda g, f: (f["cfg"]["initial_position"] != "random"
                                                      and f["autoreset"]),
    "duration_max": lambda g, f: f["dur"] == "max",
    "duration_le10": lambda g, f: f["dur"] != "max" and f["dur"] <= 10,
    "duration_tight_start": lambda g, f: _tight(f),
    "truncated_end_of_data": lambda g, f: f["trunc_end"],
    "truncated_by_duration": lambda g, f: f["trunc_dur"],
    "reward_basic_window": lambda g, f: f["reward"] == "basic" and f["W"] is not None,
    "reward_basic_nowindow": lambda g, f: f["reward"] == "basic" and f["W"] is None,
    "reward_clipped_window": lambda g, f: f["reward"] == "clipped" and f["W"] is not None,
    "reward_clipped_nowindow": lambda g, f: f["reward"] == "clipped" and f["W"] is None,
    "reward_scaled_window": lambda g, f: f["reward"] == "scaled" and f["W"] is not None,
    "reward_scaled_nowindow": lambda g, f: f["reward"] == "scaled" and f["W"] is None,
    "multids_switch1": lambda g, f: f["D"] > 1 and f["switch"] == 1,
    "multids_switch2": lambda g, f: f["D"] > 1 and f["switch"] == 2,
    "multids_switch3": lambda g, f: f["D"] > 1 and f["switch"] == 3,
    "multids_persist": lambda g, f: f["D"] > 1 and f["persist"],
    "multids_no_persist": lambda g, f: f["D"] > 1 and not f["persist"],
    "multids_limit_orders": lambda g, f: f["D"] > 1 and f["limit"] and f["high_low"],
    "limit_several_per_env": lambda g, f: _several_orders(g, f),
    "limit_fill_with_market_action": lambda g, f: _fill_with_market_action(g, f),
    "no_autoreset_steps_after_end": lambda g, f: _steps_after_end(g, f),
    "dyn_persist_single_ds_window": lambda g, f: (f["D"] == 1 and f["persist"] and f["W"] is not None
                                                  and f["W"] > 1),
    "long_trace": lambda g, f: f["K"] >= 600 and int(f["episodes"].min()) >= 10,
}

# every fused rollout kernel replays the reference's hardest rollout semantics directly: drawdown
# terminations, limit-order fills, dataset switches
for _kernel in ("resident", "gather", "state"):
    STRATA[f"{_kernel}_done"] = lambda g, f, k=_kernel: _fused(f, k) and bool(g["done"].any())
    STRATA[f"{_kernel}_limit_orders"] = lambda g, f, k=_kernel: _fused(f, k) and f["limit"]
    STRATA[f"{_kernel}_multids"] = lambda g, f, k=_kernel: _fused(f, k) and f["D"] > 1
STRATA["resident_multids_limit_orders"] = lambda g, f: _fused(f, "resident") and f["D"] > 1 and f["limit"]

#: rows that must hold in at least this many traces (all others: one)
MIN_TRACES = {"drawdown_done": 3}


def rows_of(g):
    """The strata rows trace g covers."""
    f = facts(g)
    rows = [name for name, pred in STRATA.items() if pred(g, f)]
    if g["done"].any():
        rows.append("drawdown_done")
    return rows


def missing(traces):
    """Rows of the table (and MIN_TRACES) that the given loaded traces leave uncovered."""
    count = {name: 0 for name in list(STRATA) + list(MIN_TRACES)}
    for g in traces:
        for r in rows_of(g):
            count[r] += 1
    return {name: n for name, n in count.items() if n < MIN_TRACES.get(name, 1)}


# -- the numeric family (tests/golden/numeric_NN.npz, make_golden.py --numeric) ------------------
# STRATA above sweeps the configurations the kernels branch on; these rows sweep the VALUES the
# arithmetic and the copy loops run on.  Predicates read the fixture's data and recorded values.
DBL_MIN = 2.2250738585072014e-308


def _closes(g):
    return [ds[1] for ds in g["datasets"]]


def _dyn_obs(g, f, kind=None):
    """The recorded dynamic observation columns (of one kind, if given)."""
    cols = [f["Fs"] + i for i, k in enumerate(f["kinds"]) if kind is None or k == kind]
    return g["obs"][..., cols]


def _finite_abs(x):
    x = np.asarray(x, np.float64)
    return np.abs(x[np.isfinite(x)])


def _subnormal_state(g, f):
    v = np.abs(np.stack([g[k] for k in ("asset", "fiat", "interest_asset", "interest_fiat")]))
    return bool(((v > 0) & (v < DBL_MIN)).any())


def _tiny_rewards(g, f):
    r = np.abs(g["reward"])
    return int(((r > 0) & (r <= 1e-13)).sum()) >= 100


def _zero_reward_on_step(g, f):
    # a step inside an episode (not the reset, not `done`), the position held since the call
    # before and not 0, and a reward of exactly 0.0
    pos = np.asarray(f["positions"])[g["pos_index"]]
    held = (g["op"][1:] == 1) & (g["done"][1:] == 0) & (g["pos_index"][1:] == g["pos_index"][:-1])
    return bool((held & (pos[1:] != 0) & (g["reward"][1:] == 0.0) & ~np.signbit(g["reward"][1:])).any())


def _nonfinite(g, f):
    return bool(np.isnan(g["portfolio_valuation"]).any() and np.isnan(g["reward"]).any()
                and f["nd"] > 0 and np.isnan(_dyn_obs(g, f)).any())


def _special_features(g, f):
    import special_words
    return all(special_words.has_every_special_word(ds[0]) for ds in g["datasets"])


def _negative_valuation(g, f):
    return bool((g["portfolio_valuation"] < 0).any())


def _price_le_1e_6(g, f):
    return max(float(c.max()) for c in _closes(g)) <= 1e-6


def _reward_ge_half(g, f):
    return bool((_finite_abs(g["reward"]) >= 0.5).any())


def _extreme_fused(g, f):
    return (hot_shape(f) and f["W"] is not None and f["W"] >= 2
            and (_negative_valuation(g, f) or _price_le_1e_6(g, f) or _reward_ge_half(g, f)))


def _price_scales_apart(g, f):
    if f["D"] < 2:
        return False
    lo = min(float(c.max()) for c in _closes(g))
    hi = max(float(c.min()) for c in _closes(g))
    return lo > 0 and hi / lo >= 1e10


NUMERIC_STRATA = {
    "price_le_1e-6": _price_le_1e_6,
    "price_ge_1e8": lambda g, f: min(float(c.min()) for c in _closes(g)) >= 1e8,
    "value0_le_1e-8": lambda g, f: f["cfg"]["portfolio_initial_value"] <= 1e-8,
    "value0_ge_1e15": lambda g, f: f["cfg"]["portfolio_initial_value"] >= 1e15,
    # the `pv / V0 <= 0.7` division decided on a real quotient
    "value0_not_pow2_done": lambda g, f: (np.frexp(float(f["cfg"]["portfolio_initial_value"]))[0] != 0.5
                                          and bool(g["done"].any())),
    "subnormal_state": _subnormal_state,
    "negative_valuation": _negative_valuation,   # a leveraged crash inside one step
    "reward_abs_ge_0.5": _reward_ge_half,
    "reward_abs_le_1e-13": _tiny_rewards,        # valuation ratios of 1 +- a few ulp
    "reward_exact_zero_on_step": _zero_reward_on_step,
    "real_position_ge_10": lambda g, f: bool((_finite_abs(_dyn_obs(g, f, "real_position")) >= 10).any()),
    "fees_ge_0.1": lambda g, f: f["cfg"]["trading_fees"] >= 0.1,
    "borrow_ge_1e-2": lambda g, f: f["cfg"]["borrow_interest_rate"] >= 1e-2,
    "zero_close_nonfinite": lambda g, f: any((c == 0.0).any() for c in _closes(g)) and _nonfinite(g, f),
    "nonfinite_clipped": lambda g, f: f["reward"] == "clipped" and _nonfinite(g, f),
    "nonfinite_scaled": lambda g, f: f["reward"] == "scaled" and _nonfinite(g, f),
    "special_features_lean": lambda g, f: _special_features(g, f) and _lean(f, f["nd"]) and 1 <= f["nd"] <= 4,
    "special_features_4byte": lambda g, f: _special_features(g, f) and f["Fobs"] % 4 != 0,
    "special_features_nowindow": lambda g, f: _special_features(g, f) and f["W"] is None,
    # the resident, gather and state-only rollout kernels see these numbers
    "extreme_fused_done": lambda g, f: _extreme_fused(g, f) and bool(g["done"].any()),
    "extreme_fused_limit_orders": lambda g, f: _extreme_fused(g, f) and f["limit"],
    "extreme_multids": _price_scales_apart,
}


def numeric_rows_of(g):
    """The NUMERIC_STRATA rows trace g covers."""
    f = facts(g)
    return [name for name, pred in NUMERIC_STRATA.items() if pred(g, f)]


def numeric_missing(traces):
    """Rows of NUMERIC_STRATA that none of the given loaded traces covers."""
    covered = {r for g in traces for r in numeric_rows_of(g)}
    return [name for name in NUMERIC_STRATA if name not in covered]


# -- the slide family (tests/golden/slide_NN.npz, make_golden.py --slide) -------------------------
# The sliding observation buffer (gte.h, gte_bind_sliding_obs) keeps W - 1 rows of every env that
# merely advanced from earlier launches, dynamic columns included.  These rows put what the other
# two families hold (datasets that switch, limit-order fills, drawdown ends, envs that step on after
# their end, NaN valuations, special feature words) on shapes that are granted a slack, and sweep the
# geometry of the slide loop itself (gte_step.h, phase_b_slide).
def auto_slack(W):
    """The automatic slack M of a window of W rows (gte_plan.h, plan_create: 2 W / 5)."""
    return 2 * W // 5


def slides(f):
    """plan_create's grant of a sliding buffer (gte_plan.h), restated: 16-byte rows with dynamic columns staged
    raw in LDS (F_obs % 4 == 0, nd > 0, no dyn_persist), a window of at least one wave instruction
    of 16-byte vectors, and an automatic slack of at least one row.  (The traces have neither
    final_obs nor a log; cooperative phase A holds at up to 16 envs per wave.)"""
    return (f["W"] is not None and f["Fobs"] % 4 == 0 and f["nd"] > 0 and not f["persist"]
            and f["W"] * f["Fobs"] // 4 >= 64 and auto_slack(f["W"]) >= 1)


def slide_counts(g, M):
    """What a replay of trace g exercises with a slack of M rows, from the trace alone: after the
    reset() at call 0 the head at call k is k % (M + 1); a call with a head other than 0 slides, a
    call k > 0 at head 0 is a wrap (full windows).  Counts the slide calls, the wraps, the per-env
    resets (op == 0, k > 0) on slide calls, and the env-steps taken after the env's episode ended
    (no auto-reset: its flags stay raised and it is stepped on, environments.py:233-272) on slide
    calls."""
    op = g["op"]
    K = op.shape[0]
    head = np.arange(K) % (M + 1)
    slide = head != 0
    ends = (g["done"] | g["truncated"]).astype(bool)
    after_end = np.zeros_like(ends)
    if not (op[1:] == 0).any():
        after_end[1:] = np.maximum.accumulate(ends, axis=0)[:-1] & (op[1:] == 1)
    return dict(slide_calls=int(slide.sum()), wraps=int((~slide[1:]).sum()),
                resets_on_slide=int((op[slide] == 0).sum()),
                after_end_on_slide=int(after_end[slide].sum()))


def slacks_tested(f):
    """The obs_slack_rows values the GPU test replays a trace with, as slack rows M."""
    return sorted({1, 3, auto_slack(f["W"])})


def _mixed_real_first(f, nd):
    return f["nd"] == nd and len(set(f["kinds"])) == 2 and f["kinds"][0] == "real_position"


def _nan_survives_the_window(g, f):
    # a NaN real_position in the OLDEST row of a recorded window: written W - 1 calls earlier
    return bool(f["W"] > 1 and np.isnan(_dyn_obs(g, f, "real_position")[:, :, 0]).any())


def _leveraged_crash(g, f):
    return bool(g["done"].any() and _negative_valuation(g, f) and f["nd"] > 0
                and (_finite_abs(_dyn_obs(g, f, "real_position")) >= 10).any()
                and (max(f["positions"]) > 1 or min(f["positions"]) < -1))


SLIDE_STRATA = {
    "multids_switch1": lambda g, f: f["D"] >= 2 and len(set(f["Ts"])) == f["D"] and f["switch"] == 1,
    "multids_switch_ge2": lambda g, f: f["D"] >= 2 and len(set(f["Ts"])) == f["D"] and f["switch"] >= 2,
    "limit_fill_with_market_action": _fill_with_market_action,
    "limit_several_per_env": _several_orders,
    "multids_limit_orders_high_low": lambda g, f: f["D"] >= 2 and f["limit"] and f["high_low"],
    "leveraged_crash_done": _leveraged_crash,
    "no_autoreset_steps_after_end": _steps_after_end,
    "zero_close_nonfinite": lambda g, f: any((c == 0.0).any() for c in _closes(g)) and _nonfinite(g, f),
    "nan_row_survives_the_window": _nan_survives_the_window,
    "special_features": _special_features,
    "fobs4_window_ge64": lambda g, f: f["Fobs"] == 4 and f["W"] >= 64,
    "fobs_ge64_window4": lambda g, f: f["Fobs"] >= 64 and f["W"] == 4,
    "window8_fobs32": lambda g, f: f["W"] == 8 and f["Fobs"] == 32,
    "nd1": lambda g, f: f["nd"] == 1,
    "nd3_mixed_real_position_first": lambda g, f: _mixed_real_first(f, 3),
    "nd4_mixed_real_position_first": lambda g, f: _mixed_real_first(f, 4),
    "duration_le_auto_slack": lambda g, f: f["dur"] != "max" and f["dur"] <= auto_slack(f["W"]),
    "duration_max_truncated_end_of_data": lambda g, f: f["dur"] == "max" and f["trunc_end"],
}

#: rows that must hold in at least this many slide traces (all others: one)
SLIDE_MIN_TRACES = {"drawdown_done": 2}
#: per slack the GPU test uses, every slide trace has this many per-env resets on slide calls (the
#: trace without auto-reset: env-steps after the end instead)
SLIDE_MIN_EVENTS = 3


def slide_rows_of(g):
    """The SLIDE_STRATA rows trace g covers: none unless the trace slides."""
    f = facts(g)
    if not slides(f):
        return []
    rows = [name for name, pred in SLIDE_STRATA.items() if pred(g, f)]
    if g["done"].any():
        rows.append("drawdown_done")
    return rows


def slide_missing(traces):
    """Rows of SLIDE_STRATA (and SLIDE_MIN_TRACES) the given loaded traces leave uncovered."""
    count = {name: 0 for name in list(SLIDE_STRATA) + list(SLIDE_MIN_TRACES)}
    for g in traces:
        for r in slide_rows_of(g):
            count[r] += 1
    return {name: n for name, n in count.items() if n < SLIDE_MIN_TRACES.get(name, 1)}


def slide_vacuous(g):
    """Why a replay of slide trace g would prove too little at one of slacks_tested: a list of
    reasons, empty when at every slack the trace has SLIDE_MIN_EVENTS resets (without auto-reset:
    env-steps after the end) on slide calls and at least one wrap."""
    f = facts(g)
    what = "resets_on_slide" if f["autoreset"] else "after_end_on_slide"
    out = []
    for M in slacks_tested(f):
        c = slide_counts(g, M)
        if c[what] < SLIDE_MIN_EVENTS or c["wraps"] < 1:
            out.append(f"M={M}: {c}")
    return out
