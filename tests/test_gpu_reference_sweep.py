"""Every sweep trace (tests/golden/sweep_NN.npz: the configurations the kernels branch on), every
numeric trace (numeric_NN.npz: the values the arithmetic and the copy loops run on) and every slide
trace (slide_NN.npz: their hardest semantics at shapes with lean, slidable windows), all generated
by the reference itself (strata in tests/strata.py), through the HIP library on every step and
rollout path, held to what the code claims: indices and flags exact, static observation columns
bit for bit (NaN payloads, -0.0 and subnormals included), the fp64 portfolio state, the valuation
and the dynamic observation columns equal by value (replay.same_value: the bit pattern, any NaN for
any NaN), reward64 within replay.reward_ulp_bound ulp of the reference (1 for the log return
itself; NaN, inf and the sign of a zero as the reference's), the f32 reward equal to float32 of the
kernel's own reward64.  Needs an MI355X.

  (a) the default step, untiled
  (b) the envs tiled x67 at envs-per-wave geometries with full waves (the lean copy loop's shape
      where the trace allows it)
  (c) every kernel_variant bit that selects a kernel structure, crossed with the store policies
  (d) gte_rollout: window-resident, gather-per-step, state-only and per-step, in chunks of random
      length cut at the calls that add limit orders; the path each call took (reported by the
      library under GTE_DEBUG_GEOMETRY) is asserted
"""
import glob
import os
import re

import numpy as np
import pytest

import backtest_trace
import replay
import strata
from gym_trading_env_amd import _abi
from test_gpu_parity import GpuAdapter

pytestmark = pytest.mark.gpu

SWEEP = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(replay.GOLDEN_DIR, "sweep_*.npz")))
NUMERIC = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(replay.GOLDEN_DIR, "numeric_*.npz")))
# (the slide family: multi-dataset, limit-order, crash and zero-close traces at lean shapes; its sliding
# replays are in tests/test_gpu_sliding_reference.py)
SLIDE = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(replay.GOLDEN_DIR, "slide_*.npz")))
TRACES = SWEEP + NUMERIC + SLIDE
WORST_ULPS = {}


def _cut(g, K):
    """The first K calls of trace g."""
    K0 = g["op"].shape[0]
    for k in list(g):
        if isinstance(g[k], np.ndarray) and g[k].ndim >= 2 and g[k].shape[0] == K0:
            g[k] = g[k][:K]
    return g


def _replay_exact(a, g, tile=1, tag=""):
    stats = {}
    worst = replay.replay(a, g, tile=tile, reward_ulps=replay.reward_ulp_bound(g), stats=stats)
    assert worst == 0.0
    WORST_ULPS[tag] = stats["reward_ulps"]
    print(f"[sweep] {tag}: worst reward64 distance {stats['reward_ulps']:.0f} ulp")


def _lean_epws(f):
    """envs per wave (<= 16, cooperative phase A) at which whole waves take the lean copy loop
    (gte_step.h: n_env * W <= 512 rows, whole passes of 4 wave instructions)."""
    if not strata._lean(f, f["nd"]) or f["nd"] == 0:
        return []
    vpe = f["W"] * f["Fobs"] // 4
    return [e for e in range(1, 17) if e * f["W"] <= 512 and (e * vpe) % 256 == 0]


@pytest.mark.parametrize("name", TRACES)
def test_step_untiled(name):
    g = replay.load(name)
    a = GpuAdapter(g)
    _replay_exact(a, g, tag=f"{name} step")
    a.env.close()


def _tiled_cases():
    out = []
    for name in TRACES:
        f = strata.facts(replay.load(name))
        lean = _lean_epws(f)
        for epw in (lean[:2] if lean else [3, 16]):
            out.append((name, epw))
    return out


@pytest.mark.parametrize("name,epw", _tiled_cases())
def test_step_tiled(name, epw):
    g = _cut(replay.load(name), 160)
    f = strata.facts(g)
    a = GpuAdapter(g, tile=67, envs_per_wave=epw)
    info = a.env.launch_info()
    if _lean_epws(f):
        assert info["envs_per_wave"] == epw
        # the shape the lean loop is written for: 16-byte vectors, cooperative phase A, the raw
        # rings staged in LDS, and 67 x E envs fill whole waves of `epw`
        assert (info["vector_bytes"], info["phase_a"], info["dyn_columns"]) == (16, "cooperative",
                                                                                  "lds-raw-rings")
        assert 67 * f["E"] >= epw
    _replay_exact(a, g, tile=67, tag=f"{name} tiled epw={epw}")
    a.env.close()


# (numeric_04: special f32 words in the lean shape; numeric_00: leveraged crashes, negative valuations)
VARIANT_TRACES = ["sweep_03", "sweep_06", "sweep_12", "sweep_23", "sweep_26", "numeric_04", "numeric_00"]
VARIANTS = [_abi.KV_PER_WAVE_PHASE_A, _abi.KV_NO_LDS_STAGING, _abi.KV_SHARED_TU, _abi.KV_GENERIC_COPY,
            _abi.KV_RECORD_DIRECT]


def _variant_cases():
    # each (variant, store) on the nd=4 lean trace, the wide 4-byte one, the nd=4 4-byte one, a
    # multi-dataset one, the two numeric ones, and one more that rotates over the rest of the sweep
    out = []
    rest = [n for n in SWEEP if n not in VARIANT_TRACES]
    i = 0
    for v in VARIANTS:
        for store in (0, 1, 2):
            for name in VARIANT_TRACES + [rest[i % len(rest)]]:
                out.append((name, v, store))
            i += 1
    return out


@pytest.mark.parametrize("name,variant,store", _variant_cases())
def test_step_kernel_variants(name, variant, store):
    g = _cut(replay.load(name), 120)
    a = GpuAdapter(g, tile=5, kernel_variant=variant, nontemporal_obs=store)
    _replay_exact(a, g, tile=5, tag=f"{name} variant={variant} store={store}")
    a.env.close()


TILE_R = 16
PATH_LINE = re.compile(r"\[gte\] rollout path: ([a-z-]+), (\d+) steps")


def _chunks(g, rng):
    """[start, stop) call ranges covering calls 1..K-1: random lengths up to 39, and a new chunk at every
    call that adds limit orders (backtest_trace.chunks, which the backtest replays share)."""
    return backtest_trace.chunks(g, rng, 39)


@pytest.mark.parametrize("mode", sorted(strata.ROLLOUT_MODES))
@pytest.mark.parametrize("name", TRACES)
def test_rollout(name, mode, monkeypatch, capfd):
    import torch
    from gym_trading_env_amd.batched import BatchedTradingEnv
    g = replay.load(name)
    f = strata.facts(g)
    kv, keep = strata.ROLLOUT_MODES[mode]
    # every gte_rollout call names the path it took (gte_api.hip, report_rollout_path)
    monkeypatch.setenv("GTE_DEBUG_GEOMETRY", "1")
    kw = replay.config_kwargs(g, TILE_R, kernel_variant=kv, envs_per_wave=4)
    N = kw.pop("n_envs")
    kw.pop("n_static"); kw.pop("n_datasets")
    env = BatchedTradingEnv(list(g["datasets"]) if f["D"] > 1 else g["datasets"][0], num_envs=N,
                            output="torch", **kw)
    info = env.launch_info()
    shape_fused = (info["vector_bytes"], info["phase_a"], info["dyn_columns"]) == (16, "cooperative",
                                                                                   "lds-raw-rings")
    assert shape_fused == strata.hot_shape(f), info
    taken = set()
    t = lambda a: np.tile(a, TILE_R)
    tt = lambda a: np.tile(a, (TILE_R,) + (1,) * (a.ndim - 1))
    q, n = replay.injection_queue(g, TILE_R)
    if n:
        env.set_autoreset_injection(q["idx"], q["pos_index"], q["dataset"])
    env.reset(inject_idx=t(g["idx"][0]), inject_position_index=t(g["pos_index"][0]),
              inject_dataset=t(g["dataset"][0]))
    capfd.readouterr()
    bound = replay.reward_ulp_bound(g)
    rng = np.random.default_rng(int(name[-2:]))
    worst = 0.0
    for start, stop in _chunks(g, rng):
        if "lo_pos" in g and (g["lo_pos"][start] >= 0).any():
            env.add_limit_order(t(g["lo_pos"][start]), t(g["lo_limit"][start]), np.ones(N, np.uint8))
        acts = torch.from_numpy(np.ascontiguousarray(np.tile(g["action"][start:stop], (1, TILE_R)))).cuda()
        out = env.rollout(acts, keep_obs=keep, valuation=True, reward64=True)
        torch.cuda.synchronize()
        paths = PATH_LINE.findall(capfd.readouterr().err)
        expect = strata.rollout_path(f, mode, stop - start)
        assert paths == [(expect, str(stop - start))], (name, mode, start, stop, paths)
        taken.add(expect)
        r64 = out["reward64"].cpu().numpy()
        r32 = out["reward"].cpu().numpy()
        term = out["terminated"].cpu().numpy()
        trunc = out["truncated"].cpu().numpy()
        val = out["valuation"].cpu().numpy()
        for j, k in enumerate(range(start, stop)):
            tag = f"{name} {mode} call {k}"
            worst = max(worst, replay.assert_reward64(r64[j], t(g["reward"][k]), bound, tag))
            replay.assert_same_value(r32[j], replay.to_float32(r64[j]), tag + " f32 reward")
            np.testing.assert_array_equal(term[j], t(g["done"][k]).astype(bool), err_msg=tag)
            np.testing.assert_array_equal(trunc[j], t(g["truncated"][k]).astype(bool), err_msg=tag)
            replay.assert_same_value(val[j], t(g["portfolio_valuation"][k]), tag + " valuation")
            if keep:
                replay.assert_obs(out["obs"][j].cpu().numpy(), tt(g["obs"][k]), f["Fs"], tag + " obs")
        if not keep:
            replay.assert_obs(out["obs"].cpu().numpy(), tt(g["obs"][stop - 1]), f["Fs"],
                              f"{name} {mode} call {stop - 1} obs")
        for gk, sk in replay.STATE_I32.items():
            np.testing.assert_array_equal(env.state(sk), t(g[gk][stop - 1]),
                                          err_msg=f"{name} {mode} after call {stop - 1}: {sk}")
        for gk, sk in replay.STATE_F64.items():
            replay.assert_same_value(env.state(sk), t(g[gk][stop - 1]), f"{name} {mode} after call {stop - 1}: {sk}")
    WORST_ULPS[f"{name} rollout {mode}"] = worst
    print(f"[sweep] {name} rollout {mode}: path taken {', '.join(sorted(taken))}, "
          f"worst reward64 distance {worst:.0f} ulp")
    env.close()


@pytest.mark.parametrize("max_dur", ["max", 2, 3, 40])
def test_reset_draws_land_in_reference_ranges(max_dur):
    """One reset of 65 536 envs: the start rows are randint(W-1, T - max_dur - (W-1))
    (environments.py:173-177) — every row of that range occurs and none outside it —, every
    position index occurs under initial_position='random' (:167), and the dataset picks follow
    next_dataset's least-used rule (:380-388): each env's first D picks are a permutation of
    range(D).  (The device's low + bounded(r, high - low) mapping is restated by the oracle, so
    parity alone cannot catch a range error in it.)"""
    from gym_trading_env_amd.batched import BatchedTradingEnv
    N, W, D = 65536, 7, 3
    rng = np.random.default_rng(4)
    # 'max': every start is W-1; durations 2 and 3 leave start ranges 2 and 1 rows wide; 40: three
    # datasets with ranges of 248, 288 and 328 rows (~70 envs per row)
    Ts = {"max": [50], 2: [2 * (W - 1) + 2 + 2], 3: [2 * (W - 1) + 3 + 1], 40: [300, 340, 380]}[max_dur]
    sets = [(rng.normal(0, 1, (T, 2)).astype(np.float32), 100 * np.exp(np.cumsum(rng.normal(0, 1e-2, T))))
            for T in Ts]
    positions = [-1.5 + 0.25 * i for i in range(32)]
    env = BatchedTradingEnv(sets if len(sets) > 1 else sets[0], num_envs=N, positions=positions, windows=W,
                            max_episode_duration=max_dur, episodes_between_dataset_switch=2, seed=77,
                            output="numpy")
    env.reset()
    idx, ds, pos = env.state("idx"), env.state("dataset_index"), env.state("position_index")
    np.testing.assert_array_equal(np.unique(pos), np.arange(len(positions)))
    for d, T in enumerate(Ts):
        got = np.unique(idx[ds == d])
        if max_dur == "max":
            want = np.array([W - 1])
        else:
            want = np.arange(W - 1, T - max_dur - (W - 1))
        np.testing.assert_array_equal(got, want, err_msg=f"dataset {d} (T={T})")
    if len(sets) > 1:
        # switch every 2 episodes: the constructor's pick serves episodes 0 and the reset of
        # episode 1 makes the second pick, episode 3 the third -> episodes 0, 1, 3 are picks 0-2
        picks = [ds]
        for ep in range(1, 2 * D - 2):
            env.reset()
            if ep % 2 == 1:
                picks.append(env.state("dataset_index"))
        picks = np.sort(np.stack(picks), axis=0)
        np.testing.assert_array_equal(picks, np.tile(np.arange(D)[:, None], (1, N)))
    env.close()
