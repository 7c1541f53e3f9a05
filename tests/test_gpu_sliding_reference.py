"""The sliding observation buffer (gte.h, gte_bind_sliding_obs) against the reference's own traces.
Every committed trace whose shape is granted a slack (strata.slides: six of the older fixtures and the
slide family, tests/golden/slide_NN.npz) is replayed through a torch-output env whose window slides,
and held to what the classic replays are held to (tests/test_gpu_reference_sweep.py): indices and
flags exact, static observation columns bit for bit, the fp64 state, the valuation and the dynamic
observation columns equal by value, reward64 within replay.reward_ulp_bound ulp.  An env that merely
advanced keeps W - 1 rows earlier launches wrote, so the traces are ones whose rows differ and whose
resets land on slide calls (tests/test_slide_strata.py).  Needs an MI355X.

  (a) untiled, with a slack of 1, of 3 and the automatic one
  (b) the envs tiled x67: full lean waves, ragged last waves, waves that mix sliding, reset and
      stepped-on-after-the-end envs
  (c) every kernel_variant bit whose kernel slides, crossed with the store policies
  (d) GTE_SLIDE_FULL_WINDOWS: the moving head with full windows
  (e) plain steps interleaved with rollouts that keep and that drop the per-step observations

After every replay the heads the library reported are k % (M + 1), so a run that fell back to the
classic buffer, or to full windows at head 0, fails.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import replay
import strata
from gym_trading_env_amd import _abi
from test_gpu_reference_sweep import _chunks, _cut, _lean_epws

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _facts(name):
    return strata.facts(replay.load(name))


ELIGIBLE = [n for n in replay.golden_names() if strata.slides(_facts(n))]
SLIDE = [n for n in ELIGIBLE if n.startswith("slide_")]
WORST_ULPS = {}
EXERCISED = {}  # parametrisation -> [replays, slide calls, wraps, resets on slide calls]


def _with_row(row, taken=()):
    """The first slide trace (not in `taken`) whose note records strata row `row`."""
    return next(n for n in SLIDE if n not in taken and row in strata.slide_rows_of(replay.load(n)))


class SlidingAdapter:
    """BatchedTradingEnv with torch output and a sliding observation buffer behind the replay
    interface.  The observation is the strided view at the library's head; every 7th call the packed
    read (gte_read_obs) must be the same bits.  The head gte_obs_view reports is recorded per call."""

    def __init__(self, g, tile=1, obs_slack_rows=0, **over):
        from gym_trading_env_amd.batched import BatchedTradingEnv
        kw = replay.config_kwargs(g, tile, obs_slack_rows=obs_slack_rows, **over)
        n_envs = kw.pop("n_envs")
        kw.pop("n_static"); kw.pop("n_datasets")
        self.env = BatchedTradingEnv(list(g["datasets"]) if len(g["datasets"]) > 1 else g["datasets"][0],
                                     num_envs=n_envs, output="torch", **kw)
        W = g["cfg"]["windows"]
        # a shape strata.slides calls eligible is granted a slack, the one asked for
        assert self.env.sliding_obs, "no sliding buffer for a shape strata.slides calls eligible"
        self.M = self._view().slack_rows
        assert self.M == (obs_slack_rows or strata.auto_slack(W))
        assert self.env._t["obs"].stride()[0] == (W + self.M) * self.env.obs_shape[1]
        self.heads = []

    def _view(self):
        v = _abi.GteObsView()
        _abi.check(self.env._lib, self.env._lib.gte_obs_view(self.env._h, C.byref(v)))
        return v

    def _called(self):
        v = self._view()
        assert v.sliding == 1 and self.env.sliding_obs
        self.heads.append(int(v.head))

    def reset(self, mask, idx, pos, ds):
        self.env.reset(mask=mask, inject_idx=idx, inject_position_index=pos, inject_dataset=ds)
        self._called()

    def set_autoreset_injection(self, idx, pos, ds):
        self.env.set_autoreset_injection(idx, pos, ds)

    def step(self, actions):
        self.env.step(np.asarray(actions, np.int32))
        self._called()

    def add_limit_orders(self, pos, limit, persistent):
        self.env.add_limit_order(pos, limit, persistent)

    def obs(self):
        obs = self.env._t["obs"].cpu().numpy()
        if (len(self.heads) - 1) % 7 == 0:
            replay.assert_same_bits(self.env.read_output("obs"), obs, f"call {len(self.heads) - 1}: packed read")
        return obs

    reward64 = lambda s: s.env.read_output("reward64")
    reward32 = lambda s: s.env.read_output("reward")
    terminated = lambda s: s.env.read_output("terminated")
    truncated = lambda s: s.env.read_output("truncated")

    def state(self):
        names = ("idx", "step", "position_index", "dataset_index", "asset", "fiat",
                 "interest_asset", "interest_fiat", "portfolio_valuation", "real_position")
        return {n: self.env.state(n) for n in names}


def _replay_sliding(a, g, tile, tag, group, full_run_of=None):
    """Replay g through SlidingAdapter a exactly, then hold the recorded heads to the trace."""
    stats = {}
    worst = replay.replay(a, g, tile=tile, reward_ulps=replay.reward_ulp_bound(g), stats=stats)
    assert worst == 0.0
    WORST_ULPS[tag] = stats["reward_ulps"]
    K, M = g["op"].shape[0], a.M
    assert a.heads == [k % (M + 1) for k in range(K)], a.heads
    want = strata.slide_counts(g, M)
    sliding = np.array(a.heads) != 0
    got = dict(slide_calls=int(sliding.sum()), wraps=int((~sliding[1:]).sum()),
               resets_on_slide=int((g["op"][sliding] == 0).sum()))
    assert got == {k: want[k] for k in got} and got["wraps"] >= 1 and got["slide_calls"] >= 1
    if full_run_of in SLIDE:  # the whole trace of the slide family: what test_slide_strata.py promised
        f = strata.facts(g)
        events = got["resets_on_slide"] if f["autoreset"] else want["after_end_on_slide"]
        assert events >= strata.SLIDE_MIN_EVENTS
    tot = EXERCISED.setdefault(group, [0, 0, 0, 0])
    for i, v in enumerate((1, got["slide_calls"], got["wraps"], got["resets_on_slide"])):
        tot[i] += v
    print(f"[slide] {tag}: M={M}, {got['slide_calls']} slide calls, {got['wraps']} wraps, "
          f"{got['resets_on_slide']} resets on slide calls, worst reward64 distance {stats['reward_ulps']:.0f} ulp; "
          f"{group} so far: {tot}")


@pytest.mark.parametrize("slack", [1, 3, 0])
@pytest.mark.parametrize("name", ELIGIBLE)
def test_slide_untiled(name, slack):
    g = replay.load(name)
    a = SlidingAdapter(g, obs_slack_rows=slack)
    _replay_sliding(a, g, 1, f"{name} slack={slack}", "untiled", full_run_of=name)
    a.env.close()


def _granted_epw(f, epw):
    """step_geometry's bound on a requested envs-per-wave: the LDS-staged dynamic columns of a
    workgroup of 4 waves stay within 32 KiB."""
    while epw > 1 and epw * 4 * f["W"] * f["nd"] * 4 > 32 * 1024:
        epw >>= 1
    return epw


def _tiled_cases():
    out = []
    for name in ELIGIBLE:
        f = _facts(name)
        lean = _lean_epws(f)[:2]
        for epw in lean + [e for e in (3, 16) if e not in lean]:
            out.append((name, epw))
    return out


@pytest.mark.parametrize("name,epw", _tiled_cases())
def test_slide_tiled(name, epw):
    g = _cut(replay.load(name), 160)
    f = strata.facts(g)
    a = SlidingAdapter(g, tile=67, obs_slack_rows=3, envs_per_wave=epw)
    info = a.env.launch_info()
    assert info["envs_per_wave"] == _granted_epw(f, epw)
    assert (info["vector_bytes"], info["phase_a"], info["dyn_columns"]) == (16, "cooperative", "lds-raw-rings")
    if epw in _lean_epws(f):
        assert info["envs_per_wave"] == epw and 67 * f["E"] >= epw
    _replay_sliding(a, g, 67, f"{name} tiled epw={epw}", "tiled")
    a.env.close()


SLIDING_VARIANTS = [0, _abi.KV_SHARED_TU, _abi.KV_GENERIC_COPY, _abi.KV_RECORD_DIRECT]
CLASSIC_VARIANTS = [_abi.KV_PER_WAVE_PHASE_A, _abi.KV_NO_LDS_STAGING]


def _variant_traces():
    """The nd = 4 trace, an F_obs = 4 trace, the multi-dataset limit-order trace, the zero-close trace
    and the trace without auto-reset."""
    picked = []
    for row in ("nd4_mixed_real_position_first", "multids_limit_orders_high_low", "zero_close_nonfinite",
                "no_autoreset_steps_after_end", "fobs4_window_ge64"):
        picked.append(_with_row(row, picked))
    return picked


def _variant_cases():
    picked = _variant_traces()
    rest = [n for n in ELIGIBLE if n not in picked]
    out, i = [], 0
    for v in SLIDING_VARIANTS:
        for store in (0, 1, 2):
            for name in picked + [rest[i % len(rest)]]:
                out.append((name, v, store))
            i += 1
    return out


@pytest.mark.parametrize("name,variant,store", _variant_cases())
def test_slide_kernel_variants(name, variant, store):
    g = _cut(replay.load(name), 120)
    a = SlidingAdapter(g, tile=5, obs_slack_rows=3, kernel_variant=variant, nontemporal_obs=store)
    _replay_sliding(a, g, 5, f"{name} variant={variant} store={store}", "variants")
    a.env.close()


@pytest.mark.parametrize("variant", CLASSIC_VARIANTS)
def test_variants_without_the_hot_shape_stay_classic(variant):
    """Per-wave phase A and unstaged dynamic columns are not the shape that slides: such an env keeps
    the classic buffer (tests/test_gpu_reference_sweep.py replays them)."""
    from gym_trading_env_amd.batched import BatchedTradingEnv
    g = replay.load(SLIDE[0])
    kw = replay.config_kwargs(g, 5, kernel_variant=variant)
    n_envs = kw.pop("n_envs")
    kw.pop("n_static"); kw.pop("n_datasets")
    env = BatchedTradingEnv(list(g["datasets"]), num_envs=n_envs, output="torch", **kw)
    assert not env.sliding_obs and env._t["obs"].is_contiguous()
    env.close()


def test_slide_full_windows_switch(monkeypatch):
    """GTE_SLIDE_FULL_WINDOWS=1 while the env is created: the head moves, every window is written."""
    name = _with_row("multids_limit_orders_high_low")
    g = replay.load(name)
    monkeypatch.setenv("GTE_SLIDE_FULL_WINDOWS", "1")
    a = SlidingAdapter(g, obs_slack_rows=3)
    monkeypatch.delenv("GTE_SLIDE_FULL_WINDOWS")
    _replay_sliding(a, g, 1, f"{name} full windows", "full-windows")
    a.env.close()


TILE_I = 16
INTERLEAVED = {"multids_limit_orders": "multids_limit_orders_high_low", "zero_close": "zero_close_nonfinite",
               "c3_window20": None}
M_I = 3


def interleaved_trace(key):
    return _with_row(INTERLEAVED[key]) if INTERLEAVED[key] else key


def interleave_plan(g, M=M_I, seed=2):
    """[(kind, start, stop, heads)]: seeded random chunks of calls (cut at the calls that add limit
    orders), each a run of plain step() calls ("step", two in four), one rollout(keep_obs=True) ("keep")
    or one rollout(keep_obs=False) ("drop"), with the head the window ledger (gte_api.hip) must report
    after every step, or after the rollout.  A rollout withdraws the buffer's validity; one that drops
    the per-step observations ends with a full write at head 0; one that keeps them does not write the
    env's own buffer, so the head stays and the first step after it writes in full at head 0; from
    there the heads count up again."""
    rng = np.random.default_rng(seed)
    plan, head, valid = [], 0, True
    for start, stop in _chunks(g, rng):
        kind = ("step", "step", "keep", "drop")[int(rng.integers(4))]
        if kind == "step":
            heads = []
            for _ in range(start, stop):
                head, valid = (head + 1 if valid and head < M else 0), True
                heads.append(head)
        elif kind == "keep":
            valid, heads = False, [head]
        else:
            head, valid, heads = 0, True, [0]
        plan.append((kind, start, stop, heads))
    return plan


def plan_counts(g, plan):
    """What a plan exercises: rollouts of either kind, slide steps, per-env resets on slide steps, and
    full steps that follow a rollout which kept its observations."""
    c = dict(keep=0, drop=0, slide_steps=0, resets_on_slide=0, full_step_after_keep=0)
    prev = None
    for kind, start, stop, heads in plan:
        if kind != "step":
            c[kind] += 1
        else:
            for k, h in zip(range(start, stop), heads):
                c["slide_steps"] += h != 0
                c["resets_on_slide"] += int((g["op"][k] == 0).sum()) if h != 0 else 0
            c["full_step_after_keep"] += prev == "keep" and heads[0] == 0
        prev = kind
    return c


@pytest.mark.parametrize("key", list(INTERLEAVED))
def test_steps_interleaved_with_rollouts(key):
    """interleave_plan on a trace, every call's outputs compared with the trace as
    test_gpu_reference_sweep.test_rollout does, the state after every step and rollout, and the head
    after each against the plan's.  (tests/test_slide_strata.py holds the plans to resets on slide
    steps, rollouts of both kinds and full steps after a rollout that kept its observations.)"""
    import torch
    from gym_trading_env_amd.batched import BatchedTradingEnv
    name = interleaved_trace(key)
    g = replay.load(name)
    f = strata.facts(g)
    kw = replay.config_kwargs(g, TILE_I, envs_per_wave=4, obs_slack_rows=M_I)
    N = kw.pop("n_envs")
    kw.pop("n_static"); kw.pop("n_datasets")
    env = BatchedTradingEnv(list(g["datasets"]) if f["D"] > 1 else g["datasets"][0], num_envs=N,
                            output="torch", **kw)
    assert env.sliding_obs
    view = _abi.GteObsView()

    def head():
        _abi.check(env._lib, env._lib.gte_obs_view(env._h, C.byref(view)))
        assert view.sliding == 1 and view.slack_rows == M_I
        return int(view.head)

    t = lambda a: np.tile(a, TILE_I)
    tt = lambda a: np.tile(a, (TILE_I,) + (1,) * (a.ndim - 1))
    bound = replay.reward_ulp_bound(g)
    worst = 0.0

    def check_call(k, r64, r32, term, trunc, val, obs, tag):
        nonlocal worst
        worst = max(worst, replay.assert_reward64(r64, t(g["reward"][k]), bound, tag))
        replay.assert_same_value(r32, replay.to_float32(r64), tag + " f32 reward")
        np.testing.assert_array_equal(term.astype(bool), t(g["done"][k]).astype(bool), err_msg=tag)
        np.testing.assert_array_equal(trunc.astype(bool), t(g["truncated"][k]).astype(bool), err_msg=tag)
        replay.assert_same_value(val, t(g["portfolio_valuation"][k]), tag + " valuation")
        if obs is not None:
            replay.assert_obs(obs, tt(g["obs"][k]), f["Fs"], tag + " obs")

    def check_state(k, tag):
        for gk, sk in replay.STATE_I32.items():
            np.testing.assert_array_equal(env.state(sk), t(g[gk][k]), err_msg=f"{tag}: {sk}")
        for gk, sk in replay.STATE_F64.items():
            replay.assert_same_value(env.state(sk), t(g[gk][k]), f"{tag}: {sk}")

    q, n = replay.injection_queue(g, TILE_I)
    if n:
        env.set_autoreset_injection(q["idx"], q["pos_index"], q["dataset"])
    env.reset(inject_idx=t(g["idx"][0]), inject_position_index=t(g["pos_index"][0]),
              inject_dataset=t(g["dataset"][0]))
    replay.assert_obs(env._t["obs"].cpu().numpy(), tt(g["obs"][0]), f["Fs"], f"{name} call 0 obs")
    assert head() == 0
    plan = interleave_plan(g)
    for kind, start, stop, heads in plan:
        if "lo_pos" in g and (g["lo_pos"][start] >= 0).any():
            env.add_limit_order(t(g["lo_pos"][start]), t(g["lo_limit"][start]), np.ones(N, np.uint8))
        if kind == "step":
            for k, h in zip(range(start, stop), heads):
                env.step(t(g["action"][k]))
                tag = f"{name} step call {k}"
                assert head() == h, tag
                check_call(k, env.read_output("reward64"), env.read_output("reward"),
                           env.read_output("terminated"), env.read_output("truncated"),
                           env.state("portfolio_valuation"), env._t["obs"].cpu().numpy(), tag)
                check_state(k, tag)
            continue
        keep = kind == "keep"
        acts = torch.from_numpy(np.ascontiguousarray(np.tile(g["action"][start:stop], (1, TILE_I)))).cuda()
        out = env.rollout(acts, keep_obs=keep, valuation=True, reward64=True)
        torch.cuda.synchronize()
        assert head() == heads[0] and (keep or heads[0] == 0), (name, kind, start)
        r64, r32 = out["reward64"].cpu().numpy(), out["reward"].cpu().numpy()
        term, trunc = out["terminated"].cpu().numpy(), out["truncated"].cpu().numpy()
        val = out["valuation"].cpu().numpy()
        for j, k in enumerate(range(start, stop)):
            check_call(k, r64[j], r32[j], term[j], trunc[j], val[j],
                       out["obs"][j].cpu().numpy() if keep else None, f"{name} rollout({kind}) call {k}")
        if not keep:
            assert out["obs"] is env._t["obs"]
            replay.assert_obs(out["obs"].cpu().numpy(), tt(g["obs"][stop - 1]), f["Fs"],
                              f"{name} rollout(drop) call {stop - 1} obs")
        check_state(stop - 1, f"{name} after rollout({kind}) call {stop - 1}")
    WORST_ULPS[f"{name} interleaved"] = worst
    print(f"[slide] {name} interleaved: {plan_counts(g, plan)}, worst reward64 distance {worst:.0f} ulp")
    env.close()
