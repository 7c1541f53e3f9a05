"""The lean slide launch ("Sliding window"): a step that stores one row per env runs in env
order, and a re-sort that falls due in a run of such launches waits for the next launch that writes full
windows.  Nothing a caller reads may change: the sliding env equals a classic twin
(`obs_slack_rows=-1`) bit for bit after EVERY call — observations, rewards, flags, terminal ids and every
state column — through frozen envs on the table's last row, dataset switches, re-sorts, limit orders,
rollouts and backtests, under every store policy, and whatever GTE_SLIDE_AB (gte.h) keeps.  Each case
asserts from the state it read that it met what it is about.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from gym_trading_env_amd import _abi

pytestmark = pytest.mark.gpu

STATE = ("idx", "step", "position_index", "dataset_index", "start_idx", "episode", "needs_reset", "asset",
         "fiat", "interest_asset", "interest_fiat", "portfolio_valuation", "real_position")
SENTINEL = 0x7FC0DEAD  # a NaN pattern no observation holds
N_TAIL = 1000          # 15 workgroups of 64 and one of 40: two full waves, a partial one (8), an empty one
N_ORDER = 4096 + 37    # 65 workgroups of 64: the L2-affinity order engages (at least 64 workgroups)


def _data(f_obs, T, seed=3):
    rng = np.random.default_rng(seed)
    close = 100.0 * np.exp(np.cumsum(rng.normal(-1e-3, 2e-2, T)))
    feat = rng.normal(0, 1, (T, f_obs - 2)).astype(np.float32)  # + the two default dynamic columns
    return feat, close, close * 1.01, close * 0.99


def _env(data, n, W, **kw):
    from gym_trading_env_amd.batched import BatchedTradingEnv
    args = dict(num_envs=n, positions=[-1, 0, 1], windows=W, trading_fees=1e-3, borrow_interest_rate=1e-4,
                max_episode_duration=7, seed=21, output="torch", verbose=0, envs_per_wave=16, obs_slack_rows=0)
    args.update(kw)
    return BatchedTradingEnv(data, **args)


def _pair(data, n, W, **kw):
    """The sliding env and its classic twin."""
    env, twin = _env(data, n, W, **kw), _env(data, n, W, **dict(kw, obs_slack_rows=-1))
    assert env.sliding_obs and not twin.sliding_obs and twin._t["obs"].is_contiguous()
    return env, twin


def _same(a, b, what):
    import torch
    torch.cuda.synchronize()
    assert a._t["obs"].shape == b._t["obs"].shape
    assert torch.equal(a._t["obs"].view(torch.int32), b._t["obs"].view(torch.int32)), f"{what}: obs"
    for k in ("reward", "reward64", "terminated", "truncated"):
        assert torch.equal(a._t[k], b._t[k]), f"{what}: {k}"
    np.testing.assert_array_equal(a.terminal_ids(), b.terminal_ids(), err_msg=what)
    for k in STATE:
        np.testing.assert_array_equal(a.state(k), b.state(k), err_msg=f"{what}: {k}")


def _actions(k, n, seed=5):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-1, 3, (k, n), generator=g, device="cuda", dtype=torch.int32)


def _since_rebuild(env):
    s = _abi.GteSchedule()
    _abi.check(env._lib, env._lib.gte_get_schedule(env._h, C.byref(s)))
    return int(s.steps_since_rebuild)


class Seen:
    """What the steps of a case met, from the state read around them."""

    def __init__(self):
        self.slides = self.wraps = self.full_in_slide = self.frozen = self.switches = 0
        self.wraps_after_due_resort = self.held = 0


def _steps(env, twin, acts, lo, hi, seen, mode, period=0):
    """Steps lo .. hi-1 of both envs, compared after each; `mode` is the autoreset mode."""
    M = int(env._obs_view.slack_rows)
    for i in range(lo, hi):
        h0 = int(env._obs_view.head)
        pending = env.state("needs_reset") != 0  # next_step: resets in this step; None: frozen envs
        ds0 = env.state("dataset_index").copy()
        last_row0 = (env.state("idx") >= np.asarray([d.T for d in env.datasets])[ds0] - 1).astype(np.int8)
        aged = _since_rebuild(env)
        env.step(acts[i])
        twin.step(acts[i])
        h = int(env._obs_view.head)
        _same(env, twin, f"step {i}")
        slide = h == h0 + 1
        assert slide or h == 0, (h0, h)
        assert slide == (h0 < M), (h0, h, M)  # nothing in these runs withdraws the window claim
        if mode == "same_step":
            fresh = env.state("step") == 0  # ended and reset inside this launch
        else:
            fresh = pending if mode == "next_step" else pending & (last_row0 == 1)
        seen.slides += int(slide)
        seen.wraps += int(not slide)
        if slide:
            seen.full_in_slide += int(fresh.sum())  # envs that got a full window from a slide launch
            if mode is None:  # ended, no auto-reset, no row left: frozen (gte_phase_a.h)
                seen.frozen += int((pending & (last_row0 == 1)).sum())
        seen.switches += int((env.state("dataset_index") != ds0).sum())
        if period > 0:
            now = _since_rebuild(env)
            if slide:  # the order is not used: the count goes on, past the period
                assert now == aged + 1, (aged, now)
                seen.held += int(now >= period)
            else:
                due = aged + 1 >= period
                assert now == (0 if due else aged + 1), (aged, now)
                seen.wraps_after_due_resort += int(due and aged >= period)


def _run(env, twin, mode, n_periods=3, seen=None, period=0, seed=5, **reset_kw):
    seen = seen or Seen()
    M = int(env._obs_view.slack_rows)
    n_steps = n_periods * (M + 1) + 2
    acts = _actions(n_steps, env.num_envs, seed)
    env.reset(**reset_kw)
    twin.reset(**reset_kw)
    _same(env, twin, "reset")
    _steps(env, twin, acts, 0, n_steps, seen, mode, period)
    assert seen.slides >= n_periods * M and seen.wraps >= n_periods - 1, vars(seen)
    return seen


# (W, n, envs_per_wave): the smallest hot shape; the headline window at the automatic geometry; the headline
# window past the size at which the order engages.  All with the automatic slack (3 rows at W = 8, 8 at 20).
SHAPES = [(8, N_TAIL, 16), (20, N_TAIL, 0), (20, N_ORDER, 16)]


@pytest.mark.parametrize("mode", [None, "next_step"])
@pytest.mark.parametrize("W,n,epw", SHAPES)
def test_end_of_the_table(W, n, epw, mode):
    """T = 64 and no episode limit: every episode starts on row W - 1 and runs onto the last row.  Two masked
    resets put the thirds of the batch 3 steps apart, so the envs of a wave arrive there at different steps.
    Without auto-reset they freeze on it, and a frozen env gets its full window from every slide launch;
    with next_step the truncation at T - 1 and the reset after it happen inside slide launches."""
    T = 64
    env, twin = _pair(_data(32, T), n, W, max_episode_duration="max", autoreset=mode, envs_per_wave=epw)
    M = int(env._obs_view.slack_rows)
    assert M == 2 * W // 5
    n_steps = 6 + (T - W) + 2 * (M + 1)  # the youngest third has stood on the last row for two periods
    acts = _actions(n_steps, n, seed=5)
    seen = Seen()
    env.reset()
    twin.reset()
    _same(env, twin, "reset")
    at = 0
    for third in range(2):
        _steps(env, twin, acts, at, at + 3, seen, mode)
        at += 3
        mask = (np.arange(n) % 3 == third).astype(np.uint8)
        env.reset(mask=mask)
        twin.reset(mask=mask)
        _same(env, twin, f"masked reset {third}")
    _steps(env, twin, acts, at, n_steps, seen, mode)
    assert seen.slides >= 3 * M and seen.wraps >= 3 and seen.full_in_slide > 0, vars(seen)
    if mode is None:
        assert seen.frozen > n and (env.state("idx") == T - 1).all(), vars(seen)
    else:
        # every env ran off the end and started again (the masked thirds had a reset more)
        assert (env.state("episode") >= np.where(np.arange(n) % 3 == 2, 2, 3)).all()
    env.close()
    twin.close()


@pytest.mark.parametrize("W,n,epw", [(20, N_TAIL, 0), (8, N_ORDER, 16)])
def test_dataset_switches(W, n, epw):
    """Three datasets of different length, a switch at every episode end, episodes of 7 steps: an env that
    switches continues at another table's rows, and resets fall in some waves and not in others."""
    data = [_data(32, T, seed=s) for s, T in ((3, 64), (4, 90), (5, 130))]
    env, twin = _pair(data, n, W, autoreset="next_step", episodes_between_dataset_switch=1, envs_per_wave=epw)
    seen = _run(env, twin, "next_step")
    assert seen.full_in_slide > 0 and seen.switches > 0, vars(seen)
    env.close()
    twin.close()


def test_slides_in_env_order_and_a_due_resort_waits_for_the_wrap():
    """affinity_period = 2 at 4 133 envs: slides run in env order, the re-sort that falls due inside every
    run of slides is held (the count goes on) and runs with the wrap, which is permuted."""
    env, twin = _pair(_data(32, 400), N_ORDER, 20, autoreset="next_step", affinity_period=2)
    seen = _run(env, twin, "next_step", period=2)
    assert seen.full_in_slide > 0 and seen.held > 0 and seen.wraps_after_due_resort >= 2, vars(seen)
    env.close()
    twin.close()


def test_rows_written_by_slides_in_env_order_and_permuted_wraps():
    """The sentinel check of test_gpu_sliding_obs.py::test_a_slide_step_writes_only_the_new_row with the order
    engaged: an env that merely advanced has exactly its newest row written, an env that reset its whole
    window at the new head, and a wrap (in the L2-affinity order, after the held re-sort) rows 0 .. W - 1."""
    import torch
    W, M, n = 20, 8, N_ORDER
    env = _env(_data(32, 400), n, W, autoreset="next_step", affinity_period=2)
    assert env.sliding_obs and int(env._obs_view.slack_rows) == M
    acts = _actions(40, n, seed=8)
    env.reset()
    k = 0
    for third in range(3):  # episodes out of phase: every step sees resets in some waves and none in others
        for _ in range(2):
            env.step(acts[k]); k += 1
        env.reset(mask=(np.arange(n) % 3 == third).astype(np.uint8))
    slab = env._obs_slab.view(torch.int32)
    rows = torch.arange(W + M, device="cuda")
    seen = {"slide": 0, "reset_in_slide": 0, "wrap": 0, "wrap_after_due_resort": 0}
    for _ in range(2 * (M + 1) + 2):
        h0 = int(env._obs_view.head)
        aged = _since_rebuild(env)
        resets = torch.from_numpy(env.state("needs_reset") != 0).cuda()
        torch.cuda.synchronize()
        slab.fill_(SENTINEL)
        env.step(acts[k]); k += 1
        torch.cuda.synchronize()
        h = int(env._obs_view.head)
        written = (slab != SENTINEL).any(dim=2)  # [n, W + M]
        window = (rows >= h) & (rows < h + W)
        if h0 < M:  # a slide step
            assert h == h0 + 1
            expect = torch.where(resets[:, None], window[None, :], (rows == h + W - 1)[None, :])
            seen["slide"] += 1
            seen["reset_in_slide"] += int(resets.sum())
        else:  # the wrap: every window in full at head 0
            assert h == 0
            expect = window[None, :].expand(n, -1)
            seen["wrap"] += 1
            seen["wrap_after_due_resort"] += int(aged >= 2 and _since_rebuild(env) == 0)
        assert torch.equal(written, expect), (h0, h)
        assert bool((slab[:, h:h + W][resets] != SENTINEL).all())  # all of it for the envs that reset
    assert seen["slide"] >= 2 * M and seen["wrap"] >= 2 and seen["reset_in_slide"] > 0, seen
    assert seen["wrap_after_due_resort"] >= 1, seen
    env.close()


CASES = {
    "next_step": dict(autoreset="next_step"),
    "same_step": dict(autoreset="same_step"),
    # (T = 48: episodes start on rows 19 .. 23, and an env that ended keeps stepping until the last row, where
    # it freezes — during the last steps of the case)
    "no_autoreset": dict(autoreset=None, max_episode_duration=5, T=48),
    "store_plain": dict(autoreset="next_step", nontemporal_obs=0),
    "store_nt": dict(autoreset="next_step", nontemporal_obs=1),
    "store_sc1": dict(autoreset="next_step", nontemporal_obs=2),
    "shared_tu": dict(autoreset="next_step", kernel_variant=_abi.KV_SHARED_TU),
    "record_direct": dict(autoreset="same_step", kernel_variant=_abi.KV_RECORD_DIRECT),
    # a backtest one launch per step, in same-step mode: its steps carry terminal records, so they slide
    # through the shared unit's instantiation
    "backtest_per_step": dict(autoreset="same_step", kernel_variant=_abi.KV_ROLLOUT_PER_STEP),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_modes_and_variants(name):
    """Limit orders, the three autoreset modes, the three store policies, the shared unit and direct record
    stores, with a rollout(keep_obs=False) and a backtest() between steps (slack 3: four wraps in 20 steps)."""
    import torch
    kw = dict(CASES[name])
    T = kw.pop("T", 400)
    mode, n, W, M = kw["autoreset"], N_TAIL, 20, 3
    env, twin = _pair(_data(32, T), n, W, obs_slack_rows=M, **kw)
    acts = _actions(30, n, seed=6)
    seen = Seen()
    env.reset()
    twin.reset()
    _same(env, twin, "reset")
    _steps(env, twin, acts, 0, 3, seen, mode)
    rng = np.random.default_rng(9)
    pi = np.where(rng.random(n) < 0.5, rng.integers(0, 3, n), -1).astype(np.int32)
    lim = np.asarray(_data(32, T)[1])[env.state("idx")] * (1 + rng.normal(0, 0.01, n))
    per = (rng.random(n) < 0.5).astype(np.uint8)
    env.add_limit_order(pi, lim, per)
    twin.add_limit_order(pi, lim, per)
    _steps(env, twin, acts, 3, 10, seen, mode)
    ra, rb = env.rollout(acts[10:13]), twin.rollout(acts[10:13])
    for k in ("reward", "terminated", "truncated"):
        assert torch.equal(ra[k], rb[k]), k
    _same(env, twin, "rollout")
    _steps(env, twin, acts, 13, 19, seen, mode)
    a, b = env.backtest(acts[19:23]), twin.backtest(acts[19:23])
    _same(env, twin, "backtest")
    assert torch.equal(a.reward_sum, b.reward_sum) and torch.equal(a.steps, b.steps)
    if name == "backtest_per_step":
        assert int(env._obs_view.head) == 3  # a full step at head 0, then three slides
    else:
        assert int(env._obs_view.head) == 0
    _steps(env, twin, acts, 23, 30, seen, mode)
    assert seen.slides >= 12 and seen.wraps >= 3 and seen.full_in_slide > 0, vars(seen)
    env.close()
    twin.close()


@pytest.mark.parametrize("bits", [1, 2, 4, 8, 15])
def test_switch_bits(bits, monkeypatch):
    """GTE_SLIDE_AB (gte.h): with the earlier order kept in slides (bit 1), and with the reserved bits, which
    are ignored, the values are the twin's."""
    monkeypatch.setenv("GTE_SLIDE_AB", str(bits))
    env = _env(_data(32, 400), N_ORDER, 20, autoreset="next_step", affinity_period=2)
    monkeypatch.delenv("GTE_SLIDE_AB")
    twin = _env(_data(32, 400), N_ORDER, 20, autoreset="next_step", affinity_period=2, obs_slack_rows=-1)
    assert env.sliding_obs and not twin.sliding_obs
    seen = _run(env, twin, "next_step", period=0)
    assert seen.full_in_slide > 0, vars(seen)
    if bits & 1:  # the order stays in use: a due re-sort runs at once, the count never passes the period
        assert _since_rebuild(env) < 2
    env.close()
    twin.close()
