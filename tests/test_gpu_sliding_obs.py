"""Sliding observation buffer (gte.h, `gte_bind_sliding_obs`): every env owns W + M rows, the window
moves one row forward per step and a step stores only the newest row of the envs that merely
advanced.  The observation a caller sees — a strided [N, W, F_obs] view at the library's head — must
equal the classic contiguous one bit for bit, through resets, frozen envs, limit orders, rollouts and
wraps; and the property that makes the step fast (one row written) is pinned.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from gym_trading_env_amd import _abi

pytestmark = pytest.mark.gpu

N = 165  # two full workgroups of 4 x 16 envs and a partial one
STATE = ("idx", "step", "position_index", "dataset_index", "start_idx", "episode", "needs_reset", "asset",
         "fiat", "interest_asset", "interest_fiat", "portfolio_valuation", "real_position")
SENTINEL = 0x7FC0DEAD  # a NaN pattern no observation holds


def _data(f_obs, T=400, seed=3):
    rng = np.random.default_rng(seed)
    close = 100.0 * np.exp(np.cumsum(rng.normal(-1e-3, 2e-2, T)))
    feat = rng.normal(0, 1, (T, f_obs - 2)).astype(np.float32)  # + the two default dynamic columns
    return feat, close, close * 1.01, close * 0.99


def _env(W, f_obs, **kw):
    from gym_trading_env_amd.batched import BatchedTradingEnv
    args = dict(num_envs=N, positions=[-1, 0, 1], windows=W, trading_fees=1e-3, borrow_interest_rate=1e-4,
                max_episode_duration=7, seed=21, output="torch", verbose=0, envs_per_wave=16,
                obs_slack_rows=3)
    args.update(kw)
    return BatchedTradingEnv(_data(f_obs), **args)


def _hot(W, f_obs):
    return W * f_obs // 4 >= 64  # windows of at least one wave instruction of 16-byte vectors


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


def _actions(n, seed=5):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-1, 3, (n, N), generator=g, device="cuda", dtype=torch.int32)


# (W, F_obs, obs_slack_rows, envs_per_wave): the smallest hot shape; the headline window with an explicit
# slack of 3 (several wraps within a few steps), with the automatic slack and with the automatic geometry;
# a shape below one wave instruction per env (not hot: both envs run the classic buffer)
SHAPES = [(8, 32, 3, 16), (20, 32, 3, 16), (20, 32, 0, 16), (20, 32, 3, 0), (20, 8, 3, 16)]


@pytest.mark.parametrize("mode", ["next_step", None, "same_step"])
@pytest.mark.parametrize("W,f_obs,slack,epw", SHAPES)
def test_sliding_env_equals_its_classic_twin(W, f_obs, slack, epw, mode):
    env = _env(W, f_obs, autoreset=mode, obs_slack_rows=slack, envs_per_wave=epw)
    twin = _env(W, f_obs, autoreset=mode, obs_slack_rows=-1, envs_per_wave=epw)
    assert env.sliding_obs == _hot(W, f_obs) and not twin.sliding_obs
    assert twin._t["obs"].is_contiguous()
    M = int(env._obs_view.slack_rows)
    if env.sliding_obs:
        assert M == (slack if slack else 2 * W // 5)
        assert env._t["obs"].stride() == ((W + M) * f_obs, f_obs, 1)
        assert env._t["obs"].view(N, -1).shape == (N, W * f_obs)  # still a view
    n_steps = max(16, 3 * (M + 1) + 2)
    acts = _actions(n_steps + 3)
    heads = []

    def steps(lo, hi):
        for i in range(lo, hi):
            env.step(acts[i])
            twin.step(acts[i])
            heads.append(int(env._obs_view.head))
            _same(env, twin, f"step {i}")

    env.reset()
    twin.reset()
    _same(env, twin, "reset")
    steps(0, 5)
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)  # a masked reset: full windows at the current head
    env.reset(mask=mask)
    twin.reset(mask=mask)
    _same(env, twin, "masked reset")
    steps(5, 7)
    rng = np.random.default_rng(9)
    pi = np.where(rng.random(N) < 0.5, rng.integers(0, 3, N), -1).astype(np.int32)
    lim = np.asarray(_data(f_obs)[1])[env.state("idx")] * (1 + rng.normal(0, 0.01, N))
    per = (rng.random(N) < 0.5).astype(np.uint8)
    env.add_limit_order(pi, lim, per)
    twin.add_limit_order(pi, lim, per)
    steps(7, 10)
    ra, rb = env.rollout(acts[10:13]), twin.rollout(acts[10:13])
    import torch
    for k in ("reward", "terminated", "truncated"):
        assert torch.equal(ra[k], rb[k]), k
    assert ra["obs"] is env._t["obs"]
    _same(env, twin, "rollout")
    # the packed reads go through the same (base, head, stride)
    view = env._t["obs"].cpu().numpy()
    snaps, obs = env.read_envs(3, 100)
    np.testing.assert_array_equal(obs.view(np.int32), view[3:103].view(np.int32))
    np.testing.assert_array_equal(snaps["idx"], env.state("idx")[3:103])
    _, one = env.read_env(N - 1)
    np.testing.assert_array_equal(one.view(np.int32), view[N - 1].view(np.int32))
    np.testing.assert_array_equal(env.read_output("obs").view(np.int32), view.view(np.int32))
    steps(13, n_steps + 3)
    if env.sliding_obs:
        # the head really moved: every head 0..M was written at, through at least three wraps
        assert set(heads) == set(range(M + 1)), heads
        assert sum(1 for a, b in zip(heads, heads[1:]) if b == 0 and a == M) >= 3, heads
    env.close()
    twin.close()


def test_sliding_env_equals_the_oracle(oracle_mod):
    """Observations, flags and state against the scalar oracle (the device Philox draws on both sides,
    as tests/test_gpu_parity.py does), through 3 periods of M + 1 steps and episode ends in every wave."""
    W, f_obs = 20, 32
    env = _env(W, f_obs, autoreset="next_step")
    assert env.sliding_obs
    feat, close, high, low = _data(f_obs)
    full = np.zeros((feat.shape[0], f_obs), np.float32)
    full[:, :f_obs - 2] = feat
    ora = oracle_mod.OracleEnv(env.cfg, [(full, close, high, low)])
    env.reset()
    ora.reset()
    rng = np.random.default_rng(22)
    ended = 0
    for k in range(3 * 4 + 2 + 1):
        if k > 0:
            a = rng.integers(-1, 3, N).astype(np.int32)
            env.step(a)
            ora.step(a, threads=4)
            ended += len(ora.term_ids)
        np.testing.assert_array_equal(env._t["obs"].cpu().numpy().view(np.int32), ora.obs.view(np.int32),
                                      err_msg=f"step {k}")
        np.testing.assert_array_equal(env.read_output("terminated"), ora.terminated, err_msg=f"step {k}")
        np.testing.assert_array_equal(env.read_output("truncated"), ora.truncated, err_msg=f"step {k}")
        so = ora.state()
        for n in ("idx", "step", "position_index", "portfolio_valuation"):
            np.testing.assert_array_equal(env.state(n), so[n], err_msg=f"step {k} {n}")
    assert ended > N
    env.close()
    ora.close()


def test_a_slide_step_writes_only_the_new_row():
    """What makes the step fast.  The whole slab is overwritten with a sentinel before a step; afterwards
    an env that merely advanced has exactly row h + W - 1 written, an env that reset exactly rows
    h .. h + W - 1 (h the new head), and a wrap step writes rows 0 .. W - 1 of every env."""
    import torch
    W, f_obs, M = 20, 32, 3
    env = _env(W, f_obs, autoreset="next_step")
    assert env.sliding_obs
    acts = _actions(24, seed=8)
    env.reset()
    # episodes out of phase, so that every step sees resets in some waves and none in others
    k = 0
    for third in range(3):
        for _ in range(2):
            env.step(acts[k]); k += 1
        env.reset(mask=(np.arange(N) % 3 == third).astype(np.uint8))
    slab = env._obs_slab.view(torch.int32)
    rows = torch.arange(W + M, device="cuda")
    seen = {"slide": 0, "reset_in_slide": 0, "wrap": 0, "pure_wave": 0, "mixed_wave": 0}
    for _ in range(12):
        h0 = int(env._obs_view.head)
        resets = torch.from_numpy(env.state("needs_reset") != 0).cuda()
        torch.cuda.synchronize()
        slab.fill_(SENTINEL)
        env.step(acts[k]); k += 1
        torch.cuda.synchronize()
        h = int(env._obs_view.head)
        written = (slab != SENTINEL).any(dim=2)  # [N, W + M]
        window = (rows >= h) & (rows < h + W)
        if h0 < M:  # a slide step
            assert h == h0 + 1
            newest = rows == h + W - 1
            expect = torch.where(resets[:, None], window[None, :], newest[None, :])
            seen["slide"] += 1
            seen["reset_in_slide"] += int(resets.sum())
            per_wave = resets[:160].view(10, 16).sum(dim=1)  # (identity order: wave w steps envs 16 w ..)
            seen["pure_wave"] += int((per_wave == 0).sum())
            seen["mixed_wave"] += int(((per_wave > 0) & (per_wave < 16)).sum())
        else:  # the wrap: today's step, every window in full at head 0
            assert h == 0
            expect = window[None, :].expand(N, -1)
            seen["wrap"] += 1
        assert torch.equal(written, expect), (h0, h)
        # and what was written is the observation: all of it for the envs that reset
        full_rows = slab[:, h:h + W]
        assert bool((full_rows[resets] != SENTINEL).all())
    assert seen["slide"] >= 8 and seen["wrap"] >= 2 and seen["reset_in_slide"] > 0, seen
    assert seen["pure_wave"] > 0 and seen["mixed_wave"] > 0, seen
    env.close()


def _reward(history):
    return np.log(history["portfolio_valuation", -1] / history["portfolio_valuation", -2])


@pytest.mark.parametrize("kw", [dict(f_obs=5), dict(autoreset="same_step", final_obs=True), dict(dyn_persist=True),
                                dict(log_steps=4), dict(reward_function=_reward)],
                         ids=["not_hot", "final_obs", "dyn_persist", "log", "python_reward"])
def test_what_does_not_slide_keeps_the_classic_buffer(kw):
    kw = dict(kw)
    env = _env(20, kw.pop("f_obs", 32), **kw)
    view = _abi.GteObsView()
    _abi.check(env._lib, env._lib.gte_obs_view(env._h, C.byref(view)))
    assert not env.sliding_obs and view.sliding == 0 and view.slack_rows == 0 and view.rows_per_env == 20
    obs, _ = env.reset()
    assert obs.is_contiguous() and env._t["obs"].is_contiguous()
    # and the library refuses a sliding buffer for it
    import torch
    slab = torch.zeros((N, 23, obs.shape[2]), device="cuda")
    with pytest.raises(_abi.GteError, match="does not slide"):
        _abi.check(env._lib, env._lib.gte_bind_sliding_obs(env._h, C.c_void_p(slab.data_ptr()), 23))
    env.close()


def _policy(obs):
    import torch
    row = obs[:, -1]
    return ((row[:, 0] > 0).to(torch.int32) + (row[:, 1] > 0.5).to(torch.int32)).contiguous()


def test_captured_steps_leave_sliding_and_equal_an_eager_sliding_twin():
    import torch
    graphed, eager = _env(20, 32), _env(20, 32)
    o1, _ = graphed.reset()
    o2, _ = eager.reset()
    for _ in range(2):  # off head 0 before the capture
        graphed.step(_policy(graphed._t["obs"]))
        eager.step(_policy(eager._t["obs"]))
    assert graphed.sliding_obs and int(graphed._obs_view.head) == 2
    before = graphed._t["obs"].clone()
    g = graphed.capture_steps(lambda i: graphed.step(_policy(graphed._t["obs"])), 4)
    assert not graphed.sliding_obs and graphed._t["obs"].is_contiguous()  # classic from here on
    assert torch.equal(graphed._t["obs"], before)  # the capture ran nothing
    for r in range(4):
        for _ in range(4):
            eager.step(_policy(eager._t["obs"]))
        g.replay()
        _same(graphed, eager, f"replay {r}")
    assert eager.sliding_obs
    graphed.step(_policy(graphed._t["obs"]))
    eager.step(_policy(eager._t["obs"]))
    _same(graphed, eager, "eager step after the replays")
    graphed.close()
    eager.close()


def test_allgather_obs_on_a_sliding_env_is_an_error():
    env = _env(20, 32)
    env.reset()
    import torch
    dst = torch.zeros((N, 20, 32), device="cuda")
    with pytest.raises(_abi.GteError, match="sliding observation buffer"):
        _abi.check(env._lib, env._lib.gte_allgather_obs(env._h, C.c_void_p(dst.data_ptr()), 0))
    env.close()


def test_bind_outputs_after_sliding_steps_returns_to_classic():
    """gte_bind_outputs through the C ABI in the middle of a run of slides: the next observation is a
    full, correct, contiguous one; and binding a sliding buffer again starts with a full write."""
    import torch
    env, twin = _env(20, 32), _env(20, 32, obs_slack_rows=-1)
    acts = _actions(12, seed=4)
    env.reset()
    twin.reset()
    for i in range(2):
        env.step(acts[i]); twin.step(acts[i])
    assert int(env._obs_view.head) == 2
    classic = torch.full((N, 20, 32), float("nan"), device="cuda")
    b = _abi.GteOutputs()
    _abi.check(env._lib, env._lib.gte_get_outputs(env._h, C.byref(b)))
    slab_ptr = b.obs
    b.obs = classic.data_ptr()
    _abi.check(env._lib, env._lib.gte_bind_outputs(env._h, C.byref(b)))
    for i in range(2, 5):
        env.step(acts[i]); twin.step(acts[i])
        assert not env.sliding_obs and env._t["obs"].data_ptr() == classic.data_ptr()
        _same(env, twin, f"classic step {i}")
    # back to the slab (now stale): the first step must not slide
    _abi.check(env._lib, env._lib.gte_bind_sliding_obs(env._h, C.c_void_p(slab_ptr), 23))
    view = _abi.GteObsView()
    for i in range(5, 11):
        env.step(acts[i]); twin.step(acts[i])
        _abi.check(env._lib, env._lib.gte_obs_view(env._h, C.byref(view)))
        assert view.sliding == 1 and view.head == (i - 5) % 4
        window = env._obs_slab[:, view.head:view.head + 20]
        torch.cuda.synchronize()
        assert torch.equal(window.view(torch.int32), twin._t["obs"].view(torch.int32)), f"step {i}"
    env.close()
    twin.close()


def test_backtests_off_head_0_leave_the_current_observation():
    """backtest() and backtest_signals() end with a full write at head 0: `_t["obs"]` must follow it."""
    import torch
    env, twin = _env(20, 32), _env(20, 32, obs_slack_rows=-1)
    acts = _actions(12, seed=6)
    rng = np.random.default_rng(5)
    table = rng.integers(-1, 3, (3, 400)).astype(np.int8)
    for e in (env, twin):
        e.reset()
        e.bind_signals(table)
    for i in range(2):
        env.step(acts[i]); twin.step(acts[i])
    assert int(env._obs_view.head) == 2
    a, b = env.backtest(acts[2:6]), twin.backtest(acts[2:6])
    assert int(env._obs_view.head) == 0
    _same(env, twin, "backtest")
    assert torch.equal(a.reward_sum, b.reward_sum) and torch.equal(a.steps, b.steps)
    for i in range(6, 8):
        env.step(acts[i]); twin.step(acts[i])
    assert int(env._obs_view.head) == 2
    env.backtest_signals(5)
    twin.backtest_signals(5)
    assert int(env._obs_view.head) == 0
    _same(env, twin, "backtest_signals")
    env.step(acts[8]); twin.step(acts[8])
    _same(env, twin, "step after the backtests")
    env.close()
    twin.close()


@pytest.mark.parametrize("call", ["set_schedule", "reset"])
def test_calls_that_withdraw_the_window_claim_off_head_0(call):
    """gte_set_schedule outside a capture, and an unmasked reset in the middle of a run of slides (the table
    in gte_ledger.h): the next observation is a full one at head 0, and the heads count up from there.  128
    envs of the smallest shape that slides, beside a classic twin, past two wraps of the head."""
    env = _env(8, 32, num_envs=128)
    twin = _env(8, 32, num_envs=128, obs_slack_rows=-1)
    assert env.sliding_obs and not twin.sliding_obs
    acts = _actions(12, seed=9)[:, :128].contiguous()
    env.reset(); twin.reset()
    for i in range(2):
        env.step(acts[i]); twin.step(acts[i])
    assert int(env._obs_view.head) == 2
    if call == "set_schedule":  # (what StepGraph does around a capture, with nothing captured)
        for e in (env, twin):
            s = _abi.GteSchedule()
            _abi.check(e._lib, e._lib.gte_get_schedule(e._h, C.byref(s)))
            _abi.check(e._lib, e._lib.gte_set_schedule(e._h, C.byref(s)))
        expect = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]  # the first step after it writes every window
    else:
        env.reset(); twin.reset()
        assert int(env._obs_view.head) == 0
        _same(env, twin, "reset off head 0")
        expect = [1, 2, 3, 0, 1, 2, 3, 0, 1, 2]  # the reset wrote every window
    heads = []
    for i in range(2, 12):
        env.step(acts[i]); twin.step(acts[i])
        heads.append(int(env._obs_view.head))
        _same(env, twin, f"{call}, step {i}")
    assert heads == expect, heads
    env.close()
    twin.close()


def test_full_window_switch_keeps_the_layout_and_the_values(monkeypatch):
    """GTE_SLIDE_FULL_WINDOWS (gte.h): the moving head, full windows every step — the A/B twin."""
    import torch
    monkeypatch.setenv("GTE_SLIDE_FULL_WINDOWS", "1")
    full = _env(20, 32)
    monkeypatch.delenv("GTE_SLIDE_FULL_WINDOWS")
    env = _env(20, 32)
    assert full.sliding_obs and env.sliding_obs
    acts = _actions(10, seed=7)
    full.reset(); env.reset()
    slab = full._obs_slab.view(torch.int32)
    for i in range(10):
        torch.cuda.synchronize()
        slab.fill_(SENTINEL)
        full.step(acts[i]); env.step(acts[i])
        h = int(full._obs_view.head)
        assert h == int(env._obs_view.head) == (i + 1) % 4
        _same(full, env, f"step {i}")
        written = (slab != SENTINEL).any(dim=2)
        assert bool(written[:, h:h + 20].all()) and int(written.sum()) == N * 20  # every window, nothing else
    full.close()
    env.close()


def test_observation_gathers_leave_sliding():
    """Whoever gathers observations sends one contiguous buffer: ShardedTradingEnv(gather_obs=True) and a
    ReturnPipeline whose ReturnGather has an observation buffer make the env classic, once."""
    import os
    import torch
    import torch.distributed as dist
    from gym_trading_env_amd.batched import BatchedTradingEnv
    from gym_trading_env_amd.distributed import ReturnGather, ReturnPipeline, ShardedTradingEnv
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 1000))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        kw = dict(positions=[-1, 0, 1], windows=20, max_episode_duration=7, seed=21, verbose=0)
        G = 192  # (the packed returns of a shard are viewed as f32: a multiple of 4 envs)
        sharded = ShardedTradingEnv(_data(32), G, gather_obs=True, device=0, **kw)
        plain = ShardedTradingEnv(_data(32), G, device=0, **kw)
        assert not sharded.env.sliding_obs and sharded.env._t["obs"].is_contiguous()
        assert plain.env.sliding_obs  # nothing gathers observations: the window slides
        obs, _ = sharded.reset()
        plain.reset()
        a = torch.randint(-1, 3, (3, G), generator=torch.Generator(device="cuda").manual_seed(2), device="cuda",
                          dtype=torch.int32)
        for i in range(3):
            obs = sharded.step(a[i])[0]
            plain.step(a[i])
            assert obs.is_contiguous() and sharded.env._t["obs"].is_contiguous()
            assert torch.equal(obs.view(torch.int32), plain.env._t["obs"].view(torch.int32))
        sharded.close()
        plain.close()
        env = BatchedTradingEnv(_data(32), num_envs=G, output="torch", return_slots=2, **kw)
        assert env.sliding_obs
        ReturnPipeline(env, ReturnGather(G, env.packed_returns.device, obs_shape=env.obs_shape, depth=2), 1, 2)
        assert not env.sliding_obs and env._t["obs"].is_contiguous()
        env.close()
    finally:
        dist.destroy_process_group()
