"""Sparse terminated / truncated stores (gte_phase_a.h store_flags, the FLAGS claim of gte_ledger.h): a
step stores only the flags that change when the host has proved that the buffers hold what the env's
previous step stored there.  Every case below runs an env next to an untouched twin that always
stores densely (kernel_variant KV_DENSE_FLAGS) and compares all four return arrays and the terminal list
after every call, through L2-affinity re-sorts and auto-resets, while the buffers rotate, are rebound,
shared with another env, replayed from a graph or written by a rollout.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from gym_trading_env_amd import _abi

pytestmark = pytest.mark.gpu

DENSE = _abi.KV_DENSE_FLAGS  # kernel_variant bit: never sparse


def _data(seed=3, T=900, Fs=30):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (T, Fs)).astype(np.float32),
            100 * np.exp(np.cumsum(rng.normal(-1e-3, 4e-2, T))))


def _pair(N=5000, seed=11, **kw):
    """(env, dense twin): the headline kernel's shape (windows 20 x 32 columns), short episodes so
    that envs end in every step, a re-sort every 3 steps."""
    from gym_trading_env_amd.batched import BatchedTradingEnv
    args = dict(num_envs=N, positions=[-1, 0, 1], windows=20, trading_fees=1e-3,
                borrow_interest_rate=1e-4, max_episode_duration=9, seed=seed, output="torch",
                affinity_period=3, verbose=0)
    env = BatchedTradingEnv(_data(), **{**args, **kw})
    twin = BatchedTradingEnv(_data(), **{**args, "kernel_variant": DENSE})
    env.reset()
    twin.reset()
    return env, twin


def _outputs(env):
    """The buffers the env's last call wrote (whatever is bound now), read on the host."""
    env._torch.cuda.synchronize()
    _check(env, env._lib.gte_get_outputs(env._h, C.byref(env._out)))
    return {k: env.read_output(k) for k in ("reward", "reward64", "terminated", "truncated")}


def _check(env, rc):
    _abi.check(env._lib, rc)


def _same(env, twin, what=""):
    a, b = _outputs(env), _outputs(twin)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(env.terminal_ids(), twin.terminal_ids(), err_msg=what)
    np.testing.assert_array_equal(env.state("idx"), twin.state("idx"), err_msg=what)


def _actions(env, n, seed=5):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-1, 3, (n, env.num_envs), generator=g, device="cuda", dtype=torch.int32)


def _steps(env, twin, steps, acts):
    """steps on both, compared after each -> episodes that ended in them"""
    ended = 0
    for i in range(steps):
        env.step(acts[i])
        twin.step(acts[i])
        _same(env, twin, f"step {i}")
        ended += len(twin.terminal_ids())
    return ended


@pytest.mark.parametrize("slots", [2, 3])
def test_rotated_return_buffers(slots):
    env, twin = _pair(return_slots=slots)
    acts = _actions(env, 24)
    assert _steps(env, twin, 24, acts) > 0
    env.close()
    twin.close()


def test_rebinding_outputs_mid_episode():
    env, twin = _pair()
    acts = _actions(env, 30)
    ended = _steps(env, twin, 8, acts)
    old = type(env._out)()
    _check(env, env._lib.gte_get_outputs(env._h, C.byref(old)))
    old_t, old_packed = dict(env._t), env._packed_all  # (kept alive: rebound below)
    env._bind_torch_outputs()  # fresh, zero-filled buffers
    ended += _steps(env, twin, 8, acts[8:])
    # back to the first buffers: they hold the flags of step 8, not of the last step
    _check(env, env._lib.gte_bind_outputs(env._h, C.byref(old)))
    env._t = old_t
    ended += _steps(env, twin, 14, acts[16:])
    assert ended > 0
    del old_packed
    env.close()
    twin.close()


def test_two_envs_sharing_return_buffers():
    """Two envs bound to the same return buffers, stepped in turn: each step overwrites the other env's
    flags (each keeps its own observations and terminal list)."""
    a, twin_a = _pair(seed=11)
    b, twin_b = _pair(seed=12)
    shared, mine = type(a._out)(), type(b._out)()
    _check(a, a._lib.gte_get_outputs(a._h, C.byref(shared)))
    _check(b, b._lib.gte_get_outputs(b._h, C.byref(mine)))
    for k in ("reward", "reward64", "terminated", "truncated"):
        setattr(mine, k, getattr(shared, k))
    _check(b, b._lib.gte_bind_outputs(b._h, C.byref(mine)))
    acts = _actions(a, 20)
    ended = 0
    for i in range(20):
        a.step(acts[i])
        twin_a.step(acts[i])
        _same(a, twin_a, f"a, step {i}")
        b.step(acts[i])
        twin_b.step(acts[i])
        _same(b, twin_b, f"b, step {i}")
        ended += len(twin_b.terminal_ids())
    assert ended > 0
    for e in (a, b, twin_a, twin_b):
        e.close()


def test_graph_replays_beside_eager_steps():
    import torch
    env, twin = _pair()
    acts = _actions(env, 40)
    ended = _steps(env, twin, 4, acts)
    buf = torch.empty((2, env.num_envs), dtype=torch.int32, device="cuda")
    g = env.capture_steps(lambda i: env.step(buf[i]), 2)
    k = 4
    for r in range(6):
        buf.copy_(acts[k:k + 2])
        g.replay()
        for i in range(2):
            twin.step(acts[k + i])
        _same(env, twin, f"replay {r}")
        ended += len(twin.terminal_ids())
        k += 2
        for i in range(2):  # an even number of eager steps between replays
            env.step(acts[k + i])
            twin.step(acts[k + i])
            _same(env, twin, f"eager step after replay {r}")
            ended += len(twin.terminal_ids())
        k += 2
    assert ended > 0
    env.close()
    twin.close()


def test_rollout_after_step_and_step_after_rollout():
    env, twin = _pair()
    acts = _actions(env, 40)
    ended = _steps(env, twin, 5, acts)
    k = 5
    for keep_obs, K in ((False, 4), (True, 3), (False, 1)):
        ra = env.rollout(acts[k:k + K], keep_obs=keep_obs, reward64=True)
        rb = twin.rollout(acts[k:k + K], keep_obs=keep_obs, reward64=True)
        for name in ("reward", "reward64", "terminated", "truncated"):
            assert env._torch.equal(ra[name], rb[name]), name
        _same(env, twin, f"rollout of {K} (keep_obs={keep_obs})")
        ended += int(rb["terminated"].sum() + rb["truncated"].sum())
        k += K
        ended += _steps(env, twin, 5, acts[k:])
        k += 5
    assert ended > 0
    env.close()
    twin.close()


@pytest.mark.parametrize("call", ["backtest", "backtest_signals", "reset", "masked_reset"])
def test_step_after_a_call_that_writes_the_flags(call):
    """The entry points that withdraw the flag claim without rebinding anything (the table in
    gte_ledger.h): a backtest of either kind and a reset, masked or not, in the middle of a run of sparse
    steps.  128 envs of the smallest shape that slides (windows 8 x 32 columns, 3 slack rows) beside a twin
    that stores every flag and writes every window (KV_DENSE_FLAGS, obs_slack_rows=-1), compared after
    every call, observations included, until the head has wrapped twice."""
    from gym_trading_env_amd.batched import BatchedTradingEnv
    N = 128
    args = dict(num_envs=N, positions=[-1, 0, 1], windows=8, trading_fees=1e-3, borrow_interest_rate=1e-4,
                max_episode_duration=9, seed=11, output="torch", verbose=0, envs_per_wave=16)
    env = BatchedTradingEnv(_data(), obs_slack_rows=3, **args)
    twin = BatchedTradingEnv(_data(), obs_slack_rows=-1, kernel_variant=DENSE, **args)
    assert env.sliding_obs and not twin.sliding_obs

    def same(what):
        _same(env, twin, what)
        assert env._torch.equal(env._t["obs"].view(env._torch.int32), twin._t["obs"].view(env._torch.int32)), what

    def steps(acts, what):
        ended = 0
        for i in range(len(acts)):
            env.step(acts[i])
            twin.step(acts[i])
            same(f"{what}, step {i}")
            ended += len(twin.terminal_ids())
        return ended

    acts = _actions(env, 24)
    table = np.random.default_rng(5).integers(-1, 3, (2, 900)).astype(np.int8)
    for e in (env, twin):
        e.reset()
        e.bind_signals(table)
    ended = steps(acts[:6], "before")  # (flags sparse from the second step on, one wrap of the head)
    for e in (env, twin):
        if call == "backtest":
            e.backtest(acts[6:10])
        elif call == "backtest_signals":
            e.backtest_signals(4)
        else:
            e.reset(mask=(np.arange(N) % 3 == 0).astype(np.uint8) if call == "masked_reset" else None)
    same(call)
    ended += steps(acts[10:20], f"after {call}")
    assert ended > 0
    env.close()
    twin.close()
