"""Signal tables on the GPU (gte_bind_signals / gte_signal_actions / gte_backtest_signals,
csrc/gte_backtest.hip): `backtest_signals(K)` against a twin that reads its rows back after every
step, looks the action up on the host (tests/signal_model.py) and calls `step()` — records, state,
outputs, terminal ids and the step after, bit for bit; K = 1 and 2; chunks; the fused path against
the step-by-step ones; `backtest(acts)` over the materialised actions; `signal_actions()`; the
reference-made fixtures; refusals; the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import backtest_model as bm
import replay
import signal_model as sm
import test_gpu_backtest as tb
from gym_trading_env_amd import _abi

pytestmark = pytest.mark.gpu

MODES = tb.MODES
N, T, K = 193, 403, 96
BASE = dict(positions=[-1, 0, 1], trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration=24, seed=11)


def _table(seed, S, T, P=3):
    """int8 [S, T]: position indices with -1 / P and a few extreme bytes among them."""
    rng = np.random.default_rng(seed)
    t = rng.integers(-1, P + 1, (S, T)).astype(np.int8)
    t[rng.random((S, T)) < 0.04] = -128
    t[rng.random((S, T)) < 0.04] = 127
    return t


def _strategy(explicit, n, S, seed=5):
    return np.random.default_rng(seed).integers(0, S, n).astype(np.int32) if explicit else None


class _HostLookup:
    """The [K, N] actions of twin a, made one row at a time: row k is looked up on the host from the
    rows the env stands on when step k is about to run (what tb._single_step_columns asks for)."""

    def __init__(self, env, tables, strategy, K):
        self.env, self.tables, self.strategy, self.shape, self.rows = env, tables, strategy, (K,), []

    def __getitem__(self, k):
        import torch
        assert k == len(self.rows)
        a = sm.lookup(self.tables, self.strategy, self.env.state("idx"), self.env.state("dataset_index"),
                      len(self.env.positions))
        self.rows.append(a)
        return torch.from_numpy(a).cuda()


def _prepare(data, tables, mode, kw, n=N, before=None, phase=True):
    """Twins (a: single steps, b: backtest_signals) with tables bound, reset, out of phase."""
    import torch
    a, b = tb._twins(data, n, mode, **kw)
    tb._both(a, b, lambda e: e.bind_signals(tables))
    tb._both(a, b, lambda e: e.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    if phase:
        tb._phase(a, b, n, len(kw["positions"]), gen)
    if before:
        tb._both(a, b, before)
    return a, b, gen


def _against_host_lookup(data, tables, mode, kw, tag, strategy=None, n=N, k=K, before=None):
    """-> (model records, step dicts, the actions twin a took)."""
    import torch
    a, b, gen = _prepare(data, tables, mode, kw, n=n, before=before)
    acts = _HostLookup(a, tables, strategy, k)
    recs, steps = tb._single_step_columns(a, acts)
    want = [bm.run(r, s) for r, s in zip(recs, steps)]
    stats = b.backtest_signals(k, strategy=strategy)
    tb._assert_records(stats, want, tag)
    tb._assert_same_env(a, b, tag)
    one = torch.randint(-1, len(kw["positions"]), (n,), dtype=torch.int32, device="cuda", generator=gen)
    for x, y in zip(a.step(one)[:4], b.step(one)[:4]):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=f"{tag}: the step after")
    a.close()
    b.close()
    return want, steps, np.stack(acts.rows)


SHAPES = [(None, 1, False), (5, 1, True), (None, 7, True), (5, 7, False), (None, 300, False), (5, 300, True)]


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
@pytest.mark.parametrize("windows,S,explicit", SHAPES)
def test_backtest_signals_equals_host_lookup_and_single_steps(windows, S, explicit, mode):
    """N = 193: a partial wave and a partial workgroup at 32 and at 64 envs per wave; T = 403 is no
    multiple of 16; 24-step episodes over K = 96: every env resets and crosses 16-row pieces several
    times.  S = 1, S that does not divide N, S > N; explicit and default strategy."""
    data = tb._data(31, T, 6)[:2]
    kw = dict(BASE, windows=windows)
    want, steps, acts = _against_host_lookup(data, _table(S, S, T), mode, kw, f"S={S} W={windows} {mode}",
                                             strategy=_strategy(explicit, N, S))
    assert (acts == -1).any() and (acts >= 0).any()
    assert sum(r["episodes"] for r in want) > (N if mode else 0)
    assert sum(r["trades"] for r in want) > 0
    if mode == "next_step":
        assert any(s.get("reset") and not s["stepped"] for e in steps for s in e)


def test_env_frozen_on_the_last_row_of_a_full_piece():
    """T = 400 = 25 pieces: rows are exactly their stride, and with auto-reset off envs go on after
    their episode and end frozen on row 399, the last byte of the last piece — the piece after it
    does not exist."""
    data = tb._data(32, 400, 6)[:2]
    kw = dict(BASE, windows=None)
    a, b, gen = _prepare(data, _table(3, 7, 400), None, kw, n=65, phase=False)
    start = np.linspace(310, 375, 65).astype(np.int32)  # 24-step episodes, then on to the last row
    tb._both(a, b, lambda e: e.reset(inject_idx=start))
    acts = _HostLookup(a, [_table(3, 7, 400)], None, K)
    recs, steps = tb._single_step_columns(a, acts)
    tb._assert_records(b.backtest_signals(K), [bm.run(r, s) for r, s in zip(recs, steps)], "frozen")
    tb._assert_same_env(a, b, "frozen")
    assert (a.state("idx") == 399).all() and any(not s["stepped"] for e in steps for s in e)
    a.close()
    b.close()


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_three_datasets_with_a_table_each(mode):
    sets = [tb._data(40 + d, 403 - 57 * d, 6)[:2] for d in range(3)]
    tables = [_table(50 + d, 7, len(c)) for d, (_, c) in enumerate(sets)]
    kw = dict(BASE, windows=5, episodes_between_dataset_switch=1)
    import torch
    a, b, gen = _prepare(sets, tables, mode, kw)
    seen = set(a.state("dataset_index").tolist())
    acts = _HostLookup(a, tables, None, K)
    recs, steps = tb._single_step_columns(a, acts)
    seen |= set(a.state("dataset_index").tolist())
    tb._assert_records(b.backtest_signals(K), [bm.run(r, s) for r, s in zip(recs, steps)], f"3 datasets {mode}")
    tb._assert_same_env(a, b, f"3 datasets {mode}")
    assert seen == {0, 1, 2}
    a.close()
    b.close()


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_pending_persistent_limit_orders(mode):
    data = tb._data(33, T, 6, sigma=1.5e-2)
    want, _, _ = _against_host_lookup(data, _table(9, 7, T), mode, dict(BASE, windows=5), f"orders {mode}",
                                      before=tb._add_orders)
    assert sum(r["trades"] for r in want) > 0


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
@pytest.mark.parametrize("k", [1, 2])
def test_one_and_two_steps(k, mode):
    """K = 1: lookup + step + fold only; K = 2: one fused step before it."""
    _against_host_lookup(tb._data(34, T, 6)[:2], _table(2, 7, T), mode, dict(BASE, windows=5),
                         f"K={k} {mode}", k=k)


def _pair(mode, tables=None, **over):
    import torch
    kw = dict(BASE, windows=5, **over)
    data = tb._data(35, T, 6)[:2]
    tables = _table(4, 7, T) if tables is None else tables
    x, y = tb._env(data, N, mode, **kw), tb._env(data, N, mode, **kw)
    tb._both(x, y, lambda e: e.bind_signals(tables))
    tb._both(x, y, lambda e: e.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    tb._phase(x, y, N, 3, gen)
    return x, y


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_chunked_calls(mode):
    x, y = _pair(mode)
    whole = x.backtest_signals(96).numpy()
    y.backtest_signals(40)
    tb._assert_same_records(y.backtest_signals(56, resume=True).numpy(), whole, f"{mode}: 40 + 56 resumed")
    tb._assert_same_env(x, y, f"{mode}: chunks")
    assert whole["steps"].sum() > 0 and whole["episodes"].sum() > 0
    x.close()
    y.close()


def test_reset_between_chunks_restarts_peak_and_position_and_keeps_the_sums():
    x, y = _pair("next_step")
    mask = (np.arange(N) % 2).astype(np.uint8)
    first = x.backtest_signals(40).numpy().copy()
    x.reset(mask=mask)
    got = x.backtest_signals(56, resume=True).numpy()
    y.backtest_signals(40)
    y.reset(mask=mask)
    positions = np.asarray(y.positions, np.float64)
    v0, p0 = y.state("portfolio_valuation"), positions[y.state("position_index")]
    recs, steps = tb._single_step_columns(y, _HostLookup(y, [_table(4, 7, T)], None, 56))
    want = []
    for e in range(N):
        r = {f: first[f][e] for f in bm.F64_FIELDS}
        r.update({f: int(first[f][e]) for f in bm.INT_FIELDS})
        r["ended"] = bool(first["ended"][e])
        if mask[e]:
            bm.reset(r, v0[e], p0[e])
        want.append(bm.run(r, steps[e]))
    tb._assert_records(got, want, "reset(mask) between chunks")
    assert (got["steps"] > first["steps"]).all()
    x.close()
    y.close()


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
@pytest.mark.parametrize("unfused", ["per_step_variant", "log_steps"])
def test_fused_and_per_step_paths_give_the_same_records(unfused, mode, capfd, monkeypatch):
    monkeypatch.setenv("GTE_DEBUG_GEOMETRY", "1")
    import torch
    over = dict(kernel_variant=_abi.KV_ROLLOUT_PER_STEP) if unfused == "per_step_variant" else dict(log_steps=8)
    kw = dict(BASE, windows=5)
    data = tb._data(36, T, 6)[:2]
    x, y = tb._env(data, N, mode, **kw), tb._env(data, N, mode, **dict(kw, **over))
    tb._both(x, y, lambda e: e.bind_signals(_table(6, 7, T)))
    tb._both(x, y, lambda e: e.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(29)
    tb._phase(x, y, N, 3, gen)
    capfd.readouterr()
    fused = x.backtest_signals(K).numpy()
    assert f"rollout path: backtest signals summary, {K} steps" in capfd.readouterr().err
    stepwise = y.backtest_signals(K).numpy()
    assert f"rollout path: backtest signals per-step, {K} steps" in capfd.readouterr().err
    tb._assert_same_records(fused, stepwise, f"{mode}: fused against {unfused}")
    tb._assert_same_env(x, y, f"{mode}: fused against {unfused}")
    assert fused["episodes"].sum() > (N if mode else 0)
    x.close()
    y.close()


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_backtest_over_the_materialised_actions_gives_the_same_records(mode):
    """The parent's feature as the yardstick: the [K, N] actions twin a's lookups produced, fed to
    backtest() on a third twin."""
    import torch
    data, tables, kw = tb._data(37, T, 6)[:2], _table(8, 7, T), dict(BASE, windows=5)
    a, b, gen = _prepare(data, tables, mode, kw)
    c = tb._env(data, N, mode, **kw)  # no table bound: it is given the actions
    c.reset()
    gen3 = torch.Generator(device="cuda")
    gen3.manual_seed(17)
    tb._phase(c, _Null(), N, 3, gen3)  # the steps and masked resets a and b went through
    lookups = _HostLookup(a, tables, None, K)
    tb._single_step_columns(a, lookups)
    got = b.backtest_signals(K).numpy()
    ref = c.backtest(torch.from_numpy(np.stack(lookups.rows)).cuda()).numpy()
    tb._assert_same_records(got, ref, f"{mode}: backtest_signals against backtest(acts)")
    tb._assert_same_env(b, c, f"{mode}: backtest_signals against backtest(acts)")
    for e in (a, b, c):
        e.close()


class _Null:
    """Stands in for the second twin of tb._phase / tb._both: every call is dropped."""
    def reset(self, **kw):
        pass

    def step(self, a):
        pass


@pytest.mark.parametrize("explicit", [False, True])
def test_signal_actions_equals_the_host_model(explicit):
    import torch
    tables = _table(12, 7, T)
    strategy = _strategy(explicit, N, 7)
    env = tb._env(tb._data(38, T, 6)[:2], N, "same_step", **dict(BASE, windows=5, max_episode_duration=6))
    env.bind_signals(tables)
    host = lambda: sm.lookup(tables, strategy, env.state("idx"), env.state("dataset_index"), 3)
    env.reset()
    got = env.signal_actions(strategy)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (N,)
    np.testing.assert_array_equal(got.cpu().numpy(), host(), err_msg="after reset")
    env.step(got)
    np.testing.assert_array_equal(env.signal_actions(strategy).cpu().numpy(), host(), err_msg="after a step")
    out = torch.empty(N, dtype=torch.int32, device="cuda")
    ended = 0
    for _ in range(8):  # 6-step episodes: same-step terminal steps (the env is already on its new row)
        assert env.signal_actions(strategy, out=out) is out
        _, _, term, trunc, _ = env.step(out)
        ended += int((term | trunc).sum())
        np.testing.assert_array_equal(env.signal_actions(strategy).cpu().numpy(), host(),
                                      err_msg="after a same-step terminal step")
    assert ended >= N
    assert set(np.unique(host())) == {-1, 0, 1, 2}
    env.close()


def test_signal_actions_captured_with_step_replays_like_eager():
    import torch
    tables = _table(13, 7, T)
    kw = dict(BASE, windows=5, max_episode_duration=10)
    data = tb._data(39, T, 6)[:2]
    eager, graphed = tb._env(data, N, "next_step", **kw), tb._env(data, N, "next_step", **kw)
    tb._both(eager, graphed, lambda e: e.bind_signals(tables))
    tb._both(eager, graphed, lambda e: e.reset())
    buf = torch.empty(N, dtype=torch.int32, device="cuda")
    g = graphed.capture_steps(lambda i: graphed.step(graphed.signal_actions(out=buf)), 4)
    np.testing.assert_array_equal(graphed.state("step"), 0)  # the capture ran nothing
    for _ in range(6):  # 24 steps: every env through two episodes
        for _ in range(4):
            eager.step(eager.signal_actions())
        g.replay()
        tb._assert_same_env(eager, graphed, "replay against eager")
    assert (eager.state("episode") >= 2).all()
    eager.close()
    graphed.close()


@pytest.mark.parametrize("name", ["signal_trace", "signal_trace_multi"])
def test_backtest_signals_against_the_reference_fixture(name):
    """The reference driven closed-loop by the tables (tests/golden/make_signal_golden.py): with its
    draws injected, backtest_signals ends on the fixture's final rows, and the records are the model's
    over the reference's own columns — integers and the fields made of valuations by value, the three
    reward sums within the bound test_gpu_backtest derives (B ulp per reward, one rounding per
    addition on either side)."""
    from gym_trading_env_amd.batched import BatchedTradingEnv
    g = replay.load(name)
    Kc, E = g["op"].shape
    kw = replay.config_kwargs(g)
    for k in ("n_envs", "n_static", "n_datasets"):
        kw.pop(k)
    sets = g["datasets"] if len(g["datasets"]) > 1 else g["datasets"][0]
    env = BatchedTradingEnv(sets, num_envs=E, **kw)
    env.bind_signals(sm.trace_tables(g))
    q, n = replay.injection_queue(g)
    env.set_autoreset_injection(q["idx"], q["pos_index"], q["dataset"])
    env.reset(inject_idx=g["idx"][0], inject_position_index=g["pos_index"][0], inject_dataset=g["dataset"][0])
    got = env.backtest_signals(Kc - 1, strategy=g["strategy"]).numpy()
    for f, s in (("idx", "idx"), ("step", "step"), ("pos_index", "position_index"), ("dataset", "dataset_index")):
        np.testing.assert_array_equal(env.state(s), g[f][Kc - 1], err_msg=f)
    replay.assert_same_value(env.state("portfolio_valuation"), g["portfolio_valuation"][Kc - 1], "final valuation")
    B = replay.reward_ulp_bound(g)
    for e in range(E):
        rec = bm.new_record(g["portfolio_valuation"][0, e], g["position"][0, e])
        bound, largest, adds = 0.0, 0.0, 0
        for s in bm.trace_steps(g, e):
            eps = rec["episodes"]
            bm.run(rec, [s])
            if s["stepped"]:
                bound += B * np.spacing(abs(np.float64(s["r"])))
                adds += 1 + (rec["episodes"] - eps)
                largest = max(largest, abs(rec["reward_sum"]), abs(rec["cur_return"]), abs(rec["ep_return_sum"]))
        bound += adds * np.spacing(np.float64(largest))
        for f in bm.INT_FIELDS:
            assert got[f][e] == rec[f], (name, e, f, got[f][e], rec[f])
        for f in ("peak", "max_drawdown", "valuation_last", "prev_position"):
            assert replay.same_value(np.array([got[f][e]]), np.array([rec[f]])).all(), (name, e, f, got[f][e], rec[f])
        for f in ("reward_sum", "cur_return", "ep_return_sum"):
            d = abs(got[f][e] - rec[f])
            print(f"{name} env {e} {f}: |difference| {d:.3e}, bound {bound:.3e}")
            assert d <= bound, (name, e, f, got[f][e], rec[f], bound)
    assert got["episodes"].sum() >= 3 * E
    env.close()


def _bind_raw(env, d, ptr, S, stride):
    return env._lib.gte_bind_signals(env._h, d, C.c_void_p(ptr) if ptr else None, S, stride)


def test_refusals_leave_env_and_records_untouched():
    import torch
    from gym_trading_env_amd.batched import BatchedTradingEnv
    sets = [tb._data(60 + d, 200 + 40 * d, 6)[:2] for d in range(2)]
    tables = [_table(70 + d, 5, len(c)) for d, (_, c) in enumerate(sets)]
    kw = dict(BASE, windows=4, episodes_between_dataset_switch=1)
    env, twin = tb._env(sets, 64, "next_step", **kw), tb._env(sets, 64, "next_step", **kw)
    tb._both(env, twin, lambda e: e.reset())
    lib, h = env._lib, env._h
    err = lambda: lib.gte_last_error().decode()
    ptr = C.c_void_p()
    out = torch.full((64,), -7, dtype=torch.int32, device="cuda")

    def refused(status, text):
        """both calls return `status` with `text`; nothing moved"""
        assert lib.gte_backtest_signals(h, None, 3, 1, C.byref(ptr)) == status and text in err(), err()
        assert lib.gte_signal_actions(h, None, C.c_void_p(out.data_ptr())) == status and text in err(), err()
        assert (out == -7).all()
        tb._assert_same_env(env, twin, text)

    # no table bound; one of two bound
    refused(_abi.GTE_ERR_STATE, "dataset 0 has no signal table")
    with pytest.raises(_abi.GteError, match="no signal table"):
        env.backtest_signals(3)
    env.bind_signals(tables[0], dataset=0)
    refused(_abi.GTE_ERR_STATE, "dataset 1 has no signal table")
    # wrong T, mismatched S: refused in Python and by the ABI
    with pytest.raises(ValueError, match="columns"):
        env.bind_signals(tables[0], dataset=1)
    with pytest.raises(ValueError, match="one number of strategies"):
        env.bind_signals(_table(1, 6, 240), dataset=1)
    with pytest.raises(ValueError, match="fit int8"):
        env.bind_signals(np.full((5, 240), 300), dataset=1)
    buf = torch.zeros((6, 256 + 16), dtype=torch.int8, device="cuda")
    base = buf.data_ptr()
    assert base % 16 == 0
    assert _bind_raw(env, 1, base, 6, 256) == _abi.GTE_ERR_INVALID and "n_strategies 6" in err()
    assert _bind_raw(env, 1, base, 5, 224) == _abi.GTE_ERR_INVALID and "row_stride" in err()  # < round_up(240, 16)
    assert _bind_raw(env, 1, base, 5, 248) == _abi.GTE_ERR_INVALID and "row_stride" in err()  # no multiple of 16
    assert _bind_raw(env, 1, base + 8, 5, 256) == _abi.GTE_ERR_INVALID and "16-byte aligned" in err()
    assert _bind_raw(env, 1, base, 0, 256) == _abi.GTE_ERR_INVALID and "n_strategies" in err()
    assert _bind_raw(env, 2, base, 5, 256) == _abi.GTE_ERR_INVALID and "out of range" in err()
    refused(_abi.GTE_ERR_STATE, "dataset 1 has no signal table")
    # a host strategy outside [0, S)
    env.bind_signals(tables[1], dataset=1)
    twin.bind_signals(tables)
    with pytest.raises(IndexError, match="outside"):
        env.backtest_signals(3, strategy=np.full(64, 5))
    with pytest.raises(ValueError, match="shape"):
        env.signal_actions(strategy=np.zeros(63, np.int32))
    # n_steps < 1
    assert lib.gte_backtest_signals(h, None, 0, 1, C.byref(ptr)) == _abi.GTE_ERR_INVALID and "n_steps must be >= 1" in err()
    tb._assert_same_env(env, twin, "n_steps = 0")
    # now it runs, like the twin
    tb._assert_same_records(env.backtest_signals(7).numpy(), twin.backtest_signals(7).numpy(), "bound")
    before = env.backtest_signals(5).numpy().copy()
    twin.backtest_signals(5)
    # inside a stream capture: refused with its reason (the capture fails, the env works on)
    seen = []

    def body(i):
        try:
            env.backtest_signals(2)
        except _abi.GteError as e:
            seen.append(e)
            raise
    with pytest.raises(Exception):
        env.capture_steps(body, 2)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].status == _abi.GTE_ERR_STATE and "stream capture" in str(seen[0])
    # after the dataset was uploaded again its table is unbound
    env.upload_dataset(1, env.datasets[1])
    refused(_abi.GTE_ERR_STATE, "dataset 1 has no signal table")
    assert 1 not in env._signals
    tb._assert_same_records(_stats(env), before, "records after the refusals")
    # unbinding: None
    env.bind_signals(None)
    refused(_abi.GTE_ERR_STATE, "dataset 0 has no signal table")
    env.bind_signals(tables)
    tb._assert_same_records(env.backtest_signals(4).numpy(), twin.backtest_signals(4).numpy(), "bound again")
    tb._assert_same_env(env, twin, "bound again")
    env.close()
    twin.close()
    # before gte_reset; another output mode
    fresh = tb._env(sets, 8, "next_step", **kw)
    fresh.bind_signals(tables)
    with pytest.raises(_abi.GteError, match="before gte_reset"):
        fresh.backtest_signals(2)
    fresh.close()
    host = BatchedTradingEnv(sets[0], num_envs=4, positions=[0, 1], windows=4, output="numpy")
    with pytest.raises(ValueError, match="needs output='torch'"):
        host.bind_signals(tables[0])
    host.close()


def _stats(env):
    rec = np.empty(env.num_envs, np.dtype(_abi.BACKTEST_DTYPE))
    _abi.check(env._lib, env._lib.gte_read_backtest_stats(env._h, 0, env.num_envs, rec.ctypes.data))
    return rec


def test_signals_example(capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import backtest_signals
    mean = backtest_signals.main(strategies=64, replicas=4, K=400, duration=48)
    assert mean.shape == (64,) and np.isfinite(mean).all() and mean.std() > 0
    out = capsys.readouterr().out
    assert "mean episode return" in out and "random starts" in out
