"""`backtest()` (gte_backtest: K steps that leave one statistics record per env,
csrc/gte_backtest.hip) against the model of tests/backtest_model.py run over what K single
`step()` calls of a twin env return, bit for bit; chunked calls; the fused path against the
step-by-step one; the reference's golden traces; refusals; the example."""
import os
import sys

import numpy as np
import pytest

import backtest_model as bm
import backtest_trace
import replay
from gym_trading_env_amd import _abi

pytestmark = pytest.mark.gpu

STATE = ("idx", "step", "position_index", "dataset_index", "start_idx", "episode", "needs_reset",
         "asset", "fiat", "interest_asset", "interest_fiat", "portfolio_valuation", "real_position")
MODES = [None, "next_step", "same_step"]


def _data(seed, T, Fs, sigma=1e-2, drift=0.0):
    rng = np.random.default_rng(seed)
    close = 100 * np.exp(np.cumsum(rng.normal(drift, sigma, T)))
    feat = rng.normal(0, 1, (T, Fs)).astype(np.float32)
    return feat, close, close * 1.004, close * 0.996


def _env(data, N, mode, final_obs=False, **kw):
    from gym_trading_env_amd.batched import BatchedTradingEnv
    return BatchedTradingEnv(data, num_envs=N, autoreset=mode, final_obs=final_obs, **kw)


def _twins(data, N, mode, **kw):
    """(a, b): a takes single steps — in same-step mode with final_obs, whose terminal records
    hold the terminal valuation; b runs backtest()."""
    a = _env(data, N, mode, final_obs=(mode == "same_step"), **kw)
    b = _env(data, N, mode, **kw)
    return a, b


def _both(a, b, f):
    f(a)
    f(b)


def _phase(a, b, N, P, gen, steps=6):
    """Single steps with a third of the envs reset again now and then: episodes out of phase."""
    import torch
    for i in range(steps):
        if i in (1, 3):
            mask = (np.arange(N) % 3 == i // 2).astype(np.uint8)
            _both(a, b, lambda e: e.reset(mask=mask))
        one = torch.randint(-1, P, (N,), dtype=torch.int32, device="cuda", generator=gen)
        _both(a, b, lambda e: e.step(one))


def _single_step_columns(a, acts):
    """K single steps of env a -> (records cleared at the state before them, step dicts per env):
    what the issue of this feature lists — step, position index, portfolio_valuation and
    needs_reset of the record, reward64 and the flags, the terminal valuation from final_state."""
    N, mode = a.num_envs, a.cfg.autoreset
    positions = np.asarray(a.positions, np.float64)
    prev_step, prev_nr = a.state("step"), a.state("needs_reset")
    recs = [bm.new_record(v, positions[p], ended=bool(nr))
            for v, p, nr in zip(a.state("portfolio_valuation"), a.state("position_index"), prev_nr)]
    steps = [[] for _ in range(N)]
    for k in range(acts.shape[0]):
        a.step(acts[k])
        step, pos, pv, nr = (a.state(f) for f in ("step", "position_index", "portfolio_valuation", "needs_reset"))
        r, term, trunc = (a.read_output(f) for f in ("reward64", "terminated", "truncated"))
        if mode == _abi.AUTORESET_SAME_STEP:
            fpv, fpos = a.final_state("portfolio_valuation"), a.final_state("position_index")
        for e in range(N):
            if prev_nr[e] and mode == _abi.AUTORESET_NEXT_STEP:
                s = dict(stepped=False, reset=True, v0=pv[e], p0=positions[pos[e]])
            elif prev_nr[e] and step[e] == prev_step[e]:
                s = dict(stepped=False)  # frozen on the last row
            else:
                s = dict(stepped=True, v=pv[e], p=positions[pos[e]], r=r[e], terminated=bool(term[e]),
                         truncated=bool(trunc[e]))
                if mode == _abi.AUTORESET_SAME_STEP and (term[e] or trunc[e]):
                    s.update(v=fpv[e], p=positions[fpos[e]], reset=True, v0=pv[e], p0=positions[pos[e]])
            steps[e].append(s)
        prev_step, prev_nr = step, nr
    return recs, steps


def _assert_records(stats, want, tag):
    """A BacktestStats (or its numpy() array) against model records, every field bit for bit."""
    got = stats if isinstance(stats, np.ndarray) else stats.numpy()
    ref = bm.as_arrays(want)
    for f in bm.INT_FIELDS:
        np.testing.assert_array_equal(got[f], ref[f], err_msg=f"{tag}: {f}")
    for f in bm.F64_FIELDS:
        replay.assert_same_value(np.ascontiguousarray(got[f]), ref[f], f"{tag}: {f}")


def _assert_same_records(x, y, tag):
    for f in x.dtype.names:
        if x[f].dtype.kind == "f":
            replay.assert_same_value(np.ascontiguousarray(x[f]), np.ascontiguousarray(y[f]), f"{tag}: {f}")
        else:
            np.testing.assert_array_equal(x[f], y[f], err_msg=f"{tag}: {f}")


def _assert_same_env(a, b, tag):
    for f in STATE:
        np.testing.assert_array_equal(a.state(f), b.state(f), err_msg=f"{tag}: {f}")
    for f in ("reward", "reward64", "terminated", "truncated", "obs"):
        np.testing.assert_array_equal(a.read_output(f), b.read_output(f), err_msg=f"{tag}: {f}")
    np.testing.assert_array_equal(a.terminal_ids(), b.terminal_ids(), err_msg=f"{tag}: terminal ids")


def _against_single_steps(data, N, K, mode, kw, tag, before=None):
    """-> (records, step dicts): twin a by single steps and the model, twin b by backtest()."""
    import torch
    a, b = _twins(data, N, mode, **kw)
    _both(a, b, lambda e: e.reset())
    P = len(kw["positions"])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    _phase(a, b, N, P, gen)
    if before:
        _both(a, b, before)
    acts = torch.randint(-1, P, (K, N), dtype=torch.int32, device="cuda", generator=gen)
    recs, steps = _single_step_columns(a, acts)
    want = [bm.run(r, s) for r, s in zip(recs, steps)]
    stats = b.backtest(acts)
    _assert_records(stats, want, tag)
    # the views show the same records as the one-transfer read
    np.testing.assert_array_equal(stats.steps.cpu().numpy(), stats.numpy()["steps"])
    assert replay.same_value(stats.max_drawdown.cpu().numpy(), stats.numpy()["max_drawdown"]).all()
    _assert_same_env(a, b, tag)
    # ... and the rings too: the steps that follow agree
    one = torch.randint(-1, P, (N,), dtype=torch.int32, device="cuda", generator=gen)
    for x, y in zip(a.step(one)[:4], b.step(one)[:4]):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=f"{tag}: the step after")
    a.close()
    b.close()
    return want, steps


BASE = dict(positions=[-1, 0, 1], windows=3, trading_fees=1e-3, borrow_interest_rate=1e-4,
            max_episode_duration=5, seed=11)


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
@pytest.mark.parametrize("K", [1, 2, 23])
@pytest.mark.parametrize("N", [1, 33, 129, 257])
def test_backtest_equals_model_over_single_steps(N, K, mode):
    """The lane, wave and workgroup edges of 32 envs per wave x 4 waves; K = 1 has no fused step.
    T = 40 rows and 5-step episodes: several episodes per env, next-step reset rows and, with
    auto-reset off, envs frozen on the last row."""
    want, steps = _against_single_steps(_data(1, 40, 6)[:2], N, K, mode, BASE, f"N={N} K={K} {mode}")
    if K == 23 and N >= 33:
        # (auto-reset off: an env ends one episode per reset() and is not reset inside the call)
        assert sum(r["episodes"] for r in want) > (N if mode else 0)
        if mode == "next_step":
            assert any(s.get("reset") and not s["stepped"] for e in steps for s in e)
        if mode is None:
            assert any(not s["stepped"] for e in steps for s in e), "no env froze on the last row"


CASES = {
    "nowindow": (lambda: _data(2, 40, 6)[:2], dict(BASE, windows=None), None),
    "window7": (lambda: _data(3, 60, 14)[:2], dict(BASE, windows=7), None),
    "fobs_not_multiple_of_4": (lambda: _data(4, 40, 3)[:2], dict(BASE), None),
    "three_datasets": (lambda: [_data(20 + d, 40 + 3 * d, 6)[:2] for d in range(3)],
                       dict(BASE, episodes_between_dataset_switch=1), None),
    "limit_orders": (lambda: _data(5, 60, 6, sigma=1.5e-2), dict(BASE, max_episode_duration=9), "orders"),
}


def _add_orders(env):
    rng = np.random.default_rng(3)
    N = env.num_envs
    close = env.datasets[0].close
    limit = close[env.state("idx")] * rng.uniform(0.995, 1.005, N)
    env.add_limit_order(rng.integers(0, 3, N).astype(np.int32), limit, np.ones(N, np.uint8))


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
@pytest.mark.parametrize("name", sorted(CASES))
def test_backtest_cases_equal_model_over_single_steps(name, mode):
    data, kw, before = CASES[name]
    want, steps = _against_single_steps(data(), 129, 23, mode, kw, f"{name} {mode}",
                                        before=_add_orders if before else None)
    assert sum(r["episodes"] for r in want) > 0
    if name == "limit_orders":
        assert sum(r["trades"] for r in want) > 0


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_backtest_with_crashing_prices(mode):
    """Prices that fall fast under positions [-1, 0, 2]: the 0.7 rule ends episodes; with
    auto-reset off the envs go on stepping after done."""
    kw = dict(BASE, positions=[-1, 0, 2], max_episode_duration=30, trading_fees=1e-2)
    want, steps = _against_single_steps(_data(6, 80, 6, sigma=0.12, drift=-0.04)[:2], 129, 23, mode, kw,
                                        f"crash {mode}")
    assert sum(r["terminations"] for r in want) > 0, "the data ended no episode by the 0.7 rule"
    if mode is None:
        def steps_after_done(e):
            done = False
            for s in e:
                if s["stepped"] and done:
                    return True
                done = done or (s["stepped"] and (s["terminated"] or s["truncated"]))
            return False
        assert any(steps_after_done(e) for e in steps), "no env kept stepping after done"


def _pair(mode, N=129, **over):
    import torch
    kw = dict(BASE, **over)
    data = _data(7, 60, 6)[:2]
    x, y = _env(data, N, mode, **kw), _env(data, N, mode, **kw)
    _both(x, y, lambda e: e.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    _phase(x, y, N, 3, gen)
    acts = torch.randint(-1, 3, (23, N), dtype=torch.int32, device="cuda", generator=gen)
    return x, y, acts


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_backtest_in_chunks(mode):
    x, y, a = _pair(mode)
    whole = x.backtest(a).numpy()
    y.backtest(a[:9])
    _assert_same_records(y.backtest(a[9:], resume=True).numpy(), whole, f"{mode}: 9 + 14 steps resumed")
    _assert_same_env(x, y, f"{mode}: chunks")
    assert whole["steps"].sum() > 0 and whole["episodes"].sum() > 0
    # resume=False: the second chunk alone, from the state the first left
    x.reset()
    y.reset()
    x.backtest(a[:9])
    second = x.backtest(a[9:]).numpy()
    for k in range(9):
        y.step(a[k])
    _assert_same_records(y.backtest(a[9:]).numpy(), second, f"{mode}: second chunk alone")
    assert (second["steps"] <= 14).all()
    x.close()
    y.close()


def test_reset_between_chunks_restarts_peak_and_position_and_keeps_the_sums():
    x, y, a = _pair("next_step")
    first = x.backtest(a[:9]).numpy().copy()
    x.reset()
    got = x.backtest(a[9:], resume=True).numpy()
    # the model: the first chunk's record, a reset row at the env's state after reset(), the rest
    y.backtest(a[:9])
    y.reset()
    positions = np.asarray(y.positions, np.float64)
    v0, p0 = y.state("portfolio_valuation"), positions[y.state("position_index")]
    recs, steps = _single_step_columns(y, a[9:])
    want = []
    for e in range(y.num_envs):
        r = {f: first[f][e] for f in bm.F64_FIELDS}
        r.update({f: int(first[f][e]) for f in bm.INT_FIELDS})
        r["ended"] = bool(first["ended"][e])
        bm.reset(r, v0[e], p0[e])
        want.append(bm.run(r, steps[e]))
    _assert_records(got, want, "reset between chunks")
    assert (got["steps"] >= first["steps"]).all() and (got["steps"] > first["steps"]).any()
    assert replay.same_value(got["reward_sum"], first["reward_sum"]).mean() < 1  # the sums went on
    x.close()
    y.close()


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_fused_and_per_step_paths_give_the_same_records(mode, capfd, monkeypatch):
    """kernel_variant = KV_ROLLOUT_PER_STEP: every step is a step launch folded in by
    gte_backtest_fold_kernel; the default runs K - 1 steps in gte_backtest_kernel."""
    import torch
    monkeypatch.setenv("GTE_DEBUG_GEOMETRY", "1")
    data = _data(8, 60, 6)[:2]
    N = 257
    x = _env(data, N, mode, **BASE)
    y = _env(data, N, mode, **dict(BASE, kernel_variant=_abi.KV_ROLLOUT_PER_STEP))
    _both(x, y, lambda e: e.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(29)
    _phase(x, y, N, 3, gen)
    acts = torch.randint(-1, 3, (23, N), dtype=torch.int32, device="cuda", generator=gen)
    capfd.readouterr()
    fused = x.backtest(acts).numpy()
    assert "rollout path: backtest summary, 23 steps" in capfd.readouterr().err
    stepwise = y.backtest(acts).numpy()
    assert "rollout path: backtest per-step, 23 steps" in capfd.readouterr().err
    _assert_same_records(fused, stepwise, f"{mode}: fused against per-step")
    _assert_same_env(x, y, f"{mode}: fused against per-step")
    assert fused["episodes"].sum() > (N if mode else 0)
    x.close()
    y.close()


@pytest.mark.parametrize("name", ["c2_nowindow", "drawdown_done", "limit_orders"])
def test_backtest_against_the_reference_trace(name):
    """backtest() driven by the trace's actions and injected draws (as replay.replay drives
    step()), against the model over the REFERENCE's own columns.  Integers exact; peak,
    max_drawdown and valuation_last by value (the valuations are held bit for bit on these traces,
    and the fields are comparisons and one division of them); the three reward sums within a bound
    derived here: each reward lies within B = replay.reward_ulp_bound ulp of the trace's, and each
    addition rounds once on either side (half an ulp each, of a partial sum no larger than the
    largest one) -> sum_t B ulp(|r_t|) + (additions) ulp(largest partial sum).  The two sums of squares
    within the bounds backtest_trace.run_with_bounds derives for them by the same rule: a square r'^2 lies
    within (2 |r| + e) e of r^2 for a reward within e, and is rounded once more on either side."""
    import torch
    from gym_trading_env_amd.batched import BatchedTradingEnv
    g = replay.load(name)
    K, E = g["op"].shape
    kw = replay.config_kwargs(g)
    for k in ("n_envs", "n_static", "n_datasets"):
        kw.pop(k)
    env = BatchedTradingEnv(g["datasets"][0], num_envs=E, **kw)
    q, n = replay.injection_queue(g)
    if n:
        env.set_autoreset_injection(q["idx"], q["pos_index"], q["dataset"])
    env.reset(inject_idx=g["idx"][0], inject_position_index=g["pos_index"][0], inject_dataset=g["dataset"][0])
    acts = torch.from_numpy(np.ascontiguousarray(g["action"].astype(np.int32))).cuda()
    # chunks end where the reference added limit orders (before the call they precede)
    cuts = [k for k in range(2, K) if "lo_pos" in g and (g["lo_pos"][k] >= 0).any()]
    lo, stats = 1, None
    for hi in cuts + [K]:
        if "lo_pos" in g and (g["lo_pos"][lo] >= 0).any():
            env.add_limit_order(g["lo_pos"][lo], g["lo_limit"][lo], np.ones(E, np.uint8))
        stats = env.backtest(acts[lo:hi], resume=lo > 1)
        lo = hi
    got = stats.numpy()
    np.testing.assert_array_equal(env.state("idx"), g["idx"][K - 1])
    B = replay.reward_ulp_bound(g)
    worst = 0.0
    whole, sq_bounds, _ = backtest_trace.chunk_records(g, 1, K)
    for e in range(E):
        for f in ("reward_sq_sum", "ep_return_sq_sum"):
            d, b = abs(got[f][e] - whole[e][f]), sq_bounds[e][f]
            print(f"{name} env {e} {f}: |difference| {d:.3e}, bound {b:.3e}, ratio {d / b:.4f}")
            assert np.isfinite(whole[e][f]) and d <= b, (name, e, f, got[f][e], whole[e][f], b)
            worst = max(worst, d / b)
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
            print(f"{name} env {e} {f}: |difference| {d:.3e}, bound {bound:.3e}, ratio {d / bound:.4f}")
            worst = max(worst, d / bound)
            assert d <= bound, (name, e, f, got[f][e], rec[f], bound)
    print(f"{name}: largest distance {worst:.4f} of the bound")
    assert got["episodes"].sum() > 0
    env.close()


def test_backtest_errors_and_refusals():
    import ctypes as C
    import torch
    from gym_trading_env_amd.batched import BatchedTradingEnv
    feat, close = _data(9, 200, 6)[:2]
    env = BatchedTradingEnv((feat, close), num_envs=64, positions=[0, 1], windows=4)
    acts = torch.zeros((3, 64), dtype=torch.int32, device="cuda")
    lib, h = env._lib, env._h
    ptr = C.c_void_p()
    err = lambda: lib.gte_last_error().decode()
    assert lib.gte_backtest(h, C.c_void_p(acts.data_ptr()), 3, 1, C.byref(ptr)) == _abi.GTE_ERR_STATE
    assert "gte_backtest before gte_reset" in err()
    with pytest.raises(_abi.GteError, match="before gte_reset"):
        env.backtest(acts)
    env.reset()
    assert lib.gte_backtest(None, C.c_void_p(acts.data_ptr()), 3, 1, C.byref(ptr)) == _abi.GTE_ERR_INVALID
    assert "env is NULL" in err()
    assert lib.gte_backtest(h, None, 3, 1, C.byref(ptr)) == _abi.GTE_ERR_INVALID
    assert "actions is NULL" in err()
    assert lib.gte_backtest(h, C.c_void_p(acts.data_ptr()), 0, 1, C.byref(ptr)) == _abi.GTE_ERR_INVALID
    assert "n_steps must be >= 1" in err()
    rec = np.empty(64, np.dtype(_abi.BACKTEST_DTYPE))
    assert lib.gte_read_backtest_stats(h, 0, 64, rec.ctypes.data) == _abi.GTE_ERR_STATE
    assert "before gte_backtest" in err()
    with pytest.raises(ValueError, match="expected actions of shape"):
        env.backtest(torch.zeros((3, 63), dtype=torch.int32, device="cuda"))
    with pytest.raises(IndexError):
        env.backtest(np.full((2, 64), 5))
    # inside a stream capture: refused with its reason (the capture fails, the env works on)
    seen = []

    def body(i):
        try:
            env.backtest(acts)
        except _abi.GteError as e:
            seen.append(e)
            raise
    with pytest.raises(Exception):
        env.capture_steps(body, 2)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].status == _abi.GTE_ERR_STATE
    assert "stream capture" in str(seen[0]) and "one launch already" in str(seen[0])
    stats = env.backtest([[None] * 64, [1] * 64])  # None = hold, like step(); the stats pointer is stable
    assert stats.steps.shape == (64,) and (stats.steps == 2).all()
    assert lib.gte_read_backtest_stats(h, 60, 5, rec.ctypes.data) == _abi.GTE_ERR_INVALID
    assert "outside" in err()
    clipped = BatchedTradingEnv((feat, close), num_envs=4, positions=[0, 1], windows=4,
                                reward_function=("clipped_log_return", 1.0, -0.002, 0.005))
    clipped.reset()
    with pytest.raises(ValueError, match="log-return reward"):
        clipped.backtest(torch.zeros((1, 4), dtype=torch.int32, device="cuda")).total_return
    clipped.close()
    env.close()
    # Python callables need step(), like rollout()
    env = BatchedTradingEnv((feat, close), num_envs=4, positions=[0, 1], windows=4,
                            reward_function=lambda h: h["portfolio_valuation", -1] * 0)
    env.reset()
    with pytest.raises(NotImplementedError, match="callables need step"):
        env.backtest(torch.zeros((1, 4), dtype=torch.int32, device="cuda"))
    env.close()
    env = BatchedTradingEnv((feat, close), num_envs=4, positions=[0, 1], windows=4, output="numpy")
    with pytest.raises(ValueError, match="needs output='torch'"):
        env.backtest([[0] * 4])
    env.close()


def test_derived_statistics():
    import torch
    from gym_trading_env_amd.batched import BatchedTradingEnv
    import gym_trading_env_amd as gte
    feat, close = _data(10, 300, 6)[:2]
    env = BatchedTradingEnv((feat, close), num_envs=96, positions=[-1, 0, 1], windows=4, max_episode_duration=12,
                            seed=2)
    env.reset()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    acts = torch.randint(-1, 3, (40, 96), dtype=torch.int32, device="cuda", generator=gen)
    out = env.rollout(acts, reward64=True)
    twin = BatchedTradingEnv((feat, close), num_envs=96, positions=[-1, 0, 1], windows=4, max_episode_duration=12,
                             seed=2)
    twin.reset()
    stats = twin.backtest(acts)
    assert isinstance(stats, gte.BacktestStats)
    r = out["reward64"].cpu().numpy()
    stepped = np.ones_like(r, bool)
    ended = (out["terminated"] | out["truncated"]).cpu().numpy()
    stepped[1:] = ~ended[:-1]  # next-step mode: the step after an end is the reset step
    n = stepped.sum(0)
    np.testing.assert_array_equal(stats.steps.cpu().numpy(), n)
    mean = (r * stepped).sum(0) / n
    np.testing.assert_allclose(stats.mean_reward.cpu().numpy(), mean, rtol=1e-9, atol=1e-15)
    std = np.sqrt(np.maximum(((r * stepped) ** 2).sum(0) / n - mean ** 2, 0))
    np.testing.assert_allclose(stats.reward_std.cpu().numpy(), std, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(stats.sharpe(365).cpu().numpy(), mean / std * np.sqrt(365), rtol=1e-6)
    np.testing.assert_allclose(stats.total_return.cpu().numpy(), np.exp((r * stepped).sum(0)), rtol=1e-9)
    eps = stats.episodes.cpu().numpy()
    assert (eps > 0).all()
    np.testing.assert_allclose(stats.mean_episode_return.cpu().numpy(),
                               stats.ep_return_sum.cpu().numpy() / eps, rtol=1e-12)
    env.close()
    twin.close()


def test_backtest_example(capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import backtest_rollout
    final = backtest_rollout.main(strategies=512, K=800)
    assert final.shape == (512,) and np.isfinite(final).all() and final.std() > 0
    out = capsys.readouterr().out
    assert "max drawdown" in out and "trades" in out
