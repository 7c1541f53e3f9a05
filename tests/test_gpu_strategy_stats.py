"""Per-strategy statistics and ranking on the device (`gte_reduce_backtest_stats`, `gte_rank_strategies`)
against tests/strategy_model.py: crafted records through both reduction kernels byte for byte, the real
pipeline at a small shape, the scores, the ranking given the device's own scores, and the refusals.

Square-root scores (SHARPE, EPISODE_SHARPE): on an MI355X 0 of this file's scores differ from NumPy's
(division and square root are correctly rounded on both sides), so they are held equal like the others."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import strategy_model as sm
from gym_trading_env_amd import _abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FIX = 2048


def _env(N, T=300, env_id_base=0, seed=4, **kw):
    import gym_trading_env_amd as gte
    rng = np.random.default_rng(11)
    close = 100.0 * np.exp(np.cumsum(rng.normal(0, 1e-2, T)))
    feat = rng.normal(0, 1, (T, 3)).astype(np.float32)
    args = dict(positions=[-1, 0, 1], windows=None, trading_fees=1e-4, borrow_interest_rate=3e-6,
                max_episode_duration=20, autoreset="next_step", seed=seed, env_id_base=env_id_base)
    args.update(kw)
    return gte.BatchedTradingEnv((feat, close), num_envs=N, **args)


@pytest.fixture(scope="module")
def envs():
    made = {}

    def get(N, base=0):
        if (N, base) not in made:
            made[(N, base)] = _env(N, env_id_base=base)
        return made[(N, base)]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def crafted():
    return sm.craft_records(N_FIX, seed=0)


def _check(got, want, what):
    assert got.dtype == sm.STRATEGY and got.shape == want.shape
    if not sm.same_bytes(got, want):
        bad = [(s, n) for s in range(len(want)) for n in want.dtype.names
               if sm.canonical(got[s:s + 1])[n].tobytes() != sm.canonical(want[s:s + 1])[n].tobytes()]
        pytest.fail(f"{what}: {len(bad)} fields differ, first {bad[:5]}: "
                    f"{[(got[n][s], want[n][s]) for s, n in bad[:5]]}")


# ---- crafted records through from_records -----------------------------------------------------------------

@pytest.mark.parametrize("base", [0, 7])
@pytest.mark.parametrize("S", [1, 3, 64, 65, N_FIX, N_FIX + 5])
def test_default_map_records_equal_the_model(envs, crafted, S, base):
    """S = 1, 3, 64: a workgroup per strategy (N >= 32 S); 65, N, N + 5: eight strategies per wavefront; N % S
    != 0 except for S = 1, 64, N; S = N + 5 leaves five strategies empty"""
    from gym_trading_env_amd import StrategyStats
    env = envs(N_FIX, base)
    got = StrategyStats.from_records(env, crafted, n_strategies=S).numpy()
    _check(got, sm.reduce_vector(crafted, sm.default_groups(N_FIX, S, base)), f"S={S} base={base}")
    assert not got["reserved"].any()


@pytest.mark.parametrize("extra", [0, 40])
def test_skewed_explicit_map_records_equal_the_model(envs, extra):
    """member counts 0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600 through both kernels: 17 strategies
    over 1 636 envs run a workgroup per strategy, the same lists followed by 40 empty strategies eight per
    wavefront"""
    import torch
    from gym_trading_env_amd import StrategyStats
    m, S = sm.skewed_map(extra_strategies=extra)
    N = len(m)
    assert N == 1636 and (N >= 32 * S) == (extra == 0)
    rec = sm.craft_records(N, seed=2)
    env = envs(N)
    want = sm.reduce_vector(rec, sm.map_groups(m, S))
    _check(StrategyStats.from_records(env, rec, strategy=m, n_strategies=S).numpy(), want, "host map")
    dev = env._t["obs"].device
    raw = torch.from_numpy(rec.view(np.uint8).reshape(N, 128).copy()).to(dev)
    on_device = StrategyStats.from_records(env, raw, strategy=torch.from_numpy(m).to(dev), n_strategies=S)
    _check(on_device.numpy(), want, "device map, device records")
    assert on_device.envs.cpu().numpy().tolist() == want["envs"].tolist()
    assert on_device.trades.dtype == torch.int64 and on_device.reward_sum.dtype == torch.float64


def test_member_ids_outside_the_records_are_skipped(envs):
    """the C entry point with hand-made CSR lists: ids -1, N and 2^31 - 1 keep their place and read nothing;
    a device map with strategies outside [0, S) leaves those envs out"""
    import torch
    from gym_trading_env_amd import StrategyStats
    N, S = 200, 5
    env = envs(N)
    rec = sm.craft_records(N, seed=3)
    groups = sm.default_groups(N, S)
    groups[1][3], groups[1][9], groups[4][0] = -1, N, 2 ** 31 - 1
    offsets, members = sm.csr(groups)
    dev = env._t["obs"].device
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(N, 128).copy()).to(dev)
    d_off, d_mem = torch.from_numpy(offsets).to(dev), torch.from_numpy(members).to(dev)
    out = torch.full((S, 128), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    _abi.check(env._lib, env._lib.gte_reduce_backtest_stats(
        env._h, C.c_void_p(d_rec.data_ptr()), S, C.c_void_p(d_off.data_ptr()), C.c_void_p(d_mem.data_ptr()),
        C.c_void_p(out.data_ptr())))
    env.synchronize()
    got = out.cpu().numpy().view(sm.STRATEGY).reshape(S)
    _check(got, sm.reduce_vector(rec, groups), "skipped ids")
    assert got["envs"].tolist() == [40, 38, 40, 40, 39]
    m = torch.arange(N, device=dev, dtype=torch.int32) % 7 - 1   # strategies -1 .. 5 with S = 5
    got = StrategyStats.from_records(env, d_rec, strategy=m, n_strategies=S).numpy()
    _check(got, sm.reduce_vector(rec, sm.map_groups(m.cpu().numpy(), S)), "map outside [0, S)")


# ---- the real pipeline ---------------------------------------------------------------------------------------

def _pipeline(N=100, S=12, T=300, seed=4):
    env = _env(N, T=T, seed=seed)
    rng = np.random.default_rng(5)
    env.bind_signals(rng.integers(-1, 3, (S, T)).astype(np.int8))
    env.reset()
    return env


def _state_bytes(env):
    snap, obs = env.read_envs()
    return snap.tobytes() + obs.tobytes()


def test_pipeline_by_strategy_equals_the_model_and_changes_nothing():
    import torch
    N, S, K = 100, 12, 120
    env, twin = _pipeline(N, S), _pipeline(N, S)
    try:
        stats = env.backtest_signals(K)
        before, state = stats.numpy(), _state_bytes(env)
        assert before["episodes"].sum() > N and (before["steps"] > 0).all()
        board = stats.by_strategy()
        assert board.num_strategies == S and tuple(board.steps.shape) == (S,)
        _check(board.numpy(), sm.reduce_vector(before, sm.default_groups(N, S)), "default map")
        # derived figures are the pooled ones
        np.testing.assert_array_equal(board.mean_reward.cpu().numpy(), sm.scores_vector(board.numpy(), "mean_reward"))
        np.testing.assert_array_equal(board.mean_episode_return.cpu().numpy(),
                                      sm.scores_vector(board.numpy(), "mean_episode_return"))
        assert torch.isfinite(board.reward_std).all() and torch.isfinite(board.episode_return_std).all()
        # the call left the env's records and state alone
        assert stats.numpy().tobytes() == before.tobytes() and _state_bytes(env) == state
        # a following chunk gives what it gives without the call
        twin.backtest_signals(K)
        after = env.backtest_signals(K, resume=True)
        assert after.numpy().tobytes() == twin.backtest_signals(K, resume=True).numpy().tobytes()
        _check(after.by_strategy().numpy(), sm.reduce_vector(after.numpy(), sm.default_groups(N, S)), "second chunk")
        # a shuffled explicit map: the backtest ran with it, by_strategy() follows it
        env.reset()
        m = np.random.default_rng(9).permutation(np.arange(N) % S).astype(np.int32)
        shuffled = env.backtest_signals(K, strategy=m)
        _check(shuffled.by_strategy().numpy(), sm.reduce_vector(shuffled.numpy(), sm.map_groups(m, S)), "shuffled")
        # the same records under other maps, asked for explicitly
        _check(shuffled.by_strategy(n_strategies=7).numpy(),
               sm.reduce_vector(shuffled.numpy(), sm.default_groups(N, 7)), "n_strategies=7")
        # records of backtest(): no strategies on record
        acts = torch.zeros((4, N), dtype=torch.int32, device=env._t["obs"].device)
        plain = env.backtest(acts)
        with pytest.raises(ValueError):
            plain.by_strategy()
        _check(plain.by_strategy(n_strategies=S).numpy(), sm.reduce_vector(plain.numpy(), sm.default_groups(N, S)),
               "backtest()")
    finally:
        env.close()
        twin.close()


# ---- scores and ranking -----------------------------------------------------------------------------------------

def _board(env, stats):
    """a StrategyStats over crafted STRATEGY records (uploaded as they are)"""
    import torch
    from gym_trading_env_amd import StrategyStats
    raw = torch.from_numpy(stats.view(np.uint8).reshape(len(stats), 128).copy()).to(env._t["obs"].device)
    torch.cuda.synchronize()
    return StrategyStats(env, raw)


@pytest.mark.parametrize("S", [1, 300, 3000])
def test_scores_equal_the_model(envs, crafted, S):
    env = envs(N_FIX)
    for stats in (sm.craft_stats(S, seed=S), sm.reduce_vector(crafted, sm.default_groups(N_FIX, min(S, 65)))):
        board = _board(env, stats)
        for metric in sm.METRICS:
            got, want = board.score(metric).cpu().numpy(), sm.scores_vector(stats, metric)
            differ = int((~(np.where(np.isnan(got), np.nan, got).view(np.uint64) ==
                            np.where(np.isnan(want), np.nan, want).view(np.uint64))).sum())
            print(f"S={len(stats)} {metric}: {differ} of {len(want)} scores differ from the model")
            assert sm.same_f64(got, want), (metric, differ)
        np.testing.assert_array_equal(board.sharpe(252).cpu().numpy(),
                                      board.score("sharpe").cpu().numpy() * 252 ** 0.5)


def _rank(env, board, metric, min_episodes, k):
    import torch
    dev = env._t["obs"].device
    index = torch.full((k,), 77, dtype=torch.int32, device=dev)
    top = torch.zeros((k,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    _abi.check(env._lib, env._lib.gte_rank_strategies(
        env._h, C.c_void_p(board._records.data_ptr()), board.num_strategies, _abi.STRATEGY_METRICS.index(metric),
        min_episodes, k, C.c_void_p(index.data_ptr()), C.c_void_p(top.data_ptr()), None))
    env.synchronize()
    return index.cpu().numpy(), top.cpu().numpy()


@pytest.mark.parametrize("S,k,min_episodes", [(1, 1, 0), (1, 256, 1), (16, 5, 1), (300, 1, 1), (300, 256, 0),
                                               (300, 256, 30), (1024, 256, 1), (1025, 7, 1), (300, 40, 10 ** 9),
                                               (70000, 256, 1), (70000, 1, 45)])
def test_ranking_equals_the_model_given_the_device_scores(envs, S, k, min_episodes):
    """duplicates, +-0.0, +-inf, NaN, nobody ranked (min_episodes = 10^9), k beyond the ranked count, k = 1 and
    256, S = 1, one workgroup's 1 024 candidates exactly and one more, and 70 000 strategies (four passes)"""
    env = envs(N_FIX)
    stats = sm.craft_stats(S, seed=S + k)
    board = _board(env, stats)
    for metric in sm.METRICS if S <= 1025 else ("mean_reward", "worst_reward_sum", "episode_sharpe"):
        scores = board.score(metric).cpu().numpy()   # the device's own scores
        want_i, want_s = sm.rank_vector(stats, scores, min_episodes, k)
        got_i, got_s = _rank(env, board, metric, min_episodes, k)
        assert got_i.tolist() == want_i.tolist(), metric
        assert sm.same_f64(got_s, want_s), metric
        ranked = int(sm.ranked_mask(stats, scores, min_episodes).sum())
        index, top = board.top(k, metric, min_episodes)
        assert len(index) == len(top) == min(k, ranked) and index.cpu().numpy().tolist() == want_i[:len(index)].tolist()
    if min_episodes == 10 ** 9:
        assert set(got_i.tolist()) == {-1} and np.isnan(got_s).all()


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_refusals_and_errors(envs):
    """every refusal the two entry points can make with an env in hand.  GTE_ERR_NO_DEVICE is deliberately not
    among them: like every other device entry point they take an env, and without a gfx950 device
    `gte_create` returns that code and no env exists to call them with (tests/test_host_cpu.py holds
    gte_create to it on a host without a GPU)."""
    import torch
    from gym_trading_env_amd import StrategyStats
    fresh = _env(64)
    try:
        lib, dev = fresh._lib, fresh._t["obs"].device
        out = torch.zeros((8, 128), dtype=torch.uint8, device=dev)
        lists = torch.zeros((80,), dtype=torch.int32, device=dev)
        idx = torch.zeros((256,), dtype=torch.int32, device=dev)
        top = torch.zeros((256,), dtype=torch.float64, device=dev)
        p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
        reduce = lambda *a: lib.gte_reduce_backtest_stats(fresh._h, *a)
        rank = lambda *a: lib.gte_rank_strategies(fresh._h, *a)
        INVALID, STATE = _abi.GTE_ERR_INVALID, _abi.GTE_ERR_STATE
        # no backtest yet: the env has no records of its own
        assert reduce(None, 8, None, None, p(out)) == STATE
        assert b"before gte_backtest" in lib.gte_last_error()
        rec = torch.zeros((64, 128), dtype=torch.uint8, device=dev)
        assert reduce(p(rec), 8, None, None, p(out)) == _abi.GTE_OK
        why = lambda text: text in lib.gte_last_error()  # (each refusal for ITS reason)
        assert reduce(p(rec), 0, None, None, p(out)) == INVALID and why(b"n_strategies must be >= 1")
        assert reduce(p(rec), 8, None, None, None) == INVALID and why(b"out_device must be a 16-byte aligned")
        assert reduce(p(rec), 8, None, None, p(out, 8)) == INVALID and why(b"out_device must be a 16-byte aligned")
        assert reduce(p(rec, 8), 8, None, None, p(out)) == INVALID and why(b"records must be 16-byte aligned")
        assert reduce(p(rec), 8, p(lists), None, p(out)) == INVALID and why(b"both or neither")
        assert reduce(p(rec), 8, None, p(lists), p(out)) == INVALID and why(b"both or neither")
        assert reduce(p(rec), 8, p(lists, 2), p(lists), p(out)) == INVALID and why(b"group lists must be 4-byte aligned")
        assert reduce(p(rec), 8, p(lists), p(lists, 2), p(out)) == INVALID and why(b"group lists must be 4-byte aligned")
        assert reduce(None, 8, None, None, p(out)) == STATE and why(b"before gte_backtest")
        # wrong in two ways: the check that stands first reports
        assert reduce(p(rec, 8), 0, None, None, None) == INVALID and why(b"n_strategies must be >= 1")
        assert reduce(p(rec, 8), 8, p(lists), None, None) == INVALID and why(b"out_device")
        assert reduce(None, 8, p(lists), None, p(out)) == INVALID and why(b"both or neither")
        assert lib.gte_reduce_backtest_stats(None, p(rec), 0, None, None, None) == INVALID and why(b"env is NULL")
        assert rank(p(out), 8, 0, 1, 8, p(idx), p(top), None) == _abi.GTE_OK
        assert rank(p(out), 0, 0, 1, 8, p(idx), p(top), None) == INVALID and why(b"n_strategies must be >= 1")
        for k in (0, -1, 257):
            assert rank(p(out), 8, 0, 1, k, p(idx), p(top), None) == INVALID and why(b"k must lie in [1, 256]")
        for metric in (-1, 6):
            assert rank(p(out), 8, metric, 1, 8, p(idx), p(top), None) == INVALID
            assert why(b"metric %d unknown" % metric)
        stats_text, top_text = b"stats_device must be a 16-byte aligned", b"top_index_device (int32 [k]) and top_score_device"
        assert rank(None, 8, 0, 1, 8, p(idx), p(top), None) == INVALID and why(stats_text)
        assert rank(p(out, 8), 8, 0, 1, 8, p(idx), p(top), None) == INVALID and why(stats_text)
        assert rank(p(out), 8, 0, 1, 8, None, p(top), None) == INVALID and why(top_text)
        assert rank(p(out), 8, 0, 1, 8, p(idx), None, None) == INVALID and why(top_text)
        assert rank(p(out), 8, 0, 1, 8, p(idx, 2), p(top), None) == INVALID and why(top_text)
        assert rank(p(out), 8, 0, 1, 8, p(idx), p(top, 4), None) == INVALID and why(top_text)
        assert rank(p(out), 8, 0, 1, 8, p(idx), p(top), p(top, 4)) == INVALID and why(b"scores_device must be 8-byte aligned")
        assert rank(None, 0, -1, 1, 0, None, None, p(top, 4)) == INVALID and why(b"n_strategies must be >= 1")
        assert rank(None, 8, -1, 1, 0, None, None, p(top, 4)) == INVALID and why(b"k must lie")
        assert rank(None, 8, -1, 1, 8, None, None, p(top, 4)) == INVALID and why(b"metric -1 unknown")
        assert rank(None, 8, 0, 1, 8, None, None, p(top, 4)) == INVALID and why(stats_text)
        assert rank(p(out), 8, 0, 1, 8, None, None, p(top, 4)) == INVALID and why(top_text)
        # the reads: gte_read_backtest_stats
        host = np.empty(64, dtype=sm.BACKTEST)
        read = lib.gte_read_backtest_stats
        assert read(fresh._h, 0, 64, host.ctypes.data) == STATE and why(b"gte_read_backtest_stats before gte_backtest")
        assert read(fresh._h, 60, 5, None) == INVALID and why(b"NULL argument")
        assert read(None, 0, 1, host.ctypes.data) == INVALID and why(b"NULL argument")
        assert read(fresh._h, 60, 5, host.ctypes.data) == STATE and why(b"before gte_backtest")  # (state before range)
        fresh.synchronize()
        # inside a stream capture: refused with its reason (the capture fails, the env works on)
        fresh.reset()
        seen = []

        def body(i):
            seen.append((reduce(p(rec), 8, None, None, p(out)), lib.gte_last_error()))
            seen.append((rank(p(out), 8, 0, 1, 8, p(idx), p(top), None), lib.gte_last_error()))
            raise RuntimeError("refused inside the capture")
        with pytest.raises(Exception):
            fresh.capture_steps(body, 2)
        torch.cuda.synchronize()
        assert [c for c, _ in seen] == [STATE, STATE] and all(b"stream capture" in m for _, m in seen), seen
        assert reduce(p(rec), 8, None, None, p(out)) == _abi.GTE_OK
        fresh.synchronize()
        # the Python layer
        rec_host = sm.craft_records(64)
        with pytest.raises(ValueError):
            StrategyStats.from_records(fresh, rec_host)                                   # no n_strategies
        with pytest.raises(TypeError):
            StrategyStats.from_records(fresh, rec_host.view(np.uint8), n_strategies=4)    # not BACKTEST_DTYPE
        with pytest.raises(ValueError):
            StrategyStats.from_records(fresh, rec_host[:60], n_strategies=4)              # wrong N
        with pytest.raises(TypeError):
            StrategyStats.from_records(fresh, rec.to(torch.int8), n_strategies=4)         # wrong tensor dtype
        with pytest.raises(ValueError):
            StrategyStats.from_records(fresh, rec[:, :64], n_strategies=4)                # wrong shape
        with pytest.raises(ValueError):
            StrategyStats.from_records(fresh, rec.cpu(), n_strategies=4)                  # wrong device
        with pytest.raises(ValueError):
            StrategyStats.from_records(fresh, rec_host, n_strategies=0)
        with pytest.raises(IndexError):
            StrategyStats.from_records(fresh, rec_host, strategy=np.full(64, 4), n_strategies=4)
        with pytest.raises(TypeError):
            StrategyStats.from_records(fresh, rec_host, strategy=np.zeros(64), n_strategies=4)
        with pytest.raises(ValueError):
            StrategyStats.from_records(fresh, rec_host, strategy=np.zeros(63, dtype=np.int32), n_strategies=4)
        board = StrategyStats.from_records(fresh, rec_host, n_strategies=4)
        for k in (0, 257):
            with pytest.raises(ValueError):
                board.top(k)
        with pytest.raises(ValueError):
            board.top(3, "median")
    finally:
        fresh.close()


# ---- the example -------------------------------------------------------------------------------------------------------

def test_leaderboard_example(capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import backtest_leaderboard
    leaders, records, board = backtest_leaderboard.main(strategies=96, envs=500, K=400, top=5, details=True)
    S, N = 96, 500
    assert sm.same_bytes(board, sm.reduce_vector(records, sm.default_groups(N, S)))
    assert sorted(set(board["envs"].tolist())) == [5, 6]
    for metric, (index, score) in leaders.items():
        want_i, want_s = sm.rank_vector(board, sm.scores_vector(board, metric), 4, 5)
        assert index.tolist() == want_i.tolist() and sm.same_f64(score, want_s), metric
    out = capsys.readouterr().out
    assert "by episode_sharpe" in out and "5 to 6 envs each" in out
