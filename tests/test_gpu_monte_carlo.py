"""The trade Monte Carlo on the device (gte_pool_trades, gte_trade_monte_carlo, include/gte.h) against its model
(tests/monte_carlo_model.py), bit for bit on every output, NaN as NaN, no tolerance anywhere: synthetic pools over
the slab and Philox block edges with every subset of the per-path columns left out; both pool paths on either side of
GTE_MC_LDS_POOL; special values; independence of R, slot, seed and stream; the pools of a real backtest with
truncated lists, the default and an explicit map; the Python pipeline end to end; every refusal, with the outputs
untouched; the example."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

import monte_carlo_model as mm
from gym_trading_env_amd import _abi
from leaderboard_gpu import GUARD, assert_arrays_same, guarded, make_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (0x7EAD << 32) | 20240607   # the high word set
LEVELS = (0.0, 0.05, 0.2, 0.5)
FLOATS = ("final", "max_drawdown", "low")
FILL = -7


@pytest.fixture(scope="module")
def env():
    e = make_env()
    yield e
    e.close()


def _p(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


class Call:
    """One gte_trade_monte_carlo over host-made pools, every output between guards"""

    def __init__(self, env, factors, first, streams, R, levels=LEVELS, keep=mm.COLUMNS):
        import torch
        self.env, self.torch, self.R, self.levels, self.keep = env, torch, R, tuple(levels), tuple(keep)
        self.dev = dev = env._t["obs"].device
        self.Q = Q = len(first) - 1
        self.factors = torch.from_numpy(np.ascontiguousarray(factors, dtype=np.float64)).to(dev) if len(factors) \
            else torch.zeros(1, dtype=torch.float64, device=dev)
        self.first = torch.from_numpy(np.ascontiguousarray(first, dtype=np.int64)).to(dev)
        self.streams = None if streams is None else \
            torch.from_numpy(np.asarray(streams, np.uint32).view(np.int32).copy()).to(dev)
        f64, i32, i64 = torch.float64, torch.int32, torch.int64
        self.whole, self.mine = {}, {}
        for name in mm.COLUMNS:
            self.whole[name], self.mine[name] = guarded(torch, dev, Q * R, i32 if name == "max_loss_streak" else f64, FILL)
        self.whole["pool"], self.mine["pool"] = guarded(torch, dev, Q * 6, i64, FILL)   # (48 bytes a record, 16-aligned)
        self.whole["dd_count"], self.mine["dd_count"] = guarded(torch, dev, Q * len(self.levels), i32, FILL)
        self.out = _abi.GteMcOut(pool=self.mine["pool"].data_ptr(), dd_count=self.mine["dd_count"].data_ptr(),
                                 **{name: self.mine[name].data_ptr() for name in self.keep})
        self.host_levels = (C.c_double * max(len(self.levels), 1))(*self.levels)

    def status(self, path_len=0, seed=SEED, ruin=0.5, wait=True, **change):
        """the call's status; `change`: arguments put in place of the staged ones; `wait`: for the staging copies
        first (not inside a stream capture)"""
        a = dict(factors=_p(self.factors), first=_p(self.first), streams=_p(self.streams), Q=self.Q, R=self.R,
                 path_len=path_len, seed=seed, ruin=ruin, levels=self.host_levels, n_levels=len(self.levels),
                 out=C.byref(self.out), h=self.env._h)
        a.update(change)
        if wait:
            self.torch.cuda.synchronize()
        return self.env._lib.gte_trade_monte_carlo(a["h"], a["factors"], a["first"], a["streams"], a["Q"], a["R"],
                                                   a["path_len"], a["seed"], a["ruin"], a["levels"], a["n_levels"],
                                                   a["out"])

    def guards_untouched(self):
        for name, whole in self.whole.items():
            host = whole.cpu().numpy()
            assert (host[:GUARD] == FILL).all() and (host[len(host) - GUARD:] == FILL).all(), name

    def untouched(self):
        self.env.synchronize()
        for name, whole in self.whole.items():
            assert (whole.cpu().numpy() == FILL).all(), name

    def run(self, path_len=0, seed=SEED, ruin=0.5):
        """-> dict of host arrays shaped like the model's; a column that was not kept must still hold its fill"""
        _abi.check(self.env._lib, self.status(path_len, seed, ruin))
        self.env.synchronize()
        self.guards_untouched()
        Q, R = self.Q, self.R
        got = {}
        for name in mm.COLUMNS:
            host = self.mine[name].cpu().numpy().reshape(Q, R)
            if name in self.keep:
                got[name] = host
            else:
                assert (host == FILL).all(), name
        got["pool"] = self.mine["pool"].cpu().numpy().view(mm.POOL).reshape(Q)
        got["dd_count"] = self.mine["dd_count"].cpu().numpy().reshape(Q, len(self.levels))
        return got


def assert_same(got, want, tag, keep=mm.COLUMNS):
    names = tuple(keep) + ("dd_count",)
    assert_arrays_same(got, want, names, FLOATS, tag)
    pool = lambda d: {n: np.ascontiguousarray(d["pool"][n]) for n in mm.POOL.names}
    assert_arrays_same(pool(got), pool(want), mm.POOL.names, ("final_sum", "final_sq_sum", "mdd_sum", "mdd_sq_sum"), tag)


def synthetic():
    rng = np.random.default_rng(3)
    sizes = (0, 1, 7, 64, 300)
    factors = np.exp(rng.normal(0.0, 0.08, sum(sizes)))
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return factors, first, np.array([9, 0, 0xFFFFFFFF, 4, 123456], np.uint32)


# ---- synthetic pools against the model ------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 255, 256, 257, 600])
def test_synthetic_pools_equal_the_model(env, R):
    factors, first, streams = synthetic()
    call = Call(env, factors, first, streams, R)
    for path_len in (0, 1, 3, 4, 5, 37):
        want = mm.monte_carlo(factors, first, streams, R, path_len, SEED, 0.9, LEVELS)
        assert_same(call.run(path_len, ruin=0.9), want, (R, path_len))
    assert list(want["pool"]["pool_size"]) == [0, 1, 7, 64, 300] and list(want["pool"]["path_len"]) == [0] + [37] * 4


def test_every_subset_of_columns_left_out_leaves_the_others_as_they_are(env):
    factors, first, streams = synthetic()
    R, path_len = 257, 5
    want = mm.monte_carlo(factors, first, streams, R, path_len, SEED, 0.9, LEVELS)
    for n in range(len(mm.COLUMNS) + 1):
        for keep in itertools.combinations(mm.COLUMNS, n):
            got = Call(env, factors, first, streams, R, keep=keep).run(path_len, ruin=0.9)
            assert_same(got, want, keep, keep)
    # no levels at all: dd_count may be NULL
    call = Call(env, factors, first, streams, R, levels=())
    call.out.dd_count = None
    got = call.run(path_len, ruin=0.9)
    assert_same(got, mm.monte_carlo(factors, first, streams, R, path_len, SEED, 0.9, ()), "no levels")


def test_stream_defaults_to_the_slot(env):
    factors, first, _ = synthetic()
    want = mm.monte_carlo(factors, first, None, 70, 6, SEED, 0.5, LEVELS)
    assert_same(Call(env, factors, first, None, 70).run(6), want, "stream NULL")


# ---- both pool paths --------------------------------------------------------------------------------------------

def test_both_pool_paths_equal_the_model(env):
    """pools of GTE_MC_LDS_POOL - 1, GTE_MC_LDS_POOL (staged into LDS), GTE_MC_LDS_POOL + 1 and 3 * GTE_MC_LDS_POOL + 5
    factors (read in place); the odd sizes put the later pools on addresses that are not 16-byte aligned, and the
    leading pool of one factor does so for the first"""
    T = _abi.GTE_MC_LDS_POOL
    sizes = (1, T - 1, T, T + 1, 3 * T + 5)
    rng = np.random.default_rng(5)
    factors = np.exp(rng.normal(0.0, 0.05, sum(sizes)))
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    R, L = 70, 9
    want = mm.monte_carlo(factors, first, None, R, L, SEED, 0.8, LEVELS)
    assert_same(Call(env, factors, first, None, R).run(L, ruin=0.8), want, "both paths")
    assert list(want["pool"]["pool_size"]) == list(sizes)


def test_the_two_pool_paths_give_the_same_rows(env):
    """Two pools of one repeated value, one on either side of the threshold, and the same stream: whatever is drawn,
    the factors coincide, so the rows must.  Then a pool whose first GTE_MC_LDS_POOL factors repeat: with one more
    factor it is read in place, and a row whose draws all fall among the repeated ones — where the drawn factor is
    the same by construction — must equal the staged pool's row of the same draws."""
    T = _abi.GTE_MC_LDS_POOL
    first = np.array([0, T, 2 * T + 1], np.int64)
    factors = np.full(2 * T + 1, 0.97)
    got = Call(env, factors, first, [4, 4], 300).run(11)
    for name in mm.COLUMNS:
        assert got[name][0].tobytes() == got[name][1].tobytes(), name
    for name in mm.POOL.names[:6]:
        assert got["pool"][name][0].tobytes() == got["pool"][name][1].tobytes(), name
    assert list(got["pool"]["pool_size"]) == [T, T + 1]
    # period 2 in the factors, an even pool: index j of T + 1 and index j' of T draw the same factor when j = j' (mod 2)
    pattern = np.tile([1.02, 0.99], T)
    factors = np.concatenate([pattern[:T], pattern[:T + 1]])
    R, L = 600, 2   # (a draw falls on the same factor in both pools about every other time)
    got = Call(env, factors, first, [4, 4], R).run(L)
    same = ((mm.indices(SEED, 4, R, L, T) % 2) == (mm.indices(SEED, 4, R, L, T + 1) % 2)).all(axis=1)
    assert same.sum() > 50 and (~same).sum() > 50
    for name in mm.COLUMNS:
        assert got[name][0][same].tobytes() == got[name][1][same].tobytes(), name


def test_special_values_bit_for_bit(env):
    factors, first = mm.special_pools()
    levels = (0.0, 0.1, 0.5, 1.0)
    for R, path_len in ((257, 0), (600, 5)):
        want = mm.monte_carlo(factors, first, None, R, path_len, SEED, 0.5, levels)
        assert_same(Call(env, factors, first, None, R, levels=levels).run(path_len), want, (R, path_len))
    assert np.isnan(want["final"]).any() and np.isinf(want["final"]).any() and (want["final"] == 0.0).any()


def test_unusable_pools_are_empty_and_nothing_outside_the_span_is_read(env):
    """reversed pools and pools that reach outside [first[0], first[n_pools]): the factors outside the span are NaN
    here, and no output may show one"""
    factors = np.full(400, np.nan)
    factors[10:20] = np.exp(np.random.default_rng(4).normal(0.0, 0.1, 10))
    first = np.array([10, 5, 300, 20, 12, 20], np.int64)
    want = mm.monte_carlo(factors, first, None, 40, 0, SEED, 0.5, LEVELS)
    got = Call(env, factors, first, None, 40).run(0)
    assert_same(got, want, "unusable")
    assert list(got["pool"]["pool_size"]) == [0, 0, 0, 0, 8] and not np.isnan(got["final"]).any()


# ---- independence -----------------------------------------------------------------------------------------------

def test_rows_do_not_depend_on_R_or_the_slot(env):
    factors, first, streams = synthetic()
    big = Call(env, factors, first, streams, 600).run(5)
    small = Call(env, factors, first, streams, 256).run(5)
    for name in mm.COLUMNS:
        assert big[name][:, :256].tobytes() == small[name].tobytes(), name
    # pool 3 (64 factors) in slot 0 and in slot 3 of another call, the same stream
    lo, hi = int(first[3]), int(first[4])
    mine = factors[lo:hi]
    pools = np.concatenate([mine, factors[:7], factors[:1], mine])
    table = np.array([0, 64, 71, 72, 136], np.int64)
    got = Call(env, pools, table, [4, 1, 2, 4], 256).run(5)
    for name in mm.COLUMNS:
        assert got[name][0].tobytes() == got[name][3].tobytes() == small[name][3].tobytes(), name
    other_seed = Call(env, pools, table, [4, 1, 2, 4], 256).run(5, seed=SEED + 1)
    other_stream = Call(env, pools, table, [4, 1, 2, 5], 256).run(5)
    assert other_seed["final"][0].tobytes() != got["final"][0].tobytes()
    assert other_stream["final"][3].tobytes() != got["final"][3].tobytes()
    assert other_stream["final"][0].tobytes() == got["final"][0].tobytes()


# ---- the pools of a real backtest ----------------------------------------------------------------------------------

S = 6
CAPACITY = 4


@pytest.fixture(scope="module")
def backtest():
    """64 envs, six strategies that flip their position every 2, 3, 5, 11, 17 and 29 rows, lists of four trades: the
    envs of the fast ones truncate, those of the slow ones do not"""
    e = make_env()
    t = np.arange(60)
    table = np.stack([np.where((t // every) % 2 == 0, 2, 0) for every in (2, 3, 5, 11, 17, 29)]).astype(np.int8)
    e.bind_signals(table)
    e.reset()
    e.track_trades(list_capacity=CAPACITY)
    stats = e.backtest_signals(40)
    e.synchronize()
    yield e, stats
    e.close()


def _pool_call(env, offsets, members, strategies, max_factors, n_strategies=S):
    """gte_pool_trades with guarded outputs -> (status, first, truncated, factors with its guards)"""
    import torch
    dev = env._t["obs"].device
    Q = len(strategies)
    ids = torch.tensor(list(strategies), dtype=torch.int32, device=dev)
    w_first, first = guarded(torch, dev, Q + 1, torch.int64, FILL)
    w_trunc, trunc = guarded(torch, dev, Q, torch.int32, FILL)
    w_fact, fact = guarded(torch, dev, max(max_factors, 1), torch.float64, FILL)
    d_off = None if offsets is None else torch.tensor(offsets, dtype=torch.int32, device=dev)
    d_mem = None if members is None else torch.tensor(members, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    status = env._lib.gte_pool_trades(env._h, n_strategies, _p(d_off), _p(d_mem), _p(ids), Q, _p(first), _p(trunc),
                                      _p(fact) if max_factors else None, max_factors)
    env.synchronize()
    return status, (w_first, first), (w_trunc, trunc), (w_fact, fact)


def _inner_guards(*pairs):
    for whole, _ in pairs:
        host = whole.cpu().numpy()
        assert (host[:GUARD] == FILL).all() and (host[len(host) - GUARD:] == FILL).all()


def test_pools_of_a_backtest(backtest):
    env, stats = backtest
    N = env.num_envs
    everything = stats.trade_stats.trades()
    closed = everything.closed
    assert (closed > CAPACITY).any() and (closed <= CAPACITY).any(), closed
    asked = [2, -1, 5, 2, S, 0]                    # the padding of a ranking, a repeat, an id past the end
    default = [[e for e in range(N) if e % S == s] for s in range(S)]
    explicit = [[5, 3, N + 5, 9], [], [63, -1, 0, 0, 17], list(range(20, 50)), [1], [2, 4]]   # members outside [0, N)
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in explicit])]).tolist()
    members = [e for g in explicit for e in g] + [0] * (N - offsets[-1])     # (N entries: include/gte.h)
    for tag, lists, off, mem in (("default", default, None, None), ("explicit", explicit, offsets, members)):
        want_first, want_trunc, want = mm.trade_pools(asked, lists, everything.first, closed, CAPACITY,
                                                      everything.open_value, everything.close_value)
        total = int(want_first[-1])
        assert total > 0
        # the count pass: nothing but first and truncated
        status, first, trunc, fact = _pool_call(env, off, mem, asked, 0)
        assert status == _abi.GTE_OK
        _inner_guards(first, trunc)
        np.testing.assert_array_equal(first[1].cpu().numpy(), want_first, err_msg=tag)
        np.testing.assert_array_equal(trunc[1].cpu().numpy(), want_trunc, err_msg=tag)
        assert (fact[0].cpu().numpy() == FILL).all()
        # the pack
        status, first, trunc, fact = _pool_call(env, off, mem, asked, total)
        assert status == _abi.GTE_OK
        _inner_guards(first, trunc, fact)
        np.testing.assert_array_equal(first[1].cpu().numpy(), want_first, err_msg=tag)
        assert fact[1].cpu().numpy().tobytes() == want.tobytes(), tag
        # a block below the total: nothing past it, the total still reported
        short = total // 2
        status, first, trunc, fact = _pool_call(env, off, mem, asked, short)
        assert status == _abi.GTE_OK
        _inner_guards(first, trunc, fact)
        assert int(first[1][-1]) == total and fact[1].cpu().numpy().tobytes() == want[:short].tobytes(), tag
    # the default map's pools are the TradeList's, strategy by strategy
    want_first, want_trunc, want = mm.trade_pools(asked, default, everything.first, closed, CAPACITY,
                                                  everything.open_value, everything.close_value)
    with np.errstate(all="ignore"):
        parts = [(lambda t: t.close_value / t.open_value)(stats.trade_stats.trades(strategy=s)) if 0 <= s < S
                 else np.zeros(0) for s in asked]
    assert np.concatenate(parts).tobytes() == want.tobytes()
    assert want_trunc[0] == sum(closed[e] > CAPACITY for e in default[2]) and want_trunc[1] == 0


def test_monte_carlo_of_a_leaderboard(backtest):
    import torch
    env, stats = backtest
    board = stats.trade_stats.by_strategy()
    index, _ = board.top(4, "profit_factor")
    assert index.is_cuda and index.dtype == torch.int32
    padded = torch.cat([index, torch.tensor([-1], dtype=torch.int32, device=index.device)])
    R, levels = 300, (0.01, 0.05, 0.2)
    mc = board.monte_carlo(padded, n_resamples=R, seed=SEED, ruin=0.95, drawdown_levels=levels,
                           keep=("final", "max_drawdown", "low", "max_loss_streak"))
    ids = padded.cpu().numpy()
    everything = stats.trade_stats.trades()
    default = [[e for e in range(env.num_envs) if e % S == s] for s in range(S)]
    first, trunc, factors = mm.trade_pools(ids.tolist(), default, everything.first, everything.closed, CAPACITY,
                                           everything.open_value, everything.close_value)
    want = mm.monte_carlo(factors, first, ids.astype(np.uint32), R, 0, SEED, 0.95, levels)
    got = mc.numpy()
    got["pool"] = want["pool"].copy()
    for name in mm.POOL.names:
        got["pool"][name] = got[name] if name in got else getattr(mc, name).cpu().numpy()
    assert_same(got, want, "pipeline")
    np.testing.assert_array_equal(got["truncated"], trunc)
    np.testing.assert_array_equal(got["strategies"], ids)
    assert got["pool_size"][-1] == 0 and (got["final"][-1] == 1.0).all()
    Rf = np.float64(R)
    assert got["prob_loss"].tobytes() == (want["pool"]["count_loss"] / Rf).tobytes()
    assert got["risk_of_ruin"].tobytes() == (want["pool"]["count_ruin"] / Rf).tobytes()
    assert got["prob_drawdown"].tobytes() == (want["dd_count"] / Rf).tobytes()
    assert got["mean_final"].tobytes() == (want["pool"]["final_sum"] / Rf).tobytes()
    assert got["mean_drawdown"].tobytes() == (want["pool"]["mdd_sum"] / Rf).tobytes()
    for column in ("final", "max_drawdown", "max_loss_streak"):
        ordered = np.sort(want[column], axis=1)
        for q in (0.0, 0.05, 0.5, 0.95, 1.0):
            place = max(int(np.ceil(q * R)) - 1, 0)
            assert mc.quantile(column, q).cpu().numpy().tobytes() == ordered[:, place].tobytes(), (column, q)
        both = mc.quantile(column, (0.05, 0.95)).cpu().numpy()
        assert both.shape == (len(ids), 2) and (both[:, 0] == ordered[:, max(int(np.ceil(0.05 * R)) - 1, 0)]).all()
    # a strategy's rows do not depend on who else was asked for; host ids do what the tensor does
    alone = board.monte_carlo([int(ids[1])], n_resamples=R, seed=SEED, ruin=0.95, drawdown_levels=levels)
    assert alone.final.cpu().numpy().tobytes() == want["final"][1:2].tobytes()
    assert alone.low is None and alone.max_loss_streak is None
    with pytest.raises(ValueError, match="was not kept"):
        alone.quantile("low", 0.5)
    # an explicit map through the fold: the pools follow the fold's own member lists
    strategy = torch.tensor([(e * 7) % (S + 1) - 1 for e in range(env.num_envs)], dtype=torch.int32, device=index.device)
    folded = stats.trade_stats.by_strategy(strategy=strategy, n_strategies=S)
    lists = [[e for e in range(env.num_envs) if (e * 7) % (S + 1) - 1 == s] for s in range(S)]
    first, trunc, factors = mm.trade_pools([3, 0], lists, everything.first, everything.closed, CAPACITY,
                                           everything.open_value, everything.close_value)
    mc = folded.monte_carlo([3, 0], n_resamples=64, n_trades=5, seed=SEED)
    want = mm.monte_carlo(factors, first, np.array([3, 0], np.uint32), 64, 5, SEED, 0.5, (0.1, 0.2, 0.3, 0.5))
    assert mc.final.cpu().numpy().tobytes() == want["final"].tobytes()
    assert mc.factors.cpu().numpy()[:len(factors)].tobytes() == factors.tobytes()


def test_resample_of_own_pools(env):
    from gym_trading_env_amd import monte_carlo
    factors, first, streams = synthetic()
    mc = monte_carlo.resample(env, factors, first, n_resamples=100, n_trades=6, seed=SEED, ruin=0.9,
                              drawdown_levels=LEVELS, keep=mm.COLUMNS, streams=streams)
    want = mm.monte_carlo(factors, first, streams, 100, 6, SEED, 0.9, LEVELS)
    for name in mm.COLUMNS:
        assert getattr(mc, name).cpu().numpy().tobytes() == want[name].tobytes(), name
    assert (mc.truncated.cpu().numpy() == 0).all() and mc.strategies is None
    np.testing.assert_array_equal(mc.dd_count.cpu().numpy(), want["dd_count"])


# ---- refusals --------------------------------------------------------------------------------------------------------

def test_monte_carlo_refusals_leave_the_outputs_untouched(env):
    factors, first, streams = synthetic()
    INVALID, STATE = _abi.GTE_ERR_INVALID, _abi.GTE_ERR_STATE
    call = Call(env, factors, first, streams, 40)
    nan = float("nan")
    odd = lambda t: _p(t, 4)   # misaligned for an 8-byte type
    cases = [dict(h=None), dict(factors=None), dict(first=None), dict(out=None), dict(factors=odd(call.factors)),
             dict(first=odd(call.first)), dict(streams=_p(call.streams, 2)),
             dict(Q=0), dict(Q=-1), dict(Q=_abi.GTE_MC_MAX_POOLS + 1), dict(R=0), dict(R=_abi.GTE_MC_MAX_RESAMPLES + 1),
             dict(path_len=-1), dict(path_len=_abi.GTE_MC_MAX_PATH + 1), dict(n_levels=-1),
             dict(n_levels=_abi.GTE_MC_MAX_LEVELS + 1), dict(ruin=nan), dict(levels=None)]
    for change in cases:
        assert call.status(**change) == INVALID, change
    for field, off in (("pool", 8), ("pool", None), ("dd_count", 2), ("dd_count", None), ("final", 4), ("low", 4),
                       ("max_drawdown", 4), ("max_loss_streak", 2)):
        broken = Call(env, factors, first, streams, 40)
        setattr(broken.out, field, None if off is None else broken.mine[field].data_ptr() + off)
        assert broken.status() == INVALID, (field, off)
        broken.untouched()
    call.untouched()
    seen = []

    def body(i):
        seen.append(call.status(wait=False))
        raise RuntimeError("refused inside the capture")
    with pytest.raises(Exception):
        env.capture_steps(body, 2)
    call.torch.cuda.synchronize()
    assert seen == [STATE] and "stream capture" in env._lib.gte_last_error().decode()
    call.untouched()
    assert call.status() == _abi.GTE_OK     # ... and the same call goes through outside
    env.synchronize()
    call.guards_untouched()


def test_python_refusals(backtest):
    _, stats = backtest
    board = stats.trade_stats.by_strategy()
    for bad, error in ((dict(n_resamples=0), ValueError), (dict(n_resamples=_abi.GTE_MC_MAX_RESAMPLES + 1), ValueError),
                       (dict(n_resamples=2.5), TypeError), (dict(n_trades=0), ValueError),
                       (dict(n_trades=_abi.GTE_MC_MAX_PATH + 1), ValueError), (dict(ruin=float("nan")), ValueError),
                       (dict(drawdown_levels=(0.1,) * 9), ValueError), (dict(drawdown_levels=(float("nan"),)), ValueError),
                       (dict(keep=("final", "median")), ValueError), (dict(seed=1.5), TypeError)):
        with pytest.raises(error):
            board.monte_carlo([0], **bad)
    with pytest.raises(ValueError):
        board.monte_carlo([])
    with pytest.raises(TypeError):
        board.monte_carlo([0.5])


def test_pool_refusals(backtest, env):
    import torch
    INVALID, STATE = _abi.GTE_ERR_INVALID, _abi.GTE_ERR_STATE
    b, _ = backtest
    dev = b._t["obs"].device
    lib = b._lib
    ids = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    w_first, first = guarded(torch, dev, 3, torch.int64, FILL)
    w_trunc, trunc = guarded(torch, dev, 2, torch.int32, FILL)
    w_fact, fact = guarded(torch, dev, 16, torch.float64, FILL)
    off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    mem = torch.zeros(b.num_envs, dtype=torch.int32, device=dev)
    good = dict(h=b._h, S=S, off=None, mem=None, ids=_p(ids), Q=2, first=_p(first), trunc=_p(trunc), fact=_p(fact), n=16)

    def status(wait=True, **change):
        a = dict(good)
        a.update(change)
        if wait:
            torch.cuda.synchronize()
        return lib.gte_pool_trades(a["h"], a["S"], a["off"], a["mem"], a["ids"], a["Q"], a["first"], a["trunc"],
                                   a["fact"], a["n"])
    for change in (dict(h=None), dict(Q=0), dict(Q=_abi.GTE_MC_MAX_POOLS + 1), dict(S=0), dict(off=_p(off)),
                   dict(mem=_p(mem)), dict(ids=None), dict(first=None), dict(trunc=None), dict(fact=None),
                   dict(n=-1), dict(ids=_p(ids, 2)), dict(first=_p(first, 4)), dict(trunc=_p(trunc, 2)),
                   dict(fact=_p(fact, 4)), dict(off=_p(off, 2), mem=_p(mem))):
        assert status(**change) == INVALID, change
    # refused where gte_pack_trade_list is refused: no list kept ...
    closed = torch.zeros(64, dtype=torch.int32, device=dev)
    first_all = torch.zeros(65, dtype=torch.int64, device=dev)
    pack = lambda e: e._lib.gte_pack_trade_list(e._h, None, 0, _p(first_all), _p(closed), None, 0)
    assert pack(env) == STATE and status(h=env._h) == STATE and "trade list is off" in lib.gte_last_error().decode()
    # ... inside a stream capture ...
    seen = []

    def body(i):
        seen.append(status(wait=False))
        raise RuntimeError("refused inside the capture")
    with pytest.raises(Exception):
        b.capture_steps(body, 2)
    torch.cuda.synchronize()
    assert seen == [STATE] and "stream capture" in lib.gte_last_error().decode()
    b.synchronize()
    for whole in (w_first, w_trunc, w_fact):
        assert (whole.cpu().numpy() == FILL).all()
    assert status() == _abi.GTE_OK
    # ... and between a switch of the list and the backtest that clears (last: it leaves the fixture's lists stale)
    from gym_trading_env_amd import monte_carlo
    with pytest.raises(ValueError, match="no trade list is kept"):
        monte_carlo.run(_Owner(env), [0])
    b.track_trades(list_capacity=CAPACITY + 1)
    assert pack(b) == STATE and status() == STATE and "no backtest call has cleared" in lib.gte_last_error().decode()


class _Owner:
    """what monte_carlo.run reads of a fold before it asks the library anything"""

    def __init__(self, env):
        self._env = env


# ---- the example -------------------------------------------------------------------------------------------------------

def test_monte_carlo_example(capsys):
    """examples/backtest_monte_carlo.py runs at a small size and returns finite quantiles, ordered as quantiles are"""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import backtest_monte_carlo as ex
    finally:
        sys.path.pop(0)
    out = ex.main(strategies=12, K=600, replicas=4, T=1500, top=10, resamples=200, min_trades=2)
    text = capsys.readouterr().out
    q = out["quantiles"]
    assert q.shape == (len(out["index"]), 3) and len(out["index"]) >= 1
    assert np.isfinite(q).all() and (q >= 0.0).all() and (q[:, 0] <= q[:, 1]).all() and (q[:, 1] <= q[:, 2]).all()
    assert "risk of ruin" in text and "lists truncated at 64 trades" in text
    mc = out["monte_carlo"]
    assert (mc.pool_size.cpu().numpy() > 0).all() and tuple(mc.final.shape) == (len(out["index"]), 200)
