"""Signal tables composed on the device (gte_compose_signals, csrc/gte_compose.hip): every table is
compared byte for byte with the host model of the rule (tests/signal_compose_model.py, held to a second
statement of it in tests/test_signal_compose_cpu.py) — over prefixes of the fixture around the 16-byte
and 1 024-byte edges, with guard rows and guard bytes around the table; wide clause strides with
poisoned padding; host and device inputs; chaining; two datasets; the whole pipeline from indicator
specs to backtest records; refusals; the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import signal_compose_model as cm
import signal_rule_model as rm
import test_gpu_backtest as tb
from gym_trading_env_amd import _abi, signals
from gym_trading_env_amd.config import make_config

pytestmark = pytest.mark.gpu

GUARD = 0x55
POISON = 0x33  # what the padding of a clause table holds here: no code, and not -1 either
BASE = dict(positions=[-1, 0, 1], trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration=24, seed=11)


@pytest.fixture(scope="module")
def fix():
    """(clauses int8 [12, 2500], specs [~100], the model's table) — a prefix of the clauses gives a prefix
    of the table (test_signal_compose_cpu.py), so one model table serves every T"""
    clauses, specs = cm.fixture()
    table = cm.compose_table(clauses, specs, cm.T_FIX)
    table.setflags(write=False)
    return clauses, specs, table


def _market(T, seed=31):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1, (T, 2)).astype(np.float32), 100 * np.exp(np.cumsum(rng.normal(0, 1e-2, T)))


def _env(T, n=4, **kw):
    from gym_trading_env_amd.batched import BatchedTradingEnv
    return BatchedTradingEnv(_market(T), num_envs=n, positions=[-1, 0, 1], windows=None, **kw)


def _specs_tensor(specs):
    import torch
    return torch.from_numpy(np.ascontiguousarray(specs).view(np.uint8).reshape(-1, 128).copy()).cuda()


def _clause_tensor(clauses, T, stride=None, fill=POISON):
    """the first T columns of `clauses` as a device tensor [R, stride] whose padding holds `fill`"""
    import torch
    stride = signals.row_stride(T) if stride is None else stride
    host = np.full((clauses.shape[0], stride), fill, np.int8)
    host[:, :T] = clauses[:, :T]
    return torch.from_numpy(host).cuda()


def _raw(env, d, clauses_ptr, n_rows, clause_stride, specs_ptr, n_specs, table_ptr, row_stride):
    return env._lib.gte_compose_signals(env._h, d, C.c_void_p(clauses_ptr), n_rows, clause_stride,
                                        C.c_void_p(specs_ptr), n_specs, C.c_void_p(table_ptr), row_stride)


@pytest.mark.parametrize("T", [2, 15, 16, 17, 1023, 1024, 1025, 2500])
def test_prefixes_of_the_fixture_with_guards(T, fix):
    """S = 1, 3 and all (a partial workgroup of four waves, and whole ones) x row_stride minimal + 16 and
    minimal + 48; one guard row before and after the table and the bytes beyond round_up(T, 16) hold 0x55
    before the call and after it.  (T = 2 is the smallest dataset that can be resident.)"""
    import torch
    clauses, specs, model = fix
    env = _env(T)
    d_clauses = _clause_tensor(clauses, T)
    T16 = signals.row_stride(T)
    for S in (1, 3, len(specs)):
        pick = np.arange(len(specs))[-S:] if S > 1 else np.array([38])  # (38: the enter/exit spec on rows 10, 11)
        d_specs = _specs_tensor(specs[pick])
        for stride in (T16 + 16, T16 + 48):
            guard = torch.full((S + 2, stride), GUARD, dtype=torch.int8, device="cuda")
            assert guard[1].data_ptr() % 16 == 0
            _abi.check(env._lib, _raw(env, 0, d_clauses.data_ptr(), d_clauses.shape[0], d_clauses.shape[1],
                                      d_specs.data_ptr(), S, guard[1].data_ptr(), stride))
            env.synchronize()
            got = guard.cpu().numpy()
            tag = f"T={T} S={S} stride={stride}"
            np.testing.assert_array_equal(got[1:-1, :T], model[pick, :T], err_msg=tag)
            assert (got[1:-1, T:T16] == -1).all(), f"{tag}: padding"
            assert (got[1:-1, T16:] == GUARD).all(), f"{tag}: bytes beyond round_up(T, 16)"
            assert (got[0] == GUARD).all() and (got[-1] == GUARD).all(), f"{tag}: guard rows"
    env.close()


@pytest.fixture(scope="module")
def env2500():
    env = _env(cm.T_FIX)
    yield env
    env.close()


def test_wide_clause_strides_with_poisoned_padding(fix, env2500):
    clauses, specs, model = fix
    T, T16 = cm.T_FIX, signals.row_stride(cm.T_FIX)
    for stride, fill in ((T16, -1), (T16 + 16, POISON), (T16 + 4096, 0)):
        d_clauses = _clause_tensor(clauses, T, stride, fill)
        got = env2500.compose_signals(d_clauses[:, :T], specs[:-4], bind=False)  # a view: read in place
        assert tuple(got.shape) == (len(specs) - 4, T) and got.is_cuda and str(got.dtype) == "torch.int8"
        np.testing.assert_array_equal(got.cpu().numpy(), model[:-4], err_msg=f"clause_stride {stride}")
    assert env2500.num_strategies == 0  # bind=False bound nothing


def test_host_and_device_inputs_give_the_same_table(fix, env2500):
    import torch
    clauses, specs, model = fix
    T = cm.T_FIX
    ok = specs[:-4]
    d_plain = torch.from_numpy(clauses).cuda()           # [12, 2500]: rows not padded -> copied
    d_padded = _clause_tensor(clauses, T)[:, :T]         # read in place
    for c, s in ((clauses, ok), (d_plain, ok), (d_padded, _specs_tensor(ok)), (clauses.astype(np.int64), _specs_tensor(ok))):
        np.testing.assert_array_equal(env2500.compose_signals(c, s, bind=False).cpu().numpy(), model[:-4])
    # on the host the specs are checked; on the device they are the kernel's to refuse: rows of -1
    with pytest.raises(ValueError, match="n_in"):
        env2500.compose_signals(clauses, specs[-4:-2], bind=False)
    with pytest.raises(IndexError, match="outside"):
        env2500.compose_signals(clauses, specs[-2:], bind=False)
    got = env2500.compose_signals(d_padded, _specs_tensor(specs), bind=False).cpu().numpy()
    np.testing.assert_array_equal(got, model)
    assert (got[-4:] == -1).all()
    with pytest.raises(ValueError, match="columns"):
        env2500.compose_signals(clauses[:, :2000], ok, bind=False)
    with pytest.raises(TypeError, match="COMPOSE_DTYPE"):
        env2500.compose_signals(clauses, np.zeros((3, 128), np.uint8), bind=False)
    with pytest.raises(TypeError, match="COMPOSE_DTYPE"):
        env2500.compose_signals(clauses, _specs_tensor(ok).view(torch.int32), bind=False)
    with pytest.raises(TypeError, match="int8"):
        env2500.compose_signals(d_plain.float(), ok, bind=False)
    assert env2500.num_strategies == 0


def test_a_composed_table_is_a_clause_table(fix, env2500):
    """Trees deeper than four inputs: the second call reads what the first wrote, in place.  The second
    level sees codes, -1 / 7 / -128 (no codes: pos_invalid) and the rows of -1 of the invalid specs."""
    clauses, specs, model = fix
    T = cm.T_FIX
    first = env2500.compose_signals(clauses, _specs_tensor(specs), bind=False)
    rng = np.random.default_rng(21)
    S1 = len(specs)
    second = np.concatenate([
        signals.compose(rng.integers(0, S1, (20, 2)), cm._enter_exit, initial=1, invalid=7),
        signals.compose(rng.integers(0, S1, (12, 4)), cm._and4, initial=0, invalid=-1),
        signals.compose(rng.integers(0, S1, (12, 3)), cm._majority, initial=2, invalid=1)])
    want = cm.compose_table(cm.compose_table(clauses, specs, T), second, T)
    assert {-1, 0, 1, 2, 7} <= set(np.unique(want))
    got = env2500.compose_signals(first, second, bind=False)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_two_datasets_of_different_length_share_one_spec_array(fix):
    clauses, specs, model = fix
    ok = specs[:-4]
    sets = [_market(403, 40), _market(346, 41)]
    other = np.random.default_rng(9).integers(-1, 3, (cm.R_FIX, 346)).astype(np.int8)
    env = tb._env(sets, 8, "next_step", **dict(BASE, windows=None, episodes_between_dataset_switch=1))
    tables = env.compose_signals([clauses[:, :403], other], ok)
    assert isinstance(tables, list) and [tuple(t.shape) for t in tables] == [(len(ok), 403), (len(ok), 346)]
    np.testing.assert_array_equal(tables[0].cpu().numpy(), model[:-4, :403])
    np.testing.assert_array_equal(tables[1].cpu().numpy(), cm.compose_table(other, ok, 346))
    assert env.num_strategies == len(ok) and sorted(env._signals) == [0, 1]
    one = env.compose_signals(other, ok, dataset=1)  # one dataset again, the same S
    np.testing.assert_array_equal(one.cpu().numpy(), tables[1].cpu().numpy())
    with pytest.raises(ValueError, match="one number of strategies"):
        env.compose_signals(other, ok[:5], dataset=1)
    with pytest.raises(ValueError, match="list of 2"):
        env.compose_signals(other, ok)
    env.close()


@pytest.mark.parametrize("kernel_variant", [0, _abi.KV_ROLLOUT_PER_STEP], ids=["fused", "per-step"])
def test_pipeline_from_indicator_specs_to_backtest_records(kernel_variant):
    """256 envs x 300 steps (T = 403): build_indicators() -> build_signals(clauses, bind=False) ->
    compose_signals() + backtest_signals() against bind_signals(the model's table) + backtest_signals()
    on a twin."""
    T, N, K = 403, 256, 300
    feat, close = tb._data(31, T, 6)[:2]
    ind = np.concatenate([signals.indicators("ema", [3, 8, 21]), signals.indicators("rsi", [5, 14]),
                          signals.indicators("zscore", [10, 30])])
    rules = np.concatenate([
        signals.clauses(a=[0, 0, 1], b=[1, 2, 2], hi=[0.0, 0.2, 0.1], lo=[0.0, -0.2, -0.1], warmup=[8, 21, 21], latch=[0, 1, 1]),
        signals.clauses(a=[3, 4], hi=[65.0, 60.0], lo=[35.0, 40.0], warmup=[5, 14]),
        signals.clauses(a=[5, 6], hi=[1.0, 0.8], lo=[-1.0, -0.8], warmup=[9, 29])])
    pairs = np.array([(t, r) for t in (0, 1, 2) for r in (3, 4)])
    composed = np.concatenate([
        signals.compose(pairs, lambda trend, rsi: 2 if trend == 2 and rsi != 2 else 0 if trend == 0 and rsi != 0 else 1,
                        initial=1),
        signals.compose(np.array([(z, t) for z in (5, 6) for t in (0, 1, 2)]),
                        lambda z, trend: 2 if z == 2 else 0 if trend == 0 else signals.KEEP, initial=1),
        signals.compose([[0, 3, 5], [1, 4, 6]], cm._majority, initial=-1, invalid=1)])
    kw = dict(BASE, windows=5, kernel_variant=kernel_variant)
    a, b = tb._env((feat, close), N, "next_step", **kw), tb._env((feat, close), N, "next_step", **kw)
    bank = a.build_indicators(ind)
    clauses = a.build_signals(bank, rules, bind=False)
    model_clauses = rm.build_table(bank.cpu().numpy(), rules, T)
    np.testing.assert_array_equal(clauses.cpu().numpy(), model_clauses)
    assert a.num_strategies == 0
    built = a.compose_signals(clauses, composed)     # the [:, :T] view of the padded tensor: read in place
    want = cm.compose_table(model_clauses, composed, T)
    np.testing.assert_array_equal(built.cpu().numpy(), want)
    assert (want == 2).any() and (want == 0).any() and (want == -1).any() and (want == 1).any()
    b.bind_signals(want)
    assert a.num_strategies == b.num_strategies == len(composed)
    tb._both(a, b, lambda e: e.reset())
    got, ref = a.backtest_signals(K).numpy(), b.backtest_signals(K).numpy()
    tb._assert_same_records(got, ref, "composed against bound")
    tb._assert_same_env(a, b, "composed against bound")
    assert got["trades"].sum() > 0 and got["episodes"].sum() > 0 and got["steps"].sum() > N
    a.close()
    b.close()


def test_refusals(fix, env2500):
    import torch
    clauses, specs, model = fix
    env, T, T16 = env2500, cm.T_FIX, signals.row_stride(cm.T_FIX)
    err = lambda: env._lib.gte_last_error().decode()
    S, R = len(specs), cm.R_FIX
    d_clauses = _clause_tensor(clauses, T)
    d_specs = _specs_tensor(specs)
    W = T16 + 16
    whole = torch.full((S + R, W), GUARD, dtype=torch.int8, device="cuda")  # the table, and room for clauses behind it
    table = whole[:S]
    c, s, t = d_clauses.data_ptr(), d_specs.data_ptr(), table.data_ptr()
    INVALID, STATE = _abi.GTE_ERR_INVALID, _abi.GTE_ERR_STATE
    assert _raw(env, 0, c, R, T16, s, S, t + 8, W) == INVALID and "16-byte aligned" in err()
    assert _raw(env, 0, c + 8, R, T16, s, S, t, W) == INVALID and "16-byte aligned" in err()
    assert _raw(env, 0, c, R, T16, s + 2, S, t, W) == INVALID and "4-byte aligned" in err()
    assert _raw(env, 0, c, R, T16, s, S, t, T16 - 16) == INVALID and "row_stride" in err()
    assert _raw(env, 0, c, R, T16, s, S, t, T16 + 8) == INVALID and "row_stride" in err()
    assert _raw(env, 0, c, R, T16 - 16, s, S, t, W) == INVALID and "clause_stride" in err()
    assert _raw(env, 0, c, R, T16 + 8, s, S, t, W) == INVALID and "clause_stride" in err()
    assert _raw(env, 0, c, R, T16, s, 0, t, W) == INVALID and "n_specs" in err()
    assert _raw(env, 0, c, 0, T16, s, S, t, W) == INVALID and "n_clause_rows" in err()
    assert _raw(env, 1, c, R, T16, s, S, t, W) == INVALID and "out of range" in err()
    assert _raw(env, -1, c, R, T16, s, S, t, W) == INVALID and "out of range" in err()
    for null in ((0, s, t), (c, 0, t), (c, s, 0)):
        assert _raw(env, 0, null[0], R, T16, null[1], S, null[2], W) == INVALID and "NULL" in err()
    # the clause table inside the output, the output's last row the clause table's first, and in place
    inside = whole[S - 1:S - 1 + R]
    assert _raw(env, 0, inside.data_ptr(), R, W, s, S, t, W) == INVALID and "overlap" in err()
    assert _raw(env, 0, whole[5].data_ptr(), R, W, s, S, t, W) == INVALID and "overlap" in err()
    assert _raw(env, 0, t, S, W, s, S, t, W) == INVALID and "overlap" in err()
    assert _raw(env, 0, c, R, T16, s, 1, c + (R - 1) * T16, T16) == INVALID and "overlap" in err()
    # inside a stream capture: refused with its reason (the capture fails, the env works on)
    env.reset()
    seen = []

    def body(i):
        seen.append(_raw(env, 0, c, R, T16, s, S, t, W))
        seen.append(err())
        raise RuntimeError("refused inside the capture")
    with pytest.raises(Exception):
        env.capture_steps(body, 2)
    torch.cuda.synchronize()
    assert seen[0] == STATE and "stream capture" in seen[1], seen
    # a dataset that was never uploaded
    lib = env._lib
    cfg = make_config(n_envs=4, n_static=2, n_datasets=2, positions=[-1, 0, 1])
    h = C.c_void_p()
    _abi.check(lib, lib.gte_create(C.byref(cfg), C.byref(h)))
    try:
        feat, close = np.zeros((T, 4), np.float32), np.ones(T)
        _abi.check(lib, lib.gte_upload_dataset(h, 0, feat.ctypes.data, close.ctypes.data, None, None, T))
        args = (C.c_void_p(c), R, T16, C.c_void_p(s), S, C.c_void_p(t), W)
        assert lib.gte_compose_signals(h, 1, *args) == STATE and "never uploaded" in err()
        assert lib.gte_compose_signals(h, 2, *args) == INVALID and "out of range" in err()
        _abi.check(lib, lib.gte_synchronize(h))
        assert (whole == GUARD).all(), "a refused call wrote to the table"
        assert (d_clauses.cpu().numpy()[:, :T] == clauses).all()
        # ... and then it runs: the clause table right behind the output is no overlap
        behind = whole[S:]
        behind[:, :T] = d_clauses[:, :T]
        torch.cuda.synchronize()
        assert lib.gte_compose_signals(h, 0, C.c_void_p(behind.data_ptr()), R, W, C.c_void_p(s), S, C.c_void_p(t), W) \
            == _abi.GTE_OK
        _abi.check(lib, lib.gte_synchronize(h))
    finally:
        lib.gte_destroy(h)
    got = table.cpu().numpy()
    np.testing.assert_array_equal(got[:, :T], model)
    assert (got[:, T:T16] == -1).all() and (got[:, T16:] == GUARD).all()
    env.step(torch.zeros(env.num_envs, dtype=torch.int32, device="cuda"))
    host = _env(50, output="numpy")
    with pytest.raises(ValueError, match="needs output='torch'"):
        host.compose_signals(clauses[:, :50], specs[:-4])
    host.close()


def test_composed_rules_example(capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import backtest_composed_rules as ex
    leaders, table, clauses, composed = ex.main(envs=960, K=400, duration=48, top=3, details=True)
    out = capsys.readouterr().out
    assert "strategies composed from" in out and "trend and entry, by mean episode return" in out \
        and "enter / exit, by mean episode return" in out
    assert sorted(leaders) == ["enter / exit", "trend and entry"]
    n_first = int((composed["lut"] != signals.KEEP).all(axis=1).sum())
    for family, (index, score) in leaders.items():
        assert len(index) == 3 and np.isfinite(score).all() and (np.diff(score) <= 0).all()
        assert ((index < n_first) if family == "trend and entry" else (index >= n_first)).all()
    assert table.shape == (len(composed), clauses.shape[1]) and set(np.unique(clauses)) == {-1, 0, 1, 2}
    np.testing.assert_array_equal(table, cm.compose_table(clauses, composed, clauses.shape[1]))
    assert (table == 2).any() and (table == 1).any() and (table[:, 0] == -1).all()
    assert (composed["lut"] == signals.KEEP).any()
