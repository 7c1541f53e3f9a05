"""Indicator banks built on the device (gte_build_indicators, csrc/gte_indicators.hip): every bank is
compared float for float with the host model of the header's table (tests/indicator_model.py, held to a
second statement of it in tests/test_indicators_cpu.py) — over prefixes of the fixture around the 16-row
and 256-row edges, with guard rows and guard floats around the bank; every source, present and absent;
an input bank from the host, in place, and chained; two datasets; the bank through build_signals and a
backtest against the model's table; refusals; the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import indicator_model as im
import signal_rule_model as rm
import test_gpu_backtest as tb
from gym_trading_env_amd import _abi, signals
from gym_trading_env_amd.config import make_config
from replay import same_value

pytestmark = pytest.mark.gpu

GUARD = np.float32(-1234.5)
PIECE = 256   # rows of one piece of the kernel (IND_PIECE, gte_indicators.hip)
BASE = dict(positions=[-1, 0, 1], trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration=24, seed=11)
ROOTED = (signals.IND_STD, signals.IND_ZSCORE)   # the kinds that take the compiler's expansion of the f64 sqrt


@pytest.fixture(scope="module")
def fix():
    """(data, specs [557], the model's bank f32 [557, 2500]) — a prefix of the sources gives a prefix of
    every row (test_indicators_cpu.py), so one model bank serves every T"""
    data, specs = im.fixture()
    bank = im.build_bank(specs, data)
    bank.setflags(write=False)
    return data, specs, bank


def _env(data, T, n=4, hl=True, **kw):
    from gym_trading_env_amd.batched import BatchedTradingEnv
    ds = (data["features"][:T], data["close"][:T]) + ((data["high"][:T], data["low"][:T]) if hl else ())
    return BatchedTradingEnv(ds, num_envs=n, positions=[-1, 0, 1], windows=None, **kw)


def _specs_tensor(specs):
    import torch
    return torch.from_numpy(np.ascontiguousarray(specs).view(np.uint8).reshape(-1, 16).copy()).cuda()


def _raw(env, d, specs_ptr, n_specs, in_ptr, n_in, in_stride, bank_ptr, stride):
    return env._lib.gte_build_indicators(env._h, d, C.c_void_p(specs_ptr), n_specs, C.c_void_p(in_ptr) if in_ptr else None,
                                         n_in, in_stride, C.c_void_p(bank_ptr), stride)


def _assert_bank(got, want, specs, tag):
    """every float equal: bit pattern, or NaN for NaN — every kind, STD and ZSCORE included (see
    test_how_each_kind_is_held)"""
    ok = same_value(got, want)
    if not ok.all():
        s, t = np.argwhere(~ok)[0]
        raise AssertionError(f"{tag}: spec {s} {specs[s]} row {t}: {got[s, t]!r} != {want[s, t]!r} "
                             f"({int((~ok).sum())} floats differ)")


def _pick(specs, C):
    """1: an RSI; 3: a windowed sum on a feature column, an EMA of an input row, an invalid spec
    (a partial workgroup of four waves); else the whole fixture"""
    if C >= len(specs):
        return np.arange(len(specs))
    find = lambda kind, src, n: int(np.flatnonzero((specs["kind"] == kind) & (specs["source"] == src) &
                                                   (specs["n"] == n))[0])
    one = [find(signals.IND_RSI, signals.SRC_CLOSE, 15)]
    return np.array(one if C == 1 else [find(signals.IND_STD, signals.SRC_FEATURE, 15),
                                        find(signals.IND_EMA, signals.SRC_INPUT, 16), len(specs) - 7])


@pytest.mark.parametrize("T", [2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500])
def test_prefixes_of_the_fixture_with_guards(T, fix):
    """n_specs = 1, 3, 557 x ind_stride minimal and minimal + 48; one guard row before and after the bank
    and the floats beyond round_up(T, 16) hold their pattern before the call and after it; the padding
    is 0."""
    import torch
    data, specs, model = fix
    env = _env(data, T)
    assert env.n_obs % 4 != 0   # (feature rows are not 16-byte aligned)
    inputs = torch.from_numpy(signals.pad_bank(data["inputs"][:, :T])).cuda()
    T16 = signals.bank_stride(T)
    for n_specs in (1, 3, len(specs)):
        pick = _pick(specs, n_specs)
        d_specs = _specs_tensor(specs[pick])
        for stride in (T16, T16 + 48):
            guard = torch.full((n_specs + 2, stride), float(GUARD), dtype=torch.float32, device="cuda")
            assert guard[1].data_ptr() % 16 == 0
            _abi.check(env._lib, _raw(env, 0, d_specs.data_ptr(), n_specs, inputs.data_ptr(), 2, inputs.shape[1],
                                      guard[1].data_ptr(), stride))
            env.synchronize()
            got = guard.cpu().numpy()
            tag = f"T={T} n_specs={n_specs} stride={stride}"
            _assert_bank(got[1:-1, :T], model[pick, :T], specs[pick], tag)
            pad = got[1:-1, T:T16]
            assert (pad == 0).all() and not np.signbit(pad).any(), f"{tag}: padding"
            assert (got[1:-1, T16:] == GUARD).all(), f"{tag}: floats beyond round_up(T, 16)"
            assert (got[0] == GUARD).all() and (got[-1] == GUARD).all(), f"{tag}: guard rows"
    env.close()


@pytest.fixture(scope="module")
def env2500(fix):
    env = _env(fix[0], im.T_FIX)
    yield env
    env.close()


def test_how_each_kind_is_held(fix, env2500):
    """Every kind is held to equality on every float.  STD and ZSCORE go through the compiler's expansion
    of the f64 square root, which was allowed the f32 neighbour in at most 1 of 10 000 floats until it was
    measured: on an MI355X 0 of the fixture's 275 000 STD / ZSCORE floats differ from the model (the model
    against itself has none, test_indicators_cpu.py), so these two kinds are held like the others.  The
    count is still printed."""
    data, specs, model = fix
    got = env2500.build_indicators(specs[:-7], inputs=data["inputs"])   # (host specs: the valid ones)
    assert tuple(got.shape) == (len(specs) - 7, im.T_FIX) and got.is_cuda and str(got.dtype) == "torch.float32"
    assert got.stride(0) == signals.bank_stride(im.T_FIX) and got.data_ptr() % 16 == 0
    got, want, sp = got.cpu().numpy(), model[:-7], specs[:-7]
    rooted = np.isin(sp["kind"], ROOTED)
    unequal = int((~same_value(got[rooted], want[rooted])).sum())
    print(f"STD / ZSCORE floats unequal to the model: {unequal} of {int(rooted.sum()) * im.T_FIX}")
    assert unequal == 0
    _assert_bank(got, want, sp, "the whole fixture")
    # the same from a device spec tensor, the invalid specs included: rows of NaN
    got = env2500.build_indicators(_specs_tensor(specs), inputs=data["inputs"]).cpu().numpy()
    _assert_bank(got, model, specs, "device specs")
    assert np.isnan(got[-7:]).all()


def test_sources_present_and_absent(fix, env2500):
    import torch
    data, specs, model = fix
    T = 300
    hl = (specs["source"] == signals.SRC_HIGH) | (specs["source"] == signals.SRC_LOW)
    uses_input = specs["source"] == signals.SRC_INPUT
    valid = np.arange(len(specs)) < len(specs) - 7
    # no high / low: NaN rows from a device spec tensor, ValueError from host specs
    env = _env(data, T, hl=False)
    got = env.build_indicators(_specs_tensor(specs), inputs=data["inputs"][:, :T]).cpu().numpy()
    assert np.isnan(got[hl]).all()
    _assert_bank(got[~hl], model[~hl, :T], specs[~hl], "no high / low")
    with pytest.raises(ValueError, match="does not have"):
        env.build_indicators(specs[valid], inputs=data["inputs"][:, :T])
    # no input bank: the same for the specs that name one
    got = env.build_indicators(_specs_tensor(specs)).cpu().numpy()
    assert np.isnan(got[uses_input | hl]).all()
    _assert_bank(got[~(uses_input | hl)], model[~(uses_input | hl), :T], specs[~(uses_input | hl)], "no input")
    with pytest.raises(ValueError, match="input rows"):
        env.build_indicators(specs[valid & ~hl])
    ok = valid & ~hl & ~uses_input
    _assert_bank(env.build_indicators(specs[ok]).cpu().numpy(), model[ok, :T], specs[ok], "host specs")
    for i, what in ((-4, "feature columns"), (-3, "input rows"), (-7, "unknown"), (-6, "window"), (-2, "unknown")):
        with pytest.raises(ValueError, match=what):
            env.build_indicators(specs[[0, i]], inputs=data["inputs"][:, :T])
    with pytest.raises(ValueError, match="columns"):
        env.build_indicators(specs[ok], inputs=data["inputs"][:, :T - 1])
    with pytest.raises(TypeError, match="INDICATOR_DTYPE"):
        env.build_indicators(np.zeros((3, 4), np.int32))
    env.close()
    # the input bank: NumPy, an unpadded CUDA tensor (copied), a padded one read in place; int32 specs
    env, T = env2500, im.T_FIX
    want, sp = model[uses_input & valid], specs[uses_input & valid]
    padded = torch.from_numpy(signals.pad_bank(data["inputs"])).cuda()
    d32 = _specs_tensor(sp).view(torch.int32)
    assert tuple(d32.shape) == (len(sp), 4)
    for x, s in ((data["inputs"], sp), (torch.from_numpy(data["inputs"]).cuda(), sp), (padded[:, :T], d32)):
        _assert_bank(env.build_indicators(s, inputs=x).cpu().numpy(), want, sp, "input bank")
    # chained: an EMA of an EMA that an earlier call wrote equals the model applied twice
    first = env.build_indicators(signals.indicators("ema", [12, 26]))
    second = env.build_indicators(signals.indicators(["ema", "diff"], [9, 1], "input", [1, 0]), inputs=first)
    once = np.stack([im.row("ema", data["close"], n) for n in (12, 26)])
    assert same_value(first.cpu().numpy(), once).all()
    twice = np.stack([im.row("ema", once[1].astype(np.float64), 9), im.row("diff", once[0].astype(np.float64), 1)])
    assert same_value(second.cpu().numpy(), twice).all()


def test_two_datasets_of_different_length_share_one_spec_array(fix):
    data, specs, model = fix
    rng = np.random.default_rng(9)
    T0, T1 = 403, 346
    close1 = 50 * np.exp(np.cumsum(rng.normal(0, 2e-2, T1)))
    other = dict(close=close1, high=close1 * 1.01, low=close1 * 0.99,
                 features=rng.normal(0, 1, (T1, 3)).astype(np.float32),
                 inputs=np.cumsum(rng.normal(0, 1, (2, T1)), 1).astype(np.float32))
    sets = [(data["features"][:T0], data["close"][:T0], data["high"][:T0], data["low"][:T0]),
            (other["features"], other["close"], other["high"], other["low"])]
    env = tb._env(sets, 8, "next_step", **dict(BASE, windows=None, episodes_between_dataset_switch=1))
    sp = specs[:-7]
    banks = env.build_indicators(sp, inputs=[data["inputs"][:, :T0], other["inputs"]])
    assert isinstance(banks, list) and [tuple(b.shape) for b in banks] == [(len(sp), T0), (len(sp), T1)]
    _assert_bank(banks[0].cpu().numpy(), model[:-7, :T0], sp, "dataset 0")
    _assert_bank(banks[1].cpu().numpy(), im.build_bank(sp, other), sp, "dataset 1")
    no_in = sp[sp["source"] != signals.SRC_INPUT]
    one = env.build_indicators(no_in, dataset=1)
    assert same_value(one.cpu().numpy(), banks[1].cpu().numpy()[sp["source"] != signals.SRC_INPUT]).all()
    with pytest.raises(ValueError, match="list of 2"):
        env.build_indicators(sp, inputs=other["inputs"])
    with pytest.raises(IndexError):
        env.build_indicators(no_in, dataset=2)
    env.close()


@pytest.mark.parametrize("kernel_variant", [0, _abi.KV_ROLLOUT_PER_STEP], ids=["fused", "per-step"])
def test_through_build_signals_and_a_backtest(kernel_variant):
    """96 envs x 40 steps on the config of test_gpu_signal_build.py (T = 403): build_indicators() +
    build_signals() + backtest_signals() against bind_signals(the model's table) + backtest_signals()
    on a twin."""
    T, N, K = 403, 96, 40
    feat, close = tb._data(31, T, 6)[:2]
    specs = np.concatenate([signals.indicators("ema", [3, 8, 21]), signals.indicators("rsi", [5, 14]),
                            signals.indicators("zscore", [10, 30]), signals.indicators("value", source="feature", column=4)])
    rules = np.concatenate([
        signals.rules(a=[0, 0, 1], b=[1, 2, 2], hi=[0.0, 0.2, 0.1], lo=[0.0, -0.2, -0.1], warmup=[8, 21, 21],
                      pos_up=2, pos_down=0, pos_neutral=-1, latch=[0, 1, 1]),
        signals.rules(a=[3, 4], b=-1, hi=70.0, lo=30.0, warmup=[5, 14], pos_up=0, pos_down=2, pos_neutral=-1, latch=True),
        signals.rules(a=[5, 6, 7], b=-1, hi=[1.0, 1.5, 0.5], lo=[-1.0, -1.5, -0.5], warmup=[9, 29, 0], pos_up=2,
                      pos_down=0, pos_neutral=1)])
    kw = dict(BASE, windows=5, kernel_variant=kernel_variant)
    a, b = tb._env((feat, close), N, "next_step", **kw), tb._env((feat, close), N, "next_step", **kw)
    bank = a.build_indicators(specs)
    host_bank = bank.cpu().numpy()
    model_bank = im.build_bank(specs, dict(close=close, high=None, low=None, features=feat, inputs=None))
    _assert_bank(host_bank, model_bank, specs, "bank")
    built = a.build_signals(bank, rules)    # the [:, :T] view of the padded tensor: read in place
    want = rm.build_table(host_bank, rules, T)
    np.testing.assert_array_equal(built.cpu().numpy(), want)
    assert (want == 2).any() and (want == 0).any() and (want == -1).any() and (want == 1).any()
    b.bind_signals(want)
    assert a.num_strategies == b.num_strategies == len(rules)
    tb._both(a, b, lambda e: e.reset())
    got, ref = a.backtest_signals(K).numpy(), b.backtest_signals(K).numpy()
    tb._assert_same_records(got, ref, "built against bound")
    tb._assert_same_env(a, b, "built against bound")
    assert got["trades"].sum() > 0 and got["episodes"].sum() > 0 and got["steps"].sum() > N
    a.close()
    b.close()


def test_refusals(fix, env2500):
    import torch
    data, specs, model = fix
    env, T, T16 = env2500, im.T_FIX, signals.bank_stride(im.T_FIX)
    err = lambda: env._lib.gte_last_error().decode()
    n = 12
    pick = np.arange(0, len(specs), len(specs) // n)[:n]
    d_specs = _specs_tensor(specs[pick])
    inputs = torch.from_numpy(signals.pad_bank(data["inputs"])).cuda()
    whole = torch.full((n + 2, T16 + 16), float(GUARD), dtype=torch.float32, device="cuda")
    bank = whole[2:]
    s, i, o = d_specs.data_ptr(), inputs.data_ptr(), bank.data_ptr()
    W = T16 + 16
    INVALID, STATE = _abi.GTE_ERR_INVALID, _abi.GTE_ERR_STATE
    assert _raw(env, 0, s, n, i, 2, T16, o + 8, W) == INVALID and "16-byte aligned" in err()
    assert _raw(env, 0, s, n, i + 8, 2, T16, o, W) == INVALID and "16-byte aligned" in err()
    assert _raw(env, 0, s + 2, n, i, 2, T16, o, W) == INVALID and "4-byte aligned" in err()
    assert _raw(env, 0, s, n, i, 2, T16, o, T16 - 16) == INVALID and "ind_stride" in err()
    assert _raw(env, 0, s, n, i, 2, T16, o, T16 + 2) == INVALID and "ind_stride" in err()
    assert _raw(env, 0, s, n, i, 2, T16 - 16, o, W) == INVALID and "input_stride" in err()
    assert _raw(env, 0, s, n, i, 2, T16 + 2, o, W) == INVALID and "input_stride" in err()
    assert _raw(env, 0, s, 0, i, 2, T16, o, W) == INVALID and "n_specs" in err()
    assert _raw(env, 0, s, n, 0, 2, T16, o, W) == INVALID and "exactly when" in err()
    assert _raw(env, 0, s, n, i, 0, T16, o, W) == INVALID and "exactly when" in err()
    assert _raw(env, 0, s, n, i, -1, T16, o, W) == INVALID and "n_inputs" in err()
    assert _raw(env, 0, 0, n, i, 2, T16, o, W) == INVALID and "NULL" in err()
    assert _raw(env, 0, s, n, i, 2, T16, 0, W) == INVALID and "NULL" in err()
    assert _raw(env, 1, s, n, i, 2, T16, o, W) == INVALID and "out of range" in err()
    assert _raw(env, -1, s, n, i, 2, T16, o, W) == INVALID and "out of range" in err()
    # the input inside the output, and the output's first row the input's last
    assert _raw(env, 0, s, n, o + 4 * W, 2, W, o, W) == INVALID and "overlap" in err()
    assert _raw(env, 0, s, n, whole.data_ptr(), 3, W, o, W) == INVALID and "overlap" in err()
    # inside a stream capture: refused with its reason (the capture fails, the env works on)
    env.reset()
    seen = []

    def body(k):
        seen.append(_raw(env, 0, s, n, i, 2, T16, o, W))
        seen.append(err())
        raise RuntimeError("refused inside the capture")
    with pytest.raises(Exception):
        env.capture_steps(body, 2)
    torch.cuda.synchronize()
    assert seen[0] == STATE and "stream capture" in seen[1], seen
    assert (whole == float(GUARD)).all(), "a refused call wrote to the bank"
    # ... and then it runs: the input two rows in front of the output (adjacent, not overlapping)
    whole[:2, :T] = torch.from_numpy(data["inputs"]).cuda()
    _abi.check(env._lib, _raw(env, 0, s, n, whole.data_ptr(), 2, W, o, W))
    env.synchronize()
    got = whole.cpu().numpy()
    _assert_bank(got[2:, :T], model[pick], specs[pick], "after the refusals")
    assert (got[2:, T:T16] == 0).all() and (got[2:, T16:] == GUARD).all() and (got[:2, T:] == GUARD).all()
    env.step(torch.zeros(env.num_envs, dtype=torch.int32, device="cuda"))
    # a dataset that was never uploaded
    lib = env._lib
    cfg = make_config(n_envs=4, n_static=2, n_datasets=2, positions=[-1, 0, 1])
    h = C.c_void_p()
    _abi.check(lib, lib.gte_create(C.byref(cfg), C.byref(h)))
    try:
        feat, close = np.zeros((T, 4), np.float32), np.ones(T)
        _abi.check(lib, lib.gte_upload_dataset(h, 0, feat.ctypes.data, close.ctypes.data, None, None, T))
        args = (C.c_void_p(s), n, C.c_void_p(i), 2, T16, C.c_void_p(o), W)
        assert lib.gte_build_indicators(h, 1, *args) == STATE and "never uploaded" in err()
        assert lib.gte_build_indicators(h, 2, *args) == INVALID and "out of range" in err()
        assert lib.gte_build_indicators(h, 0, *args) == _abi.GTE_OK
        _abi.check(lib, lib.gte_synchronize(h))
    finally:
        lib.gte_destroy(h)
    host = _env(data, 50, output="numpy")
    with pytest.raises(ValueError, match="needs output='torch'"):
        host.build_indicators(signals.indicators("sma", 5))
    host.close()


def test_indicator_sweep_example(capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import backtest_indicator_sweep as ex
    mean, family, bank, table, specs, rules = ex.main(strategies=48, replicas=2, K=400, duration=48, details=True)
    assert mean.shape == (48,) and np.isfinite(mean).all() and mean.std() > 0
    out = capsys.readouterr().out
    assert all(name in out for name in ex.FAMILIES) and "mean episode return" in out
    assert sorted(set(family)) == [0, 1, 2] and set(specs["kind"]) == {signals.IND_EMA, signals.IND_RSI, signals.IND_ZSCORE}
    assert bank.shape == (len(specs), 6000) and table.shape == (48, 6000)
    np.testing.assert_array_equal(table, rm.build_table(bank, rules, 6000))
    for f in range(3):
        assert (table[family == f] == 2).any() and (table[family == f] == 0).any()
