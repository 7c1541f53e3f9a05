"""Exit rules on the GPU (gte_bind_exit_rules, csrc/gte_exits.hip): `backtest_signals(K)` with rules
bound against a twin that reads its rows back after every step, chooses the action with
tests/exit_model.py from the GPU's own values and calls `step()` — statistics records, env state and
exit state bit for bit; the fused path against the per-step one; chunks; `signal_actions()` twice;
graph capture; unbinding; the reference-made fixtures; refusals."""
import ctypes as C

import numpy as np
import pytest

import backtest_model as bm
import exit_model as xm
import replay
import test_gpu_backtest as tb
from gym_trading_env_amd import _abi, signals as sig

pytestmark = pytest.mark.gpu

MODES = tb.MODES
N, T, K, S = 200, 240, 96, 5
BASE = dict(positions=[-1, 0, 1], trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration=24, seed=11)
P = 3


def _data(seed, rows=T):
    return tb._data(seed, rows, 6, sigma=1.2e-2)[:2]


def _table(seed, rows=T, strategies=S):
    """int8 [S, T]: runs of one position index (so that a latch has something to wait for), with hold
    and extreme bytes sprinkled in."""
    rng = np.random.default_rng(seed)
    t = np.empty((strategies, rows), np.int8)
    for s in range(strategies):
        row = []
        while len(row) < rows:
            row += [int(rng.integers(0, P))] * int(rng.integers(1, 9))
        t[s] = row[:rows]
    t[rng.random(t.shape) < 0.05] = -1
    t[rng.random(t.shape) < 0.02] = -128
    t[rng.random(t.shape) < 0.02] = 127
    return t


def _rules(n, seed=3):
    """n rules: each exit alone, mixtures, a rule that is off, exit positions flat and short."""
    rng = np.random.default_rng(seed)
    r = xm.make_rules(stop_loss=[0.012, 0, 0, 0, 0.02, 0.015, 0.01], trailing=[0, 0.01, 0, 0, 0.012, 0, 0.01],
                      take_profit=[0, 0, 0.012, 0, 0.02, 0.01, np.nan], max_hold=[0, 0, 0, 5, 9, -3, 0],
                      exit_position=[1, 1, 1, 1, 0, 1, 3])
    out = np.resize(r, n)
    if n > len(r):
        out["stop_loss"][len(r):] = rng.uniform(0.005, 0.03, n - len(r)).astype(np.float32)
    return out


def _bindable(rules):
    """rules as bind_exits takes them: the host array where every exit_position names a position (then it
    is checked), else the same bytes as a CUDA tensor — the caller's contract, a rule may be off."""
    import torch
    rules = np.ascontiguousarray(rules)
    if ((rules["exit_position"] >= 0) & (rules["exit_position"] < P)).all():
        return rules.view(sig.EXIT_DTYPE)
    return torch.from_numpy(rules.view(np.uint8).reshape(-1, 32).copy()).cuda()


def _phase_one(env, gen, steps=6):
    """tb._phase for one env: with the same generator seed it takes the same actions."""
    import torch
    for i in range(steps):
        if i in (1, 3):
            env.reset(mask=(np.arange(N) % 3 == i // 2).astype(np.uint8))
        env.step(torch.randint(-1, P, (N,), dtype=torch.int32, device="cuda", generator=gen))


def _maps(explicit, n_rules, seed=5):
    """(strategy, rule_of_env): explicit int32 [N] maps, or None / None (the library's defaults), or with
    explicit == "strategy" an explicit strategy and the default rule map, strategy[e] % n_rules."""
    if not explicit:
        return None, None
    rng = np.random.default_rng(seed)
    strategy, rule_of_env = rng.integers(0, S, N).astype(np.int32), rng.integers(0, n_rules, N).astype(np.int32)
    return (strategy, None) if explicit == "strategy" else (strategy, rule_of_env)


class _ModelLookup:
    """The [K, N] actions of twin a, made one row at a time by exit_model from the rows the env stands
    on when step k is about to run (what tb._single_step_columns asks for)."""

    def __init__(self, env, tables, strategy, model, steps):
        self.env, self.tables, self.strategy, self.model, self.shape, self.rows = env, tables, strategy, model, (steps,), []

    def row(self):
        st = self.env.state
        raw = xm.raw_bytes(self.tables, self.strategy, st("idx"), st("dataset_index"))
        return self.model.actions(raw, st("episode"), st("step"), st("portfolio_valuation"), st("position_index"),
                                  st("needs_reset"))

    def __getitem__(self, k):
        import torch
        assert k == len(self.rows)
        self.rows.append(self.row())
        return torch.from_numpy(self.rows[-1]).cuda()


def _model(rules, strategy, rule_of_env, n=N):
    return xm.ExitModel(n, rules, P, xm.rule_of(n, len(rules), strategy, S, rule_of_env))


def _assert_exit_state(got, want, tag):
    got = got if isinstance(got, np.ndarray) else got.numpy()
    assert got.dtype == want.dtype == np.dtype(_abi.EXIT_STATE_DTYPE)
    for f in want.dtype.names:
        if want[f].dtype.kind == "f":
            replay.assert_same_value(np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f]), f"{tag}: exit state {f}")
        else:
            np.testing.assert_array_equal(got[f], want[f], err_msg=f"{tag}: exit state {f}")


def _prepare(data, tables, mode, kw, before=None):
    """Twins (a: single steps, b: backtest_signals) with tables bound, reset, out of phase."""
    import torch
    a, b = tb._twins(data, N, mode, **kw)
    tb._both(a, b, lambda e: e.bind_signals(tables))
    tb._both(a, b, lambda e: e.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    tb._phase(a, b, N, P, gen)
    if before:
        tb._both(a, b, before)
    return a, b, gen


def _against_model(data, tables, mode, kw, tag, n_rules, explicit, k=K, before=None):
    """-> (model records, step dicts, the actions twin a took, the model)."""
    import torch
    a, b, gen = _prepare(data, tables, mode, kw, before=before)
    rules = _rules(n_rules)
    strategy, rule_of_env = _maps(explicit, n_rules)
    b.bind_exits(_bindable(rules), rule_of_env=rule_of_env)
    model = _model(rules, strategy, rule_of_env)
    acts = _ModelLookup(a, tables, strategy, model, k)
    recs, steps = tb._single_step_columns(a, acts)
    want = [bm.run(r, s) for r, s in zip(recs, steps)]
    stats = b.backtest_signals(k, strategy=strategy)
    tb._assert_records(stats, want, tag)
    tb._assert_same_env(a, b, tag)
    _assert_exit_state(b.exit_state(), model.state, tag)
    # the views show the same state as the one-transfer read
    view, host = b.exit_state(), b.exit_state().numpy()
    np.testing.assert_array_equal(view.exits.cpu().numpy(), host["exits"])
    np.testing.assert_array_equal(view.held.cpu().numpy(), host["held"])
    assert replay.same_value(view.entry.cpu().numpy(), host["entry"]).all()
    # ... and the step after, decided on either side, agrees too
    nxt = acts.row()
    np.testing.assert_array_equal(b.signal_actions(strategy=strategy).cpu().numpy(), nxt, err_msg=f"{tag}: the decision after")
    _assert_exit_state(b.exit_state(), model.state, f"{tag}: after the decision after")
    a.close()
    b.close()
    return want, steps, np.stack(acts.rows), model


SHAPES = [(None, 1, False), (5, 1, True), (None, S, True), (5, S, False), (None, 7, False), (5, 7, True),
          (5, 3, "strategy"), (None, 7, "strategy")]


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
@pytest.mark.parametrize("windows,n_rules,explicit", SHAPES)
def test_backtest_with_exits_equals_model_over_single_steps(windows, n_rules, explicit, mode):
    """N = 200: a partial last wave and more than one workgroup; T = 240: fifteen 16-row pieces;
    24-step episodes over K = 96: every env resets several times inside the launch.  One rule for all,
    as many rules as strategies, a number that divides neither; explicit and default maps."""
    tables = _table(21)
    want, steps, acts, model = _against_model(_data(31), tables, mode, dict(BASE, windows=windows),
                                              f"R={n_rules} W={windows} {mode}", n_rules, explicit)
    exits = model.state["exits"].sum(axis=0)
    assert exits.sum() > 0, exits
    if n_rules == 7 and mode is not None:
        assert (exits > 0).all(), exits     # every kind fired
    assert (model.state["latched"] == 1).any() and sum(r["episodes"] for r in want) > (N if mode else 0)
    if mode == "next_step":
        assert any(s.get("reset") and not s["stepped"] for e in steps for s in e)


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
@pytest.mark.parametrize("k", [1, 2])
def test_one_and_two_steps(k, mode):
    """K = 1: decision + step + fold only; K = 2: one fused step before it."""
    _against_model(_data(34), _table(22), mode, dict(BASE, windows=5), f"K={k} {mode}", 7, True, k=k)


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_three_datasets_with_a_table_each(mode):
    sets = [_data(40 + d, T - 37 * d) for d in range(3)]
    tables = [_table(50 + d, len(c)) for d, (_, c) in enumerate(sets)]
    kw = dict(BASE, windows=5, episodes_between_dataset_switch=1)
    want, steps, acts, model = _against_model(sets, tables, mode, kw, f"3 datasets {mode}", 7, False)
    assert model.state["exits"].sum() > 0


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_pending_limit_orders_fill_as_entries(mode):
    data = tb._data(33, T, 6, sigma=1.2e-2)
    want, steps, acts, model = _against_model(data, _table(23), mode, dict(BASE, windows=5), f"orders {mode}", 7, True,
                                              before=tb._add_orders)
    assert sum(r["trades"] for r in want) > 0 and model.state["exits"].sum() > 0


def _pair(mode, n_rules=7, explicit=True, **over):
    """Two envs in the same state with the same tables and rules bound -> (x, y, strategy)."""
    import torch
    kw = dict(BASE, windows=5)
    data = _data(35)
    x, y = tb._env(data, N, mode, **kw), tb._env(data, N, mode, **dict(kw, **over))
    tb._both(x, y, lambda e: e.bind_signals(_table(24)))
    tb._both(x, y, lambda e: e.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    tb._phase(x, y, N, P, gen)
    strategy, rule_of_env = _maps(explicit, n_rules)
    tb._both(x, y, lambda e: e.bind_exits(_bindable(_rules(n_rules)), rule_of_env=rule_of_env))
    return x, y, strategy


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_fused_and_per_step_paths_give_the_same_bits(mode, capfd, monkeypatch):
    monkeypatch.setenv("GTE_DEBUG_GEOMETRY", "1")
    x, y, strategy = _pair(mode, log_steps=8)
    capfd.readouterr()
    fused = x.backtest_signals(K, strategy=strategy).numpy()
    assert f"rollout path: backtest signals summary, {K} steps" in capfd.readouterr().err
    stepwise = y.backtest_signals(K, strategy=strategy).numpy()
    assert f"rollout path: backtest signals per-step, {K} steps" in capfd.readouterr().err
    tb._assert_same_records(fused, stepwise, f"{mode}: fused against per-step")
    tb._assert_same_env(x, y, f"{mode}: fused against per-step")
    _assert_exit_state(x.exit_state(), y.exit_state().numpy(), f"{mode}: fused against per-step")
    assert x.exit_state().numpy()["exits"].sum() > 0
    x.close()
    y.close()


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_chunked_calls(mode):
    x, y, strategy = _pair(mode)
    whole = x.backtest_signals(96, strategy=strategy).numpy()
    y.backtest_signals(40, strategy=strategy)
    tb._assert_same_records(y.backtest_signals(56, strategy=strategy, resume=True).numpy(), whole, f"{mode}: 40 + 56")
    tb._assert_same_env(x, y, f"{mode}: chunks")
    _assert_exit_state(x.exit_state(), y.exit_state().numpy(), f"{mode}: chunks")
    assert whole["steps"].sum() > 0 and x.exit_state().numpy()["exits"].sum() > 0
    x.close()
    y.close()


def _unaligned(rules):
    """the rules' bytes as a CUDA uint8 [R, 32] tensor that starts 4 bytes into its buffer: all the ABI asks"""
    import torch
    raw = torch.from_numpy(np.ascontiguousarray(rules).view(np.uint8).reshape(-1).copy())
    buf = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device="cuda")
    view = buf[4:4 + raw.numel()]
    view.copy_(raw)
    view = view.view(-1, 32)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_a_decision_made_by_signal_actions_is_taken_by_the_fused_backtest(mode, capfd, monkeypatch):
    """signal_actions() memoises its decision for the row the env stands on; a backtest_signals() that follows
    must act on that memo in its first step — fused or per-step — and decide nothing twice: a stop that the
    lookup fired (latched, counted) is executed.  x: fused, its rules bound from a base that is only 4-byte
    aligned; y: per-step (log_steps); a: single steps with the model."""
    import torch
    monkeypatch.setenv("GTE_DEBUG_GEOMETRY", "1")
    data, kw, tables = _data(35), dict(BASE, windows=5), _table(24)
    envs = [tb._env(data, N, mode, **kw), tb._env(data, N, mode, **kw), tb._env(data, N, mode, **dict(kw, log_steps=8))]
    a, x, y = envs
    for e in envs:
        e.bind_signals(tables)
        e.reset()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(23)
        _phase_one(e, gen)
    rules = _rules(7)
    strategy, rule_of_env = _maps(True, 7)
    x.bind_exits(_unaligned(rules), rule_of_env=rule_of_env)
    y.bind_exits(_bindable(rules), rule_of_env=rule_of_env)
    model = _model(rules, strategy, rule_of_env)
    look = _ModelLookup(a, tables, strategy, model, 0)
    for i in range(40):  # on to a row where the decision itself fires an exit for some env
        fired = model.state["exits"].sum()
        row = look.row()
        fired = model.state["exits"].sum() - fired
        if i >= 5 and fired > 0:
            break
        a.step(torch.from_numpy(row).cuda())
        tb._both(x, y, lambda e: e.backtest_signals(1, strategy=strategy, resume=i > 0))
    assert fired > 0, "no exit fired in a decision: the test shows nothing"
    tb._assert_same_env(a, x, f"{mode}: before the lookup")
    for e in (x, y):  # the lookup whose actions the caller throws away
        np.testing.assert_array_equal(e.signal_actions(strategy=strategy).cpu().numpy(), row, err_msg=f"{mode}: lookup")
        _assert_exit_state(e.exit_state(), model.state, f"{mode}: after the lookup")
    capfd.readouterr()
    fused = x.backtest_signals(K, strategy=strategy, resume=True).numpy()
    assert f"rollout path: backtest signals summary, {K} steps" in capfd.readouterr().err
    stepwise = y.backtest_signals(K, strategy=strategy, resume=True).numpy()
    assert f"rollout path: backtest signals per-step, {K} steps" in capfd.readouterr().err
    a.step(torch.from_numpy(row).cuda())
    for _ in range(K - 1):
        a.step(torch.from_numpy(look.row()).cuda())
    tb._assert_same_records(fused, stepwise, f"{mode}: fused against per-step after a lookup")
    tb._assert_same_env(x, y, f"{mode}: fused against per-step after a lookup")
    tb._assert_same_env(a, x, f"{mode}: fused against single steps with the model")
    _assert_exit_state(x.exit_state(), model.state, f"{mode}: fused against the model")
    _assert_exit_state(y.exit_state(), model.state, f"{mode}: per-step against the model")
    for e in envs:
        e.close()


def test_signal_actions_twice_equals_itself_and_the_model():
    import torch
    x, y, strategy = _pair("next_step", explicit=False)
    y.close()
    model = _model(_rules(7), None, None)
    look = _ModelLookup(x, [_table(24)], None, model, 0)
    for k in range(30):
        first = x.signal_actions().clone()
        state = x.exit_state().numpy()
        second = x.signal_actions()
        assert torch.equal(first, second), k
        assert x.exit_state().numpy().tobytes() == state.tobytes(), k
        np.testing.assert_array_equal(first.cpu().numpy(), look.row(), err_msg=f"step {k}")
        _assert_exit_state(state, model.state, f"step {k}")
        if k % 7 == 3:
            x.step(torch.full((N,), -1, dtype=torch.int32, device="cuda"))  # a step the rules did not decide: a gap
        x.step(first)
    assert model.state["exits"].sum() > 0
    x.close()


def test_signal_actions_captured_with_step_replays_like_eager():
    import torch
    eager, graphed, strategy = _pair("next_step", explicit=False)
    buf = torch.empty(N, dtype=torch.int32, device="cuda")
    before = graphed.state("step").copy()
    g = graphed.capture_steps(lambda i: graphed.step(graphed.signal_actions(out=buf)), 4)
    np.testing.assert_array_equal(graphed.state("step"), before)  # the capture ran nothing
    for _ in range(8):
        for _ in range(4):
            eager.step(eager.signal_actions())
        g.replay()
        tb._assert_same_env(eager, graphed, "replay against eager")
        _assert_exit_state(graphed.exit_state(), eager.exit_state().numpy(), "replay against eager")
    assert eager.exit_state().numpy()["exits"].sum() > 0
    eager.close()
    graphed.close()


@pytest.mark.parametrize("mode", MODES, ids=lambda m: str(m))
def test_after_unbinding_records_equal_a_twin_that_never_had_rules(mode):
    import torch
    x, y, strategy = _pair(mode)
    plain = tb._env(_data(35), N, mode, **dict(BASE, windows=5))
    plain.bind_signals(_table(24))
    plain.reset()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    _phase_one(plain, gen)
    tb._assert_same_env(x, plain, f"{mode}: before")
    x.signal_actions(strategy=strategy)  # the rules decide once (that moves exit state only) ...
    x.bind_exits(None)                   # ... and go
    assert x.num_exit_rules == 0
    unbound = x.backtest_signals(K, strategy=strategy).numpy()
    tb._assert_same_records(unbound, plain.backtest_signals(K, strategy=strategy).numpy(), f"{mode}: unbound")
    tb._assert_same_env(x, plain, f"{mode}: unbound")
    np.testing.assert_array_equal(x.signal_actions(strategy=strategy).cpu().numpy(),
                                  plain.signal_actions(strategy=strategy).cpu().numpy())
    # (the twin that kept its rules computed something else)
    assert y.backtest_signals(K, strategy=strategy).numpy().tobytes() != unbound.tobytes()
    for e in (x, y, plain):
        e.close()


@pytest.mark.parametrize("name", ["exit_trace", "exit_trace_multi"])
def test_backtest_with_exits_against_the_reference_fixture(name):
    """The reference driven closed-loop by tables and exit rules (tests/golden/make_exit_golden.py):
    with its draws injected, backtest_signals ends on the fixture's final rows, the exit state is the
    model's over the reference's own columns (integers by value, valuations to the 1e-12 the project
    states against the reference), and the records are the model's as in test_gpu_signals."""
    from gym_trading_env_amd.batched import BatchedTradingEnv
    g = replay.load(name)
    Kc, E = g["op"].shape
    kw = replay.config_kwargs(g)
    for k in ("n_envs", "n_static", "n_datasets"):
        kw.pop(k)
    sets = g["datasets"] if len(g["datasets"]) > 1 else g["datasets"][0]
    env = BatchedTradingEnv(sets, num_envs=E, **kw)
    env.bind_signals(xm.trace_tables(g))
    rules, rule_of_env = xm.trace_rules(g)
    env.bind_exits(_bindable(rules), rule_of_env=rule_of_env)
    q, n = replay.injection_queue(g)
    env.set_autoreset_injection(q["idx"], q["pos_index"], q["dataset"])
    env.reset(inject_idx=g["idx"][0], inject_position_index=g["pos_index"][0], inject_dataset=g["dataset"][0])
    got = env.backtest_signals(Kc - 1, strategy=g["strategy"]).numpy()
    for f, s in (("idx", "idx"), ("step", "step"), ("pos_index", "position_index"), ("dataset", "dataset_index")):
        np.testing.assert_array_equal(env.state(s), g[f][Kc - 1], err_msg=f)
    np.testing.assert_allclose(env.state("portfolio_valuation"), g["portfolio_valuation"][Kc - 1], rtol=1e-12, atol=0)
    actions, margin, counts, model = xm.trace_actions(g)
    state = env.exit_state().numpy()
    for f in state.dtype.names:
        if state[f].dtype.kind == "f":
            np.testing.assert_allclose(state[f], model.state[f], rtol=1e-12, atol=0, err_msg=f)
        else:
            np.testing.assert_array_equal(state[f], model.state[f], err_msg=f)
    np.testing.assert_array_equal(state["exits"].sum(axis=0), g["exit_counts"])
    B = replay.reward_ulp_bound(g)
    for e in range(E):
        rec = bm.new_record(g["portfolio_valuation"][0, e], g["position"][0, e])
        bound, largest, adds = 0.0, 0.0, 0
        for st in bm.trace_steps(g, e):
            eps = rec["episodes"]
            bm.run(rec, [st])
            if st["stepped"]:
                bound += B * np.spacing(abs(np.float64(st["r"])))
                adds += 1 + (rec["episodes"] - eps)
                largest = max(largest, abs(rec["reward_sum"]), abs(rec["cur_return"]), abs(rec["ep_return_sum"]))
        bound += adds * np.spacing(np.float64(largest))
        for f in bm.INT_FIELDS:
            assert got[f][e] == rec[f], (name, e, f, got[f][e], rec[f])
        for f in ("peak", "valuation_last"):
            np.testing.assert_allclose(got[f][e], rec[f], rtol=1e-12, atol=0, err_msg=f"{name} env {e} {f}")
        # d = 1 - v / peak with v and peak each within 1e-12 (relative) of the reference's: |error| < 4e-12
        assert abs(got["max_drawdown"][e] - rec["max_drawdown"]) <= 4e-12, (name, e, got["max_drawdown"][e], rec["max_drawdown"])
        assert got["prev_position"][e] == rec["prev_position"]
        for f in ("reward_sum", "cur_return", "ep_return_sum"):
            d = abs(got[f][e] - rec[f])
            print(f"{name} env {e} {f}: |difference| {d:.3e}, bound {bound:.3e}")
            assert d <= bound, (name, e, f, got[f][e], rec[f], bound)
    assert got["episodes"].sum() >= 3 * E
    env.close()


def test_refusals_and_their_messages():
    import torch
    from gym_trading_env_amd.batched import BatchedTradingEnv
    data = _data(60)
    env = tb._env(data, 64, "next_step", **dict(BASE, windows=4))
    env.bind_signals(_table(70))
    env.reset()
    lib, h = env._lib, env._h
    err = lambda: lib.gte_last_error().decode()
    ptr = C.c_void_p()
    host = np.empty(64, np.dtype(_abi.EXIT_STATE_DTYPE))
    with pytest.raises(ValueError, match="before bind_exits"):
        env.exit_state()
    assert lib.gte_read_exit_state(h, 0, 64, host.ctypes.data) == _abi.GTE_ERR_STATE and "before gte_bind_exit_rules" in err()
    rules = sig.exit_rules(stop_loss=[0.01, 0.02], exit_position=1)
    with pytest.raises(IndexError, match="exit_position outside"):
        env.bind_exits(sig.exit_rules(stop_loss=0.01, exit_position=3))
    with pytest.raises(IndexError, match=r"rule_of_env outside \[0, 2\)"):
        env.bind_exits(rules, rule_of_env=np.full(64, 2))
    with pytest.raises(ValueError, match="rule_of_env of shape"):
        env.bind_exits(rules, rule_of_env=np.zeros(63, np.int32))
    with pytest.raises(TypeError, match="EXIT_DTYPE"):
        env.bind_exits(np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="rule_of_env without rules"):
        env.bind_exits(None, rule_of_env=np.zeros(64, np.int32))
    assert env.num_exit_rules == 0
    dev = torch.zeros((3, 33), dtype=torch.uint8, device="cuda")
    raw = lambda p, n, m=None: lib.gte_bind_exit_rules(h, C.c_void_p(p), n, C.c_void_p(m) if m else None, C.byref(ptr))
    assert raw(dev.data_ptr() + 1, 2) == _abi.GTE_ERR_INVALID and "exit rules must be 4-byte aligned" in err()
    assert raw(dev.data_ptr(), 0) == _abi.GTE_ERR_INVALID and "n_rules must be >= 1" in err()
    assert raw(dev.data_ptr(), 2, dev.data_ptr() + 2) == _abi.GTE_ERR_INVALID and "rule_of_env must be 4-byte aligned" in err()
    assert lib.gte_bind_exit_rules(None, None, 0, None, None) == _abi.GTE_ERR_INVALID and "env is NULL" in err()
    # nothing of that bound anything
    twin = tb._env(data, 64, "next_step", **dict(BASE, windows=4))
    twin.bind_signals(_table(70))
    twin.reset()
    tb._assert_same_records(env.backtest_signals(5).numpy(), twin.backtest_signals(5).numpy(), "after the refusals")
    # a bind works, range checks of the read, and the capture refusal
    env.bind_exits(rules)
    assert env.num_exit_rules == 2
    assert lib.gte_read_exit_state(h, 60, 5, host.ctypes.data) == _abi.GTE_ERR_INVALID and "outside [0, 64)" in err()
    assert lib.gte_read_exit_state(h, 0, 64, host.ctypes.data) == _abi.GTE_OK and (host["episode_seen"] == -1).all()
    seen = []

    d_rules = torch.from_numpy(rules.view(np.uint8).reshape(-1, 32).copy()).cuda()

    def body(i):
        try:  # (the C call: the Python method stages host arrays first, which a capture refuses on its own)
            _abi.check(lib, lib.gte_bind_exit_rules(h, C.c_void_p(d_rules.data_ptr()), 2, None, C.byref(ptr)))
        except _abi.GteError as e:
            seen.append(e)
            raise
    with pytest.raises(Exception):
        env.capture_steps(body, 2)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].status == _abi.GTE_ERR_STATE and "gte_bind_exit_rules inside a stream capture" in str(seen[0])
    env.backtest_signals(5)
    assert (env.exit_state().numpy()["episode_seen"] >= 1).all()
    env.bind_exits(rules)   # every bind starts the state afresh
    assert (env.exit_state().numpy()["episode_seen"] == -1).all() and not env.exit_state().numpy()["exits"].any()
    env.close()
    twin.close()
    numpy_env = BatchedTradingEnv(data, num_envs=4, positions=[0, 1], windows=4, output="numpy")
    with pytest.raises(ValueError, match="needs output='torch'"):
        numpy_env.bind_exits(rules)
    numpy_env.close()
