"""Period statistics on the GPU (gte_track_periods, csrc/gte_periods.hip, csrc/gte_period_strategy.hip) against
tests/period_model.py.  Needs an MI355X.

On twelve traces the reference itself generated (each env tiled x16 at 4 envs per wave) and under a period map
that changes period every five rows, leaves every third block uncounted and uses seven periods, the period
records are held to the model run over the REFERENCE's own columns — integer fields exactly, the two sums within
the bound backtest_trace.run_with_bounds derives for reward_sum / reward_sq_sum, applied per period — on every
path that maintains them: backtest(actions) resumed over the whole trace and cleared per random chunk,
backtest_signals() with and without never-firing exit rules, all of it step by step, and same-step auto-reset.
The 16 copies of an env give identical bytes, the fused records are byte for byte the step-by-step ones, and the
gte_backtest_stats records, the env state and the exit state are byte for byte those of a twin with tracking
off.  Then: one period (the identity with gte_backtest_stats), 128 periods (a change on every step), exact
arithmetic against a single-stepped twin's own rows, firing exit rules, a row map per dataset, calls of one and
two steps, a reset() between chunks, re-binding, the refusals, the fold per strategy, the scores and the ranking,
and the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import backtest_model as bm
import backtest_trace as bt
import period_model as pm
import replay
import strategy_model as sm
import test_gpu_backtest as tb
import test_gpu_backtest_reference as ref
import test_gpu_exits as tx
from gym_trading_env_amd import _abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILE = ref.TILE
NAMES = ("c1_btc_example", "drawdown_done", "limit_orders", "multidataset_k3", "no_autoreset", "numeric_03",
         "numeric_07", "numeric_09", "slide_03", "sweep_15", "sweep_17", "reward_clipped_nodyn")
B7 = 7
traces = ref.traces
_STEPS = {}


def _steps(g):
    """pm.trace_steps of every env, made once per loaded trace"""
    if id(g) not in _STEPS:
        _STEPS[id(g)] = (g, [pm.trace_steps(g, e) for e in range(g["op"].shape[1])])
    return _STEPS[id(g)][1]


def _assert_periods(got, want, tag, worst=None):
    """PERIOD_DTYPE [E, B] against the model's [(records, bound, exact)] per env: integers exactly, the two sums
    within their bound (bit for bit where the bound is zero or every reward was +-0.0; NaN and inf as such)."""
    assert got.dtype == pm.PERIOD, tag
    ref_ = pm.as_array([w[0] for w in want])
    assert got.shape == ref_.shape, (tag, got.shape, ref_.shape)
    for f in pm.INT_FIELDS:
        np.testing.assert_array_equal(got[f], ref_[f], err_msg=f"{tag}: {f}")
    for f in pm.F64_FIELDS:
        for e, (_, bound, exact) in enumerate(want):
            for b in range(got.shape[1]):
                x, w = np.float64(got[f][e, b]), ref_[f][e, b]
                what = f"{tag}: {f} of env {e}, period {b}: {x!r}, the model over the reference's columns {w!r}"
                if np.isnan(w):
                    assert np.isnan(x), what
                elif np.isinf(w):
                    assert x == w, what
                elif bound is None or exact[b] or bound[b][f] == 0:
                    assert replay.same_bits(np.array([x]), np.array([w])).all(), what + " (an exact sum)"
                else:
                    d, lim = abs(x - w), bound[b][f]
                    assert np.isfinite(lim), (what, lim)
                    if worst is not None:
                        worst[f] = max(worst.get(f, 0.0), float(d / lim))
                    assert d <= lim, f"{what}: |difference| {d:.3e} above the bound {lim:.3e}"


def _track(r, rows, B):
    r.env.track_periods(rows if len(rows) > 1 else rows[0], B)
    return r


class Trio:
    """A tracked env, its untracked twin and (stepwise=True) a tracked env on the step-by-step path, all driven
    through trace g like ref.Replayed drives one."""

    def __init__(self, g, rows, B, monkeypatch, capfd, kernel_variant=0, autoreset="trace", stepwise=False, twin=True):
        mk = lambda kv: ref.Replayed(g, monkeypatch, capfd, kv, autoreset)
        self.on = _track(mk(kernel_variant), rows, B)
        self.off = mk(kernel_variant) if twin else None
        self.slow = _track(mk(kernel_variant | _abi.KV_ROLLOUT_PER_STEP), rows, B) if stepwise else None
        self.all = [x for x in (self.on, self.off, self.slow) if x is not None]
        self.g, self.E, self.B = g, self.on.E, B

    def each(self, f):
        for x in self.all:
            f(x)

    def _records(self, run, what, n, tag):
        """run(env) -> BacktestStats on every env; -> the period records [E, B] of the tracked one"""
        stats = run(self.on.env)
        self.on._path(what, n, tag)
        periods = stats.period_stats
        host = periods.numpy()
        assert host.shape == (self.on.N, self.B) and periods.steps.shape == host.shape
        np.testing.assert_array_equal(periods.steps.cpu().numpy(), host["steps"])
        np.testing.assert_array_equal(periods.episodes.cpu().numpy(), host["episodes"])
        assert replay.same_value(periods.reward_sum.cpu().numpy(), np.ascontiguousarray(host["reward_sum"])).all()
        if self.off is not None:
            plain = run(self.off.env)
            self.off._path(what, n, tag + " untracked")
            assert plain.period_stats is None
            a, b = ref._one(stats.numpy(), tag + " records"), ref._one(plain.numpy(), tag + " untracked records")
            assert a.tobytes() == b.tobytes(), f"{tag}: tracking changed the statistics records"
        if self.slow is not None:
            other = run(self.slow.env)
            self.slow._path(what, n, tag + " step by step")
            assert other.period_stats.numpy().tobytes() == host.tobytes(), f"{tag}: fused and step-by-step records differ"
            assert other.numpy().tobytes() == stats.numpy().tobytes(), tag
        return ref._one(host, tag + " period records")

    def backtest(self, actions, resume, tag):
        import torch
        acts = torch.from_numpy(np.ascontiguousarray(np.tile(actions, (1, TILE)).astype(np.int32))).cuda()
        return self._records(lambda env: env.backtest(acts, resume=resume), "", acts.shape[0], tag)

    def backtest_signals(self, n, resume, tag):
        return self._records(lambda env: env.backtest_signals(n, resume=resume), "signals ", n, tag)

    def assert_same_env(self, tag):
        for other in self.all[1:]:
            for f in tb.STATE:
                np.testing.assert_array_equal(self.on.env.state(f), other.env.state(f), err_msg=f"{tag}: {f}")

    def close(self):
        self.each(lambda x: x.close())


def _chunk_model(g, rows, B, start, stop):
    """Per env: (period records, bound, exact) of calls [start, stop), cleared at the row of call start - 1."""
    ended = bt.ended_at(g, start - 1)
    steps = _steps(g)
    ulp = replay.reward_ulp_bound(g)
    out = []
    for e in range(g["op"].shape[1]):
        stats = bm.new_record(g["portfolio_valuation"][start - 1, e], g["position"][start - 1, e], ended=bool(ended[e]))
        recs = pm.new_records(B)
        bound, exact = pm.run_with_bounds(recs, stats, steps[e][start - 1:stop - 1], rows, ulp)
        out.append((recs, bound, exact))
    return out


def _report(name, path, worst):
    print(f"[period-reference] {name} {path}: largest distance / bound " +
          (", ".join(f"{f} {v:.4f}" for f, v in sorted(worst.items())) or "none (every compared sum exact)"))


def _run_actions(g, name, monkeypatch, capfd, rows=None, B=B7, path="actions"):
    K = g["op"].shape[0]
    rows = pm.trace_rows(g) if rows is None else rows
    x = Trio(g, rows, B, monkeypatch, capfd, stepwise=True)   # cleared per chunk; fused, untracked, step by step
    y = Trio(g, rows, B, monkeypatch, capfd, twin=False)       # one set of records continued through the same chunks
    got_y, worst = None, {}
    for start, stop in bt.chunks(g, np.random.default_rng(ref._seed(name)), bt.longest(name)):
        tag = f"{name} {path} calls [{start}, {stop})"
        x.each(lambda r: r.orders(start))
        y.each(lambda r: r.orders(start))
        _assert_periods(x.backtest(g["action"][start:stop], False, tag), _chunk_model(g, rows, B, start, stop), tag, worst)
        got_y = y.backtest(g["action"][start:stop], start > 1, tag + " resumed")
    tag = f"{name} {path} resumed over the whole trace"
    whole = _chunk_model(g, rows, B, 1, K)
    _assert_periods(got_y, whole, tag, worst)
    x.assert_same_env(tag)
    _report(name, path, worst)
    x.close()
    y.close()
    return whole


def _run_signals(g, name, monkeypatch, capfd, exits=False):
    import torch
    K, E = g["op"].shape
    P = len(g["cfg"]["positions"])
    path = "signals+exits" if exits else "signals"
    end = ref._exit_replay_end(g) if exits else K
    assert end > 1
    rows = pm.trace_rows(g)
    x = Trio(g, rows, B7, monkeypatch, capfd, stepwise=not exits)
    rng = np.random.default_rng(ref._seed(name))
    spans = bt.table_spans(g, rng, 1, end)
    if exits:
        rules = torch.from_numpy(ref._never_firing_rules(P).view(np.uint8).reshape(-1, 32).copy()).cuda()
        x.each(lambda r: r.env.bind_exits(rules))
    cuts = sorted({c for c in [s for s, _ in bt.chunks(g, rng, bt.longest(name))] + [s[1] for s in spans] if c < end})
    first_of = {s[1]: s[0] for s in spans}
    counted, worst = 0, {}
    for start, stop in zip(cuts, cuts[1:] + [end]):
        tag = f"{name} {path} calls [{start}, {stop})"
        if start in first_of:
            x.each(lambda r: r.env.bind_signals(first_of[start]))
        x.each(lambda r: r.orders(start))
        want = _chunk_model(g, rows, B7, start, stop)
        _assert_periods(x.backtest_signals(stop - start, False, tag), want, tag, worst)
        counted += sum(r["steps"] for w in want for r in w[0])
    if exits:
        a, b = x.on.env.exit_state().numpy(), x.off.env.exit_state().numpy()
        assert a.tobytes() == b.tobytes(), f"{name} {path}: tracking changed the exit state"
    x.assert_same_env(f"{name} {path}")
    assert counted > 0
    _report(name, path, worst)
    x.close()


@pytest.mark.parametrize("name", NAMES)
def test_periods_actions(name, traces, monkeypatch, capfd):
    """backtest(actions): cleared per chunk on the fused and the step-by-step path (byte for byte each other's) and
    resumed over the whole trace."""
    whole = _run_actions(traces(name), name, monkeypatch, capfd)
    per_period = np.array([[r["steps"] for r in w[0]] for w in whole]).sum(axis=0)
    assert (per_period > 0).all(), per_period


@pytest.mark.parametrize("name", NAMES)
def test_periods_signals(name, traces, monkeypatch, capfd):
    _run_signals(traces(name), name, monkeypatch, capfd)


@pytest.mark.parametrize("name", NAMES)
def test_periods_signals_with_exit_rules_that_never_fire(name, traces, monkeypatch, capfd):
    _run_signals(traces(name), name, monkeypatch, capfd, exits=True)


SAME_STEP = [n for n in NAMES if ref._same_step(n)]


@pytest.mark.parametrize("name", SAME_STEP)
def test_periods_same_step(name, traces, monkeypatch, capfd):
    """The same-step branch: the row before the step from the terminal record on the step-by-step path, the
    terminal position for `trades`, and a reset that lands in another period."""
    g = traces(name)
    steps, actions, step_call, state_call = bt.same_step_timeline(g)
    n, E = actions.shape
    for e in range(E):
        for j, s in enumerate(steps[e]):
            k = step_call[j, e]
            s["row"], s["dataset"] = int(g["idx"][k - 1, e]), int(g["dataset"][k - 1, e])
    rows = pm.trace_rows(g)
    x = Trio(g, rows, B7, monkeypatch, capfd, autoreset="same_step", stepwise=True)
    whole = Trio(g, rows, B7, monkeypatch, capfd, autoreset="same_step", twin=False)
    rng = np.random.default_rng(ref._seed(name))
    ulp = replay.reward_ulp_bound(g)

    def records(j0, j1):
        at = state_call[j0 - 1] if j0 else np.zeros(E, np.int64)
        out = []
        for e in range(E):
            stats, recs = bm.new_record(g["portfolio_valuation"][at[e], e], g["position"][at[e], e]), pm.new_records(B7)
            out.append((recs,) + pm.run_with_bounds(recs, stats, steps[e][j0:j1], rows, ulp))
        return out

    j0 = 0
    while j0 < n:
        j1 = min(n, j0 + int(rng.integers(1, bt.longest(name) + 1)))
        tag = f"{name} same-step steps [{j0}, {j1})"
        _assert_periods(x.backtest(actions[j0:j1], False, tag), records(j0, j1), tag)
        j0 = j1
    tag = f"{name} same-step, one call of {n} steps"
    want = records(0, n)
    _assert_periods(whole.backtest(actions, False, tag), want, tag)
    assert sum(r["episodes"] for w in want for r in w[0]) >= 1
    x.close()
    whole.close()


# ---- one period, 128 periods, a map per dataset --------------------------------------------------------------

@pytest.mark.parametrize("name", ["c1_btc_example", "multidataset_k3", "numeric_07"])
def test_one_period_is_the_statistics_record(name, traces, monkeypatch, capfd):
    """B = 1 and every row in period 0: steps / reward_sum / reward_sq_sum / trades / episodes are bit for bit the
    fields of the env's gte_backtest_stats — in one fused call and step by step."""
    import torch
    g = traces(name)
    rows = [np.zeros(len(ds[1]), np.int8) for ds in g["datasets"]]
    acts = torch.from_numpy(np.ascontiguousarray(np.tile(g["action"][1:], (1, TILE)).astype(np.int32))).cuda()
    for kv in (0, _abi.KV_ROLLOUT_PER_STEP):
        r = _track(ref.Replayed(g, monkeypatch, capfd, kv), rows, 1)
        stats = r.env.backtest(acts)
        host, per = stats.numpy(), stats.period_stats.numpy()
        assert per.shape == (r.N, 1) and host["steps"].sum() > 0
        for f in pm.INT_FIELDS:
            np.testing.assert_array_equal(per[f][:, 0], host[f], err_msg=f"{name} {kv}: {f}")
        for f in pm.F64_FIELDS:
            a, b = np.ascontiguousarray(per[f][:, 0]), np.ascontiguousarray(host[f])
            assert (replay.same_bits(a, b) | (np.isnan(a) & np.isnan(b))).all(), (name, kv, f)
        r.close()


def test_128_periods_and_a_change_on_every_step(traces, monkeypatch, capfd):
    """B = 128, b = row % 128: the open record is stored and another loaded on every step."""
    g = traces("c1_btc_example")
    rows = [(np.arange(len(ds[1])) % 128).astype(np.int8) for ds in g["datasets"]]
    whole = _run_actions(g, "c1_btc_example", monkeypatch, capfd, rows=rows, B=128, path="actions B=128")
    used = np.array([[r["steps"] for r in w[0]] for w in whole]).sum(axis=0)
    assert (used > 0).sum() >= 100


def test_a_row_map_per_dataset(traces, monkeypatch, capfd):
    """multidataset_k3 with maps that share nothing: dataset d uses blocks of 3 + d rows over periods d, d + 3, 6
    and leaves other rows uncounted — a dataset switch must fetch the new dataset's period bytes."""
    g = traces("multidataset_k3")
    rows = []
    for d, ds in enumerate(g["datasets"]):
        blk = np.arange(len(ds[1])) // (3 + d)
        rows.append(np.choose(blk % 4, [d % 3, d % 3 + 3, 6, -1]).astype(np.int8))
    assert len(rows) > 1 and any((a[:50] != b[:50]).any() for a, b in zip(rows, rows[1:]))
    _run_actions(g, "multidataset_k3", monkeypatch, capfd, rows=rows, B=7, path="actions, a map per dataset")


# ---- exact arithmetic against a single-stepped twin's own rows ----------------------------------------------------

class _Recording:
    """[K, N] actions that also note the row and the dataset every env stands on when step k is about to run
    (what tb._single_step_columns asks for: acts.shape[0] and acts[k])."""

    def __init__(self, env, acts, steps=None):
        self.env, self.acts, self.shape, self.rows = env, acts, (steps if acts is None or callable(acts) else acts.shape[0],), []

    def __getitem__(self, k):
        self.rows.append((self.env.state("idx"), self.env.state("dataset_index")))
        return self.acts(k) if callable(self.acts) else self.acts[k]


def _with_rows(steps, recording):
    for k, (idx, dsi) in enumerate(recording.rows):
        for e in range(len(steps)):
            steps[e][k]["row"], steps[e][k]["dataset"] = int(idx[e]), int(dsi[e])
    return steps


def _own_model(recs, steps, rows, B):
    """[(period records, None, None)] per env: the model over a twin's own columns — compared without tolerance"""
    out = []
    for r, s in zip(recs, steps):
        per = pm.new_records(B)
        pm.run(per, r, s, rows)
        out.append((per, None, None))
    return out


ROWS60 = [((np.arange(60) // 4) % 6 - 1).astype(np.int8)]   # T = 60: blocks of four rows, -1 and periods 0 .. 4


def _plain(mode, N=129, track=(1,), **over):
    """tb._twins after the same out-of-phase start; track: which of the two keep period records"""
    import torch
    kw = dict(tb.BASE, max_episode_duration=12, **over)
    data = tb._data(1, 60, 6)[:2]
    a, b = tb._twins(data, N, mode, **kw)
    tb._both(a, b, lambda e: e.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    tb._phase(a, b, N, 3, gen)
    for i in track:
        (a, b)[i].track_periods(ROWS60[0], 5)
    return a, b, gen


@pytest.mark.parametrize("mode", tb.MODES, ids=lambda m: str(m))
@pytest.mark.parametrize("K", [1, 2, 23])
def test_periods_equal_the_model_over_single_steps(K, mode):
    """The records equal BY VALUE the model fed with a single-stepped twin's own reward64 rows, flags, rows and
    datasets: no tolerance.  K = 1 has no fused step, K = 2 one."""
    import torch
    N = 129
    a, b, gen = _plain(mode, N)
    acts = torch.randint(-1, 3, (K, N), dtype=torch.int32, device="cuda", generator=gen)
    note = _Recording(a, acts)
    recs, steps = tb._single_step_columns(a, note)
    want = _own_model(recs, _with_rows(steps, note), ROWS60, 5)
    stats = b.backtest(acts)
    tag = f"single steps K={K} {mode}"
    _assert_periods(stats.period_stats.numpy(), want, tag)
    tb._assert_records(stats, recs, tag)   # (pm.run brought the twin's statistics records to their end too)
    tb._assert_same_env(a, b, tag)
    if K == 23:
        got = stats.period_stats.numpy()
        assert (got["steps"].sum(axis=0) > 0).all() and got["steps"].sum() < stats.numpy()["steps"].sum()
    a.close()
    b.close()


class _DeviceLookup:
    """The actions of the single-stepped twin: its own signal_actions() (exits decided on the device)"""

    def __init__(self, env, strategy):
        self.env, self.strategy = env, strategy

    def __call__(self, k):
        return self.env.signal_actions(strategy=self.strategy).clone()


@pytest.mark.parametrize("mode", tb.MODES, ids=lambda m: str(m))
def test_periods_with_firing_exit_rules(mode):
    """Exit rules that fire: fused == step by step bit for bit == the model over a single-stepped twin's rows;
    statistics records and exit state are those of an untracked twin."""
    import torch
    N, K, n_rules = tx.N, tx.K, 7
    data, tables = tx._data(31), tx._table(21)
    kw = dict(tx.BASE, windows=5)
    rules = tx._rules(n_rules)
    strategy, rule_of_env = tx._maps(True, n_rules)
    rows = [((np.arange(tx.T) // 7) % 5 - 1).astype(np.int8)]
    envs = dict(single=tb._env(data, N, mode, final_obs=(mode == "same_step"), **kw), fused=tb._env(data, N, mode, **kw),
                stepwise=tb._env(data, N, mode, kernel_variant=_abi.KV_ROLLOUT_PER_STEP, **kw),
                untracked=tb._env(data, N, mode, **kw))
    gen = torch.Generator(device="cuda")
    for name, e in envs.items():
        e.bind_signals(tables)
        e.reset()
        gen.manual_seed(17)
        tx._phase_one(e, gen)
        e.bind_exits(tx._bindable(rules), rule_of_env=rule_of_env)
        if name not in ("single", "untracked"):
            e.track_periods(rows[0], 4)
    note = _Recording(envs["single"], _DeviceLookup(envs["single"], strategy), K)
    recs, steps = tb._single_step_columns(envs["single"], note)
    want = _own_model(recs, _with_rows(steps, note), rows, 4)
    tag = f"firing exits {mode}"
    got = {k: envs[k].backtest_signals(K, strategy=strategy) for k in ("fused", "stepwise", "untracked")}
    fused, stepwise = got["fused"].period_stats.numpy(), got["stepwise"].period_stats.numpy()
    assert fused.tobytes() == stepwise.tobytes(), f"{tag}: fused and step-by-step period records differ"
    _assert_periods(fused, want, tag)
    assert got["fused"].numpy().tobytes() == got["untracked"].numpy().tobytes() == got["stepwise"].numpy().tobytes()
    assert envs["fused"].exit_state().numpy().tobytes() == envs["untracked"].exit_state().numpy().tobytes()
    tb._assert_same_env(envs["single"], envs["fused"], tag)
    assert envs["fused"].exit_state().numpy()["exits"].sum() > 0 and (fused["steps"].sum(axis=0) > 0).all()
    for e in envs.values():
        e.close()


# ---- resets between calls, re-binding, switching, refusals ----------------------------------------------------

@pytest.mark.parametrize("mode", tb.MODES, ids=lambda m: str(m))
def test_reset_between_resumed_chunks_and_a_rebind(mode):
    import torch
    N, K = 129, 4
    a, b, gen = _plain(mode, N)
    acts = torch.randint(-1, 3, (3, K, N), dtype=torch.int32, device="cuda", generator=gen)
    note = _Recording(a, acts[0])
    recs, steps = tb._single_step_columns(a, note)
    _with_rows(steps, note)
    b.backtest(acts[0])
    mask = (np.arange(N) % 2 == 0).astype(np.uint8)
    tb._both(a, b, lambda e: e.reset(mask=mask))
    positions = np.asarray(a.positions, np.float64)
    for e in np.flatnonzero(mask):   # a reset row changes no period record; the statistics record starts its peak anew
        steps[e].append(dict(stepped=False, reset=True, v0=a.state("portfolio_valuation")[e],
                             p0=positions[a.state("position_index")[e]], row=0, dataset=0))
    note = _Recording(a, acts[1])
    _, more = tb._single_step_columns(a, note)
    _with_rows(more, note)
    want = _own_model(recs, [s + m for s, m in zip(steps, more)], ROWS60, 5)
    stats = b.backtest(acts[1], resume=True)
    tag = f"reset between chunks {mode}"
    _assert_periods(stats.period_stats.numpy(), want, tag)
    tb._assert_same_env(a, b, tag)
    # a re-bind (another map, the same B) clears, whatever resume says
    other = [np.roll(ROWS60[0], 7)]
    b.track_periods(other[0], 5)
    note = _Recording(a, acts[2])
    recs, last = tb._single_step_columns(a, note)
    want = _own_model(recs, _with_rows(last, note), other, 5)
    stats = b.backtest(acts[2], resume=True)
    _assert_periods(stats.period_stats.numpy(), want, tag + ", after a re-bind")
    tb._assert_records(stats, recs, tag + ", after a re-bind")
    a.close()
    b.close()


def test_switching_tracking_clears_both_records():
    import torch
    N, K = 129, 5
    a, b, gen = _plain("next_step", N, track=())
    acts = torch.randint(-1, 3, (3, K, N), dtype=torch.int32, device="cuda", generator=gen)
    assert a.backtest(acts[0]).period_stats is None and b.backtest(acts[0]).period_stats is None
    tb._both(a, b, lambda e: e.track_periods(ROWS60[0]))      # n_periods defaults to max + 1 = 5
    on_a, on_b = a.backtest(acts[1], resume=True), b.backtest(acts[1], resume=False)   # the switch clears either way
    assert on_a.period_stats.num_periods == 5
    assert on_a.numpy().tobytes() == on_b.numpy().tobytes()
    assert on_a.period_stats.numpy().tobytes() == on_b.period_stats.numpy().tobytes()
    assert (on_a.steps <= K).all() and int(on_a.period_stats.steps.sum()) > 0
    before = on_a.period_stats.steps.clone()
    more, same = a.backtest(acts[2], resume=True), b.backtest(acts[2], resume=True)     # no switch: the records go on
    assert (more.period_stats.steps >= before).all() and (more.period_stats.steps > before).any()
    assert more.period_stats.numpy().tobytes() == same.period_stats.numpy().tobytes()
    a.track_periods(ROWS60[0], 9)                             # another B: new records, cleared
    wide = a.backtest(acts[2], resume=True)
    b.backtest(acts[2], resume=True)                          # (the twin takes the same steps)
    assert wide.period_stats.numpy().shape == (N, 9) and (wide.steps <= K).all()
    assert not wide.period_stats.numpy()["steps"][:, 5:].any()
    a.track_periods(None)
    off, cleared = a.backtest(acts[2], resume=True), b.backtest(acts[2], resume=False)  # switched off: cleared again
    assert off.period_stats is None and off.numpy().tobytes() == cleared.numpy().tobytes()
    a.close()
    b.close()


def test_an_older_result_refuses_after_another_period_count():
    """track_periods() with another n_periods frees the records: a PeriodStats (and the BacktestStats it hangs on)
    from before must raise on every use — fields, numpy(), by_strategy(), and the lazily made .period_stats —
    and neither read freed device memory nor let gte_read_period_stats copy N * 9 records into an N * 5 array.
    What was taken out before the change stays good; the same B again does not revive a stale object."""
    import torch
    N, K = 129, 5
    a, b, gen = _plain("next_step", N, track=(0,))            # a tracks five periods
    acts = torch.randint(-1, 3, (2, K, N), dtype=torch.int32, device="cuda", generator=gen)
    month, unopened = a.backtest(acts[0]), a.backtest(acts[0], resume=True)   # (unopened: .period_stats never read)
    old = month.period_stats
    kept, steps5 = old.numpy(), old.steps.clone()
    folded = old.by_strategy(n_strategies=3)                  # owns its records: outlives the change
    folded_bytes = folded.numpy().tobytes()
    a.track_periods(None)                                     # off and on with the same B: the same records
    a.track_periods(ROWS60[0], 5)
    assert old.numpy().shape == (N, 5) and old.steps.shape == (N, 5)
    a.track_periods(ROWS60[0], 9)                             # another B: the library frees the five-period records
    wide = a.backtest(acts[1]).period_stats
    for use in (lambda: old.steps, lambda: old.reward_sum, old.numpy, lambda: old.by_strategy(n_strategies=3),
                lambda: month.period_stats.numpy(), lambda: unopened.period_stats):
        with pytest.raises(RuntimeError, match="stale"):
            use()
    assert wide.numpy().shape == (N, 9) and wide.steps.shape == (N, 9)
    np.testing.assert_array_equal(steps5.cpu().numpy(), kept["steps"])
    assert folded.numpy().tobytes() == folded_bytes and folded.top(2, "reward_sum")[0].numel() <= 2
    a.track_periods(ROWS60[0], 5)                             # five again: new records, not the old ones
    with pytest.raises(RuntimeError, match="stale"):
        old.numpy()
    with pytest.raises(RuntimeError, match="stale"):
        wide.steps
    assert a.backtest(acts[1]).period_stats.numpy().shape == (N, 5)
    a.close()
    b.close()


def test_a_failed_bind_leaves_tracking_off_and_an_untracked_env_keeps_its_clear():
    """track_periods() switches tracking on and then binds the rows: if a bind fails, tracking is off again, not on
    with a dataset unbound.  And with tracking off, a row published by gte_upload_dataset / gte_bind_periods does
    not make the next backtest clear the statistics records against its resume=True."""
    import torch
    N, K = 129, 4
    a, b, gen = _plain("next_step", N, track=())
    acts = torch.randint(-1, 3, (3, K, N), dtype=torch.int32, device="cuda", generator=gen)

    class FailingBind:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            return getattr(self._lib, name)

        def gte_bind_periods(self, h, d, row):                # the library's own refusal: no such dataset
            return self._lib.gte_bind_periods(h, 99, row)
    lib = a._lib
    a._lib = FailingBind(lib)
    with pytest.raises(_abi.GteError, match="out of range"):
        a.track_periods(ROWS60[0], 5)
    a._lib = lib
    tb._both(a, b, lambda e: e.backtest(acts[0]))
    first = a.backtest(acts[1], resume=True)                  # tracking is off: no "no period row" refusal
    assert first.period_stats is None
    b.backtest(acts[1], resume=True)
    # a row bound, tracking switched off again, the dataset uploaded anew: the untracked resume goes on
    a.track_periods(ROWS60[0], 5)
    a.track_periods(None)
    tb._both(a, b, lambda e: e.backtest(acts[0]))             # (a clears for the switch, b because it is told to)
    a.upload_dataset(0, a.datasets[0])                        # unbinds the row while tracking is off
    assert lib.gte_bind_periods(a._h, 0, ROWS60[0].ctypes.data) == _abi.GTE_OK   # and a bind while it is off
    on, plain = a.backtest(acts[2], resume=True), b.backtest(acts[2], resume=True)
    assert on.numpy().tobytes() == plain.numpy().tobytes() and int(on.steps.max()) > K
    a.close()
    b.close()


def test_refusals():
    import torch
    from gym_trading_env_amd.batched import BatchedTradingEnv
    feat, close = tb._data(1, 60, 6)[:2]
    env = BatchedTradingEnv((feat, close), num_envs=64, positions=[-1, 0, 1], windows=3, initial_position=0)
    lib, h = env._lib, env._h
    err = lambda: lib.gte_last_error().decode()
    ptr = C.c_void_p()
    row = np.zeros(60, np.int8)
    with pytest.raises(_abi.GteError, match="before gte_reset"):
        env.track_periods(row)
    env.reset()
    rec = np.empty((64, 2), dtype=pm.PERIOD)
    assert lib.gte_read_period_stats(h, 0, 64, rec.ctypes.data) == _abi.GTE_ERR_STATE
    assert "before gte_track_periods" in err()
    out = torch.empty((3 * 2, 48), dtype=torch.uint8, device="cuda")
    assert lib.gte_reduce_period_stats(h, None, 2, 3, None, None, C.c_void_p(out.data_ptr())) == _abi.GTE_ERR_STATE
    assert "before gte_track_periods" in err()
    assert lib.gte_track_periods(None, 1, C.byref(ptr)) == _abi.GTE_ERR_INVALID and "env is NULL" in err()
    for B in (-1, 129):
        assert lib.gte_track_periods(h, B, C.byref(ptr)) == _abi.GTE_ERR_INVALID
        assert f"n_periods {B} outside [0, 128]" in err()
    # (state before range, NULL before state)
    assert lib.gte_read_period_stats(h, 60, 5, rec.ctypes.data) == _abi.GTE_ERR_STATE and "before gte_track_periods" in err()
    assert lib.gte_read_period_stats(h, 60, 5, None) == _abi.GTE_ERR_INVALID and "NULL argument" in err()
    for B in (0, 129):
        with pytest.raises(ValueError, match="n_periods"):
            env.track_periods(row, B)
    with pytest.raises(ValueError, match="60 rows"):
        env.track_periods(np.zeros(59, np.int8))
    assert lib.gte_bind_periods(h, 1, row.ctypes.data) == _abi.GTE_ERR_INVALID and "out of range" in err()
    seen = []

    def body(i):
        try:
            env.track_periods(row)
        except _abi.GteError as e:
            seen.append(e)
            raise
    with pytest.raises(Exception):
        env.capture_steps(body, 2)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].status == _abi.GTE_ERR_STATE and "stream capture" in str(seen[0])
    # tracking on, no row bound: a backtest is refused, and launches nothing
    assert lib.gte_track_periods(h, 2, C.byref(ptr)) == _abi.GTE_OK and ptr.value
    with pytest.raises(_abi.GteError, match="no period row") as e:
        env.backtest([[2] * 64])
    assert e.value.status == _abi.GTE_ERR_STATE
    # trades + periods: whichever would turn the second on is refused
    with pytest.raises(_abi.GteError, match="together") as e:
        env.track_trades()
    assert e.value.status == _abi.GTE_ERR_STATE
    env.track_periods(None)
    env.track_trades()
    with pytest.raises(_abi.GteError, match="together") as e:
        env.track_periods(row, 2)
    assert e.value.status == _abi.GTE_ERR_STATE
    env.track_trades(False)
    env.track_periods(np.arange(60) % 2, 2)
    stats = env.backtest([[2] * 64, [None] * 64, [1] * 64])   # flat -> long, hold, -> flat
    p = stats.period_stats
    assert (p.steps.sum(dim=1) == 3).all() and (p.trades.sum(dim=1) == 2).all() and (p.steps > 0).all()
    assert lib.gte_read_period_stats(h, 60, 5, rec.ctypes.data) == _abi.GTE_ERR_INVALID and "outside" in err()
    assert lib.gte_reduce_period_stats(h, None, 3, 3, None, None, C.c_void_p(out.data_ptr())) == _abi.GTE_ERR_INVALID
    assert "the env's records have 2" in err()
    idx = torch.empty(4, dtype=torch.int32, device="cuda")
    top = torch.empty(4, dtype=torch.float64, device="cuda")
    mask = (C.c_uint64 * 2)(3, 0)
    args = (C.c_void_p(idx.data_ptr()), C.c_void_p(top.data_ptr()), None)
    o = C.c_void_p(out.data_ptr())
    assert lib.gte_rank_period_stats(h, o, 3, 2, mask, 6, 1, 4, *args) == _abi.GTE_ERR_INVALID and "metric 6 unknown" in err()
    assert lib.gte_rank_period_stats(h, o, 3, 2, mask, 0, 1, 0, *args) == _abi.GTE_ERR_INVALID
    assert "k must lie in [1, 256]" in err()
    assert lib.gte_rank_period_stats(h, o, 3, 129, mask, 0, 1, 4, *args) == _abi.GTE_ERR_INVALID
    assert "n_periods 129 outside [1, 128]" in err()
    assert lib.gte_rank_period_stats(h, o, 3, 2, None, 0, 1, 4, *args) == _abi.GTE_ERR_INVALID and "period_mask is NULL" in err()
    assert lib.gte_reduce_period_stats(h, None, 2, 0, None, None, o) == _abi.GTE_ERR_INVALID
    assert "n_strategies must be >= 1" in err()
    assert lib.gte_reduce_period_stats(h, None, 2, 3, C.c_void_p(idx.data_ptr()), None, o) == _abi.GTE_ERR_INVALID
    assert "both or neither" in err()
    # every refusal gte_reduce_backtest_stats / gte_rank_strategies make (test_gpu_strategy_stats.py), for ITS reason:
    # 64 envs, 8 strategies, 3 periods; nothing below launches
    INVALID = _abi.GTE_ERR_INVALID
    out8 = torch.zeros((8 * 3 + 1, 48), dtype=torch.uint8, device="cuda")
    rec8 = torch.zeros((64 * 3 + 1, 32), dtype=torch.uint8, device="cuda")
    lists = torch.zeros((80,), dtype=torch.int32, device="cuda")
    idx8 = torch.zeros((256 + 1,), dtype=torch.int32, device="cuda")
    top8 = torch.zeros((256 + 1,), dtype=torch.float64, device="cuda")
    q = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    reduce = lambda *a: lib.gte_reduce_period_stats(h, *a)
    rank = lambda *a: lib.gte_rank_period_stats(h, *a)
    for B in (0, 129):
        assert reduce(q(rec8), B, 8, None, None, q(out8)) == INVALID and f"n_periods {B} outside [1, 128]" in err()
    assert reduce(q(rec8), 3, 8, None, None, None) == INVALID and "out_device must be a 16-byte aligned" in err()
    assert reduce(q(rec8), 3, 8, None, None, q(out8, 8)) == INVALID and "out_device must be a 16-byte aligned" in err()
    assert reduce(q(rec8, 8), 3, 8, None, None, q(out8)) == INVALID and "records must be 16-byte aligned" in err()
    assert reduce(q(rec8), 3, 8, None, q(lists), q(out8)) == INVALID and "both or neither" in err()
    assert reduce(q(rec8), 3, 8, q(lists, 2), q(lists), q(out8)) == INVALID and "group lists must be 4-byte aligned" in err()
    assert reduce(q(rec8), 3, 8, q(lists), q(lists, 2), q(out8)) == INVALID and "group lists must be 4-byte aligned" in err()
    assert reduce(q(rec8, 8), 0, 0, q(lists), None, None) == INVALID and "n_strategies must be >= 1" in err()  # the order
    assert reduce(q(rec8, 8), 0, 8, q(lists), None, None) == INVALID and "n_periods 0 outside" in err()
    assert reduce(q(rec8, 8), 3, 8, q(lists), None, None) == INVALID and "out_device" in err()
    assert reduce(q(rec8, 8), 3, 8, q(lists), None, q(out8)) == INVALID and "records must be" in err()
    assert reduce(None, 3, 8, q(lists), None, q(out8)) == INVALID and "both or neither" in err()  # (before the env's B)
    assert lib.gte_reduce_period_stats(None, None, 0, 0, None, None, None) == INVALID and "env is NULL" in err()
    stats_text, top_text = "stats_device must be a 16-byte aligned", "top_index_device (int32 [k]) and top_score_device"
    m3 = (C.c_uint64 * 2)(7, 0)
    ok = (q(idx8), q(top8), None)
    assert rank(q(out8), 0, 3, m3, 0, 1, 8, *ok) == INVALID and "n_strategies must be >= 1" in err()
    assert rank(q(out8), 8, 0, m3, 0, 1, 8, *ok) == INVALID and "n_periods 0 outside [1, 128]" in err()
    for k in (0, -1, 257):
        assert rank(q(out8), 8, 3, m3, 0, 1, k, *ok) == INVALID and "k must lie in [1, 256]" in err()
    assert rank(q(out8), 8, 3, m3, -1, 1, 8, *ok) == INVALID and "metric -1 unknown" in err()
    assert rank(None, 8, 3, m3, 0, 1, 8, *ok) == INVALID and stats_text in err()
    assert rank(q(out8, 8), 8, 3, m3, 0, 1, 8, *ok) == INVALID and stats_text in err()
    assert rank(q(out8), 8, 3, m3, 0, 1, 8, None, q(top8), None) == INVALID and top_text in err()
    assert rank(q(out8), 8, 3, m3, 0, 1, 8, q(idx8), None, None) == INVALID and top_text in err()
    assert rank(q(out8), 8, 3, m3, 0, 1, 8, q(idx8, 2), q(top8), None) == INVALID and top_text in err()
    assert rank(q(out8), 8, 3, m3, 0, 1, 8, q(idx8), q(top8, 4), None) == INVALID and top_text in err()
    assert rank(q(out8), 8, 3, m3, 0, 1, 8, q(idx8), q(top8), q(top8, 4)) == INVALID and "scores_device must be 8-byte" in err()
    assert rank(None, 0, 0, None, -1, 1, 0, None, None, q(top8, 4)) == INVALID and "n_strategies must be" in err()  # the order
    assert rank(None, 8, 0, None, -1, 1, 0, None, None, q(top8, 4)) == INVALID and "n_periods 0 outside" in err()
    assert rank(None, 8, 3, None, -1, 1, 0, None, None, q(top8, 4)) == INVALID and "period_mask is NULL" in err()
    assert rank(None, 8, 3, m3, -1, 1, 0, None, None, q(top8, 4)) == INVALID and "k must lie" in err()
    assert rank(None, 8, 3, m3, -1, 1, 8, None, None, q(top8, 4)) == INVALID and "metric -1 unknown" in err()
    assert rank(None, 8, 3, m3, 0, 1, 8, None, None, q(top8, 4)) == INVALID and stats_text in err()
    assert rank(q(out8), 8, 3, m3, 0, 1, 8, None, None, q(top8, 4)) == INVALID and top_text in err()
    assert lib.gte_read_period_stats(h, -1, 5, rec.ctypes.data) == INVALID and "env range [-1, 4) outside [0, 64)" in err()
    assert lib.gte_read_period_stats(h, 0, -1, rec.ctypes.data) == INVALID and "outside [0, 64)" in err()
    assert lib.gte_read_period_stats(None, 60, 5, rec.ctypes.data) == INVALID and "NULL argument" in err()
    with pytest.raises(ValueError, match="n_strategies"):
        p.by_strategy()
    with pytest.raises(ValueError, match="unknown metric"):
        p.by_strategy(n_strategies=3).top(2, metric="profit_factor")
    with pytest.raises(IndexError):
        p.by_strategy(n_strategies=3).top(2, periods=[2])
    # uploading the dataset again unbinds its period row (T may have changed), and a new bind clears
    env.upload_dataset(0, env.datasets[0])
    with pytest.raises(_abi.GteError, match="no period row"):
        env.backtest([[2] * 64], resume=True)
    env.track_periods(np.arange(60) % 2, 2)
    again = env.backtest([[2] * 64], resume=True).period_stats
    assert (again.steps.sum(dim=1) == 1).all()
    env.close()


# ---- per strategy, and the ranking ------------------------------------------------------------------------------

N_FOLD = 1000


@pytest.fixture(scope="module")
def fold_env():
    from gym_trading_env_amd.batched import BatchedTradingEnv
    feat, close = tb._data(1, 60, 6)[:2]
    env = BatchedTradingEnv((feat, close), num_envs=N_FOLD, positions=[-1, 0, 1], windows=None)
    yield env
    env.close()


def _reduce(env, rec, S, groups=None):
    """gte_reduce_period_stats over caller-held records [N, B]: the default map, or the CSR lists of `groups`"""
    import torch
    dev = env._t["obs"].device
    N, B = rec.shape
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(N * B, 32).copy()).to(dev)
    out = torch.full((S * B, 48), 0xAB, dtype=torch.uint8, device=dev)
    lists = (None, None)
    if groups is not None:
        offsets, members = sm.csr(groups)
        keep = torch.from_numpy(offsets).to(dev), torch.from_numpy(np.append(members, 0).astype(np.int32)).to(dev)
        lists = tuple(C.c_void_p(t.data_ptr()) for t in keep)
    torch.cuda.synchronize()
    _abi.check(env._lib, env._lib.gte_reduce_period_stats(env._h, C.c_void_p(d_rec.data_ptr()), B, S, *lists,
                                                          C.c_void_p(out.data_ptr())))
    env.synchronize()
    return out.cpu().numpy().view(pm.STRATEGY_PERIOD).reshape(S, B).copy()


def _check_fold(got, want, what):
    if not pm.same_bytes(got, want):
        bad = [(s, b, n) for s in range(want.shape[0]) for b in range(want.shape[1]) for n in want.dtype.names
               if pm.canonical(got[s:s + 1, b:b + 1])[n].tobytes() != pm.canonical(want[s:s + 1, b:b + 1])[n].tobytes()]
        pytest.fail(f"{what}: {len(bad)} fields differ, first {bad[:5]}: {[(got[n][s, b], want[n][s, b]) for s, b, n in bad[:5]]}")


@pytest.mark.parametrize("B", [1, 7, 64, 128])
@pytest.mark.parametrize("S", [7, 40])
def test_fold_equals_the_model(fold_env, S, B):
    """N = 1 000 envs into S strategies x B periods: 256 / B strategies per workgroup (256, 36, 4, 2 — S is a
    multiple of none but 1), the threads of a strategy across its periods.  The default map, then an explicit one
    with an empty strategy, lists of 0 .. 300 members around the eight accumulators, and ids outside [0, N) that
    keep their place."""
    rec = pm.craft_records(N_FOLD, B, seed=S + B)
    got = _reduce(fold_env, rec, S)
    _check_fold(got, pm.reduce_loop(rec, sm.default_groups(N_FOLD, S)), f"default map S={S} B={B}")
    assert not got["reserved"].any()
    np.testing.assert_array_equal(got["steps"].sum(axis=0), rec["steps"].sum(axis=0))
    rng = np.random.default_rng(S)
    sizes = ([0, 1, 7, 8, 9, 63, 300] if S == 7 else [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65] + [12] * 29)
    assert len(sizes) == S
    groups = [rng.choice(N_FOLD, n, replace=False).tolist() for n in sizes]
    groups[-1][3], groups[-1][9], groups[-2][0] = -1, N_FOLD, 2 ** 31 - 1
    got = _reduce(fold_env, rec, S, groups)
    _check_fold(got, pm.reduce_loop(rec, groups), f"explicit lists S={S} B={B}")
    assert not got[0]["steps"].any() and not got[0]["envs_stepped"].any()
    assert (got["envs_stepped"][-1] <= sizes[-1] - 2).all()


def _words(mask):
    w = (C.c_uint64 * 2)(0, 0)
    for b in np.flatnonzero(mask):
        w[int(b) >> 6] |= 1 << (int(b) & 63)
    return w


@pytest.mark.parametrize("S,B,k,min_steps", [(1, 1, 1, 0), (16, 7, 5, 1), (300, 7, 256, 0), (300, 128, 7, 400),
                                             (3000, 3, 256, 2), (3, 70, 9, 1)])
def test_scores_and_ranking_equal_the_model(fold_env, S, B, k, min_steps):
    """Crafted strategy records (duplicates, +-0.0, +-inf, NaN, periods and strategies without a step, zero
    variance) under all six metrics and three masks — all periods, the first half, the last period alone (past bit
    63 for B > 64; set bits >= B are ignored): every score bit for bit, and the k best given those scores, ties by
    index; k > S pads with -1 / NaN."""
    import torch
    t = pm.craft_stats(S, B, seed=S)
    dev = fold_env._t["obs"].device
    d = torch.from_numpy(t.view(np.uint8).reshape(S * B, 48).copy()).to(dev)
    masks = [np.ones(B, bool), np.arange(B) < max(1, B // 2), np.arange(B) == B - 1]
    for which, mask in enumerate(masks):
        words = _words(mask)
        if which == 0:
            words[0], words[1] = 2 ** 64 - 1, 2 ** 64 - 1    # bits at and past B select nothing
        for code, metric in enumerate(pm.METRICS):
            scores = torch.empty(S, dtype=torch.float64, device=dev)
            index = torch.empty(k, dtype=torch.int32, device=dev)
            top = torch.empty(k, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            _abi.check(fold_env._lib, fold_env._lib.gte_rank_period_stats(
                fold_env._h, C.c_void_p(d.data_ptr()), S, B, words, code, min_steps, k, C.c_void_p(index.data_ptr()),
                C.c_void_p(top.data_ptr()), C.c_void_p(scores.data_ptr())))
            fold_env.synchronize()
            want = pm.scores_loop(t, metric, mask)
            got = scores.cpu().numpy()
            assert sm.same_f64(got, want), (metric, which, [(s, got[s], want[s]) for s in range(S)
                                                            if not sm.same_f64(got[s:s + 1], want[s:s + 1])][:5])
            w_index, w_top = pm.rank_loop(t, want, mask, min_steps, k)
            np.testing.assert_array_equal(index.cpu().numpy(), w_index, err_msg=f"{metric} mask {which}")
            assert sm.same_f64(top.cpu().numpy(), w_top), (metric, which)


def test_pipeline_by_strategy_select_and_top():
    """backtest_signals() with tracking on -> period_stats.by_strategy() -> select() / score() / top(): the fold
    of the env's own records under the default and an explicit map, and the leaders over train and test periods."""
    import gym_trading_env_amd as gte
    import torch
    from gym_trading_env_amd import periods
    N, S, T = 100, 12, 300
    rng = np.random.default_rng(11)
    close = 100.0 * np.exp(np.cumsum(rng.normal(0, 1e-2, T)))
    feat = rng.normal(0, 1, (T, 3)).astype(np.float32)
    env = gte.BatchedTradingEnv((feat, close), num_envs=N, positions=[-1, 0, 1], windows=None, trading_fees=1e-4,
                                max_episode_duration=40, autoreset="next_step", seed=4)
    env.bind_signals(np.repeat(rng.integers(0, 3, (S, T // 4)), 4, axis=1).astype(np.int8))
    env.reset()
    row = periods.blocks(T, 6)
    row[100:110] = -1
    env.track_periods(row)
    stats = env.backtest_signals(120)
    per = stats.period_stats
    rec = per.numpy()
    assert rec.shape == (N, 6) and (rec["steps"].sum(axis=0) > 0).all() and rec["steps"].sum() < stats.numpy()["steps"].sum()
    by = per.by_strategy()
    assert isinstance(by, gte.StrategyPeriodStats) and (by.num_strategies, by.num_periods) == (S, 6)
    _check_fold(by.numpy(), pm.reduce_loop(rec, sm.default_groups(N, S)), "by_strategy()")
    assert by.reward_sum.shape == (S, 6)
    assert replay.same_value(by.reward_sum.cpu().numpy(), np.ascontiguousarray(by.numpy()["reward_sum"])).all()
    m = rng.integers(-1, 6, N).astype(np.int32)   # strategies -1 .. 5 with S = 5: -1 and 5 belong to nobody
    with pytest.raises(IndexError):
        per.by_strategy(strategy=m, n_strategies=5)
    explicit = per.by_strategy(strategy=torch.from_numpy(m).cuda(), n_strategies=5)
    _check_fold(explicit.numpy(), pm.reduce_loop(rec, sm.map_groups(m, 5)), "by_strategy(map)")
    host = by.numpy()
    train, test = [0, 1, 2, 3], np.arange(6) >= 4
    for periods_, mask in ((train, np.arange(6) < 4), (test, test), (None, np.ones(6, bool))):
        for metric in pm.METRICS:
            want = pm.scores_loop(host, metric, mask)
            assert sm.same_f64(by.score(metric, periods_).cpu().numpy(), want), metric
            index, top = by.top(5, metric=metric, periods=periods_, min_steps=30)
            w_index, w_top = pm.rank_loop(host, want, mask, 30, 5)
            r = int((w_index >= 0).sum())
            np.testing.assert_array_equal(index.cpu().numpy(), w_index[:r])
            assert sm.same_f64(top.cpu().numpy(), w_top[:r])
        sel = by.select(periods_)
        np.testing.assert_array_equal(sel.steps.cpu().numpy(), pm.selected_steps(host, mask))
        assert sm.same_f64(sel.sharpe().cpu().numpy(), pm.scores_loop(host, "sharpe", mask))
        assert sm.same_f64(sel.mean_reward.cpu().numpy(), pm.scores_loop(host, "mean_reward", mask))
        assert sm.same_f64(sel.reward_sum.cpu().numpy(), pm.scores_loop(host, "reward_sum", mask))
    index, top = by.top(3)
    assert sm.same_f64(top.cpu().numpy(), pm.rank_loop(host, pm.scores_loop(host, "sharpe", np.ones(6, bool)),
                                                       np.ones(6, bool), 1, 3)[1][:len(top)])
    assert rec.tobytes() == per.numpy().tobytes()   # folding and ranking change no record
    env.close()


def test_walk_forward_example(capsys):
    """examples/backtest_walk_forward.py runs at a small size, and the table it prints is the records'."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import backtest_walk_forward as ex
    finally:
        sys.path.pop(0)
    out = ex.main(n_fast=3, n_slow=3, replicas=4, K=700, T=1500, top=5, min_steps=50)
    text = capsys.readouterr().out
    rows = [l.split() for l in text.splitlines() if len(l.split()) == 7 and l.split()[0].isdigit()]
    host = out["by_strategy"].numpy()
    lead = out["index"].cpu().numpy().tolist()
    assert 1 <= len(rows) <= 5 and len(rows) == len(lead)
    train, test = np.array([True, False]), np.array([False, True])
    want = pm.rank_loop(host, pm.scores_loop(host, "sharpe", train), train, out["min_steps"], 5)[0]
    np.testing.assert_array_equal(lead, want[:len(lead)])
    test_sharpe = pm.scores_loop(host, "sharpe", test)
    for row, s in zip(rows, lead):
        assert int(row[1]) == s and int(row[-1]) == int(host["steps"][s, 1])
        assert np.isnan(test_sharpe[s]) or abs(float(row[-2]) - test_sharpe[s]) < 5.1e-5
    assert (out["period_of_row"] == -1).sum() > 0 and host["steps"][:, 0].sum() > 0 and host["steps"][:, 1].sum() > 0
    assert "keep the sign" in text
