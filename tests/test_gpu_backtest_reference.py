"""The backtest kernels (gte_backtest_kernel, gte_backtest_signal_kernel, gte_backtest_fold_kernel of
csrc/gte_backtest.hip, gte_backtest_exit_kernel of csrc/gte_exits.hip) replaying every trace the reference
itself generated (tests/backtest_trace.names(): the originals, the configuration sweep, the numeric and the
slide family), in chunks of random length, each env tiled x16 at 4 envs per wave.  Needs an MI355X.

After every chunk the env is held to the trace as the step and rollout replays hold it — indices and flags
exact, the fp64 state by value, reward64 within replay.reward_ulp_bound ulp, the observation — and the
statistics record to tests/backtest_model.py run over the REFERENCE's own columns: the counters exact; peak,
max_drawdown, valuation_last and prev_position by value; the five sums NaN where the model's is NaN, equal where
it is infinite, the very bits where every reward was +-0.0, and elsewhere within the bound
backtest_trace.run_with_bounds derives.  The 16 copies of an env give identical bytes.  Every call's path, as
the library reports it under GTE_DEBUG_GEOMETRY, is asserted: a fall-back to the step-by-step path fails.

  (a) backtest(actions), every chunk cleared; a second env continues one record (resume) through the same
      chunks and is held to the record of the whole trace
  (b) backtest_signals(K) with the tables of backtest_trace.signal_tables, rebound where a cell is taken
  (c) (b) with exit rules bound that can never fire; the exit state against tests/exit_model.py driven by
      the trace's columns.  (Binding a signal table leaves the exit state alone — only gte_bind_exit_rules
      starts it afresh — so the model's state is never rebuilt.)  With rules bound an env whose episode has ended
      and that was not reset gets hold whatever its table says (include/gte.h), which is not what the
      reference did on the three traces that step on after the end with auto-reset off: there (c) replays the
      calls before the first such step.
  (d) (a) and (b) step by step (KV_ROLLOUT_PER_STEP: every step folded in by gte_backtest_fold_kernel)
  (e) autoreset='same_step' on backtest_trace.same_step_timeline: in chunks, and as one call
"""
import re

import numpy as np
import pytest

import backtest_model as bm
import backtest_trace as bt
import exit_model as xm
import replay
import strata
from gym_trading_env_amd import _abi

pytestmark = pytest.mark.gpu

TILE = 16
NAMES = bt.names()
PATH_LINE = re.compile(r"\[gte\] rollout path: ([a-z -]+), (\d+) steps")
WORST = {}


def _seed(name):
    return sum(name.encode())


@pytest.fixture(scope="module")
def traces():
    cache = {}

    def load(name):
        if name not in cache:
            cache[name] = replay.load(name)
        return cache[name]
    return load


def _one(a, tag):
    """[TILE * E, ...] -> [E, ...] after asserting that all copies of an env hold the same bytes."""
    a = np.ascontiguousarray(a)
    b = a.reshape(TILE, -1).view(np.uint8)
    assert (b == b[0]).all(), f"{tag}: the {TILE} copies of an env differ"
    return a[:a.shape[0] // TILE]


class Replayed:
    """One env driven through trace g, tiled, with the reference's draws injected."""

    def __init__(self, g, monkeypatch, capfd, kernel_variant=0, autoreset="trace"):
        from gym_trading_env_amd.batched import BatchedTradingEnv
        monkeypatch.setenv("GTE_DEBUG_GEOMETRY", "1")
        self.g, self.f, self.capfd = g, strata.facts(g), capfd
        over = dict(kernel_variant=kernel_variant, envs_per_wave=4)
        if autoreset != "trace":
            over["autoreset"] = autoreset
        kw = replay.config_kwargs(g, TILE, **over)
        self.N = kw.pop("n_envs")
        kw.pop("n_static"); kw.pop("n_datasets")
        self.E = self.N // TILE
        self.env = BatchedTradingEnv(list(g["datasets"]) if self.f["D"] > 1 else g["datasets"][0], num_envs=self.N,
                                     output="torch", **kw)
        info = self.env.launch_info()
        shape_fused = (info["vector_bytes"], info["phase_a"], info["dyn_columns"]) == (16, "cooperative", "lds-raw-rings")
        assert shape_fused == strata.hot_shape(self.f), info
        self.fused = shape_fused and not kernel_variant & _abi.KV_ROLLOUT_PER_STEP
        self.taken = set()
        q, n = replay.injection_queue(g, TILE)
        if n:
            self.env.set_autoreset_injection(q["idx"], q["pos_index"], q["dataset"])
        t = lambda a: np.tile(a, TILE)
        self.env.reset(inject_idx=t(g["idx"][0]), inject_position_index=t(g["pos_index"][0]),
                       inject_dataset=t(g["dataset"][0]))
        self.B = replay.reward_ulp_bound(g)
        capfd.readouterr()

    def orders(self, k):
        g = self.g
        if "lo_pos" in g and (g["lo_pos"][k] >= 0).any():
            self.env.add_limit_order(np.tile(g["lo_pos"][k], TILE), np.tile(g["lo_limit"][k], TILE),
                                     np.ones(self.N, np.uint8))

    def _path(self, what, n, tag):
        expect = f"backtest {what}summary" if self.fused and n > 1 else f"backtest {what}per-step"
        paths = PATH_LINE.findall(self.capfd.readouterr().err)
        assert paths == [(expect, str(n))], (tag, paths, expect)
        self.taken.add(expect)

    def backtest(self, actions, resume, tag):
        import torch
        acts = torch.from_numpy(np.ascontiguousarray(np.tile(actions, (1, TILE)).astype(np.int32))).cuda()
        stats = self.env.backtest(acts, resume=resume)
        self._path("", acts.shape[0], tag)
        return _one(stats.numpy(), tag + " records")

    def backtest_signals(self, n, resume, tag):
        stats = self.env.backtest_signals(n, resume=resume)
        self._path("signals ", n, tag)
        return _one(stats.numpy(), tag + " records")

    def assert_state(self, state_call, step_call, tag):
        """The env against the trace: state and observation of call state_call[e], return buffers of call
        step_call[e] (the same call but after a same-step reset).  -> worst reward64 distance in ulp."""
        g, env = self.g, self.env
        ar = np.arange(self.E)
        state_call = np.broadcast_to(state_call, (self.E,))
        step_call = np.broadcast_to(step_call, (self.E,))
        for gk, sk in replay.STATE_I32.items():
            np.testing.assert_array_equal(_one(env.state(sk), f"{tag} {sk}"), g[gk][state_call, ar], err_msg=f"{tag}: {sk}")
        for gk, sk in replay.STATE_F64.items():
            replay.assert_same_value(_one(env.state(sk), f"{tag} {sk}"), g[gk][state_call, ar], f"{tag}: {sk}")
        r64 = _one(env.read_output("reward64"), f"{tag} reward64")
        worst = replay.assert_reward64(r64, g["reward"][step_call, ar], self.B, tag)
        replay.assert_same_value(_one(env.read_output("reward"), f"{tag} reward"), replay.to_float32(r64), f"{tag}: f32 reward")
        for out, col in (("terminated", "done"), ("truncated", "truncated")):
            np.testing.assert_array_equal(_one(env.read_output(out), f"{tag} {out}").astype(bool),
                                          g[col][step_call, ar].astype(bool), err_msg=f"{tag}: {out}")
        replay.assert_obs(_one(env.read_output("obs"), f"{tag} obs"), g["obs"][state_call, ar], self.f["Fs"], f"{tag}: obs")
        return worst

    def close(self):
        self.env.close()


def _assert_records(got, recs, bounds, exact, tag, worst):
    """Structured records [E] against the model's (backtest_trace.chunk_records); worst: {sum: largest
    distance / bound seen}, updated."""
    ref = bm.as_arrays(recs)
    for f in bm.INT_FIELDS:
        np.testing.assert_array_equal(got[f], ref[f], err_msg=f"{tag}: {f}")
    np.testing.assert_array_equal(got["ended"] != 0, [r["ended"] for r in recs], err_msg=f"{tag}: ended")
    for f in bt.VALUES:
        replay.assert_same_value(np.ascontiguousarray(got[f]), ref[f], f"{tag}: {f}")
    for f in bt.SUMS:
        for e in range(len(recs)):
            x, w = np.float64(got[f][e]), ref[f][e]
            what = f"{tag}: {f} of env {e}: {x!r}, the model over the reference's columns {w!r}"
            if np.isnan(w):
                assert np.isnan(x), what
            elif np.isinf(w):
                assert x == w, what
            elif exact[e] or bounds[e][f] == 0:
                # every reward was zero; or nothing was added to this sum (no episode ended, or one just did)
                assert replay.same_bits(np.array([x]), np.array([w])).all(), what + " (an exact sum)"
            else:
                d, b = abs(x - w), bounds[e][f]
                assert np.isfinite(b), (what, b)
                worst[f] = max(worst.get(f, 0.0), float(d / b))
                assert d <= b, f"{what}: |difference| {d:.3e} above the bound {b:.3e}"


def _report(name, path, worst, taken, ulp):
    top = max(worst.values(), default=0.0)
    WORST[name, path] = top
    print(f"[backtest-reference] {name} {path}: paths {', '.join(sorted(taken))}; worst reward64 distance {ulp:.0f} ulp; "
          f"largest distance / bound {top:.4f} (" + ", ".join(f"{f} {v:.4f}" for f, v in sorted(worst.items())) + ")")


def _run_actions(g, name, monkeypatch, capfd, kernel_variant, path):
    K = g["op"].shape[0]
    x = Replayed(g, monkeypatch, capfd, kernel_variant)
    y = Replayed(g, monkeypatch, capfd, kernel_variant)
    worst, ulp = {}, 0.0
    got_y = None
    for start, stop in bt.chunks(g, np.random.default_rng(_seed(name)), bt.longest(name)):
        tag = f"{name} {path} calls [{start}, {stop})"
        x.orders(start)
        y.orders(start)
        got = x.backtest(g["action"][start:stop], False, tag)
        _assert_records(got, *bt.chunk_records(g, start, stop), tag, worst)
        ulp = max(ulp, x.assert_state(stop - 1, stop - 1, tag))
        got_y = y.backtest(g["action"][start:stop], start > 1, tag + " resumed")
    tag = f"{name} {path} resumed over the whole trace"
    whole = {}
    _assert_records(got_y, *bt.chunk_records(g, 1, K), tag, whole)
    y.assert_state(K - 1, K - 1, tag)
    _report(name, path, worst, x.taken, ulp)
    _report(name, path + " resumed", whole, y.taken, ulp)
    x.close()
    y.close()


NEVER_FIRE = dict(stop_loss=[0, 0.01, 0, 0.02], take_profit=[0, 0.01, 0, 1e-6], trailing=[0, 0.01, 0, 1e-6],
                  max_hold=[0, 1, 0, 2])


def _never_firing_rules(P):
    """Rules that are off in the two ways include/gte.h names, alternating: all thresholds 0 under an
    exit_position that names a position; live thresholds under one that names none (P, -1)."""
    return xm.make_rules(exit_position=[0, P, P - 1, -1], **NEVER_FIRE)


def _exit_replay_end(g):
    """The calls [1, end) that backtest_signals with exit rules bound can follow the reference through:
    all of them, but with auto-reset off only those before an env is stepped on after its episode's end."""
    K = g["op"].shape[0]
    if bt.has_autoreset(g):
        return K
    ended = np.maximum.accumulate((g["done"] | g["truncated"]).astype(bool), axis=0)
    late = np.nonzero((ended[:-1] & (g["op"][1:] == 1)).any(axis=1))[0]
    return int(late[0]) + 1 if len(late) else K


def _run_signals(g, name, monkeypatch, capfd, kernel_variant, path, exits=False):
    import torch
    K, E = g["op"].shape
    P = len(g["cfg"]["positions"])
    end = _exit_replay_end(g) if exits else K
    assert end > 1
    x = Replayed(g, monkeypatch, capfd, kernel_variant)
    rng = np.random.default_rng(_seed(name))
    spans = bt.table_spans(g, rng, 1, end)
    model = None
    if exits:
        rules = _never_firing_rules(P)
        # (a device tensor: the host check of bind_exits refuses an exit_position that names no position)
        x.env.bind_exits(torch.from_numpy(rules.view(np.uint8).reshape(-1, 32).copy()).cuda())
        model = xm.ExitModel(E, rules, P, np.arange(E) % len(rules))
        episode = np.cumsum(g["op"] == 0, axis=0)
        ended = (g["done"] | g["truncated"]).astype(bool)
    cuts = sorted({c for c in [s for s, _ in bt.chunks(g, rng, bt.longest(name))] + [s[1] for s in spans] if c < end})
    first_of = {s[1]: s[0] for s in spans}
    tables = None
    worst, ulp, held = {}, 0.0, False
    for start, stop in zip(cuts, cuts[1:] + [end]):
        tag = f"{name} {path} calls [{start}, {stop})"
        if start in first_of:
            tables = first_of[start]
            x.env.bind_signals(tables)
        x.orders(start)
        got = x.backtest_signals(stop - start, False, tag)
        _assert_records(got, *bt.chunk_records(g, start, stop), tag, worst)
        ulp = max(ulp, x.assert_state(stop - 1, stop - 1, tag))
        if exits:
            for k in range(start, stop):
                raw = xm.raw_bytes(tables, np.arange(E), g["idx"][k - 1], g["dataset"][k - 1])
                act = model.actions(raw, episode[k - 1], g["step"][k - 1], g["portfolio_valuation"][k - 1],
                                    g["pos_index"][k - 1], ended[k - 1])
                step = g["op"][k] == 1
                assert (act[step] == g["action"][k][step]).all() and (act[~step] == -1).all(), (tag, k)
            state = _one(x.env.exit_state().numpy(), tag + " exit state")
            for f in ("entry", "peak"):
                replay.assert_same_value(np.ascontiguousarray(state[f]), np.ascontiguousarray(model.state[f]),
                                         f"{tag}: exit state {f}")
            for f in ("held", "latched", "exits"):
                np.testing.assert_array_equal(state[f], model.state[f], err_msg=f"{tag}: exit state {f}")
            assert not state["exits"].any() and not state["latched"].any()
            held = held or bool((state["held"] > 0).any())
    assert held or not exits, "no env ever held a position over a step: the exit state showed nothing"
    _report(name, path, worst, x.taken, ulp)
    x.close()


@pytest.mark.parametrize("name", NAMES)
def test_backtest_actions(name, traces, monkeypatch, capfd):
    _run_actions(traces(name), name, monkeypatch, capfd, 0, "actions")


@pytest.mark.parametrize("name", NAMES)
def test_backtest_signals(name, traces, monkeypatch, capfd):
    _run_signals(traces(name), name, monkeypatch, capfd, 0, "signals")


@pytest.mark.parametrize("name", NAMES)
def test_backtest_signals_with_exit_rules_that_never_fire(name, traces, monkeypatch, capfd):
    _run_signals(traces(name), name, monkeypatch, capfd, 0, "signals+exits", exits=True)


def _per_step(name):
    g = replay.load(name)
    return name.startswith(("numeric_", "slide_")) or "lo_pos" in g or len(g["datasets"]) > 1


PER_STEP = [n for n in NAMES if _per_step(n)]


@pytest.mark.parametrize("name", PER_STEP)
def test_backtest_actions_per_step(name, traces, monkeypatch, capfd):
    _run_actions(traces(name), name, monkeypatch, capfd, _abi.KV_ROLLOUT_PER_STEP, "actions per-step")


@pytest.mark.parametrize("name", PER_STEP)
def test_backtest_signals_per_step(name, traces, monkeypatch, capfd):
    _run_signals(traces(name), name, monkeypatch, capfd, _abi.KV_ROLLOUT_PER_STEP, "signals per-step")


def _same_step(name):
    g = replay.load(name)
    return bt.has_autoreset(g) and "lo_pos" not in g


SAME_STEP = [n for n in NAMES if _same_step(n)]


@pytest.mark.parametrize("name", SAME_STEP)
def test_backtest_same_step(name, traces, monkeypatch, capfd):
    """The same-step branch of backtest_step reads the terminal valuation and position back from the terminal
    record; the reset that follows the transition starts the next peak."""
    g = traces(name)
    steps, actions, step_call, state_call = bt.same_step_timeline(g)
    n, E = actions.shape
    x = Replayed(g, monkeypatch, capfd, autoreset="same_step")
    whole = Replayed(g, monkeypatch, capfd, autoreset="same_step")
    rng = np.random.default_rng(_seed(name))
    worst, ulp = {}, 0.0

    def records(j0, j1):
        at = state_call[j0 - 1] if j0 else np.zeros(E, np.int64)
        out = [bt.run_with_bounds(bm.new_record(g["portfolio_valuation"][at[e], e], g["position"][at[e], e]),
                                  steps[e][j0:j1], x.B) for e in range(E)]
        return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]

    j0 = 0
    while j0 < n:
        j1 = min(n, j0 + int(rng.integers(1, bt.longest(name) + 1)))
        tag = f"{name} same-step steps [{j0}, {j1})"
        got = x.backtest(actions[j0:j1], False, tag)
        _assert_records(got, *records(j0, j1), tag, worst)
        ulp = max(ulp, x.assert_state(state_call[j1 - 1], step_call[j1 - 1], tag))
        j0 = j1
    tag = f"{name} same-step, one call of {n} steps"
    one = {}
    _assert_records(whole.backtest(actions, False, tag), *records(0, n), tag, one)
    whole.assert_state(state_call[n - 1], step_call[n - 1], tag)
    _report(name, "same-step", worst, x.taken, ulp)
    _report(name, "same-step one call", one, whole.taken, ulp)
    x.close()
    whole.close()
