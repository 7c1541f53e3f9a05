"""tests/backtest_trace.py held from the traces alone: what tests/test_gpu_backtest_reference.py asks of the
backtest kernels is only as good as the chunks, records, tables and timelines this helper makes.  No GPU."""
import numpy as np
import pytest

import backtest_model as bm
import backtest_trace as bt
import replay
import strata

NAMES = bt.names()
SEEDS = (0, 1, 2)


@pytest.fixture(scope="module")
def traces():
    return {n: replay.load(n) for n in NAMES}


def test_trace_list():
    assert len(NAMES) == len(set(NAMES))
    assert not [n for n in NAMES if n.startswith(("exit_trace", "signal_trace", "hostcb_", "portfolio_", "set_df"))]
    fam = lambda p: sum(n.startswith(p) for n in NAMES)
    assert (fam("sweep_"), fam("numeric_"), fam("slide_")) == (27, 10, 9)
    assert {"c2_nowindow", "drawdown_done", "limit_orders", "no_autoreset", "multidataset_k3"} <= set(NAMES)
    assert set(bt.NAN_TRACES) <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_tables_reproduce_every_action(traces, name):
    """A plain-Python replay through the tables, rebound at the reported stops: every step() call gets the
    trace's action, and every cell is a hold byte or a valid position index."""
    g = traces[name]
    K, E = g["op"].shape
    P = len(g["cfg"]["positions"])
    rng = np.random.default_rng(5)
    spans = bt.table_spans(g, rng)
    assert [s[1] for s in spans] == [1] + [s[2] for s in spans[:-1]] and spans[-1][2] == K
    assert len(spans) - 1 <= 20, "more rebinds than were ever measured on these traces"
    checked = 0
    for tables, first, end in spans:
        assert len(tables) == len(g["datasets"])
        filler = [np.ones(t.shape, bool) for t in tables]
        for d, t in enumerate(tables):
            assert t.dtype == np.int8 and t.shape == (E, len(g["datasets"][d][1]))
        for k in range(first, end):
            for e in range(E):
                if g["op"][k, e] != 1:
                    continue
                d, i = int(g["dataset"][k - 1, e]), int(g["idx"][k - 1, e])
                raw = int(tables[d][e, i])
                assert (raw if 0 <= raw < P else -1) == g["action"][k, e], (name, k, e)
                filler[d][e, i] = False
                checked += 1
        for t, m in zip(tables, filler):
            assert ((t[m] >= 0) & (t[m] < P)).all() and ((t >= -1) & (t < P)).all()
    assert checked == int((g["op"][1:] == 1).sum())
    # a collision stops the tables BEFORE the call that needs the other action
    if len(spans) > 1:
        tables, first, end = spans[0]
        hit = [e for e in range(E) if g["op"][end, e] == 1 and
               (lambda raw: (raw if 0 <= raw < P else -1))(int(tables[int(g["dataset"][end - 1, e])][e, int(g["idx"][end - 1, e])]))
               != g["action"][end, e]]
        assert hit, (name, end)


def _chunk_stats(g, name, seed):
    """-> per (chunk, env): (start, stop, e, record, bound, exact)."""
    out = []
    for start, stop in bt.chunks(g, np.random.default_rng(seed), bt.longest(name)):
        recs, bounds, exact = bt.chunk_records(g, start, stop)
        out += [(start, stop, e, recs[e], bounds[e], exact[e]) for e in range(len(recs))]
    return out


@pytest.fixture(scope="module")
def chunked(traces):
    return {(n, s): _chunk_stats(traces[n], n, s) for n in NAMES for s in SEEDS}


@pytest.mark.parametrize("name", NAMES)
def test_chunks_cover_the_trace_and_cut_at_limit_orders(traces, name):
    g = traces[name]
    K = g["op"].shape[0]
    for seed in SEEDS:
        cs = bt.chunks(g, np.random.default_rng(seed), bt.longest(name))
        assert cs[0][0] == 1 and cs[-1][1] == K and all(a[1] == b[0] for a, b in zip(cs, cs[1:]))
        assert all(1 <= stop - start <= bt.longest(name) for start, stop in cs)
        if "lo_pos" in g:
            starts = {c[0] for c in cs}
            assert all(int(k) in starts for k in np.nonzero((g["lo_pos"] >= 0).any(axis=1))[0] if k > 0)


@pytest.mark.parametrize("name", NAMES)
def test_most_records_are_finite(chunked, name):
    """A condition of the GPU test, not a measurement: NaN for NaN proves little, so at least half of the
    (chunk, env) records of every trace have finite reward sums, and a finite record has finite bounds.
    On every trace without NaN valuations all of them are finite."""
    for seed in SEEDS:
        recs = chunked[name, seed]
        finite = [np.isfinite(r["reward_sum"]) and np.isfinite(r["reward_sq_sum"]) for _, _, _, r, _, _ in recs]
        share = np.mean(finite)
        print(f"{name} seed {seed}: {share:.2f} of {len(recs)} records finite")
        assert share >= 0.5 if name in bt.NAN_TRACES else share == 1.0, (name, seed, share)
        for _, _, _, r, b, _ in recs:
            for f in bt.SUMS:
                if np.isfinite(r[f]):
                    assert np.isfinite(b[f]) and b[f] >= 0, (name, f, r[f], b[f])


def test_the_family_covers_what_the_kernels_branch_on(traces, chunked):
    seen = dict.fromkeys(("nan_peak_at_start", "drawdown_above_1", "termination", "two_ends_in_a_chunk",
                          "limit_fill_under_hold", "transition_after_end", "zero_reward_transition",
                          "chunk_of_one_call", "dataset_switch_in_a_chunk", "exact_record_with_steps"), 0)
    for name in NAMES:
        g = traces[name]
        pos = g["position"]
        for start, stop, e, rec, bound, exact in chunked[name, 0]:
            seen["nan_peak_at_start"] += bool(np.isnan(g["portfolio_valuation"][start - 1, e]) and rec["steps"] > 0)
            seen["drawdown_above_1"] += bool(rec["max_drawdown"] > 1)
            seen["termination"] += rec["terminations"] > 0
            seen["two_ends_in_a_chunk"] += rec["episodes"] >= 2
            seen["chunk_of_one_call"] += stop - start == 1
            seen["dataset_switch_in_a_chunk"] += len(set(g["dataset"][start - 1:stop, e])) > 1
            seen["exact_record_with_steps"] += bool(exact and rec["steps"] > 0)
            ended = bool(bt.ended_at(g, start - 1)[e])
            for k in range(start, stop):
                moved = g["op"][k, e] == 1 and g["step"][k, e] != g["step"][k - 1, e]
                if g["op"][k, e] == 0:
                    ended = False
                    continue
                if moved:
                    seen["limit_fill_under_hold"] += bool(g["action"][k, e] == -1 and pos[k, e] != pos[k - 1, e])
                    seen["transition_after_end"] += bool(ended and not bt.has_autoreset(g))
                    r = g["reward"][k, e]
                    seen["zero_reward_transition"] += bool(r == 0.0 and not np.signbit(r))
                ended = ended or bool(g["done"][k, e] or g["truncated"][k, e])
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("name", NAMES)
def test_chunk_records_over_the_whole_trace_are_the_trace_record(traces, name):
    g = traces[name]
    K, E = g["op"].shape
    recs, bounds, exact = bt.chunk_records(g, 1, K)
    for e in range(E):
        want = bm.trace_record(g, e)
        for f in bm.INT_FIELDS + ("ended",):
            assert recs[e][f] == want[f], (name, e, f)
        for f in bm.F64_FIELDS:
            assert replay.same_value(np.array([recs[e][f]]), np.array([want[f]])).all(), (name, e, f)


@pytest.mark.parametrize("name", NAMES)
def test_a_chunk_starts_ended_where_the_chunks_before_it_end_ended(traces, name):
    """`ended` of a cleared record is the env's needs_reset, not the flags of the row it is cleared at: an
    env the reference steps on after the end lowers `done` again when its valuation recovers."""
    g = traces[name]
    K, E = g["op"].shape
    cs = bt.chunks(g, np.random.default_rng(0), bt.longest(name))
    for start, stop in cs[::max(1, len(cs) // 6)]:
        before = bt.chunk_records(g, 1, stop)[0]
        assert [r["ended"] for r in before] == list(bt.ended_at(g, stop - 1)), (name, stop)
    flags = (g["done"] | g["truncated"]).astype(bool)
    if bt.has_autoreset(g):
        for k in range(0, K, 7):
            assert (bt.ended_at(g, k) == flags[k]).all()


def test_flags_are_lowered_again_after_an_end(traces):
    lowered = [n for n in NAMES if not bt.has_autoreset(traces[n]) and any(
        (bt.ended_at(traces[n], k) != (traces[n]["done"][k] | traces[n]["truncated"][k]).astype(bool)).any()
        for k in range(traces[n]["op"].shape[0]))]
    assert lowered, "no trace shows an ended env with both flags down"


def _same_step(name):
    g = replay.load(name)
    return bt.has_autoreset(g) and "lo_pos" not in g


SAME_STEP = [n for n in NAMES if _same_step(n)]


def test_every_family_has_traces_at_the_shape_of_the_fused_kernels(traces):
    """The from-registers kernels serve strata.hot_shape only (elsewhere a backtest goes step by step, which
    the GPU test asserts call by call): each family, the NaN traces, same-step and limit-order traces have it."""
    hot = [n for n in NAMES if strata.hot_shape(strata.facts(traces[n]))]
    for family in ("sweep_", "numeric_", "slide_"):
        assert [n for n in hot if n.startswith(family)], family
    assert set(bt.NAN_TRACES) <= set(hot)
    assert [n for n in hot if n in SAME_STEP] and [n for n in hot if "lo_pos" in traces[n]]
    assert [n for n in hot if not bt.has_autoreset(traces[n])]


def test_same_step_traces():
    assert len(SAME_STEP) >= 40 and "no_autoreset" not in SAME_STEP and "limit_orders" not in SAME_STEP


@pytest.mark.parametrize("name", SAME_STEP)
def test_same_step_timeline_states_the_same_record(traces, name):
    """The same calls as same-step auto-reset sees them give the record the next-step statement gives: a reset
    changes no sum, whether it takes a call of its own or follows its transition."""
    g = traces[name]
    K, E = g["op"].shape
    steps, actions, step_call, state_call = bt.same_step_timeline(g)
    n = actions.shape[0]
    assert n > 0 and actions.shape == (n, E) and step_call.shape == state_call.shape == (n, E)
    assert state_call.max() <= K - 1
    ends = (g["done"] | g["truncated"]).astype(bool)
    resets = 0
    for e in range(E):
        calls = [k for k in range(1, K) if g["op"][k, e] == 1]
        assert list(step_call[:, e]) == calls[:n]
        assert (actions[:, e] == g["action"][step_call[:, e], e]).all()
        assert (state_call[:, e] == step_call[:, e] + ends[step_call[:, e], e]).all()
        assert (g["op"][state_call[:, e], e] == 1 - ends[step_call[:, e], e]).all()
        resets += int(ends[step_call[:, e], e].sum())
        same = bm.run(bm.new_record(g["portfolio_valuation"][0, e], g["position"][0, e]), steps[e])
        last = int(state_call[n - 1, e])
        nxt = bm.run(bm.new_record(g["portfolio_valuation"][0, e], g["position"][0, e]), bm.trace_steps(g, e)[:last])
        for f in bm.INT_FIELDS + ("ended",):
            assert same[f] == nxt[f], (name, e, f)
        for f in bm.F64_FIELDS:
            assert replay.same_value(np.array([same[f]]), np.array([nxt[f]])).all(), (name, e, f)
        assert not same["ended"]
    # K' is as large as the trace allows: every call of the env with the fewest, less one only where that
    # env's last step ends an episode on the last call of the trace
    counts = [int((g["op"][1:, e] == 1).sum()) for e in range(E)]
    m = min(counts)
    cut = any(c == m and g["op"][K - 1, e] == 1 and ends[K - 1, e] for e, c in enumerate(counts))
    assert n == (m - 1 if cut else m), (name, n, m, cut)
    assert resets > 0, "no episode ends inside the timeline"


def test_bounds_by_hand():
    """Three rewards of 0.5, 0.25 and -0.75 with B = 1, the last one ending the episode; all sums exact in
    binary, so the bound is what the rule says and nothing else."""
    sp = np.spacing
    steps = [dict(stepped=True, v=1.0, p=1.0, r=0.5, terminated=False, truncated=False),
             dict(stepped=False),
             dict(stepped=True, v=1.0, p=1.0, r=0.25, terminated=False, truncated=False),
             dict(stepped=True, v=1.0, p=1.0, r=-0.75, terminated=False, truncated=True)]
    rec, b, exact = bt.run_with_bounds(bm.new_record(1.0, 1.0), steps, 1)
    assert not exact and rec["steps"] == 3 and rec["episodes"] == 1
    want = sp(0.5)
    want += sp(0.5 + want)
    want += sp(0.25)
    want += sp(0.75 + want)
    cur = want + sp(0.75)
    cur += sp(0.0 + cur)
    want += sp(0.75)
    want += sp(0.0 + want)
    assert b["reward_sum"] == want and b["cur_return"] == 0.0 and rec["cur_return"] == 0.0
    assert b["ep_return_sum"] == cur + sp(0.0 + cur)
    sq = (2 * 0.0 + cur) * cur
    sq += sp(0.0 + sq)
    assert b["ep_return_sq_sum"] == sq + sp(0.0 + sq)
    assert 0 < b["reward_sq_sum"] < 16 * sp(0.875) and rec["reward_sq_sum"] == 0.875
    # rewards of +-0.0 alone: exact; a NaN reward: NaN bounds from there on
    zero = [dict(stepped=True, v=1.0, p=1.0, r=z, terminated=False, truncated=False) for z in (0.0, -0.0)]
    rec, b, exact = bt.run_with_bounds(bm.new_record(1.0, 1.0), zero, 3)
    assert exact and all(b[f] <= 8 * sp(0.0) for f in bt.SUMS)
    nan = zero + [dict(stepped=True, v=1.0, p=1.0, r=float("nan"), terminated=False, truncated=False)]
    rec, b, exact = bt.run_with_bounds(bm.new_record(1.0, 1.0), nan, 3)
    assert not exact and np.isnan(b["reward_sum"]) and np.isnan(rec["reward_sum"])
