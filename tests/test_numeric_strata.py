"""The committed numeric fixtures (tests/golden/numeric_NN.npz, make_golden.py --numeric) cover
every row of NUMERIC_STRATA in tests/strata.py, and the value-level comparison helpers of
tests/replay.py flag exactly what they say.  CPU only."""
import glob
import os

import numpy as np
import pytest

import replay
import special_words
import strata


def _numeric_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(replay.GOLDEN_DIR, "numeric_*.npz")))


def test_numeric_family_covers_every_stratum():
    names = _numeric_names()
    assert 8 <= len(names) <= 10, names
    gaps = strata.numeric_missing([replay.load(n) for n in names])
    assert not gaps, f"numeric strata rows no trace covers: {gaps}"


@pytest.mark.parametrize("name", _numeric_names())
def test_numeric_fixture_is_a_replayable_trace(name):
    """Each numeric fixture is a batched trace of the generator's format, within the size and
    shape budget, and its recorded strata are the ones its data actually has."""
    g = replay.load(name)
    assert name in replay.golden_names()
    assert os.path.getsize(os.path.join(replay.GOLDEN_DIR, name + ".npz")) <= 200 * 1024
    K, E = g["op"].shape
    assert E <= 4 and K <= 200 and all(len(ds[1]) <= 400 for ds in g["datasets"])
    assert (g["op"][0] == 0).all()
    W = g["cfg"]["windows"]
    Fobs = strata.facts(g)["Fobs"]
    assert g["obs"].shape == ((K, E, W, Fobs) if W else (K, E, Fobs))
    note = str(g["note"])
    recorded = note.split("strata: ")[1]
    assert (recorded.split(", ") if recorded else []) == strata.numeric_rows_of(g) != []
    # datasets are identified by their length
    assert len({len(ds[1]) for ds in g["datasets"]}) == len(g["datasets"])
    assert g["obs"].dtype == np.float32 and g["reward"].dtype == np.float64
    for ds in g["datasets"]:
        assert ds[0].dtype == np.float32 and ds[1].dtype == np.float64
        # the reference quiets signalling NaNs: none may be an input
        assert not special_words.is_signalling_nan(ds[0]).any()
        assert not np.isnan(ds[1]).any()
    for k in replay.STATE_F64:
        assert g[k].dtype == np.float64 and g[k].shape == (K, E)


def test_numeric_budget():
    total = sum(os.path.getsize(os.path.join(replay.GOLDEN_DIR, n + ".npz")) for n in _numeric_names())
    assert total <= 1536 * 1024


def test_no_fixture_feeds_a_signalling_nan():
    for name in replay.golden_names():
        for ds in replay.load(name)["datasets"]:
            assert not special_words.is_signalling_nan(ds[0]).any(), name


def test_place_special_words():
    feat = np.random.default_rng(0).normal(0, 1, (50, 6)).astype(np.float32)
    out = special_words.place_special_words(feat, seed=3)
    assert special_words.has_every_special_word(out) and not special_words.has_every_special_word(feat)
    changed = out.view(np.uint32) != feat.view(np.uint32)
    assert 0.10 <= changed.mean() <= 0.20
    assert np.isin(out.view(np.uint32)[changed], special_words.SPECIAL_F32_WORDS).all()
    assert not special_words.is_signalling_nan(out).any()
    snan = np.array([0x7F800001, 0xFFA00000, 0x7FC00000, 0x7F800000], np.uint32).view(np.float32)
    assert special_words.is_signalling_nan(snan).tolist() == [True, True, False, False]


# -- the comparison helpers on hand-made arrays ---------------------------------------------------
def _f64(*words):
    return np.array(words, np.uint64).view(np.float64)


def _f32(*words):
    return np.array(words, np.uint32).view(np.float32)


QNAN, QNAN_PAYLOAD, QNAN_NEG = 0x7FF8000000000000, 0x7FF8000000012345, 0xFFF8000000000000


def test_same_value_and_same_bits_f64():
    a = _f64(QNAN, QNAN, 0x0000000000000000, 0x3FF0000000000000, 0x7FF0000000000000, 0x7FF0000000000000,
             0x7FF0000000000000)
    b = _f64(QNAN_PAYLOAD, QNAN_NEG, 0x8000000000000000, 0x3FF0000000000001, 0x7FF0000000000000,
             0xFFF0000000000000, QNAN)
    #        two payloads  two signs  0.0 vs -0.0  one-ulp neighbours  inf == inf  inf vs -inf  inf vs NaN
    assert replay.same_value(a, b).tolist() == [True, True, False, False, True, False, False]
    assert replay.same_bits(a, b).tolist() == [False, False, False, False, True, False, False]
    assert replay.same_value(a, a).all() and replay.same_bits(b, b).all()
    replay.assert_same_value(a[:2], b[:2])
    with pytest.raises(AssertionError, match=r"index 2: got 0\.0 \(0x0000000000000000\), expected -0\.0 "
                                             r"\(0x8000000000000000\)"):
        replay.assert_same_value(a, b, "state")
    with pytest.raises(AssertionError, match=r"index 0: got nan \(0x7ff8000000000000\), expected nan "
                                             r"\(0x7ff8000000012345\)"):
        replay.assert_same_bits(a, b, "copied")


def test_same_value_and_same_bits_f32():
    a = _f32(0x7FC00000, 0x7FC00000, 0x00000000, 0x3F800000, 0x7F800000, 0x00000001)
    b = _f32(0x7FC12345, 0xFFC00001, 0x80000000, 0x3F800001, 0x7F800000, 0x00000001)
    assert replay.same_value(a, b).tolist() == [True, True, False, False, True, True]
    assert replay.same_bits(a, b).tolist() == [False, False, False, False, True, True]
    with pytest.raises(AssertionError, match=r"index \(1, 0\): got nan \(0x7fc00000\), expected nan \(0xffc00001\)"):
        replay.assert_same_bits(a[[4, 5, 1, 0]].reshape(2, 2), b[[4, 5, 1, 0]].reshape(2, 2))
    with pytest.raises(AssertionError):  # one dtype on both sides: no silent widening
        replay.same_value(a, a.astype(np.float64))
    # an observation: static columns strict, dynamic columns by value
    obs = np.stack([a, a])
    ref = obs.copy()
    ref[0, 0] = b[0]
    with pytest.raises(AssertionError, match="static columns"):
        replay.assert_obs(obs, ref, 1, "obs")
    replay.assert_obs(obs, ref, 0, "obs")          # the same word as a dynamic column: NaN for NaN
    ref[1, 2] = b[2]
    with pytest.raises(AssertionError, match="dynamic columns"):
        replay.assert_obs(obs, ref, 0, "obs")      # 0.0 for -0.0 is a different value


def test_ulp_distance_with_nan_and_inf():
    one, up, inf, big = 0x3FF0000000000000, 0x3FF0000000000001, 0x7FF0000000000000, 0x7FEFFFFFFFFFFFFF
    a = _f64(one, 0x0000000000000000, 0x0000000000000001, QNAN, QNAN, inf, inf, big, one)
    b = _f64(up, 0x8000000000000000, 0x8000000000000001, QNAN_NEG, one, inf, inf | 1 << 63, inf, one + 5)
    d = replay.ulp_distance(a, b)
    assert d.tolist() == [1, 0, 2, 0, np.inf, 0, np.inf, np.inf, 5]
    assert replay.ulp_distance(b, a).tolist() == d.tolist()


def test_assert_reward64():
    one, up2 = 0x3FF0000000000000, 0x3FF0000000000002
    ref = _f64(0, one, QNAN_NEG, 0x7FF0000000000000, 0xFFF0000000000000)
    ok = _f64(0, one + 1, QNAN_PAYLOAD, 0x7FF0000000000000, 0xFFF0000000000000)
    assert replay.assert_reward64(ok, ref, 1, "t") == 1.0
    assert replay.assert_reward64(ref, ref, 1, "t") == 0.0
    for i, word, why in ((0, 0x8000000000000000, "exactly zero"),   # -0.0 where the trace has +0.0
                         (0, 0x0000000000000001, "exactly zero"),   # one ulp from zero is not zero
                         (1, up2, "2 ulp"),
                         (1, QNAN, "inf ulp"),                      # NaN where the trace is finite
                         (2, one, "not NaN"),
                         (3, 0x7FEFFFFFFFFFFFFF, "where the trace's is"),   # DBL_MAX is not inf
                         (4, 0x7FF0000000000000, "where the trace's is")):  # +inf is not -inf
        bad = ok.copy()
        bad[i] = _f64(word)[0]
        with pytest.raises(AssertionError, match=why):
            replay.assert_reward64(bad, ref, 1, "t")
    replay.assert_reward64(_f64(0, up2, QNAN, 0x7FF0000000000000, 0xFFF0000000000000), ref, 3, "t")
    # the f32 reward the device derives: out of range to inf / zero, NaN stays NaN
    r32 = replay.to_float32(np.array([1e39, -1e39, 1e-46, np.nan, -0.0]))
    assert replay.same_value(r32, _f32(0x7F800000, 0xFF800000, 0, 0x7FC00000, 0x80000000)).all()


def _correctly_rounded_log(x):
    """log(x) of a positive finite double, rounded to nearest from 50 decimal digits."""
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        return float(decimal.Decimal(float(x)).ln())


def test_reference_rewards_are_within_one_ulp_of_the_correctly_rounded_log():
    """What replay.reward_ulp_bound is measured against: over the numeric family (|log return| from
    1e-16 to 1.8), the reference's recorded basic reward lies within 1 ulp of the correctly rounded
    log of the quotient of its own recorded valuations.  A device value 1 ulp from the reference's
    is therefore at most 2 ulp from the correctly rounded one."""
    worst, n = 0.0, 0
    for name in _numeric_names():
        g = replay.load(name)
        if strata.facts(g)["reward"] != "basic":
            continue
        pv, r = g["portfolio_valuation"], g["reward"]
        with np.errstate(all="ignore"):
            q = pv[1:] / pv[:-1]
        use = (g["op"][1:] == 1) & (g["done"][1:] == 0) & np.isfinite(q) & (q > 0) & np.isfinite(r[1:])
        exact = np.array([_correctly_rounded_log(x) for x in q[use]])
        d = replay.ulp_distance(r[1:][use], exact)
        worst, n = max(worst, float(d.max())), n + int(use.sum())
    print(f"[numeric] reference reward against the correctly rounded log: worst {worst:.0f} ulp over {n} steps")
    assert n > 3000 and worst <= 1
