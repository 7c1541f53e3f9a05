"""The oracle's own reset draws (no injection) against the laws the reference states for them
(draw_laws.py): start rows, positions and dataset rounds, their independence, and how they are
keyed by (seed, global env id).  Device-vs-oracle parity cannot see a wrong law, since both sides
run the same formula; these tests can.  The power controls prove that the dataset-round checker,
at the sample sizes used here, rejects the keyed bijection the library used before (restated
below in numpy) and accepts numpy's own permutations.  CPU only.
"""
import functools

import numpy as np
import pytest

import draw_laws as L
from gym_trading_env_amd.config import make_config

N_ENVS = 65536
W = 3  # windows=3: the first row a window allows is W - 1 = 2
MAX_DUR = 2
ROUNDS_PER_ENV = 4  # x 65 536 envs = 2^18 rounds per D


def _sets(Ts):
    """Tiny datasets (one static feature): the draws do not read prices."""
    return [(np.zeros((T, 3), np.float32), np.full(T, 100.0)) for T in Ts]


def _oracle(oracle_mod, Ts, n_envs=N_ENVS, **kw):
    kw.setdefault("windows", W)
    kw.setdefault("max_episode_duration", MAX_DUR)
    cfg = make_config(n_envs=n_envs, n_static=1, n_datasets=len(Ts), **kw)
    return oracle_mod.OracleEnv(cfg, _sets(Ts))


def _T_for_span(span):
    return span + MAX_DUR + 2 * (W - 1)


@functools.lru_cache(maxsize=None)
def _single(span, P, seed=11, R=4):
    from oracle import oracle
    oracle.build()
    env = _oracle(oracle, [_T_for_span(span)], positions=list(range(P)), seed=seed)
    out = L.collect_resets(env, R)
    env.close()
    return out


@functools.lru_cache(maxsize=None)
def _rounds(D, seed=5):
    """[N, ROUNDS_PER_ENV, D] complete pick rounds of every env (switch at every episode; round 0
    is not complete, its pick 0 is the constructor's) plus the raw picks."""
    from oracle import oracle
    oracle.build()
    env = _oracle(oracle, [12] * D, windows=None, max_episode_duration="max", seed=seed)
    ds = L.collect_resets(env, (ROUNDS_PER_ENV + 1) * D - 1, fields=("dataset_index",))["dataset_index"]
    env.close()
    picks = L.picks_from_resets(ds, 1, D)
    return L.full_rounds(picks, D), picks


def _assert_laws(ps, tag):
    assert not L.rejects(ps), f"{tag}: {L.failing(ps)} (all: {ps})"


# ---------------------------------------------------------------------------------------------
# start rows and positions

@pytest.mark.parametrize("span", [1, 2, 3, 7, 64, 100_003])
def test_start_rows_uniform(span):
    """randint(W-1, T - max_dur - (W-1)) (environments.py:173-177): uniform over the span."""
    s = _single(span, 5)["start_idx"]
    low = W - 1
    assert s.min() >= low and s.max() < low + span, (s.min(), s.max())
    if span > 1:
        assert s.min() == low and s.max() == low + span - 1  # both ends occur
    _assert_laws(L.uniform_range_p(s, low, low + span), f"span {span}")


def test_start_rows_per_dataset(oracle_mod):
    """Datasets of different lengths: each env's start row follows its own dataset's span."""
    spans = [5, 333, 4000]
    env = _oracle(oracle_mod, [_T_for_span(s) for s in spans], positions=[0, 1, 2], seed=3)
    got = L.collect_resets(env, 6)
    env.close()
    for d, span in enumerate(spans):
        s = got["start_idx"][got["dataset_index"] == d]
        assert s.size > 100_000
        _assert_laws(L.uniform_range_p(s, W - 1, W - 1 + span), f"dataset {d}, span {span}")


def test_start_rows_at_max_duration(oracle_mod):
    env = _oracle(oracle_mod, [40], max_episode_duration="max", n_envs=4096, seed=1)
    got = L.collect_resets(env, 3)
    env.close()
    assert (got["start_idx"] == W - 1).all()


@pytest.mark.parametrize("P", [2, 3, 5, 32])
def test_positions_uniform(P):
    """np.random.choice(positions) (environments.py:167)."""
    pos = _single(7, P)["position_index"]
    _assert_laws({"position": L.uniform_p(pos, P)}, f"P={P}")


@pytest.mark.parametrize("fixed", [0, 3, 4])
def test_fixed_initial_position(oracle_mod, fixed):
    positions = [-1.0, -0.5, 0.0, 0.5, 1.0]
    env = _oracle(oracle_mod, [40], n_envs=4096, positions=positions, initial_position=positions[fixed])
    got = L.collect_resets(env, 3)
    env.close()
    assert (got["position_index"] == fixed).all()


# ---------------------------------------------------------------------------------------------
# dataset rounds

DS = [2, 3, 5, 6, 16, 17, 128]


@pytest.mark.parametrize("D", DS)
def test_dataset_rounds_are_permutations(D):
    rounds, picks = _rounds(D)
    assert rounds.shape == (N_ENVS, ROUNDS_PER_ENV, D)
    L.assert_rounds_are_permutations(rounds, D, f"D={D}")
    # round 0 without the constructor's pick: D - 1 different datasets
    first = np.sort(picks[1:D], axis=0)
    assert (np.diff(first, axis=0) > 0).all()
    assert (picks[1:] >= 0).all() and (picks[1:] < D).all()


@pytest.mark.parametrize("D", DS)
def test_dataset_rounds_uniform(D):
    """"Uniform among the least-used datasets" (environments.py:383-388): each round a uniformly
    random order, independent of the round before."""
    rounds, _ = _rounds(D)
    ps = L.round_laws(rounds, D)
    assert ("order" in ps) == (D <= 6)
    _assert_laws(ps, f"D={D}")


@pytest.mark.parametrize("switch", [1, 2, 3])
@pytest.mark.parametrize("D", [3, 5, 17])
def test_dataset_rounds_with_switch_interval(oracle_mod, D, switch):
    """episodes_between_dataset_switch = s: a pick at every s-th reset (:394-398); the picks, the
    constructor's first one included, still form rounds of D."""
    env = _oracle(oracle_mod, [12] * D, n_envs=4096, windows=None, max_episode_duration="max",
                  episodes_between_dataset_switch=switch, seed=9)
    ds = L.collect_resets(env, 3 * D * switch)["dataset_index"]
    env.close()
    # between two picks the dataset stays
    for t in range(ds.shape[0] - 1):
        if (t + 2) % switch != 0:
            np.testing.assert_array_equal(ds[t + 1], ds[t], err_msg=f"reset {t + 1} switched")
    picks = L.picks_from_resets(ds, switch, D)
    rounds = L.full_rounds(picks, D)
    assert rounds.shape[1] >= 2
    L.assert_rounds_are_permutations(rounds, D, f"D={D} switch={switch}")


# ---------------------------------------------------------------------------------------------
# independence

def test_start_and_position_independent():
    got = _single(64, 5)
    s, ks = L.coarse(got["start_idx"] - (W - 1), 64, 16)
    assert L.independence_p(s, got["position_index"], ks, 5) >= L.ALPHA


def _pairs_p(a, b, k):
    a, ka = L.coarse(a, k, 16)
    b, kb = L.coarse(b, k, 16)
    return L.independence_p(a, b, ka, kb)


def test_neighbour_envs_independent():
    """Env 2i against env 2i+1 (the same wave on any geometry) and env i against env i+64."""
    got = _single(64, 5)
    s = got["start_idx"] - (W - 1)
    p = got["position_index"]
    rounds, _ = _rounds(17)
    first = rounds[:, :, 0]
    ps = {"start": _pairs_p(s[:, 0::2], s[:, 1::2], 64),
          "position": _pairs_p(p[:, 0::2], p[:, 1::2], 5),
          "dataset": _pairs_p(first[0::2], first[1::2], 17)}
    idx = np.arange(N_ENVS).reshape(-1, 128)
    ps["position+64"] = _pairs_p(p[:, idx[:, :64]], p[:, idx[:, 64:]], 5)
    _assert_laws(ps, "env e vs e+1")


def test_consecutive_episodes_independent():
    got = _single(64, 5)
    s = got["start_idx"] - (W - 1)
    p = got["position_index"]
    rounds, _ = _rounds(5)
    ps = {"start": _pairs_p(s[0::2], s[1::2], 64), "position": _pairs_p(p[0::2], p[1::2], 5),
          # pick 1 of a round against pick 2 given that they differ: the order test covers it;
          # here the dataset of consecutive episodes across a round boundary
          "dataset": _pairs_p(rounds[:, :-1, -1], rounds[:, 1:, 0], 5)}
    _assert_laws(ps, "episode t vs t+1")


# ---------------------------------------------------------------------------------------------
# keying: (seed, global env id, episode)

def _draws(oracle_mod, n_envs=8192, R=3 * 5, D=5, **kw):
    env = _oracle(oracle_mod, [_T_for_span(64)] * D, n_envs=n_envs, positions=[0, 1, 2, 3, 4], **kw)
    got = L.collect_resets(env, R)
    env.close()
    return got


def test_same_seed_same_draws(oracle_mod):
    a, b = _draws(oracle_mod, seed=21), _draws(oracle_mod, seed=21)
    for f in L.FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)


def test_other_seed_matches_at_chance_rate(oracle_mod):
    a, b = _draws(oracle_mod, seed=21), _draws(oracle_mod, seed=22)
    for f, k in (("start_idx", 64), ("position_index", 5)):
        same = int((a[f] == b[f]).sum())
        n = a[f].size
        p = L.chisquare([same, n - same], [n / k, n - n / k])
        assert p >= L.ALPHA, (f, same / n, 1 / k)
    # dataset picks: one round per row; a match per pick has chance 1/D
    ra = L.full_rounds(L.picks_from_resets(a["dataset_index"], 1, 5), 5)
    rb = L.full_rounds(L.picks_from_resets(b["dataset_index"], 1, 5), 5)
    same = int((ra == rb).sum())
    p = L.chisquare([same, ra.size - same], [ra.size / 5, ra.size * 4 / 5])
    assert p >= L.ALPHA, same / ra.size


def test_shard_draws_what_the_unsharded_batch_draws(oracle_mod):
    full = _draws(oracle_mod, n_envs=4096, seed=33)
    for base, n in ((0, 1000), (1000, 1000), (2345, 1751)):
        part = _draws(oracle_mod, n_envs=n, seed=33, env_id_base=base)
        for f in L.FIELDS:
            np.testing.assert_array_equal(part[f], full[f][:, base:base + n], err_msg=f"{f} base {base}")


def test_masked_reset_draws_only_for_masked_envs(oracle_mod):
    """An env left out of a reset keeps its state and draws nothing: over its own resets it
    sees exactly the sequence of an env that is reset every time."""
    N, R, D = 2048, 40, 5
    every = _draws(oracle_mod, n_envs=N, R=R, seed=44)
    env = _oracle(oracle_mod, [_T_for_span(64)] * D, n_envs=N, positions=[0, 1, 2, 3, 4], seed=44)
    rng = np.random.default_rng(0)
    count = np.zeros(N, np.int64)
    prev = None
    while count.min() < R // 2:
        mask = (rng.random(N) < 0.3).astype(np.uint8)
        env.reset(mask=mask)
        got = L.read_state(env)
        m = mask.astype(bool) & (count < R)
        for f in L.FIELDS:
            want = every[f][np.minimum(count, R - 1), np.arange(N)]
            np.testing.assert_array_equal(got[f][m], want[m], err_msg=f)
            if prev is not None:
                np.testing.assert_array_equal(got[f][~mask.astype(bool)], prev[f][~mask.astype(bool)],
                                              err_msg=f"{f}: an unmasked env changed")
        count += mask
        prev = got
    env.close()


# ---------------------------------------------------------------------------------------------
# power controls: the same checker, the same sample size

def perm_pick_bijection(keys, D: int):
    """The dataset pick of earlier versions, restated in numpy as the negative control: for four
    32-bit keys per round, an affine + xorshift bijection on b = ceil(log2 D) bits, cycle-walked
    into [0, D).  keys: u32 [..., 4] -> rounds [..., D]."""
    b = max(1, (D - 1).bit_length())
    mask = np.uint64((1 << b) - 1)
    sh = np.uint64((b + 1) // 2)
    r0, r1, r2, r3 = (keys[..., i].astype(np.uint64) for i in range(4))
    one = np.uint64(1)

    def rnd(x):
        x = (x * (r0 | one) + r1) & mask
        x ^= x >> sh
        x = (x * (r2 | one) + r3) & mask
        x ^= x >> sh
        x = (x * np.uint64(0x9E3779B1) + (r0 >> np.uint64(7))) & mask
        x ^= x >> sh
        return x

    out = []
    for k in range(D):
        x = rnd(np.full(r0.shape, k, np.uint64))
        while (x >= D).any():
            x = np.where(x >= D, rnd(x), x)
        out.append(x.astype(np.int64))
    return np.stack(out, axis=-1)


def test_negative_control_restates_the_bijection():
    """The restatement is a bijection per key (each round a permutation), as the old one was."""
    keys = np.random.default_rng(1).integers(0, 2**32, (512, 4), dtype=np.uint64).astype(np.uint32)
    for D in (2, 3, 5, 16, 17, 128, 1000):
        L.assert_rounds_are_permutations(perm_pick_bijection(keys, D), D, f"D={D}")


@pytest.mark.parametrize("D", [3, 5, 16, 17, 128])
def test_checker_rejects_the_old_bijection(D):
    rng = np.random.default_rng(100 + D)
    keys = rng.integers(0, 2**32, (N_ENVS, ROUNDS_PER_ENV, 4), dtype=np.uint64).astype(np.uint32)
    ps = L.round_laws(perm_pick_bijection(keys, D), D)
    assert L.rejects(ps), f"D={D}: the checker accepts the old bijection: {ps}"


@pytest.mark.parametrize("D", [3, 5, 16, 17, 128])
def test_checker_accepts_numpy_permutations(D):
    rng = np.random.default_rng(200 + D)
    rounds = rng.permuted(np.broadcast_to(np.arange(D), (N_ENVS, ROUNDS_PER_ENV, D)), axis=-1)
    _assert_laws(L.round_laws(rounds, D), f"D={D}")
