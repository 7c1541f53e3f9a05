"""Replay a golden trace (tests/golden/*.npz, made by make_golden.py from the
reference itself) through any batched implementation and compare per call.

`adapter` is an object with reset(mask, inj_idx, inj_pos, inj_ds),
set_autoreset_injection(idx, pos, ds), step(actions) and numpy accessors
obs(), reward64(), terminated(), truncated(), state() -> dict.
"""
from __future__ import annotations

import glob
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

STATE_F64 = {"asset": "asset", "fiat": "fiat", "interest_asset": "interest_asset",
             "interest_fiat": "interest_fiat", "portfolio_valuation": "portfolio_valuation",
             "real_position": "real_position"}
STATE_I32 = {"idx": "idx", "step": "step", "pos_index": "position_index",
             "dataset": "dataset_index"}


def golden_names():
    """Names of the trace fixtures a BATCHED implementation can replay (portfolio_random.npz is
    a known-answer table and set_df.npz a staging fixture, not traces; hostcb_* traces need
    Python callables per env and are replayed by the N=1 drop-in only)."""
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz"))
                  if not os.path.basename(p).startswith(("portfolio_", "hostcb_", "set_df")))


def load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    return from_arrays({k: z[k] for k in z.files})


def from_arrays(arrays):
    """A trace from the arrays of its fixture file (not modified)."""
    g = dict(arrays)
    g["cfg"] = json.loads(str(g.pop("cfg_json")))
    d = 0
    sets = []
    while f"feat_{d}" in g:
        ds = (g.pop(f"feat_{d}"), g.pop(f"close_{d}"))
        if f"high_{d}" in g:
            ds += (g.pop(f"high_{d}"), g.pop(f"low_{d}"))
        sets.append(ds)
        d += 1
    g["datasets"] = sets
    return g


def config_kwargs(g, tile: int = 1, **over):
    """make_config kwargs for a trace, its E envs repeated `tile` times."""
    cfg = dict(g["cfg"])
    K, E = g["op"].shape
    rf = cfg.get("reward_function", "basic_reward_function")
    cfg["reward_function"] = tuple(rf) if isinstance(rf, list) else rf
    kw = dict(n_envs=E * tile, n_static=g["datasets"][0][0].shape[1],
              n_datasets=len(g["datasets"]),
              autoreset="next_step" if (g["op"][1:] == 0).any() else None, **cfg)
    kw.update(over)
    return kw


def staged(g, n_dyn):
    """(feat [T, F_obs] with zero dynamic columns, close) per dataset."""
    out = []
    for ds in g["datasets"]:
        feat = ds[0]
        full = np.zeros((feat.shape[0], feat.shape[1] + n_dyn), np.float32)
        full[:, :feat.shape[1]] = feat
        out.append((full,) + tuple(ds[1:]))
    return out


def injection_queue(g, tile: int = 1):
    """Per env, the reference's draws at every reset after call 0, padded with -1."""
    op = g["op"]
    K, E = op.shape
    counts = (op[1:] == 0).sum(axis=0)
    n = int(counts.max()) if counts.size else 0
    q = {f: np.full((E, max(n, 1)), -1, np.int32) for f in ("idx", "pos_index", "dataset")}
    for e in range(E):
        ks = np.nonzero(op[1:, e] == 0)[0] + 1
        for j, k in enumerate(ks):
            for f in q:
                q[f][e, j] = g[f][k, e]
    return {f: np.tile(a, (tile, 1)) for f, a in q.items()}, n


def _bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.float64), x.dtype
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    """Elementwise: a and b (f32 or f64 arrays of one dtype and shape) have the identical bit
    pattern.  -0.0 is not 0.0; a NaN equals only the NaN of the same sign and payload."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return _bits(a) == _bits(b)


def same_value(a, b):
    """Elementwise: identical bit pattern, or both NaN.  The rule for COMPUTED values: the sign
    and payload of a NaN an arithmetic unit produces are the unit's choice (x86 sets the sign bit,
    the GPU does not); everything else, the sign of zero included, is part of the value."""
    a, b = np.asarray(a), np.asarray(b)
    return same_bits(a, b) | (np.isnan(a) & np.isnan(b))


def _assert_all(ok, got, ref, err_msg, what):
    if ok.all():
        return
    got, ref = np.asarray(got), np.asarray(ref)
    bad = np.argwhere(~ok)
    i = tuple(int(j) for j in bad[0])
    width = 2 * got.dtype.itemsize
    raise AssertionError(f"{err_msg}: {len(bad)} of {ok.size} elements differ ({what}); first at index "
                         f"{i if len(i) != 1 else i[0]}: got {float(got[i])!r} (0x{int(_bits(got)[i]):0{width}x}), "
                         f"expected {float(ref[i])!r} (0x{int(_bits(ref)[i]):0{width}x})")


def assert_same_value(got, ref, err_msg=""):
    """same_value everywhere; reports the first differing index and both bit patterns."""
    _assert_all(same_value(got, ref), got, ref, err_msg, "bit pattern, any NaN equal to any NaN")


def assert_same_bits(got, ref, err_msg=""):
    """same_bits everywhere (no NaN clause): for values that are only ever copied."""
    _assert_all(same_bits(got, ref), got, ref, err_msg, "bit pattern")


def ulp_distance(a, b):
    """Integer distance of the IEEE bit patterns of f64 arrays a and b (0.0 and -0.0 are one
    value): how many representable doubles lie between them.  Where either is NaN or infinite no
    such count exists: the distance is 0 if they are the same value (both NaN, or the same
    infinity) and inf otherwise, so that a bound on the result also rejects a non-finite value
    standing in for a finite one."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    special = ~(np.isfinite(a) & np.isfinite(b))

    def key(x):
        i = np.where(special, 0.0, x).view(np.int64).astype(object)
        return np.where(i < 0, -(i & 0x7FFFFFFFFFFFFFFF), i)
    d = np.abs(key(a) - key(b)).astype(np.float64)
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    return np.where(special, np.where(same, 0.0, np.inf), d)


def assert_reward64(got, ref, bound, tag):
    """reward64 against the trace's: the very bits where the trace's is zero (resets and `done`
    are +0.0), NaN where it is NaN, equal where it is infinite, within `bound` ulp elsewhere.
    Returns the worst finite distance."""
    got = np.ascontiguousarray(got, np.float64)
    ref = np.ascontiguousarray(ref, np.float64)
    zero = ref == 0.0
    assert_same_bits(got[zero], ref[zero], f"{tag} reward64 where the trace's is exactly zero")
    nan = np.isnan(ref)
    assert np.isnan(got[nan]).all(), f"{tag} reward64: not NaN where the trace's is"
    inf = np.isinf(ref)
    assert (got[inf] == ref[inf]).all(), f"{tag} reward64: {got[inf]!r} where the trace's is {ref[inf]!r}"
    d = ulp_distance(got, ref)
    assert d.max() <= bound, (f"{tag} reward64: {d.max():.0f} ulp from the trace (bound {bound}) at env "
                              f"{int(d.argmax())}: {got[d.argmax()]!r} vs {ref[d.argmax()]!r}")
    return float(d.max())


def to_float32(r64):
    """float32(r64) as the device casts: round to nearest, overflow to inf, no warning."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(r64, np.float64).astype(np.float32)


def assert_obs(got, ref, n_static, err_msg):
    """An observation against the trace's: the static feature columns are only ever copied
    (assert_same_bits), the dynamic ones are computed (assert_same_value)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert_same_bits(got[..., :n_static], ref[..., :n_static], err_msg + " static columns")
    assert_same_value(got[..., n_static:], ref[..., n_static:], err_msg + " dynamic columns")


def reward_ulp_bound(g):
    """How many ulp reward64 may lie from the trace's: the log-return itself is within 1 ulp
    (device / libm log against NumPy's; measured).  A factor k that is not a power of two
    (scaled_log_return k=100) spreads that ulp: |k*lr' - k*lr| <= |k| ulp(lr) <= 2^-52 |k lr|,
    at most 2 ulp of the product, plus half an ulp from each of the two roundings -> 3.  (Clipping
    only replaces values by the bounds, which are exact.)"""
    rf = g["cfg"].get("reward_function", "basic_reward_function")
    k = 1.0 if isinstance(rf, str) else float(rf[1])
    return 1 if np.frexp(abs(k))[0] == 0.5 else 3


def replay(adapter, g, tile: int = 1, rtol: float = 1e-12, obs_exact: bool = True,
           check_state: bool = True, reward_ulps: int | None = None, stats: dict | None = None):
    """Drive `adapter` through trace g; assert parity at every call.

    reward_ulps=n: the exact mode.  The fp64 state is compared by value (same_value: the bit
    pattern, any NaN for any NaN; rtol is not used), the static observation columns bit for bit and
    the dynamic ones by value, reward64 as assert_reward64 says (within n ulp of the trace, the
    very bits where the trace's reward is zero, NaN / inf where it is), and, when the adapter has
    reward32(), the f32 reward is float32 of the adapter's own reward64.  stats["reward_ulps"]
    receives the worst distance seen."""
    exact = reward_ulps is not None
    worst_ulp = 0.0
    K, E = g["op"].shape
    t = lambda a: np.tile(a, tile)
    assert (g["op"][0] == 0).all()
    q, n = injection_queue(g, tile)
    if n:
        adapter.set_autoreset_injection(q["idx"], q["pos_index"], q["dataset"])
    adapter.reset(None, t(g["idx"][0]), t(g["pos_index"][0]), t(g["dataset"][0]))
    worst = 0.0
    for k in range(K):
        if k > 0:
            if "lo_pos" in g and (g["lo_pos"][k] >= 0).any():
                adapter.add_limit_orders(t(g["lo_pos"][k]), t(g["lo_limit"][k]),
                                         np.ones(E * tile, np.uint8))
            adapter.step(t(g["action"][k]))
        st = adapter.state()
        tag = f"call {k}"
        for gk, sk in STATE_I32.items():
            np.testing.assert_array_equal(st[sk], t(g[gk][k]), err_msg=f"{tag} {gk}")
        np.testing.assert_array_equal(adapter.terminated().astype(bool),
                                      t(g["done"][k]).astype(bool), err_msg=f"{tag} done")
        np.testing.assert_array_equal(adapter.truncated().astype(bool),
                                      t(g["truncated"][k]).astype(bool), err_msg=f"{tag} truncated")
        if check_state:
            for gk, sk in STATE_F64.items():
                ref = t(g[gk][k])
                got = st[sk]
                if exact:
                    assert_same_value(got, ref, f"{tag} {gk}")
                else:
                    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
                    err = np.where(ref == got, 0.0, err)
                    worst = max(worst, float(err.max()))
                    np.testing.assert_allclose(got, ref, rtol=rtol, atol=1e-14 if rtol > 0 else 0,
                                               err_msg=f"{tag} {gk}")
        r64 = adapter.reward64()
        ref_r = t(g["reward"][k])
        if exact:
            worst_ulp = max(worst_ulp, assert_reward64(r64, ref_r, reward_ulps, tag))
            if hasattr(adapter, "reward32"):
                assert_same_value(adapter.reward32(), to_float32(r64),
                                  f"{tag} f32 reward != float32(reward64)")
        else:
            np.testing.assert_allclose(r64, ref_r, rtol=max(rtol, 1e-12), atol=1e-15,
                                       err_msg=f"{tag} reward")
        obs = adapter.obs()
        ref_obs = np.tile(g["obs"][k], (tile,) + (1,) * (g["obs"][k].ndim - 1))
        if exact:
            assert_obs(obs, ref_obs, g["datasets"][0][0].shape[1], f"{tag} obs")
        elif obs_exact:
            np.testing.assert_array_equal(obs, ref_obs, err_msg=f"{tag} obs")
        else:
            np.testing.assert_allclose(obs, ref_obs, rtol=1e-6, atol=1e-7, err_msg=f"{tag} obs")
    if stats is not None:
        stats["reward_ulps"] = max(stats.get("reward_ulps", 0.0), worst_ulp)
    return worst
