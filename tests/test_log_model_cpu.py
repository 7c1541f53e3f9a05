"""tests/log_model.py (the trajectory log as History would hold it, built from the C oracle)
against oracle/py_loop.PyEnv, whose per-env `log` list restates the reference's History: on
random configurations, with full and masked resets, in the three auto-reset modes, and for a
frozen env (auto-reset disabled, ended on the last row).  The GPU log tests compare the device
with this model, so it has to be right on its own.  CPU only."""
import numpy as np
import pytest

from gym_trading_env_amd.config import make_config
from log_model import LogModel
from oracle.py_loop import PyEnv
from test_oracle_cross import _case

E = 6


def _same_rows(got, want, positions, tag):
    """model rows (dicts) == PyEnv.log entries, field by field"""
    assert len(got) == len(want), (tag, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["idx"] == w["idx"] and g["step"] == w["step"], (tag, i, g, w)
        assert positions[g["position_index"]] == w["position"], (tag, i)
        for k in ("portfolio_valuation", "real_position", "reward"):
            np.testing.assert_allclose(g[k], w[k], rtol=1e-12, atol=0, err_msg=f"{tag} row {i} {k}")


def _setup(seed, mode, oracle_mod):
    rng, feat, close, kw = _case(seed)
    T, n_static = len(close), feat.shape[1]
    first = 0 if kw["windows"] is None else kw["windows"] - 1
    full = np.zeros((T, n_static + 2), np.float32)
    full[:, :n_static] = feat
    cfg = make_config(n_envs=E, n_static=n_static, autoreset=mode, dyn_persist=True, seed=seed, **kw)
    ora = oracle_mod.OracleEnv(cfg, [(full.copy(), close)])
    envs = [PyEnv(full.copy(), close, kw["positions"], windows=kw["windows"],
                  trading_fees=kw["trading_fees"], borrow_interest_rate=kw["borrow_interest_rate"],
                  portfolio_initial_value=kw["portfolio_initial_value"],
                  max_episode_duration=kw["max_episode_duration"], persist=True) for _ in range(E)]

    def draw(n=None):
        shape = (E,) if n is None else (E, n)
        md = kw["max_episode_duration"]
        hi = T - 1 if md == "max" else T - md - first
        idx = rng.integers(first, max(first + 1, hi), shape).astype(np.int32)
        if md == "max":
            idx[...] = first
        return idx, rng.integers(0, len(kw["positions"]), shape).astype(np.int32)
    return rng, kw, T, ora, envs, draw


@pytest.mark.parametrize("mode", [None, "next_step", "same_step"])
@pytest.mark.parametrize("seed", range(12))
def test_log_model_equals_python_loop(oracle_mod, seed, mode):
    rng, kw, T, ora, envs, draw = _setup(seed, mode, oracle_mod)
    L = int(rng.integers(3, 40))
    model = LogModel(ora, L, mode, [T])
    positions = kw["positions"]
    queue = None
    if mode is not None:  # the auto-resets' draws, queued on the oracle and replayed on the PyEnvs
        queue = draw(400)
        ora.set_autoreset_injection(queue[0], queue[1], None)
    used = np.zeros(E, np.int64)
    idx, pos = draw()
    ora.reset(None, idx, pos, None)
    model.reset()
    for e, env in enumerate(envs):
        env.reset(int(idx[e]), int(pos[e]))
    pending = np.zeros(E, bool)  # next-step mode: the PyEnv resets at its next step
    ends = masked = 0
    for k in range(160):
        for e, env in enumerate(envs):
            _same_rows(model.episode(e), env.log, positions, f"seed {seed} call {k} env {e}")
            if not model.frozen[e]:
                assert len(model.logged(e)) == min(len(env.log), L), (seed, k, e)
        if mode is None and k % 7 == 6:
            # a masked reset: the ended envs and a random few more, the others carry on
            m = np.array([env.ended for env in envs]) | (rng.random(E) < 0.2)
            idx, pos = draw()
            ora.reset(m.astype(np.uint8), idx, pos, None)
            model.reset(m.astype(np.uint8))
            for e in np.flatnonzero(m):
                envs[e].reset(int(idx[e]), int(pos[e]))
            masked += int(m.sum())
            continue
        if mode is None and k % 53 == 52:
            idx, pos = draw()
            ora.reset(None, idx, pos, None)
            model.reset()
            for e, env in enumerate(envs):
                env.reset(int(idx[e]), int(pos[e]))
            continue
        a = rng.integers(-1, len(positions), E).astype(np.int32)
        ora.step(a)
        model.step()
        for e, env in enumerate(envs):
            if pending[e]:
                env.reset(int(queue[0][e, used[e]]), int(queue[1][e, used[e]]))
                used[e] += 1
                pending[e] = False
            elif mode is None and env.ended and env.idx >= T - 1:
                continue  # frozen: the reference would raise, the batch holds still
            else:
                env.step(int(a[e]))
                if env.ended:
                    ends += 1
                    if mode == "next_step":
                        pending[e] = True
                    elif mode == "same_step":
                        finished = [dict(r) for r in env.log]
                        _same_rows(model.episode(e, finished=True), finished, positions,
                                   f"seed {seed} call {k} env {e} finished")
                        env.reset(int(queue[0][e, used[e]]), int(queue[1][e, used[e]]))
                        used[e] += 1
    _ENDS[(seed, mode)] = (ends, masked)


_ENDS = {}


def test_model_cases_reach_episode_ends_and_masked_resets():
    """Runs after the parametrised cases: most of them ended episodes, every disabled one reset masks."""
    assert len(_ENDS) == 36
    assert sum(1 for v in _ENDS.values() if v[0] > 0) >= 24, _ENDS
    assert all(v[1] > 0 for (s, m), v in _ENDS.items() if m is None), _ENDS


def test_frozen_env_keeps_its_episode(oracle_mod):
    """Auto-reset disabled, "max" duration: the env on the shorter dataset ends on its last row and
    is frozen while the other goes on.  Its History is the finished episode (the model keeps it
    whole; the log keeps the rows the frozen copies have not pushed out) and its log slots are
    copies of its last state with reward 0."""
    rng = np.random.default_rng(4)
    Ts = (30, 110)
    sets = []
    for T in Ts:
        close = 100.0 * np.exp(np.cumsum(rng.normal(0, 4e-3, T)))
        full = np.zeros((T, 4), np.float32)
        full[:, :2] = rng.normal(0, 1, (T, 2))
        sets.append((full, close))
    positions = [-1, 0, 1]
    cfg = make_config(n_envs=2, n_static=2, n_datasets=2, positions=positions, windows=3,
                      trading_fees=1e-3, borrow_interest_rate=1e-4, autoreset=None, dyn_persist=True,
                      max_episode_duration="max", seed=1)
    ora = oracle_mod.OracleEnv(cfg, sets)
    L = 48
    model = LogModel(ora, L, None, Ts)
    ora.reset(None, np.array([2, 2], np.int32), np.array([1, 1], np.int32), np.array([0, 1], np.int32))
    model.reset()
    envs = [PyEnv(sets[d][0].copy(), sets[d][1], positions, windows=3, trading_fees=1e-3,
                  borrow_interest_rate=1e-4, max_episode_duration="max") for d in (0, 1)]
    for env in envs:
        env.reset(2, 1)
    gone = 0
    for k in range(100):
        a = rng.integers(-1, 3, 2).astype(np.int32)
        ora.step(a)
        model.step()
        for env, ae in zip(envs, a):
            if not env.ended:
                env.step(int(ae))
        oldest = max(0, k + 2 - L)  # row j of both episodes was appended as row number j
        for e in (0, 1):
            log = envs[e].log
            _same_rows(model.episode(e), log, positions, f"call {k} env {e}")
            n_vis = sum(1 for j in range(len(log)) if j >= oldest)
            got = model.logged(e)
            if n_vis:
                _same_rows(got, log[-n_vis:], positions, f"logged {k} {e}")
            else:  # the frozen copies filled the log: one is left
                assert e == 0 and len(got) == 1 and got[0]["reward"] == 0.0 and got[0]["step"] == 27
                gone += 1
        assert model.frozen[0] == (k >= 26) and not model.frozen[1]
    assert envs[0].step_no == 27 and envs[1].step_no == 100 and gone > 0
    # the frozen copies: the newest slot of env 0 repeats its last state with reward 0, flags raised
    newest = (model.count - 1) % L
    assert model.ring["step"][newest, 0] == 27 and model.ring["reward"][newest, 0] == 0.0
    assert model.ring["idx"][newest, 0] == 29 and model.ring["flags"][newest, 0] & 2
    mask = model.episode_mask()
    assert mask[:, 0].sum() == 1 and mask[0, 0] and mask[:, 1].all()
