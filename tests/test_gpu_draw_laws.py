"""The device's own reset draws (no injection): equal to the oracle's bit for bit, and held to the
reference's laws (draw_laws.py) on the DEVICE's arrays, so that a wrong law cannot hide behind the
oracle running the same formula.  Then the draws of auto-resets inside step() (next-step and
same-step mode) and inside every fused rollout path, against the oracle over more than two full
rounds of dataset picks; the rollout path each call took is asserted (GTE_DEBUG_GEOMETRY).
Needs an MI355X.
"""
import re

import numpy as np
import pytest

import draw_laws as L
from gym_trading_env_amd import _abi

pytestmark = pytest.mark.gpu

N_ENVS = 65536
W = 3
MAX_DUR = 2
ROUNDS_PER_ENV = 4  # x 65 536 envs = 2^18 rounds per D
PATH_LINE = re.compile(r"\[gte\] rollout path: ([a-z-]+), (\d+) steps")


def _walks(Ts, Fs, seed):
    """(features [T, Fs], close [T]) per dataset: feature 0 names the row and the dataset, so an
    observation shows where its env is."""
    rng = np.random.default_rng(seed)
    out = []
    for d, T in enumerate(Ts):
        feat = rng.normal(0, 1, (T, Fs)).astype(np.float32)
        feat[:, 0] = np.arange(T) + 1000 * d
        out.append((feat, 100.0 * np.exp(np.cumsum(rng.normal(0, 1e-2, T)))))
    return out


def _oracle_sets(sets, nd=2):
    full = []
    for feat, close in sets:
        f = np.zeros((len(close), feat.shape[1] + nd), np.float32)
        f[:, :feat.shape[1]] = feat
        full.append((f, close))
    return full


def _spans(D):
    return [40 + 3 * d for d in range(D)]


@pytest.mark.parametrize("D", [3, 5, 17, 128])
def test_reset_draws_equal_the_oracle_and_follow_the_laws(oracle_mod, D):
    from gym_trading_env_amd.batched import BatchedTradingEnv
    spans = _spans(D)
    sets = _walks([s + MAX_DUR + 2 * (W - 1) for s in spans], 1, D)
    P = 5
    env = BatchedTradingEnv(sets, num_envs=N_ENVS, positions=[-1, -0.5, 0, 0.5, 1], windows=W,
                            max_episode_duration=MAX_DUR, seed=1000 + D, output="numpy")
    ora = oracle_mod.OracleEnv(env.cfg, _oracle_sets(sets))
    R = (ROUNDS_PER_ENV + 1) * D - 1
    got = {f: [] for f in L.FIELDS}
    for t in range(R):
        env.reset()
        ora.reset()
        dev, ref = L.read_state(env, L.FIELDS + ("idx",)), L.read_state(ora, L.FIELDS + ("idx",))
        for f in dev:
            np.testing.assert_array_equal(dev[f], ref[f], err_msg=f"D={D} reset {t}: {f}")
        for f in L.FIELDS:  # (start rows and positions of the first 64 resets are sample enough)
            if f == "dataset_index" or t < 64:
                got[f].append(dev[f])
    env.close()
    ora.close()
    got = {f: np.stack(a) for f, a in got.items()}

    # the laws, on the device's own arrays
    rounds = L.full_rounds(L.picks_from_resets(got["dataset_index"], 1, D), D)
    assert rounds.shape == (N_ENVS, ROUNDS_PER_ENV, D)
    L.assert_rounds_are_permutations(rounds, D, f"D={D}")
    ps = {f"round {k}": p for k, p in L.round_laws(rounds, D).items()}
    s, pos = got["start_idx"], got["position_index"]
    ds = got["dataset_index"][:len(s)]
    for d, span in enumerate(spans):
        for k, p in L.uniform_range_p(s[ds == d], W - 1, W - 1 + span).items():
            ps[f"start of dataset {d} {k}"] = p
    ps["position"] = L.uniform_p(pos, P)
    # start row against position, env 2i against env 2i+1 (one wave), episode t against t+1
    c = (s - (W - 1)) * 8 // (np.array(spans)[ds])
    ps["start x position"] = L.independence_p(c, pos, 8, P)
    ps["position env 2i x 2i+1"] = L.independence_p(pos[:, 0::2], pos[:, 1::2], P, P)
    ps["start env 2i x 2i+1"] = L.independence_p(c[:, 0::2], c[:, 1::2], 8, 8)
    f0, kf = L.coarse(rounds[:, :, 0], D, 16)
    ps["first pick env 2i x 2i+1"] = L.independence_p(f0[0::2], f0[1::2], kf, kf)
    ps["position episode t x t+1"] = L.independence_p(pos[0:-1:2], pos[1::2], P, P)
    assert not L.rejects(ps), f"D={D}: {L.failing(ps)}"


# ---------------------------------------------------------------------------------------------
# auto-resets inside step() and the fused rollouts

D_AUTO = 5
N_AUTO = 4096
STEPS = 64  # episodes of at most 3 steps: > 2 full rounds of D_AUTO picks per env


def _auto_env(oracle_mod, autoreset, **kw):
    from gym_trading_env_amd.batched import BatchedTradingEnv
    sets = _walks([60 + 10 * d for d in range(D_AUTO)], 2, 77)
    # F_obs = 4 and a window of 4 rows: the shape the fused rollout kernels are written for
    env = BatchedTradingEnv(sets, num_envs=N_AUTO, positions=[-1, 0, 1], windows=4,
                            max_episode_duration=3, autoreset=autoreset, seed=5, output="torch",
                            envs_per_wave=4, **kw)
    return env, oracle_mod.OracleEnv(env.cfg, _oracle_sets(sets))


STATE = ("idx", "step") + L.FIELDS


def _assert_state(env, ora, tag):
    dev, ref = L.read_state(env, STATE), L.read_state(ora, STATE)
    for f in STATE:
        np.testing.assert_array_equal(dev[f], ref[f], err_msg=f"{tag}: {f}")


def _assert_rounds(env):
    """Every env went through more than two full rounds of dataset picks."""
    assert env.state("episode").min() >= 2 * D_AUTO + 1


@pytest.mark.parametrize("autoreset", ["next_step", "same_step"])
def test_step_autoreset_draws_equal_the_oracle(oracle_mod, autoreset):
    env, ora = _auto_env(oracle_mod, autoreset)
    rng = np.random.default_rng(1)
    env.reset()
    ora.reset()
    for k in range(STEPS):
        a = rng.integers(-1, 3, N_AUTO).astype(np.int32)
        obs, _, term, trunc, _ = env.step(a)
        ora.step(a)
        tag = f"{autoreset} step {k}"
        np.testing.assert_array_equal(obs.cpu().numpy(), ora.obs, err_msg=tag + " obs")
        np.testing.assert_array_equal(term.cpu().numpy(), ora.terminated.astype(bool), err_msg=tag)
        np.testing.assert_array_equal(trunc.cpu().numpy(), ora.truncated.astype(bool), err_msg=tag)
        _assert_state(env, ora, tag)
    _assert_rounds(env)
    env.close()
    ora.close()


ROLLOUTS = {"resident": (0, True), "gather": (_abi.KV_ROLLOUT_GATHER, True), "state-only": (0, False)}


@pytest.mark.parametrize("autoreset", ["next_step", "same_step"])
@pytest.mark.parametrize("path", sorted(ROLLOUTS))
def test_rollout_autoreset_draws_equal_the_oracle(oracle_mod, path, autoreset, monkeypatch, capfd):
    """The first check of non-injected draws inside the rollout kernels: chunks of two steps
    (one reset at most per env and chunk, so every draw shows in the state after its chunk), per
    step flags, valuations and (where kept) observations against the oracle."""
    import torch
    kv, keep = ROLLOUTS[path]
    monkeypatch.setenv("GTE_DEBUG_GEOMETRY", "1")
    env, ora = _auto_env(oracle_mod, autoreset, kernel_variant=kv)
    rng = np.random.default_rng(2)
    env.reset()
    ora.reset()
    capfd.readouterr()
    K = 2
    for start in range(0, STEPS, K):
        acts = rng.integers(-1, 3, (K, N_AUTO)).astype(np.int32)
        out = env.rollout(torch.from_numpy(acts).cuda(), keep_obs=keep, valuation=True)
        torch.cuda.synchronize()
        paths = PATH_LINE.findall(capfd.readouterr().err)
        assert paths == [(path, str(K))], paths
        for j in range(K):
            ora.step(acts[j])
            tag = f"{path} {autoreset} step {start + j}"
            np.testing.assert_array_equal(out["terminated"][j].cpu().numpy(), ora.terminated.astype(bool),
                                          err_msg=tag)
            np.testing.assert_array_equal(out["truncated"][j].cpu().numpy(), ora.truncated.astype(bool),
                                          err_msg=tag)
            np.testing.assert_array_equal(out["valuation"][j].cpu().numpy(),
                                          ora.state()["portfolio_valuation"], err_msg=tag + " valuation")
            if keep:
                np.testing.assert_array_equal(out["obs"][j].cpu().numpy(), ora.obs, err_msg=tag + " obs")
        if not keep:
            np.testing.assert_array_equal(out["obs"].cpu().numpy(), ora.obs, err_msg=f"{path} obs")
        _assert_state(env, ora, f"{path} {autoreset} after step {start + K - 1}")
    _assert_rounds(env)
    env.close()
    ora.close()
