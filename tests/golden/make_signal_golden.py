#!/usr/bin/env python3
"""Generate tests/golden/signal_trace.npz and signal_trace_multi.npz by running the REFERENCE
closed-loop on signal tables (see make_golden.py for where this runs and what is committed).

Every env object of the reference is driven with the rule of include/gte.h (gte_bind_signals):

    a = signals[dataset][strategy[e]][env._idx]
    env.step(a if 0 <= a < len(positions) else None)

and reset when its episode ended (the next-step convention of the trace format).  The traces are
in make_golden.py's format — actions, the reference's draws at every reset, per-call rows — plus
    signals_<d> i8 [S, T_d]   the table of dataset d
    strategy    i32 [E]       the strategy each env follows
so they replay like any other trace, and the recorded actions can be checked against the lookup
model of tests/signal_model.py.
"""
from __future__ import annotations

import glob
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the gymnasium stand-in, imports the reference)

OUT_OF_RANGE = (-1, -128, 127, 3)  # with three positions: all of them mean hold
KIB_PER_FIXTURE = 200


def make_table(rng, S, T, P):
    """Runs of one position index (a strategy holds for a while), with out-of-range entries
    sprinkled in: every value of OUT_OF_RANGE occurs in every row."""
    t = np.empty((S, T), np.int8)
    for s in range(S):
        row, pos = [], int(rng.integers(0, P))
        while len(row) < T:
            row += [pos] * int(rng.integers(1, 7))
            pos = int(rng.integers(0, P))
        t[s] = row[:T]
        where = rng.choice(T, size=T // 8, replace=False)
        t[s, where] = np.resize(np.array(OUT_OF_RANGE, np.int8), len(where))
    assert all((t == v).any(axis=1).all() for v in OUT_OF_RANGE)
    return t


def run_signal_trace(make_env, positions, tables, strategy, n_calls, ds_names=None, seed_base=1000,
                     fresh_env_each_episode=False):
    """make_golden.run_trace with the action of every step taken from the tables, on the row (and
    dataset) the env stands on before the step.  fresh_env_each_episode: a new reference object per
    episode, so that no window holds dynamic-feature values an earlier episode wrote into the
    object's table (environments.py:153-154; make_golden's c3_window20 does the same)."""
    n_envs, P = len(strategy), len(positions)
    rec = {f: np.zeros((n_calls, n_envs), np.float64) for f in mg.FIELDS_F64}
    rec.update({f: np.zeros((n_calls, n_envs), np.int32) for f in mg.FIELDS_I32})
    rec["op"] = np.ones((n_calls, n_envs), np.uint8)
    rec["action"] = np.zeros((n_calls, n_envs), np.int32)
    rec["done"] = np.zeros((n_calls, n_envs), np.uint8)
    rec["truncated"] = np.zeros((n_calls, n_envs), np.uint8)
    obs_rec = None
    for e in range(n_envs):
        env = make_env(e)
        ended, episode = True, 0
        for k in range(n_calls):
            if k == 0 or ended:
                if fresh_env_each_episode and k > 0:
                    env = make_env(e)
                np.random.seed(seed_base + 7919 * e + episode)  # (the reference draws from the global RNG)
                obs, info = env.reset()
                episode += 1
                rec["op"][k, e] = 0
                rec["action"][k, e] = -1
                reward, done, trunc = 0.0, False, False
            else:
                d = ds_names.index(len(env.df)) if ds_names else 0
                a = int(tables[d][strategy[e]][env._idx])
                a = a if 0 <= a < P else None
                rec["action"][k, e] = -1 if a is None else a
                obs, reward, done, trunc, info = env.step(a)
            ended = bool(done or trunc)
            mg.snapshot(env, rec, k, e, positions, ds_names)
            rec["reward"][k, e] = float(reward)
            rec["done"][k, e] = done
            rec["truncated"][k, e] = trunc
            obs = np.array(obs, dtype=np.float32)
            if obs_rec is None:
                obs_rec = np.zeros((n_calls, n_envs) + obs.shape, np.float32)
            obs_rec[k, e] = obs
    rec["obs"] = obs_rec
    rec["seed_base"] = np.array(seed_base)
    rec["fresh_env_each_episode"] = np.array(int(fresh_env_each_episode))
    for d, t in enumerate(tables):
        rec[f"signals_{d}"] = t
    rec["strategy"] = np.asarray(strategy, np.int32)
    return rec


def _save(name, cfg, sets, rec, note):
    mg.save(name, cfg, sets, rec, note)
    kib = os.path.getsize(os.path.join(HERE, name + ".npz")) / 1024
    assert kib <= KIB_PER_FIXTURE, f"{name}: {kib:.0f} KiB"
    episodes = (rec["op"] == 0).sum(axis=0)
    assert (episodes >= 3).all(), f"{name}: an env saw only {episodes.min()} episodes"
    out = [int(((rec["action"] == -1) & (rec["op"] == 1)).sum()), int((rec["op"] == 1).sum())]
    print(f"{name}: episodes per env {episodes.tolist()}, {out[0]} of {out[1]} steps hold")


def main():
    rng = np.random.default_rng(20261018)
    positions = [-1, 0, 1]
    S = 3

    # -- one dataset: 6 envs, random starts, 24-step episodes ------------------------------------
    feat, close = mg.random_walk(811, 200, 3, sigma=8e-3)
    df = mg.make_df(feat, close)
    cfg = mg.base_cfg(positions=positions, windows=5, trading_fees=1e-3, borrow_interest_rate=1e-5,
                      max_episode_duration=24)
    table = make_table(rng, S, 200, len(positions))
    strategy = [2, 0, 1, 1, 0, 2]
    rec = run_signal_trace(lambda e: mg.TradingEnv(df=df, **mg.ref_kwargs(cfg)), positions, [table],
                           strategy, n_calls=120, fresh_env_each_episode=True)
    _save("signal_trace", cfg, [(feat, close)], rec,
          "the reference driven closed-loop by a signal table: the action of every step is "
          "signals[strategy[e]][env._idx] (None outside [0, 3)), T=200, random starts, duration 24, "
          "fresh reference env per episode")

    # -- two datasets of different lengths, a table each, switch after every episode --------------
    with tempfile.TemporaryDirectory() as tmp:
        sets, names = [], []
        for d, T in enumerate((150, 210)):
            f, c = mg.random_walk(821 + d, T, 3, sigma=8e-3)
            sets.append((f, c))
            names.append(f"sym{d}.pkl")
            mg.make_df(f, c).to_pickle(os.path.join(tmp, names[-1]))
        cfg = mg.base_cfg(positions=positions, windows=4, trading_fees=1e-3, borrow_interest_rate=1e-5,
                          max_episode_duration=12, episodes_between_dataset_switch=1)
        tables = [make_table(rng, S, len(c), len(positions)) for _, c in sets]

        def mk(e):
            np.random.seed(555 + e)  # (the constructor picks its dataset from the global RNG)
            return mg.MultiDatasetTradingEnv(os.path.join(tmp, "*.pkl"), episodes_between_dataset_switch=1,
                                             **mg.ref_kwargs(cfg))
        rec = run_signal_trace(mk, positions, tables, [1, 2, 0, 1], n_calls=60,
                               ds_names=[len(c) for _, c in sets])
        rec["glob_order"] = np.array([names.index(os.path.basename(q))
                                      for q in glob.glob(os.path.join(tmp, "*.pkl"))], np.int32)
        assert len(set(rec["dataset"].ravel().tolist())) == 2, "one dataset was never visited"
        _save("signal_trace_multi", cfg, sets, rec,
              "MultiDatasetTradingEnv driven closed-loop by one signal table per dataset (T = 150 / 210), "
              "switch after every episode: the lookup follows the env's dataset")


if __name__ == "__main__":
    main()
