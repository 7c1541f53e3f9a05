#!/usr/bin/env python3
"""Generate tests/golden/exit_trace.npz and exit_trace_multi.npz by running the REFERENCE closed-loop
on signal tables WITH EXIT RULES (see make_golden.py for where this runs and what is committed).

Every env object of the reference is driven with the rule of include/gte.h (gte_bind_exit_rules) as
tests/exit_model.py states it: before every step the model is brought up to date with the env's own
valuation and position and chooses the argument of `env.step` — the rule's exit_position when a
stop-loss, trailing stop, take-profit or time exit holds, hold while the latch waits for the signal to
move, else the table's byte.  The traces are in make_signal_golden.py's format plus
    exit_rules   u8 [R, 32]   the bytes of the gte_exit_rule records
    rule_of_env  i32 [E]      the rule each env follows
    min_margin   f64          the smallest |v - threshold| / |threshold| of any comparison the model made
    exit_counts  i64 [4]      exits fired: stop, trail, target, time
A fixture is only written when min_margin > 1e-9 with NO step left out — three orders above the 1e-12
the project states for GPU valuations against the reference, so a GPU replay decides every exit as the
model did — and when every kind of exit fired at least five times; the generator tries seeds until both
hold.
"""
from __future__ import annotations

import glob
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import exit_model as xm  # noqa: E402
import make_golden as mg  # noqa: E402  (installs the gymnasium stand-in, imports the reference)
import make_signal_golden as msg  # noqa: E402

MIN_MARGIN = 1e-9
MIN_EXITS = 5


def run_exit_trace(make_env, positions, tables, strategy, rules, rule_of_env, n_calls, ds_names=None,
                   seed_base=1000, fresh_env_each_episode=False):
    """make_signal_golden.run_signal_trace with the action of every step chosen by exit_model."""
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
        model = xm.ExitModel(1, rules, P, [rule_of_env[e]])
        ended, episode = True, 0
        for k in range(n_calls):
            if k > 0:
                d = ds_names.index(len(env.df)) if ds_names else 0
                raw = np.array([int(tables[d][strategy[e]][env._idx])], np.int32)
                a = int(model.actions(raw, [episode], [env._step], [env.historical_info["portfolio_valuation", -1]],
                                      [positions.index(env._position)], [ended])[0])
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
                rec["action"][k, e] = a
                obs, reward, done, trunc, info = env.step(None if a < 0 else a)
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
    rec["exit_rules"] = np.ascontiguousarray(rules).view(np.uint8).reshape(len(rules), -1)
    rec["rule_of_env"] = np.asarray(rule_of_env, np.int32)
    return rec


def _accept(name, cfg, sets, rec):
    """The conditions of the docstring, checked on the trace as a test will read it."""
    g = dict(rec, cfg=cfg)
    actions, margin, counts, _ = xm.trace_actions(g)
    assert (actions == rec["action"]).all(), "the recorded actions are not the model's over the trace's rows"
    print(f"{name}: min margin {margin:.3e}, exits stop/trail/target/time {counts.tolist()}")
    if not (margin > MIN_MARGIN and (counts >= MIN_EXITS).all()):
        return False
    rec["min_margin"] = np.array(margin)
    rec["exit_counts"] = np.asarray(counts, np.int64)
    return True


def _save(name, cfg, sets, rec, note):
    mg.save(name, cfg, sets, rec, note)
    kib = os.path.getsize(os.path.join(HERE, name + ".npz")) / 1024
    assert kib <= msg.KIB_PER_FIXTURE, f"{name}: {kib:.0f} KiB"
    episodes = (rec["op"] == 0).sum(axis=0)
    assert (episodes >= 3).all(), f"{name}: an env saw only {episodes.min()} episodes"


# one exit alone per rule, then mixtures; exit_position 1 is the flat position of [-1, 0, 1]
RULES = xm.make_rules(stop_loss=[0.012, 0, 0, 0, 0.02, 0.015], trailing=[0, 0.01, 0, 0, 0.012, 0],
                      take_profit=[0, 0, 0.012, 0, 0.02, 0.01], max_hold=[0, 0, 0, 5, 9, 0], exit_position=1)


def main():
    positions = [-1, 0, 1]
    S = 3

    # -- one dataset: 8 envs, random starts and initial positions, 30-step episodes ----------------
    for seed in range(20261019, 20261019 + 50):
        rng = np.random.default_rng(seed)
        feat, close = mg.random_walk(seed % 1000 + 811, 200, 3, sigma=1.2e-2)
        df = mg.make_df(feat, close)
        cfg = mg.base_cfg(positions=positions, windows=5, trading_fees=1e-3, borrow_interest_rate=1e-5,
                          max_episode_duration=30)
        table = msg.make_table(rng, S, 200, len(positions))
        strategy = [2, 0, 1, 1, 0, 2, 1, 0]
        rule_of_env = [0, 1, 2, 3, 4, 5, 1, 3]
        rec = run_exit_trace(lambda e: mg.TradingEnv(df=df, **mg.ref_kwargs(cfg)), positions, [table],
                             strategy, RULES, rule_of_env, n_calls=150, fresh_env_each_episode=True)
        if _accept("exit_trace", cfg, [(feat, close)], rec):
            break
    else:
        raise SystemExit("exit_trace: no seed met the conditions")
    _save("exit_trace", cfg, [(feat, close)], rec,
          "the reference driven closed-loop by a signal table and exit rules (tests/exit_model.py): T=200, "
          f"random starts and initial positions, duration 30, fresh reference env per episode, seed {seed}")

    # -- two datasets of different lengths, a table each, switch after every episode --------------
    for seed in range(20261119, 20261119 + 50):
        rng = np.random.default_rng(seed)
        with tempfile.TemporaryDirectory() as tmp:
            sets, names = [], []
            for d, T in enumerate((150, 210)):
                f, c = mg.random_walk(seed % 1000 + 821 + d, T, 3, sigma=1.2e-2)
                sets.append((f, c))
                names.append(f"sym{d}.pkl")
                mg.make_df(f, c).to_pickle(os.path.join(tmp, names[-1]))
            cfg = mg.base_cfg(positions=positions, windows=4, trading_fees=1e-3, borrow_interest_rate=1e-5,
                              max_episode_duration=20, episodes_between_dataset_switch=1)
            tables = [msg.make_table(rng, S, len(c), len(positions)) for _, c in sets]

            def mk(e):
                np.random.seed(555 + e)  # (the constructor picks its dataset from the global RNG)
                return mg.MultiDatasetTradingEnv(os.path.join(tmp, "*.pkl"), episodes_between_dataset_switch=1,
                                                 **mg.ref_kwargs(cfg))
            rec = run_exit_trace(mk, positions, tables, [1, 2, 0, 1, 0, 2], RULES, [5, 4, 3, 2, 1, 0], n_calls=100,
                                 ds_names=[len(c) for _, c in sets])
            rec["glob_order"] = np.array([names.index(os.path.basename(q))
                                          for q in glob.glob(os.path.join(tmp, "*.pkl"))], np.int32)
        if len(set(rec["dataset"].ravel().tolist())) == 2 and _accept("exit_trace_multi", cfg, sets, rec):
            break
    else:
        raise SystemExit("exit_trace_multi: no seed met the conditions")
    _save("exit_trace_multi", cfg, sets, rec,
          "MultiDatasetTradingEnv driven closed-loop by one signal table per dataset (T = 150 / 210) and exit "
          f"rules (tests/exit_model.py), switch after every episode, seed {seed}")


if __name__ == "__main__":
    main()
