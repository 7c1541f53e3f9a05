"""The device trajectory log against an independent model of it (tests/log_model.py: the C oracle's
state, logged the way the reference's History logs it), not against a twin that runs the same
kernels.  After every step: the raw log (all L physical rows, every env, every column), the
packed episodes of `read_log_envs`, the `History` objects of `histories`, `episode_mask()` and
the newest two rows of `batched_history()`, and an `add_metric` function.  Then the reward kinds
the golden traces reach only for one env (`scaled_log_return`, `clipped_log_return`) on every
step path against the oracle.  Needs an MI355X."""
import numpy as np
import pytest

from gym_trading_env_amd import _abi
from log_model import COLUMNS, LogModel

pytestmark = pytest.mark.gpu

_INT = ("idx", "step", "position_index", "dataset_index", "flags")
_F64 = ("portfolio_valuation", "real_position", "asset", "fiat", "interest_asset", "interest_fiat")
_HIST = {"idx": "idx", "step": "step", "position_index": "position_index",
         "real_position": "real_position", "portfolio_valuation": "portfolio_valuation",
         "reward": "reward", "portfolio_distribution_interest_asset": "interest_asset",
         "portfolio_distribution_interest_fiat": "interest_fiat"}


def _walk(seed, T, Fs, sigma=1e-2, drift=0.0):
    rng = np.random.default_rng(seed)
    close = 100.0 * np.exp(np.cumsum(rng.normal(drift, sigma, T)))
    return rng.normal(0, 1, (T, Fs)).astype(np.float32), close


def _same(got, want, name, tag):
    if name in _INT:
        np.testing.assert_array_equal(got, want, err_msg=f"{tag} {name}")
    elif name == "reward":
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15, err_msg=f"{tag} {name}")
    else:
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=f"{tag} {name}")


def _column(h, col, name):
    """a History column as a typed array (History keeps some columns as Python objects)"""
    return np.asarray(h[col]).astype(COLUMNS[name])


def _metric(h):
    return len(h), float(np.sum(np.asarray(h["reward"], dtype=np.float64)))


class _Run:
    """A logged BatchedTradingEnv, the oracle and the log model driven with the same actions (the
    episode draws are Philox on both sides, keyed by the same seed)."""

    def __init__(self, oracle_mod, datasets, N, L, seed, **kw):
        from gym_trading_env_amd.batched import BatchedTradingEnv
        self.env = BatchedTradingEnv(datasets if len(datasets) > 1 else datasets[0], num_envs=N,
                                     log_steps=L, seed=seed, output="torch", verbose=0, **kw)
        self.env.add_metric("rows and reward", _metric)
        staged = []
        for ds in datasets:
            full = np.zeros((ds[0].shape[0], ds[0].shape[1] + self.env.cfg.n_dyn), np.float32)
            full[:, :ds[0].shape[1]] = ds[0]
            staged.append((full,) + tuple(ds[1:]))
        self.datasets = datasets
        self.ora = oracle_mod.OracleEnv(self.env.cfg, staged)
        self.model = LogModel(self.ora, L, kw.get("autoreset", "next_step"), [len(d[1]) for d in datasets])
        self.N, self.L = N, L
        self.rng = np.random.default_rng(seed + 100)
        self.masked = np.zeros(N, bool)
        self.checked_finished = 0

    def reset(self, mask=None):
        m = None if mask is None else np.asarray(mask, np.uint8)
        self.env.reset(mask=m)
        self.ora.reset(m)
        self.model.reset(m)
        self.masked = np.ones(self.N, bool) if m is None else m.astype(bool)

    def actions(self):
        return self.rng.integers(-1, len(self.env.positions), self.N).astype(np.int32)

    def step(self, a=None):
        import torch
        a = self.actions() if a is None else a
        self.env.step(torch.from_numpy(a).cuda())
        self.oracle_step(a)
        return a

    def oracle_step(self, a):
        self.ora.step(a, threads=8)
        self.model.step()
        self.masked[:] = False

    def ids(self):
        ended = np.flatnonzero(self.model.just_ended)
        picks = [[0, self.N - 1], ended[:24], np.flatnonzero(self.masked)[:24],
                 np.flatnonzero(~self.masked)[:12], self.rng.integers(0, self.N, 12)]
        return np.unique(np.concatenate(picks).astype(np.int64))

    def check(self, tag):
        import torch
        env, model = self.env, self.model
        torch.cuda.synchronize()
        assert int(env._log_view().rows) == model.count, tag
        # the raw log, every physical row
        for name in model.ring:
            _same(env._log_tensor(name).cpu().numpy(), model.ring[name], name, f"{tag} raw")
        ids = self.ids()
        # the packed episodes
        b = env.read_log_envs(ids)
        b = {k: v.copy() for k, v in b.items()}
        for j, e in enumerate(ids):
            want = model.logged(int(e))
            n = int(b["n_rows"][j])
            assert n == len(want), (tag, int(e), n, len(want))
            for name in model.ring:
                _same(b[name][j, :n], np.array([r[name] for r in want]), name, f"{tag} env {e} packed")
        # the History objects
        for e, h in zip(ids, env.histories(ids)):
            want = model.logged(int(e))
            assert len(h) == len(want), (tag, int(e))
            for col, name in _HIST.items():
                _same(_column(h, col, name), np.array([r[name] for r in want]), name, f"{tag} env {e} History {col}")
        # a custom metric over each History
        got = env.episode_metrics(ids)["rows and reward"]
        for (n, s), e in zip(got, ids):
            rows = model.logged(int(e))
            assert n == len(rows), (tag, int(e))
            np.testing.assert_allclose(s, np.sum(np.array([r["reward"] for r in rows], np.float64)),
                                       rtol=1e-12, atol=1e-15 * len(rows), err_msg=f"{tag} env {e} metric")
        # the BatchedHistory a reward / feature callable sees
        h = env.batched_history()
        host = lambda x: x.numpy() if hasattr(x, "numpy") else np.asarray(x)
        np.testing.assert_array_equal(host(h.episode_mask()), model.episode_mask(), err_msg=f"{tag} mask")
        phys = model.window_rows()
        for t in (-1, -2)[:len(phys)]:
            for name in ("idx", "step", "position_index", "portfolio_valuation", "reward", "real_position"):
                _same(host(h[name, t]), model.ring[name][phys[t]], name, f"{tag} h[{name}, {t}]")
        # same-step mode: the episodes that just ended
        if env.cfg.final_obs and model.just_ended.any():
            fin = np.flatnonzero(model.just_ended)[:32]
            b = {k: v.copy() for k, v in env.read_log_envs(fin, finished=True).items()}
            for j, e in enumerate(fin):
                want = model.logged(int(e), finished=True)
                n = int(b["n_rows"][j])
                assert n == len(want), (tag, int(e))
                for name in model.ring:
                    _same(b[name][j, :n], np.array([r[name] for r in want]), name, f"{tag} env {e} finished")
            for e, h in zip(fin[:8], env.histories(fin[:8], finished=True)):
                want = model.logged(int(e), finished=True)
                assert len(h) == len(want)
                for col, name in _HIST.items():
                    _same(_column(h, col, name), np.array([r[name] for r in want]), name, f"{tag} finished {e} {col}")
            self.checked_finished += len(fin)

    def close(self):
        self.env.close()
        self.ora.close()


def _next_step_case(oracle_mod, kernel_variant):
    feat, close = _walk(11, 300, 6, sigma=2e-2)
    r = _Run(oracle_mod, [(feat, close)], N=1001, L=7, seed=3, positions=[-1, 0, 1, 2], windows=5,
             trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration=9,
             autoreset="next_step", kernel_variant=kernel_variant)
    r.reset()
    r.check("reset")
    for k in range(24):  # the 7-row ring wraps three times
        r.step()
        r.check(f"step {k}")
    assert r.model.count > 3 * r.L
    r.close()


def test_next_step_log_equals_model(oracle_mod):
    """The log row written by the step kernel itself (F_obs = 8: 16-byte path), 1001 envs: a ragged
    last wave.  L = 7: the ring wraps."""
    _next_step_case(oracle_mod, 0)


def test_next_step_separate_log_launch_equals_model(oracle_mod):
    """kernel_variant KV_LOG_SEPARATE: the row comes from the separate gte_log_kernel launch."""
    _next_step_case(oracle_mod, _abi.KV_LOG_SEPARATE)


def test_same_step_log_equals_model(oracle_mod):
    """Same-step auto-reset with final_obs (F_obs = 7: 4-byte path): the reset rows (reward 0, the
    terminal step's flags) and `history(finished=True)` with the terminal row."""
    feat, close = _walk(12, 300, 5, sigma=2e-2)
    r = _Run(oracle_mod, [(feat, close)], N=777, L=16, seed=4, positions=[-1, 0, 1], windows=4,
             trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration=11,
             autoreset="same_step", final_obs=True)
    r.reset()
    for k in range(30):
        r.step()
        r.check(f"step {k}")
    assert r.checked_finished > 60
    r.close()


def test_disabled_masked_resets_and_frozen_envs_equal_model(oracle_mod):
    """The multi-dataset backtest: no auto-reset, "max" duration, datasets of 120 and 200 rows.
    Every 9 steps a masked reset restarts a random subset (the envs outside the mask keep their
    episode), and the envs that end on their last row are frozen until reset (they keep their
    finished episode)."""
    sets = [_walk(13, 120, 6, sigma=5e-3), _walk(14, 200, 6, sigma=5e-3)]
    N = 600
    r = _Run(oracle_mod, sets, N=N, L=64, seed=5, positions=[-1, 0, 1], windows=3,
             trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration="max", autoreset=None)
    r.reset()
    r.check("reset")
    frozen_seen = masked = 0
    for k in range(230):
        if k % 9 == 8:
            m = r.rng.random(N) < 0.1
            masked += int(m.sum())
            r.reset(m)
            r.check(f"masked reset {k}")
        r.step()
        frozen_seen = max(frozen_seen, int(r.model.frozen.sum()))
        r.check(f"step {k}")
    assert masked > 1000 and frozen_seen > 50
    r.close()


def test_episode_rows_of_frozen_envs_equal_model(oracle_mod):
    """h[col, t >= 0] (row t of every env's current episode) while the envs on the shorter dataset
    are frozen: their copies at the end of the log are skipped, so row t is the episode's own.
    Every env starts at the same row and the log holds the whole run, so every t up to the
    smallest episode's last row is valid for all envs.  Both the torch and the numpy views."""
    from gym_trading_env_amd.batched import BatchedTradingEnv
    sets = [_walk(19, 60, 6, sigma=5e-3), _walk(20, 120, 6, sigma=5e-3)]
    N, L = 300, 256
    kw = dict(positions=[-1, 0, 1], windows=3, trading_fees=1e-3, borrow_interest_rate=1e-4,
              max_episode_duration="max", autoreset=None)
    r = _Run(oracle_mod, sets, N=N, L=L, seed=8, **kw)
    host_env = BatchedTradingEnv(sets, num_envs=N, log_steps=L, seed=8, output="numpy", verbose=0, **kw)
    r.reset()
    host_env.reset()
    frozen_checked = 0
    for k in range(125):
        a = r.step()
        host_env.step(a)
        r.check(f"step {k}")
        steps = r.ora.state()["step"]
        ts = sorted({0, int(steps.min()) // 2, int(steps.min())})
        for env in (r.env, host_env):
            h = env.batched_history()
            host = lambda x: x.numpy() if hasattr(x, "numpy") else np.asarray(x)
            np.testing.assert_array_equal(host(h.episode_mask()), r.model.episode_mask(), err_msg=f"step {k}")
            for t in ts:
                for name in ("idx", "step", "portfolio_valuation", "reward"):
                    want = np.array([r.model.episode(e)[t][name] for e in range(N)])
                    _same(host(h[name, t]), want, name, f"step {k} {env.output} h[{name}, {t}]")
        frozen_checked += int(r.model.frozen.sum())
    assert r.model.frozen.any() and frozen_checked > 1000
    host_env.close()
    r.close()


def test_resorted_order_and_lds_rows_equal_model(oracle_mod):
    """8192 envs, C3-like windows (20 x 32), processing order re-sorted every step: the rows are
    staged through LDS and written in the re-sorted order.  L = 4."""
    feat, close = _walk(15, 900, 30, sigma=1e-2)
    r = _Run(oracle_mod, [(feat, close)], N=8192, L=4, seed=6, positions=[-1, 0, 1], windows=20,
             trading_fees=1e-4, borrow_interest_rate=3e-6, max_episode_duration=10,
             autoreset="next_step", affinity_period=1)
    r.reset()
    for k in range(14):
        r.step()
        r.check(f"step {k}")
    r.close()


def test_datasets_and_limit_orders_equal_model(oracle_mod):
    """Three datasets with high/low, persistent and one-shot limit orders, a dataset switch at
    every episode: the dataset and position columns."""
    sets = []
    for d in range(3):
        f, c = _walk(400 + d, 220 + 10 * d, 5, sigma=1e-2)
        g = np.random.default_rng(500 + d)
        sets.append((f, c, c * (1 + np.abs(g.normal(0, 8e-3, len(c)))), c * (1 - np.abs(g.normal(0, 8e-3, len(c))))))
    N = 900
    r = _Run(oracle_mod, sets, N=N, L=12, seed=21, positions=[-1, -0.5, 0, 1, 2], windows=3,
             trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration=8, autoreset="next_step")
    r.reset()
    P = len(r.env.positions)
    for k in range(30):
        pi = np.where(r.rng.random(N) < 0.2, r.rng.integers(0, P, N), -1).astype(np.int32)
        st = r.ora.state()
        px = np.array([sets[d][1][i] for d, i in zip(st["dataset_index"], st["idx"])])
        lim = px * (1 + r.rng.normal(0, 0.01, N))
        per = (r.rng.random(N) < 0.5).astype(np.uint8)
        r.env.add_limit_order(pi, lim, per)
        r.ora.add_limit_orders(pi, lim, per)
        r.step()
        r.check(f"step {k}")
    assert len(np.unique(r.model.ring["dataset_index"])) == 3
    r.close()


def test_rollout_on_a_logged_env_equals_model(oracle_mod):
    """rollout(K = 13) of a logged env runs every step through the per-launch path; single steps
    go on from where it left the log."""
    import torch
    feat, close = _walk(16, 400, 6, sigma=2e-2)
    r = _Run(oracle_mod, [(feat, close)], N=1500, L=9, seed=7, positions=[-1, 0, 1], windows=6,
             trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration=7, autoreset="next_step")
    r.reset()
    r.step()
    for rep in range(2):
        acts = np.stack([r.actions() for _ in range(13)])
        out = r.env.rollout(torch.from_numpy(acts).cuda(), reward64=True)
        for k in range(13):
            r.oracle_step(acts[k])
            np.testing.assert_allclose(out["reward64"][k].cpu().numpy(), r.ora.reward64, rtol=1e-12, atol=1e-15)
        r.check(f"rollout {rep}")
        for k in range(3):
            r.step()
            r.check(f"rollout {rep} step {k}")
    r.close()


def test_captured_steps_on_a_logged_env_equal_model(oracle_mod):
    """capture_steps with a log: the actions come from a device buffer the test refills before each
    of three replays, so every replay appends its rows from the device cursor; the model, not an
    eager twin, says what they are."""
    import torch
    feat, close = _walk(17, 600, 6, sigma=3e-2, drift=-1e-3)
    N, L, K = 3000, 5, 6
    r = _Run(oracle_mod, [(feat, close)], N=N, L=L, seed=17, positions=[-1, 0, 1], windows=8,
             trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration=13, autoreset="next_step")
    r.reset()
    for k in range(L):  # a full log
        r.step()
    r.check("before capture")
    buf = torch.zeros((K, N), dtype=torch.int32, device="cuda")
    g = r.env.capture_steps(lambda i: r.env.step(buf[i]), K)
    r.check("after capture")  # the capture ran nothing
    for rep in range(3):
        acts = np.stack([r.actions() for _ in range(K)])
        buf.copy_(torch.from_numpy(acts))
        g.replay()
        for k in range(K):
            r.oracle_step(acts[k])
        r.check(f"replay {rep}")
    r.close()


# ---------------------------------------------------------------------------------------------
# reward kinds on every step path

_SPECS = [("scaled_log_return", 3.7), ("clipped_log_return", 50.0, -0.02, 0.015)]
# step: the isolated hot instantiation; variant64: the shared-TU one; variant1: per-wave phase A;
# the three fused rollout kernels: window-resident (keep_obs), gather-per-step (keep_obs with
# kernel_variant KV_ROLLOUT_GATHER, which turns residency off) and state-only (no keep_obs); logged: the step
# kernel that writes the log row, whose reward column is checked too
_PATHS = ["step", "variant64", "variant1", "rollout_resident", "rollout_gather", "rollout_state", "logged"]
_KERNEL_VARIANT = {"variant64": _abi.KV_SHARED_TU, "variant1": _abi.KV_PER_WAVE_PHASE_A,
                   "rollout_gather": _abi.KV_ROLLOUT_GATHER}


@pytest.mark.parametrize("path", _PATHS)
@pytest.mark.parametrize("spec", _SPECS, ids=lambda s: s[0])
def test_reward_kinds_equal_oracle(oracle_mod, spec, path, monkeypatch, capfd):
    import torch
    from gym_trading_env_amd.batched import BatchedTradingEnv
    feat, close = _walk(18, 500, 6, sigma=1.5e-2)
    N, steps = 2000, 24
    kv = _KERNEL_VARIANT.get(path, 0)
    L = 8 if path == "logged" else 0
    # the resident rollout's geometry search reports every geometry that fits (gte_api.hip,
    # choose_resident_epb): some line <=> the window-resident kernel runs
    monkeypatch.setenv("GTE_DEBUG_GEOMETRY", "1")
    env = BatchedTradingEnv((feat, close), num_envs=N, positions=[-1, 0, 1, 2], windows=6,
                            trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration=15,
                            reward_function=spec, autoreset="next_step", seed=9, kernel_variant=kv,
                            log_steps=L, output="torch", verbose=0)
    full = np.zeros((len(close), 8), np.float32)
    full[:, :6] = feat
    ora = oracle_mod.OracleEnv(env.cfg, [(full, close)])
    model = LogModel(ora, L, "next_step", [len(close)]) if L else None
    env.reset()
    ora.reset()
    if model:
        model.reset()
    rng = np.random.default_rng(10)
    acts = rng.integers(-1, 4, (steps, N)).astype(np.int32)
    seen = []
    if path.startswith("rollout"):
        # 16-byte rows, cooperative phase A, raw dynamic rings in LDS, no log, no final_obs: the
        # shape the fused rollout kernels take (LaunchPlan::fused_rollout), not K step launches
        info = env.launch_info()
        assert (info["vector_bytes"], info["phase_a"], info["dyn_columns"]) == (16, "cooperative", "lds-raw-rings")
        capfd.readouterr()
        out = env.rollout(torch.from_numpy(acts).cuda(), keep_obs=(path != "rollout_state"), reward64=True)
        torch.cuda.synchronize()
        resident = "[gte] resident rollout" in capfd.readouterr().err
        assert resident == (path == "rollout_resident"), path
        for k in range(steps):
            ora.step(acts[k], threads=8)
            np.testing.assert_allclose(out["reward64"][k].cpu().numpy(), ora.reward64, rtol=1e-12, atol=1e-15,
                                       err_msg=f"step {k}")
            np.testing.assert_allclose(out["reward"][k].cpu().numpy(), ora.reward, rtol=1e-6, atol=1e-12)
            seen.append(ora.reward64.copy())
        np.testing.assert_allclose(env.state("portfolio_valuation"), ora.state()["portfolio_valuation"],
                                   rtol=1e-12, atol=0)
    else:
        for k in range(steps):
            _, reward, _, _, _ = env.step(torch.from_numpy(acts[k]).cuda())
            ora.step(acts[k], threads=8)
            np.testing.assert_allclose(env.read_output("reward64"), ora.reward64, rtol=1e-12, atol=1e-15,
                                       err_msg=f"step {k}")
            np.testing.assert_allclose(reward.cpu().numpy(), ora.reward, rtol=1e-6, atol=1e-12)
            seen.append(ora.reward64.copy())
            if model:
                model.step()
                np.testing.assert_allclose(env._log_tensor("reward").cpu().numpy(), model.ring["reward"],
                                           rtol=1e-12, atol=1e-15, err_msg=f"log reward, step {k}")
    seen = np.concatenate(seen)
    if spec[0] == "clipped_log_return":  # both clip bounds were hit
        assert (seen == spec[2]).sum() > 10 and (seen == spec[3]).sum() > 10
    else:
        assert np.abs(seen).max() > 0.05
    env.close()
    ora.close()
