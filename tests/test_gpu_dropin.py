"""The single-environment drop-ins (`TradingEnv`, `MultiDatasetTradingEnv`) against the
golden traces, through the reference's own API: no injection — each reset draws from
NumPy's global RNG exactly like the reference, after the same np.random.seed()."""
import os

import numpy as np
import pandas as pd
import pytest

import replay

pytestmark = pytest.mark.gpu


def make_df(feat, close, high=None, low=None):
    T = len(close)
    df = pd.DataFrame({"open": close, "high": close * 1.001 if high is None else high,
                       "low": close * 0.999 if low is None else low,
                       "close": close, "volume": np.ones(T)},
                      index=pd.date_range("2020-01-01", periods=T, freq="h"))
    for j in range(feat.shape[1]):
        df[f"feature_{j}"] = feat[:, j]
    return df


def _kwargs(g):
    from gym_trading_env_amd import envs
    cfg = g["cfg"]
    kw = {k: cfg[k] for k in ("positions", "windows", "trading_fees", "borrow_interest_rate",
                              "portfolio_initial_value", "initial_position", "max_episode_duration")}
    kw["verbose"] = 0
    rf = cfg.get("reward_function", "basic_reward_function")
    if isinstance(rf, list) and rf[0] == "scaled_log_return":
        # a CUSTOM python reward over the History, evaluated on the host by the drop-in
        k = rf[1]
        kw["reward_function"] = lambda h: k * np.log(h["portfolio_valuation", -1] / h["portfolio_valuation", -2])
    elif isinstance(rf, list) and rf[0] == "custom":
        import custom_callables
        kw["reward_function"] = custom_callables.REWARD[rf[1]]
        rf = None
    elif isinstance(rf, list):
        kw["reward_function"] = tuple(rf)
    if "dynamic_feature_functions" in cfg:
        import custom_callables
        table = {"real_position": envs.dynamic_feature_real_position,
                 "last_position_taken": envs.dynamic_feature_last_position_taken}
        table.update({"custom:" + k: v for k, v in custom_callables.DYNAMIC.items()})
        kw["dynamic_feature_functions"] = [table[n] for n in cfg["dynamic_feature_functions"]]
    return kw


def _check_call(g, k, e, env, obs, reward, done, trunc, info, P):
    tag = f"env {e} call {k}"
    assert info["idx"] == g["idx"][k, e], tag
    assert info["step"] == g["step"][k, e], tag
    assert env.positions.index(info["position"]) == g["pos_index"][k, e], tag
    assert bool(done) == bool(g["done"][k, e]) and bool(trunc) == bool(g["truncated"][k, e]), tag
    for key, gk in (("portfolio_valuation", "portfolio_valuation"), ("real_position", "real_position"),
                    ("portfolio_distribution_interest_asset", "interest_asset"),
                    ("portfolio_distribution_interest_fiat", "interest_fiat")):
        np.testing.assert_allclose(float(info[key]), g[gk][k, e], rtol=1e-12, atol=1e-14, err_msg=tag + key)
    assert info["portfolio_distribution_asset"] == max(0, g["asset"][k, e]), tag
    assert info["portfolio_distribution_borrowed_fiat"] == max(0, -g["fiat"][k, e]), tag
    np.testing.assert_allclose(float(reward), g["reward"][k, e], rtol=1e-12, atol=1e-15, err_msg=tag)
    np.testing.assert_array_equal(np.asarray(obs), g["obs"][k, e], err_msg=tag)
    assert info["data_close"] == g[f"close_ds"][int(g["dataset"][k, e])][info["idx"]], tag


def _replay_env(g, e, make_env, calls):
    seed_base = int(g["seed_base"])
    fresh = bool(int(g["fresh_env_each_episode"]))
    env = make_env(e)
    episode = 0
    P = len(g["cfg"]["positions"])
    for k in range(calls):
        if g["op"][k, e] == 0:
            if fresh and k > 0:
                env.close()
                env = make_env(e)
            np.random.seed(seed_base + 7919 * e + episode)
            episode += 1
            obs, info = env.reset()
            reward, done, trunc = 0, False, False
            assert info["reward"] == 0 and info["position_index"] == g["pos_index"][k, e]
        else:
            a = int(g["action"][k, e])
            if "lo_pos" in g and g["lo_pos"][k, e] >= 0:
                env.add_limit_order(env.positions[int(g["lo_pos"][k, e])],
                                    float(g["lo_limit"][k, e]), persistent=True)
            obs, reward, done, trunc, info = env.step(None if a < 0 else a)
            assert info["position_index"] == (None if a < 0 else a)
        _check_call(g, k, e, env, obs, reward, done, trunc, info, P)
    return env


SINGLE = ["c1_btc_default", "c1_btc_example", "c2_nowindow", "c3_window20", "drawdown_done",
          "no_autoreset", "persist_dynamic", "reward_scaled_onedyn", "reward_clipped_nodyn",
          "limit_orders",
          "hostcb_custom_callables"]  # custom Python dynamic features + reward, run by the reference
# the single-dataset traces of the reference-generated sweep and numeric family (make_golden.py
# --sweep, --numeric)
SINGLE += [n for n in replay.golden_names() if n.startswith(("sweep_", "numeric_"))
           and "feat_1" not in np.load(os.path.join(replay.GOLDEN_DIR, n + ".npz")).files]


@pytest.mark.parametrize("name", SINGLE)
def test_tradingenv_dropin_replays_reference(name):
    from gym_trading_env_amd import TradingEnv
    g = replay.load(name)
    g["close_ds"] = [ds[1] for ds in g["datasets"]]
    df = make_df(*g["datasets"][0])
    kw = _kwargs(g)
    K, E = g["op"].shape
    calls = min(K, 260)
    for e in range(min(E, 3)):
        env = _replay_env(g, e, lambda e: TradingEnv(df=df, **kw), calls)
        if name == "c1_btc_default" and e == 0:
            assert env.observation_space.shape == (7,) and env.action_space.n == 2
        env.close()


def test_tradingenv_metrics_history_and_errors(tmp_path):
    from gym_trading_env_amd import TradingEnv
    g = replay.load("c2_nowindow")
    feat, close = g["datasets"][0]
    df = make_df(feat[:40], close[:40])
    env = TradingEnv(df=df, positions=[-1, 0, 1], trading_fees=1e-4, verbose=0, name="UNIT")
    env.add_metric("Position Changes", lambda h: np.sum(np.diff(h["position"]) != 0))
    env.add_metric("Episode Lenght", lambda h: len(h["position"]))
    np.random.seed(0)
    obs, info = env.reset()
    done = trunc = False
    n = 0
    while not (done or trunc):
        obs, r, done, trunc, info = env.step(n % 3)
        n += 1
    assert n == 39 and trunc and info["idx"] == 39           # T=40: 39 steps, ends at the last row
    m = env.get_metrics()
    assert m["Episode Lenght"] == 40 and m["Market Return"].endswith("%")
    assert m["Market Return"] == f"{100 * (close[39] / close[0] - 1):5.2f}%"
    assert len(env.historical_info) == 40
    assert env.historical_info["step", -1] == 39
    with pytest.raises(IndexError):
        env.step(0)                                            # past the last row (:239)
    with pytest.raises(IndexError):
        env.reset(); env.step(7)                               # positions[7] (:234)
    env.save_for_render(dir=str(tmp_path))
    files = list(tmp_path.glob("UNIT_*.pkl"))
    assert len(files) == 1
    saved = pd.read_pickle(files[0])                           # written by our own code just now
    assert {"open", "close", "portfolio_valuation", "position", "reward"} <= set(saved.columns)
    with pytest.raises(AssertionError):
        TradingEnv(df=df, positions=[0, 1], initial_position=0.5)
    with pytest.raises(ValueError):  # a spec the device does not know, not callable
        TradingEnv(df=df, dynamic_feature_functions=["no_such_feature"])
    const = TradingEnv(df=df, dynamic_feature_functions=[lambda h: 1.0], verbose=0)  # host-side
    obs, _ = const.reset()
    assert obs[-1] == 1.0
    const.close()
    env.close()


@pytest.mark.parametrize("name,switch", [("multidataset_k1", 1), ("multidataset_k3", 3)])
def test_multidataset_dropin_replays_reference(tmp_path, monkeypatch, name, switch):
    from gym_trading_env_amd import MultiDatasetTradingEnv, envs
    g = replay.load(name)
    g["close_ds"] = [c for _, c in g["datasets"]]
    for d, (feat, close) in enumerate(g["datasets"]):
        make_df(feat, close).to_pickle(tmp_path / f"sym{d}.pkl")
    # glob order is filesystem order (environments.py:375) and decides which file the draw
    # np.random.randint(n) (:385) selects: present the files in the generator's order
    order = [str(tmp_path / f"sym{d}.pkl") for d in g["glob_order"]]
    real_glob = envs.glob.glob
    monkeypatch.setattr(envs.glob, "glob",
                        lambda pat: list(order) if pat.endswith("*.pkl") and "nothing" not in pat
                        else real_glob(pat))
    kw = _kwargs(g)
    K, E = g["op"].shape

    def mk(e):
        np.random.seed(555 + e)
        return MultiDatasetTradingEnv(str(tmp_path / "*.pkl"),
                                      episodes_between_dataset_switch=switch, **kw)
    with pytest.raises(FileNotFoundError):
        MultiDatasetTradingEnv(str(tmp_path / "nothing*.pkl"))
    for e in range(2):
        env = _replay_env(g, e, mk, min(K, 200))
        env.close()


def test_batched_from_dataset_dir(tmp_path, oracle_mod):
    """Batch-level MultiDataset constructor: all pickles resident, per-env dataset switching;
    checked against the oracle on the same seeds."""
    from gym_trading_env_amd import BatchedTradingEnv
    rng = np.random.default_rng(5)
    sets = []
    for d in range(6):
        T = 120 + 7 * d
        close = 100 * np.exp(np.cumsum(rng.normal(0, 1e-2, T)))
        feat = rng.normal(0, 1, (T, 3)).astype(np.float32)
        sets.append((feat, close))
        make_df(feat, close).to_pickle(tmp_path / f"s{d}.pkl")
    with pytest.raises(FileNotFoundError):
        BatchedTradingEnv.from_dataset_dir(str(tmp_path / "none*.pkl"), 8)
    calls = []
    env = BatchedTradingEnv.from_dataset_dir(
        str(tmp_path / "*.pkl"), 512, positions=[-1, 0, 1], windows=4, max_episode_duration=15,
        preprocess=lambda df: (calls.append(len(df)) or df), output="numpy", seed=3)
    assert len(calls) == 6 and len(env.datasets) == 6 and sorted(env.dataset_names) == [f"s{d}.pkl" for d in range(6)]
    # the oracle gets the datasets in the env's (glob) order
    staged = [(s.feat, s.close) for s in env.datasets]
    ora = oracle_mod.OracleEnv(env.cfg, staged)
    env.reset(); ora.reset()
    for k in range(60):
        a = rng.integers(-1, 3, 512).astype(np.int32)
        env.step(a); ora.step(a)
        np.testing.assert_array_equal(env.read_output("obs"), ora.obs)
        np.testing.assert_array_equal(env.state("dataset_index"), ora.state()["dataset_index"])
    assert len(np.unique(env.state("dataset_index"))) == 6   # envs spread over all datasets
    env.close()


def test_batched_episode_metrics_match_single_env_metrics():
    """`BatchedTradingEnv.episode_metrics()` == `TradingEnv.get_metrics()` for the same episode."""
    from gym_trading_env_amd import BatchedTradingEnv, TradingEnv
    g = replay.load("c2_nowindow")
    feat, close = g["datasets"][0]
    feat, close = feat[:60], close[:60]
    df = make_df(feat, close)
    kw = dict(positions=[-1, 0, 1], trading_fees=1e-4, borrow_interest_rate=3e-6)
    single = TradingEnv(df=df, initial_position=0, verbose=0, **kw)
    batch = BatchedTradingEnv((feat, close), num_envs=3, initial_position=0, output="numpy",
                              autoreset="next_step", **kw)
    single.reset(); batch.reset()
    rng = np.random.default_rng(4)
    done = trunc = False
    while not (done or trunc):
        a = int(rng.integers(0, 3))
        _, _, done, trunc, _ = single.step(a)
        batch.step(np.full(3, a, np.int32))
    m = batch.episode_metrics()
    assert list(m["env_ids"]) == [0, 1, 2] and m["episode_length"][0] == 60
    ref = single.get_metrics()
    assert m["Market Return"][0] == ref["Market Return"]
    assert m["Portfolio Return"][2] == ref["Portfolio Return"]
    single.close(); batch.close()


def test_batched_history_and_custom_metrics_match_single_env(tmp_path):
    """Device trajectory log -> History: the same columns/values the N=1 drop-in logs, and
    `add_metric` lambdas over it (examples/example_environnement.py:45-46)."""
    from gym_trading_env_amd import BatchedTradingEnv, TradingEnv
    g = replay.load("c2_nowindow")
    feat, close = g["datasets"][0]
    df = make_df(feat[:80], close[:80])
    kw = dict(positions=[-1, 0, 1], trading_fees=1e-4, borrow_interest_rate=3e-6,
              max_episode_duration=30)
    single = TradingEnv(df=df, initial_position=0, verbose=0, **kw)
    batch = BatchedTradingEnv(df, num_envs=5, initial_position=0, output="numpy",
                              autoreset="next_step", log_steps=64, **kw)
    changes = lambda history: int(np.sum(np.diff(history["position"]) != 0))
    length = lambda history: len(history["position"])
    for env in (single, batch):
        env.add_metric("Position Changes", changes)
        env.add_metric("Episode Lenght", length)
    np.random.seed(3)
    single.reset()
    start = single.historical_info["idx", 0]
    batch.reset(inject_idx=np.full(5, start, np.int32))
    rng = np.random.default_rng(8)
    done = trunc = False
    while not (done or trunc):
        a = int(rng.integers(0, 3))
        _, _, done, trunc, _ = single.step(a)
        batch.step(np.full(5, a, np.int32))
    hs, hb = single.historical_info, batch.history(3)
    assert len(hb) == len(hs) == 30
    for col in ("idx", "step", "position", "portfolio_valuation", "real_position", "reward",
                "data_close", "data_volume"):
        np.testing.assert_allclose(np.asarray(hb[col], float), np.asarray(hs[col], float),
                                   rtol=1e-12, atol=1e-15, err_msg=col)
    assert list(hb["date"]) == list(hs["date"])
    m = batch.episode_metrics()
    ref = single.get_metrics()
    assert m["Position Changes"][0] == ref["Position Changes"] and m["Episode Lenght"][4] == 30
    assert m["Market Return"][2] == ref["Market Return"]
    # save_for_render: the same joined frame as the single env's (written by our own code just now)
    single.save_for_render(dir=str(tmp_path / "one"))
    path = batch.save_for_render(3, dir=str(tmp_path / "batch"))
    a = pd.read_pickle(next((tmp_path / "one").glob("*.pkl")))
    b = pd.read_pickle(path)
    assert len(a) == len(b) == 30 and list(a.index) == list(b.index)
    for col in ("open", "high", "low", "close", "portfolio_valuation", "position", "reward"):
        np.testing.assert_allclose(np.asarray(a[col], float), np.asarray(b[col], float), rtol=1e-12)
    with pytest.raises(ValueError):
        BatchedTradingEnv(df, num_envs=2, output="numpy").add_metric("x", length)
    single.close(); batch.close()


def test_read_env_snapshot_equals_separate_reads():
    """gte_read_env (one transfer: state + returns + observation of one env) against the
    field-by-field accessors, for several envs of a batch, after reset and after steps."""
    from gym_trading_env_amd.batched import BatchedTradingEnv
    rng = np.random.default_rng(5)
    T, N = 300, 200
    close = 100 * np.exp(np.cumsum(rng.normal(0, 2e-2, T)))
    feat = rng.normal(0, 1, (T, 3)).astype(np.float32)
    env = BatchedTradingEnv((feat, close), num_envs=N, positions=[-1, 0, 1], windows=6,
                            trading_fees=1e-3, borrow_interest_rate=1e-4, max_episode_duration=15,
                            output="numpy", seed=2)
    with pytest.raises(Exception):
        env.read_env(0)  # before reset
    env.reset()
    for k in range(20):
        if k:
            obs_k, reward_k, term_k, trunc_k, _ = env.step(rng.integers(-1, 3, N).astype(np.int32))
            cached_pv = env.state("portfolio_valuation")  # numpy mode: came with the results
            env._snap_epoch = -1  # from here on state() goes through gte_get_state again
            np.testing.assert_array_equal(cached_pv, env.state("portfolio_valuation"))
            np.testing.assert_array_equal(obs_k, env.read_output("obs"))
            np.testing.assert_array_equal(reward_k, env.read_output("reward64"))
            np.testing.assert_array_equal(term_k, env.read_output("terminated").astype(bool))
            np.testing.assert_array_equal(trunc_k, env.read_output("truncated").astype(bool))
        else:
            env._snap_epoch = -1
        obs_all = env.read_output("obs")
        for e in (0, 63, 64, N - 1):
            snap, obs = env.read_env(e)
            for f in ("idx", "step", "position_index", "dataset_index", "start_idx", "episode",
                      "needs_reset", "asset", "fiat", "interest_asset", "interest_fiat",
                      "portfolio_valuation", "real_position"):
                assert getattr(snap, f) == env.state(f)[e], (k, e, f)
            assert snap.reward == env.read_output("reward64")[e]
            assert snap.terminated == env.read_output("terminated")[e]
            assert snap.truncated == env.read_output("truncated")[e]
            np.testing.assert_array_equal(obs, obs_all[e])
    snap, obs = env.read_env(3, with_obs=False)
    assert obs is None and snap.idx == env.state("idx")[3]
    some, some_obs = env.read_envs(60, 10)
    np.testing.assert_array_equal(some["idx"], env.state("idx")[60:70])
    np.testing.assert_array_equal(some_obs, env.read_output("obs")[60:70])
    with pytest.raises(Exception):
        env.read_env(N)
    env.close()


def test_custom_dynamic_feature_callables_run_on_the_host():
    """Arbitrary `dynamic_feature_functions` (docs/source/customization.rst) in the N=1 drop-in:
    callables the device does not know are evaluated over the History on the host and written
    in place like the reference's (:153-154).  Re-implementations of the two defaults under
    other names must reproduce the device-side columns bit for bit; a third, really custom,
    column is checked against its definition, window rows included."""
    import pandas as pd
    import gym_trading_env_amd as gte

    def mine_position(history):
        return history["position", -1]

    def mine_real_position(history):
        return history["real_position", -1]

    def valuation_ratio(history):
        return history["portfolio_valuation", -1] / 1000.0

    rng = np.random.default_rng(8)
    T = 400
    close = 100 * np.exp(np.cumsum(rng.normal(0, 1e-2, T)))
    df = pd.DataFrame({"close": close, "feature_a": rng.normal(0, 1, T),
                       "feature_b": rng.normal(0, 1, T)})
    kw = dict(df=df, positions=[-1, 0, 0.5, 1, 2], windows=6, trading_fees=1e-3,
              borrow_interest_rate=1e-4, max_episode_duration=40, verbose=0)
    builtin = gte.TradingEnv(**kw)
    custom = gte.TradingEnv(dynamic_feature_functions=[mine_position, mine_real_position,
                                                       valuation_ratio], **kw)
    assert custom.observation_space.shape == (6, 5) and builtin.observation_space.shape == (6, 4)
    for env in (builtin, custom):
        np.random.seed(3)
        env._trace = []
        obs, _ = env.reset()
        env._trace.append(obs.copy())
        for k in range(150):
            obs, reward, done, truncated, info = env.step(int(np.random.randint(5)))
            env._trace.append(obs.copy())
            if done or truncated:
                obs, _ = env.reset()
                env._trace.append(obs.copy())
    assert len(builtin._trace) == len(custom._trace) > 150
    for a, b in zip(builtin._trace, custom._trace):
        assert b.dtype == np.float32
        np.testing.assert_array_equal(a, b[:, :4])
    # the custom column: current row = this step's valuation / 1000 (as f32); earlier window
    # rows keep what was written when the env stood there (also by earlier episodes)
    h = custom.historical_info
    assert custom._trace[-1][-1, 4] == np.float32(h["portfolio_valuation", -1] / 1000.0)
    assert custom._trace[-1][-2, 4] == np.float32(h["portfolio_valuation", -2] / 1000.0)
    builtin.close()
    custom.close()
    # the batch takes the same callable: evaluated once per step for all envs (vectorised over a
    # BatchedHistory, tests/test_gpu_vector_api.py)
    batch = gte.BatchedTradingEnv(df, num_envs=4, dynamic_feature_functions=[valuation_ratio],
                                  positions=[-1, 0, 1])
    obs, _ = batch.reset()
    assert obs.shape == (4, 3) and (obs.cpu().numpy()[:, -1] == 1.0).all()
    batch.close()


def test_copy_false_returns_views_of_the_staging_buffer():
    """output="numpy", copy=False (Gymnasium's vector-env convention): the same values as
    copy=True, delivered as views that the next call overwrites."""
    from gym_trading_env_amd.batched import BatchedTradingEnv
    rng = np.random.default_rng(6)
    T, N = 300, 300
    close = 100 * np.exp(np.cumsum(rng.normal(0, 2e-2, T)))
    feat = rng.normal(0, 1, (T, 2)).astype(np.float32)
    kw = dict(num_envs=N, positions=[-1, 0, 1], windows=5, trading_fees=1e-3,
              max_episode_duration=12, output="numpy", seed=4)
    a = BatchedTradingEnv((feat, close), copy=True, **kw)
    b = BatchedTradingEnv((feat, close), copy=False, **kw)
    oa, _ = a.reset()
    ob, _ = b.reset()
    np.testing.assert_array_equal(oa, ob)
    assert ob.base is not None and oa.flags.owndata  # a view of foreign memory vs an own array
    first_view = ob
    first_copy = ob.copy()
    # small reads in between must not move the staging buffer under the views
    snap, one = b.read_env(7)
    np.testing.assert_array_equal(one, first_copy[7])
    for k in range(30):
        act = rng.integers(-1, 3, N).astype(np.int32)
        ra = a.step(act)
        rb = b.step(act)
        for x, y in zip(ra[:4], rb[:4]):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(a.state("portfolio_valuation"), b.state("portfolio_valuation"))
        assert rb[0].ctypes.data == first_view.ctypes.data  # same buffer every step
    assert not np.array_equal(first_view, first_copy)  # the old view shows the new step
    a.close()
    b.close()


def test_sb3_vecenv_adapter_against_single_envs():
    """SB3's VecEnv contract (reset -> obs; step_async/step_wait -> obs, rewards, dones, infos;
    self-resetting envs with infos[i]['terminal_observation'] / ['TimeLimit.truncated']) over
    the batch, checked against the oracle driven the same way."""
    import gym_trading_env_amd as gte
    from gym_trading_env_amd.config import make_config
    from oracle import oracle
    rng = np.random.default_rng(11)
    T, N = 400, 96
    close = 100 * np.exp(np.cumsum(rng.normal(-2e-3, 4e-2, T)))  # drawdowns happen
    feat = rng.normal(0, 1, (T, 3)).astype(np.float32)
    kw = dict(positions=[-1, 0, 1, 2], windows=4, trading_fees=1e-3, borrow_interest_rate=1e-4,
              max_episode_duration=25, seed=6)
    vec = gte.SB3TradingVecEnv((feat, close), N, **kw)
    full = np.zeros((T, 5), np.float32)
    full[:, :3] = feat
    ora = oracle.OracleEnv(make_config(n_envs=N, n_static=3, autoreset="same_step", final_obs=True,
                                       **kw), [(full, close)])
    obs = vec.reset()
    ora.reset()
    assert obs.shape == (N, 4, 5) and vec.observation_space.shape == (4, 5)
    np.testing.assert_array_equal(obs, ora.obs)
    seen_term = seen_trunc = 0
    for k in range(80):
        a = rng.integers(0, 4, N)
        vec.step_async(a)
        obs, rewards, dones, infos = vec.step_wait()
        pv_before = ora.state()["portfolio_valuation"].copy()
        ora.step(a.astype(np.int32))
        np.testing.assert_array_equal(obs, ora.obs)
        np.testing.assert_array_equal(rewards, ora.reward)
        np.testing.assert_array_equal(dones, (ora.terminated | ora.truncated).astype(bool))
        assert rewards.dtype == np.float32 and len(infos) == N
        for e in range(N):
            assert ("terminal_observation" in infos[e]) == bool(dones[e])
            if dones[e]:
                np.testing.assert_array_equal(infos[e]["terminal_observation"], ora.final_obs[e])
                assert infos[e]["TimeLimit.truncated"] == bool(ora.truncated[e] and not ora.terminated[e])
                seen_term += int(ora.terminated[e])
                seen_trunc += int(ora.truncated[e] and not ora.terminated[e])
            if not dones[e]:
                assert infos[e]["portfolio_valuation"] == ora.state()["portfolio_valuation"][e]
            elif ora.terminated[e]:
                # an env that ended reports its TERMINAL step's info (environments.py:272), not the
                # state after the in-launch reset (the oracle keeps no terminal record: the
                # valuation is checked through the rules it obeyed; exact values against a
                # non-resetting twin in test_gpu_vector_api.py)
                assert infos[e]["portfolio_valuation"] / 1000 <= 0.7
            else:
                np.testing.assert_allclose(np.log(infos[e]["portfolio_valuation"] / pv_before[e]),
                                           rewards[e], rtol=2e-6, atol=1e-9)
    assert seen_term > 0 and seen_trunc > 0
    assert vec.env_is_wrapped(object) == [False] * N and vec.get_attr("num_envs", [0, 1]) == [N, N]
    vec.close()


def test_get_metrics_equal_the_reference():
    """tests/golden/hostcb_metrics.npz: the reference's get_metrics() after each of five
    episodes (percentage strings formatted by environments.py:279-285 + two add_metric
    callables); the drop-in must return the same dicts for the same seeds and actions."""
    import json
    from gym_trading_env_amd import TradingEnv
    z = np.load(os.path.join(replay.GOLDEN_DIR, "hostcb_metrics.npz"), allow_pickle=False)
    cfg = json.loads(str(z["cfg_json"]))
    expected = json.loads(str(z["metrics_json"]))
    df = make_df(z["feat_0"], z["close_0"])
    env = TradingEnv(df=df, verbose=0, **{k: cfg[k] for k in (
        "positions", "windows", "trading_fees", "borrow_interest_rate", "portfolio_initial_value",
        "initial_position", "max_episode_duration")})
    env.add_metric("Position Changes", lambda h: int(np.sum(np.diff(h["position"]) != 0)))
    env.add_metric("Episode Length", lambda h: len(h["position"]))
    for ep, want in enumerate(expected):
        np.random.seed(900 + ep)
        env.reset()
        done = trunc = False
        k = 0
        while not (done or trunc):
            _, _, done, trunc, _ = env.step(int(z["actions"][ep, k]))
            k += 1
        got = {str(a): (b if isinstance(b, str) else int(b)) for a, b in env.get_metrics().items()}
        assert got == want, (ep, got, want)
    env.close()


def test_state_tensor_is_a_device_view_of_the_state():
    """state_tensor(): zero-copy torch views of the struct-of-arrays state snapshot, equal to
    the host copies, refreshed after every step — e.g. for a reward computed on the device."""
    import torch
    from gym_trading_env_amd.batched import BatchedTradingEnv
    rng = np.random.default_rng(12)
    T, N = 300, 500
    close = 100 * np.exp(np.cumsum(rng.normal(0, 1e-2, T)))
    feat = rng.normal(0, 1, (T, 2)).astype(np.float32)
    env = BatchedTradingEnv((feat, close), num_envs=N, positions=[-1, 0, 1], windows=3,
                            trading_fees=1e-3, max_episode_duration=20, seed=1)
    env.reset()
    prev = env.state_tensor("portfolio_valuation").clone()
    ptr = env.state_tensor("portfolio_valuation").data_ptr()
    for k in range(30):
        a = torch.from_numpy(rng.integers(-1, 3, N).astype(np.int32)).cuda()
        obs, reward, term, trunc, _ = env.step(a)
        pv = env.state_tensor("portfolio_valuation")
        assert pv.is_cuda and pv.dtype == torch.float64 and pv.data_ptr() == ptr
        np.testing.assert_array_equal(pv.cpu().numpy(), env.state("portfolio_valuation"))
        np.testing.assert_array_equal(env.state_tensor("idx").cpu().numpy(), env.state("idx"))
        # a device-side reward: simple return where the episode went on (needs_reset == 0 before)
        simple = pv / prev - 1
        stepped = ~(env.state_tensor("step") == 0)
        np.testing.assert_allclose(torch.log1p(simple)[stepped & ~term].cpu().numpy(),
                                   reward.double()[stepped & ~term].cpu().numpy(), rtol=1e-4, atol=1e-7)
        prev = pv.clone()
    env.close()
