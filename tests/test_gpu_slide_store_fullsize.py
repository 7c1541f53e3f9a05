"""The automatic store policy per launch kind (gte.h) at the sizes where it decides: launches that write full
windows go by the classic buffer's bytes, slide launches by the sliding slab's.  launch_info() and 12 steps
against the classic twin (`obs_slack_rows=-1`), bit for bit.  Needs an MI355X."""
import numpy as np
import pytest

from test_gpu_parity import _synthetic

pytestmark = pytest.mark.gpu

C3 = dict(windows=20, positions=[-1, 0, 1], trading_fees=1e-4, borrow_interest_rate=3e-6,
          autoreset="next_step", max_episode_duration=9, seed=5)

# n_envs, constructor arguments, obs_stores, slide_obs_stores.  The c3 shape has W + M = 28 rows of 128 bytes:
#  * 65 536 envs: 168 MB of windows (sc1), a 235 MB slab (non-temporal slides);
#  * 32 768 envs: 84 MB and 117 MB, both below 190 MB: one policy;
#  * an explicit policy governs both kinds;
#  * a numpy-output env binds no sliding buffer and never slides: one policy.
CASES = {
    "65536": (65_536, dict(output="torch"), "sc1", "non-temporal"),
    "32768": (32_768, dict(output="torch"), "sc1", "sc1"),
    "65536-explicit-sc1": (65_536, dict(output="torch", nontemporal_obs=2), "sc1", "sc1"),
    "65536-numpy": (65_536, dict(output="numpy"), "sc1", "sc1"),
}


@pytest.fixture(scope="module")
def dataset():
    return _synthetic(1234, 20_000, 30, sigma=1e-3)


@pytest.mark.parametrize("case", sorted(CASES))
def test_automatic_slide_store_policy(dataset, case):
    import torch
    from gym_trading_env_amd.batched import BatchedTradingEnv
    n, kw, stores, slide_stores = CASES[case]
    env = BatchedTradingEnv(dataset, num_envs=n, **C3, **kw)
    twin = BatchedTradingEnv(dataset, num_envs=n, obs_slack_rows=-1, **C3, **kw)
    info = env.launch_info()
    assert (info["obs_stores"], info["slide_obs_stores"]) == (stores, slide_stores), info
    tinfo = twin.launch_info()
    assert tinfo["obs_stores"] == tinfo["slide_obs_stores"] == stores, tinfo
    assert env.sliding_obs == (kw["output"] == "torch") and not twin.sliding_obs
    gen = torch.Generator(device="cuda").manual_seed(3)
    acts = torch.randint(-1, 3, (12, n), dtype=torch.int32, device="cuda", generator=gen)
    if kw["output"] != "torch":
        acts = acts.cpu().numpy()
    env.reset()
    twin.reset()
    heads = []
    for k in range(12):
        got, want = env.step(acts[k])[:4], twin.step(acts[k])[:4]
        heads.append(int(env._obs_view.head))
        for f, a, b in zip(("obs", "reward", "terminated", "truncated"), got, want):
            if kw["output"] == "torch":
                assert torch.equal(a.view(torch.int32) if f == "obs" else a, b.view(torch.int32) if f == "obs" else b), (k, f)
            else:
                assert np.array_equal(a.view(np.int32) if f == "obs" else a, b.view(np.int32) if f == "obs" else b), (k, f)
    if env.sliding_obs:
        assert heads == [1, 2, 3, 4, 5, 6, 7, 8, 0, 1, 2, 3], heads  # eleven slides and the wrap
    for f in ("idx", "step", "episode", "needs_reset", "asset", "fiat", "portfolio_valuation"):
        np.testing.assert_array_equal(env.state(f), twin.state(f), err_msg=f)
    assert (env.state("episode") >= 2).all()  # episodes of 9 steps: every env reset inside a slide or the wrap
    env.close()
    twin.close()
