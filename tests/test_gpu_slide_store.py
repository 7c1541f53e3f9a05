"""Store policy per launch kind (gte.h, "Store policy per launch kind"): launches that store one row per env
take `LaunchPlan::slide_store`, every launch that writes full windows the plan's `store`.  Nothing a caller
reads depends on either: under every pair of policies the sliding env equals its classic twin
(`obs_slack_rows=-1`) bit for bit after EVERY call, `launch_info()` reports the pair, and a slide launch
still writes exactly the newest row.  Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("idx", "step", "position_index", "dataset_index", "start_idx", "episode", "needs_reset", "asset",
         "fiat", "interest_asset", "interest_fiat", "portfolio_valuation", "real_position")
SENTINEL = 0x7FC0DEAD  # a NaN pattern no observation holds
NAMES = ("plain", "non-temporal", "sc1")
N_PERIODS = 3
STAGGER = 8  # masked resets one step apart, more of them than an episode has calls: an env ends in every step after

# name -> (W, envs, obs_slack_rows, envs_per_wave): the smallest hot shape that slides (10 waves of 16 envs:
# two full workgroups and a half one); the headline window with the automatic slack (8 rows) and the automatic
# geometry at a ragged env count
SHAPES = {"smallest": (8, 160, 3, 16), "headline": (20, 200, 0, 0)}


def _data(T=400, seed=3):
    rng = np.random.default_rng(seed)
    close = 100.0 * np.exp(np.cumsum(rng.normal(-1e-3, 2e-2, T)))
    feat = rng.normal(0, 1, (T, 30)).astype(np.float32)  # + the two default dynamic columns: F_obs = 32
    return feat, close, close * 1.01, close * 0.99


def _env(shape, **kw):
    from gym_trading_env_amd.batched import BatchedTradingEnv
    W, n, slack, epw = SHAPES[shape]
    args = dict(num_envs=n, positions=[-1, 0, 1], windows=W, trading_fees=1e-3, borrow_interest_rate=1e-4,
                max_episode_duration=7, seed=21, output="torch", verbose=0, envs_per_wave=epw,
                obs_slack_rows=slack)
    args.update(kw)
    return BatchedTradingEnv(_data(), **args)


def _actions(k, n, seed=5):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-1, 3, (k, n), generator=g, device="cuda", dtype=torch.int32)


def _snapshot(env):
    """Everything a caller can read after a call, copied."""
    import torch
    torch.cuda.synchronize()
    t = env._t
    snap = {"obs": t["obs"].clone(memory_format=torch.contiguous_format).view(torch.int32)}
    for k in ("reward", "reward64", "terminated", "truncated"):
        snap[k] = t[k].clone()
    snap["terminal_ids"] = np.array(env.terminal_ids())
    for k in STATE:
        snap[k] = np.array(env.state(k))
    return snap


def _equal(a, b, what):
    import torch
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(v, b[k], err_msg=f"{what}: {k}")
        else:
            assert v.shape == b[k].shape and torch.equal(v, b[k]), f"{what}: {k}"


def _n_steps(M):
    return STAGGER + N_PERIODS * (M + 1) + 2


def _trace(env, acts, M):
    """reset; STAGGER steps, each followed by a masked reset of one residue class of the envs, which puts the
    episodes out of phase (from then on some envs end in every step) and falls among the slides; then
    N_PERIODS wrap periods of steps and two more.  (what, snapshot, head) after every call."""
    n = env.num_envs
    out = []
    env.reset()
    out.append(("reset", _snapshot(env), int(env._obs_view.head)))
    for i in range(_n_steps(M)):
        env.step(acts[i])
        out.append(("step", _snapshot(env), int(env._obs_view.head)))
        if i < STAGGER:
            env.reset(mask=(np.arange(n) % STAGGER == i).astype(np.uint8))
            out.append(("masked reset", _snapshot(env), int(env._obs_view.head)))
    return out


_twins = {}


def _twin_trace(shape, mode, acts, M):
    """The classic twin's trace, run once per (shape, autoreset mode): its values do not depend on a policy."""
    if (shape, mode) not in _twins:
        twin = _env(shape, autoreset=mode, obs_slack_rows=-1)
        assert not twin.sliding_obs and twin._t["obs"].is_contiguous()
        _twins[shape, mode] = [(w, s) for w, s, _ in _trace(twin, acts, M)]
        twin.close()
    return _twins[shape, mode]


def _check_against_twin(env, shape, mode):
    """The env's trace equals the twin's after every call; its heads show the slides, the wraps, masked resets
    among slides, and envs that reset at every head position."""
    M = int(env._obs_view.slack_rows)
    W, n, slack, _ = SHAPES[shape]
    assert env.sliding_obs and M == (slack if slack else 2 * W // 5)
    acts = _actions(_n_steps(M), n)
    ref = _twin_trace(shape, mode, acts, M)
    got = _trace(env, acts, M)
    assert [w for w, _, _ in got] == [w for w, _ in ref]
    for i, ((what, snap, _), (_, want)) in enumerate(zip(got, ref)):
        _equal(snap, want, f"call {i} ({what})")
    whats = [w for w, _, _ in got]
    heads = [h for _, _, h in got]
    ended = [bool((s["truncated"] | s["terminated"]).any()) for _, s, _ in got]
    slides = wraps = resets_among_slides = 0
    reset_heads = set()  # heads of the launches in which an env reset
    for i in range(1, len(got)):
        if whats[i] == "masked reset":  # leaves the head where it is
            assert heads[i] == heads[i - 1], heads
            resets_among_slides += int(0 < heads[i] < M and heads[i + 1] == heads[i] + 1)
            continue
        assert heads[i] == (heads[i - 1] + 1 if heads[i - 1] < M else 0), heads  # nothing here withdraws the claim
        slides += int(heads[i] > 0)
        wraps += int(heads[i] == 0)
        # same_step: the envs that ended reset inside this launch; next_step: those flagged by the call before
        if ended[i] if mode == "same_step" else (ended[i - 1] and whats[i - 1] == "step"):
            reset_heads.add(heads[i])
    assert slides >= N_PERIODS * M and wraps >= N_PERIODS and resets_among_slides > 0, heads
    assert reset_heads == set(range(M + 1)), (reset_heads, heads)


@pytest.mark.parametrize("slide", [0, 1, 2])
@pytest.mark.parametrize("plan", [0, 1, 2])
@pytest.mark.parametrize("mode", ["next_step", "same_step"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_pair_of_policies_equals_the_twin(shape, mode, plan, slide, monkeypatch):
    """nontemporal_obs = plan for the launches that write full windows, GTE_SLIDE_STORE = slide for the
    launches that store one row: launch_info() reports the pair and every value is the twin's."""
    monkeypatch.setenv("GTE_SLIDE_STORE", str(slide))
    env = _env(shape, autoreset=mode, nontemporal_obs=plan)
    monkeypatch.delenv("GTE_SLIDE_STORE")
    info = env.launch_info()
    assert (info["obs_stores"], info["slide_obs_stores"]) == (NAMES[plan], NAMES[slide]), info
    _check_against_twin(env, shape, mode)
    env.close()


@pytest.mark.parametrize("plan", [0, 1, 2])
def test_an_explicit_policy_governs_both_kinds(plan):
    """Without the override, nontemporal_obs = 0 / 1 / 2 is the policy of slide launches too."""
    env = _env("smallest", autoreset="next_step", nontemporal_obs=plan)
    info = env.launch_info()
    assert info["obs_stores"] == info["slide_obs_stores"] == NAMES[plan], info
    env.close()


def test_switch_bit_2_keeps_the_plan_policy_in_slides(monkeypatch):
    """GTE_SLIDE_AB=2 (gte.h): slide launches store as the full-window launches do, whatever GTE_SLIDE_STORE
    says; the values are the twin's."""
    monkeypatch.setenv("GTE_SLIDE_AB", "2")
    monkeypatch.setenv("GTE_SLIDE_STORE", "1")
    env = _env("smallest", autoreset="next_step", nontemporal_obs=2)
    monkeypatch.delenv("GTE_SLIDE_STORE")
    monkeypatch.delenv("GTE_SLIDE_AB")
    info = env.launch_info()
    assert info["slide_obs_stores"] == info["obs_stores"] == "sc1", info
    _check_against_twin(env, "smallest", "next_step")
    env.close()


def test_an_env_that_never_slides_reports_one_policy(monkeypatch):
    """obs_slack_rows = -1 and a numpy-output env bind no sliding buffer: GTE_SLIDE_STORE does not show."""
    monkeypatch.setenv("GTE_SLIDE_STORE", "1")
    envs = [_env("smallest", autoreset="next_step", nontemporal_obs=2, obs_slack_rows=-1),
            _env("smallest", autoreset="next_step", nontemporal_obs=2, output="numpy")]
    monkeypatch.delenv("GTE_SLIDE_STORE")
    for env in envs:
        info = env.launch_info()
        assert not env.sliding_obs and info["slide_obs_stores"] == info["obs_stores"] == "sc1", info
        env.close()


def test_a_nontemporal_slide_step_writes_only_the_new_row(monkeypatch):
    """The sentinel check of test_gpu_sliding_obs.py::test_a_slide_step_writes_only_the_new_row with sc1 for
    full windows and non-temporal slides: an env that merely advanced has exactly row h + W - 1 written, an
    env that reset exactly its window at the new head h, and a wrap rows 0 .. W - 1 of every env."""
    import torch
    W, n, M = 20, 165, 3
    from gym_trading_env_amd.batched import BatchedTradingEnv
    monkeypatch.setenv("GTE_SLIDE_STORE", "1")
    env = BatchedTradingEnv(_data(), num_envs=n, positions=[-1, 0, 1], windows=W, trading_fees=1e-3,
                            borrow_interest_rate=1e-4, max_episode_duration=7, seed=21, output="torch", verbose=0,
                            envs_per_wave=16, obs_slack_rows=M, autoreset="next_step", nontemporal_obs=2)
    monkeypatch.delenv("GTE_SLIDE_STORE")
    info = env.launch_info()
    assert env.sliding_obs and (info["obs_stores"], info["slide_obs_stores"]) == ("sc1", "non-temporal"), info
    acts = _actions(24, n, seed=8)
    env.reset()
    k = 0
    for third in range(3):  # episodes out of phase: every step sees resets in some waves and none in others
        for _ in range(2):
            env.step(acts[k]); k += 1
        env.reset(mask=(np.arange(n) % 3 == third).astype(np.uint8))
    slab = env._obs_slab.view(torch.int32)
    rows = torch.arange(W + M, device="cuda")
    seen = {"slide": 0, "reset_in_slide": 0, "advanced_in_slide": 0, "wrap": 0}
    for _ in range(12):
        h0 = int(env._obs_view.head)
        resets = torch.from_numpy(env.state("needs_reset") != 0).cuda()
        torch.cuda.synchronize()
        slab.fill_(SENTINEL)
        env.step(acts[k]); k += 1
        torch.cuda.synchronize()
        h = int(env._obs_view.head)
        written = (slab != SENTINEL).any(dim=2)  # [n, W + M]
        window = (rows >= h) & (rows < h + W)
        if h0 < M:  # a slide step
            assert h == h0 + 1
            expect = torch.where(resets[:, None], window[None, :], (rows == h + W - 1)[None, :])
            seen["slide"] += 1
            seen["reset_in_slide"] += int(resets.sum())
            seen["advanced_in_slide"] += int((~resets).sum())
        else:  # the wrap: every window in full at head 0
            assert h == 0
            expect = window[None, :].expand(n, -1)
            seen["wrap"] += 1
        assert torch.equal(written, expect), (h0, h)
        assert bool((slab[:, h:h + W][resets] != SENTINEL).all())  # all of it for the envs that reset
        assert bool((slab[:, h + W - 1] != SENTINEL).all())        # and the whole newest row of every env
    assert seen["slide"] >= 8 and seen["wrap"] >= 2, seen
    assert seen["reset_in_slide"] > 0 and seen["advanced_in_slide"] > 0, seen
    env.close()
