#!/usr/bin/env python3
"""Record what the launch planner (csrc/gte_plan.h) decides over a table of shapes: tests/golden/launch_plans.json.

Every row goes through the C ABI with GTE_DEBUG_GEOMETRY set: create -> upload of a tiny dataset -> reset -> for
the rollout rows a 2-step rollout -> destroy.  The library prints one `[gte] plan:` line after every moment that
decides some of the plan and one `[gte] chip:` line per question the rules put to the kernels' side; the fixture
keeps, per row, the Shape, the Knobs, every question with its answer and the plans, in the order printed.

    python tools/record_launch_plans.py [library_path=libgte.so] log=run.log     # needs an MI355X: the raw lines
    python tools/record_launch_plans.py plans=a.log chips=b.log [out=...json]     # no GPU: the fixture

`plans` and `chips` may be logs of two builds (a rule is changed deliberately: plans from the new build; a
refactor: plans from the build before it, chip answers from the one after).  With neither given, the table is
run once and both come from that run.  tests/test_plan_cpu.py replays the fixture on the CPU,
tests/test_gpu_launch_plans.py holds the library to it.
"""
import ctypes as C
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_plans.json")
SWITCHES = ("GTE_SLIDE_FULL_WINDOWS", "GTE_SLIDE_AB", "GTE_SLIDE_STORE", "GTE_AFFINITY_BINS", "GTE_RESIDENT_EPB")
KV_BITS = ("PER_WAVE_PHASE_A", "NO_LDS_STAGING", "RETIRED_OVERLAPPED", "SHARED_TU", "ROLLOUT_PER_STEP",
           "ROLLOUT_GATHER", "LOG_SEPARATE", "LOG_FUSED", "GENERIC_COPY", "RECORD_DIRECT", "DENSE_FLAGS")


def rows():
    """name -> what differs from the base row: 65 536 envs x (20, 30 + 2), episodes of 500 steps, everything
    automatic.  Keys of make_config, plus env (switches), rollout ("keep" / "last": a 2-step rollout with / without
    per-step observations) and T (rows of the dataset; default: just enough)."""
    from gym_trading_env_amd import _abi
    t = {}
    # benchmark configs
    t["c2"] = dict(n_envs=4096, windows=None, n_static=14)
    t["c3"] = dict()
    t["c4"] = dict(n_envs=32768)
    t["c5"] = dict(n_envs=32768, n_datasets=128)
    # streaming regime
    for n in (262144, 131072, 100003, 81920):
        t[f"stream_{n}"] = dict(n_envs=n)
    t["stream_262144_generic_copy"] = dict(n_envs=262144, kernel_variant=_abi.KV_GENERIC_COPY)
    # off the hot shape
    t["no_dyn"] = dict(n_static=32, dynamic_feature_functions=())
    t["fobs_31"] = dict(n_static=29)
    t["tiny_window"] = dict(windows=4, n_static=6)
    t["dyn_persist"] = dict(dyn_persist=True)
    t["final_obs"] = dict(final_obs=True, autoreset="same_step")
    t["log_64"] = dict(log_steps=64)
    for n in (1, 63, 64, 1000):
        t[f"n_{n}"] = dict(n_envs=n)
    # the config's knobs
    for v in (1, 16, 64):
        t[f"epw_{v}"] = dict(envs_per_wave=v)
    for v in (0, 1, 2, 3):
        t[f"store_{v}"] = dict(nontemporal_obs=v)
    for v in (-1, 0, 8):
        t[f"slack_{v}"] = dict(obs_slack_rows=v)
    for v in (-1, 0, 32):
        t[f"affinity_{v}"] = dict(affinity_period=v)
    for bit in KV_BITS:
        t[f"kv_{bit.lower()}"] = dict(kernel_variant=getattr(_abi, "KV_" + bit))
    # the two loops that shrink a workgroup
    t["shrink_index_range"] = dict(n_envs=64, windows=2048, n_static=126, envs_per_wave=64)
    t["shrink_lds"] = dict(n_envs=256, windows=1024, envs_per_wave=16)
    # environment switches, on a row that slides
    t["env_full_windows"] = dict(env={"GTE_SLIDE_FULL_WINDOWS": "1"})
    for v in (1, 2, 3):
        t[f"env_slide_ab_{v}"] = dict(env={"GTE_SLIDE_AB": str(v)})
    for v in (0, 1, 2):
        t[f"env_slide_store_{v}"] = dict(env={"GTE_SLIDE_STORE": str(v)})
    t["env_slide_ab_2_store_1"] = dict(env={"GTE_SLIDE_AB": "2", "GTE_SLIDE_STORE": "1"})
    t["env_affinity_bins_64"] = dict(env={"GTE_AFFINITY_BINS": "64"})
    t["env_resident_epb_8"] = dict(env={"GTE_RESIDENT_EPB": "8"}, rollout="keep")
    # rollouts: the lazy choices
    for n in (1000, 16384, 65536):
        t[f"rollout_{n}_keep"] = dict(n_envs=n, rollout="keep")
        t[f"rollout_{n}_last"] = dict(n_envs=n, rollout="last")
    t["rollout_w1_keep"] = dict(n_envs=16384, windows=1, rollout="keep")
    t["rollout_gather_keep"] = dict(n_envs=16384, kernel_variant=_abi.KV_ROLLOUT_GATHER, rollout="keep")
    # the rule after upload: feature tables beyond 64 MiB turn the automatic L2-affinity order off
    t["big_table"] = dict(T=600000)
    return t


def spec(over):
    """(make_config keywords, switches, rollout, T) of a row"""
    over = dict(over)
    env, rollout, T = over.pop("env", {}), over.pop("rollout", None), over.pop("T", None)
    kw = dict(n_envs=65536, n_static=30, windows=20, positions=(-1, 0, 1), max_episode_duration=500)
    kw.update(over)
    if T is None:
        T = 2 * (kw["windows"] or 1) + kw["max_episode_duration"] + 10  # just hosts an episode
    return kw, env, rollout, T


def shape_and_knobs(over):
    """What plan_shape / read_knobs of gte_api.hip make of the row: the planner's Shape and Knobs (bools as 0 / 1)."""
    from gym_trading_env_amd.config import make_config
    kw, env, _, _ = spec(over)
    c = make_config(**kw)
    shape = dict(N=c.n_envs, D=c.n_datasets, W=max(c.window, 1), has_window=int(c.window > 0), Fobs=c.n_static + c.n_dyn,
                 nd=c.n_dyn, persist=c.dyn_persist, max_dur=c.max_episode_duration, final_obs=c.final_obs,
                 log_steps=c.log_steps, envs_per_wave=c.envs_per_wave, nontemporal_obs=c.nontemporal_obs,
                 obs_slack_rows=c.obs_slack_rows, affinity_period=c.affinity_period, kernel_variant=c.kernel_variant,
                 debug_flags=c.debug_flags)
    s = env.get("GTE_SLIDE_STORE", "")
    knobs = dict(slide_full_windows=int("GTE_SLIDE_FULL_WINDOWS" in env), slide_ab=int(env.get("GTE_SLIDE_AB", 0)),
                 slide_store=int(s) if s in ("0", "1", "2") else -1,
                 has_affinity_bins=int("GTE_AFFINITY_BINS" in env), affinity_bins=int(env.get("GTE_AFFINITY_BINS", 0)),
                 has_resident_epb=int("GTE_RESIDENT_EPB" in env), resident_epb=int(env.get("GTE_RESIDENT_EPB", 0)))
    return shape, knobs


def table_bytes(over):
    kw, _, _, T = spec(over)
    c_static, n_dyn = kw["n_static"], len(kw.get("dynamic_feature_functions", (0, 0)))
    return kw.get("n_datasets", 1) * T * (c_static + n_dyn) * 4


def run_row(lib, over, full=True, inspect=None):
    """The row through the C ABI; the library prints to stderr.  full = False: create and destroy alone;
    inspect(E): called once the env exists."""
    import numpy as np
    from gym_trading_env_amd import _abi
    from gym_trading_env_amd.config import make_config
    kw, env, rollout, T = spec(over)
    saved = {k: os.environ.pop(k, None) for k in SWITCHES + ("GTE_DEBUG_GEOMETRY",)}
    os.environ.update(env, GTE_DEBUG_GEOMETRY="1")
    E = C.c_void_p()
    try:
        cfg = make_config(**kw)
        _abi.check(lib, lib.gte_create(C.byref(cfg), C.byref(E)))
        if inspect:
            inspect(E)
        if full:
            feat = np.zeros((T, cfg.n_static + cfg.n_dyn), np.float32)
            close = np.linspace(100.0, 101.0, T)
            for d in range(cfg.n_datasets):
                _abi.check(lib, lib.gte_upload_dataset(E, d, feat.ctypes.data, close.ctypes.data, None, None, T))
            _abi.check(lib, lib.gte_reset(E, None, None, None, None))
            if rollout:
                import torch
                acts = torch.ones((2, cfg.n_envs), dtype=torch.int32, device="cuda")
                bufs = _abi.GteRolloutBufs()
                if rollout == "keep":
                    obs = torch.empty((2, cfg.n_envs, max(cfg.window, 1), cfg.n_static + cfg.n_dyn), device="cuda")
                    bufs.obs = obs.data_ptr()
                torch.cuda.synchronize()
                _abi.check(lib, lib.gte_rollout(E, acts.data_ptr(), 2, C.byref(bufs)))
            _abi.check(lib, lib.gte_synchronize(E))
    finally:
        if E:
            lib.gte_destroy(E)
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


CHIP_LINE = re.compile(r"^\[gte\] chip: (\w+) (.*) -> (-?\d+)$")
PLAN_LINE = re.compile(r"^\[gte\] plan: (.*)$")


def parse(text):
    """The events of one row's output, in order: every plan line with the chip questions printed since the one
    before -> [{"when", "chip": [[question, arguments ..., answer], ...], "plan": {key: int or [int, int, int]}}]"""
    events, chip = [], []
    for line in text.splitlines():
        m = CHIP_LINE.match(line)
        if m:
            chip.append([m.group(1)] + [int(a.split("=")[1]) for a in m.group(2).split()] + [int(m.group(3))])
            continue
        m = PLAN_LINE.match(line)
        if m:
            fields = dict(f.split("=") for f in m.group(1).split())
            when = fields.pop("when")
            plan = {k: [int(x) for x in v.split(",")] if "," in v else int(v) for k, v in fields.items()}
            events.append({"when": when, "chip": chip, "plan": plan})
            chip = []
    assert not chip, "chip questions after the last plan line"
    return events


def record(library_path, log):
    """run the table, one `# row NAME` header per row, the library's own lines below it"""
    from gym_trading_env_amd import _abi
    lib = _abi.load_library(library_path)
    with open(log, "w") as out:
        for name, over in rows().items():
            with tempfile.TemporaryFile(mode="w+") as tmp:
                sys.stderr.flush()
                keep = os.dup(2)
                os.dup2(tmp.fileno(), 2)
                try:
                    run_row(lib, over)
                finally:
                    os.dup2(keep, 2)
                    os.close(keep)
                tmp.seek(0)
                lines = [ln for ln in tmp.read().splitlines() if ln.startswith(("[gte] plan:", "[gte] chip:"))]
            out.write(f"# row {name}\n" + "".join(ln + "\n" for ln in lines))
            print(f"{name}: {len(lines)} lines", flush=True)


def read_log(path):
    out = {}
    for block in open(path).read().split("# row ")[1:]:
        name, _, body = block.partition("\n")
        out[name] = parse(body)
    return out


def build_fixture(plans_log, chips_log, out):
    plans, chips = read_log(plans_log), read_log(chips_log)
    table = rows()
    assert list(plans) == list(chips) == list(table), "the logs do not hold the whole table"
    # Kept small: a row's Shape and Knobs hold what differs from `base` (the c3 row's), and an event names its
    # chip questions and its plan by index into `chips` and `plans`, where each distinct one stands once.
    base_shape, base_knobs = shape_and_knobs(table["c3"])
    chip_table, plan_table, fixture = [], [], []

    def index(items, x):
        if x not in items:
            items.append(x)
        return items.index(x)

    for name, over in table.items():
        shape, knobs = shape_and_knobs(over)
        a, b = plans[name], chips[name]
        assert [e["when"] for e in a] == [e["when"] for e in b], name
        events = [{"when": p["when"], "chip": index(chip_table, c["chip"]), "plan": index(plan_table, p["plan"])}
                  for p, c in zip(a, b)]
        keep = spec(over)[2] == "keep"
        fixture.append({"name": name, "shape": {k: v for k, v in shape.items() if v != base_shape[k]},
                        "knobs": {k: v for k, v in knobs.items() if v != base_knobs[k]},
                        "table_bytes": table_bytes(over), "keep_obs": int(keep), "events": events})
    dumps = lambda x: json.dumps(x, separators=(",", ":"))
    lines = lambda items: "[\n" + ",\n".join(dumps(x) for x in items) + "\n]"
    with open(out, "w") as f:
        f.write('{"base":' + dumps({"shape": base_shape, "knobs": base_knobs}) + ',\n"chips":' + lines(chip_table) +
                ',\n"plans":' + lines(plan_table) + ',\n"rows":' + lines(fixture) + "}\n")
    print(f"{out}: {len(fixture)} rows, {os.path.getsize(out)} bytes")


def load_fixture(path=FIXTURE):
    """the fixture's rows in full: Shape and Knobs completed from `base`, chip questions and plans in place"""
    fx = json.load(open(path))
    return [dict(r, shape={**fx["base"]["shape"], **r["shape"]}, knobs={**fx["base"]["knobs"], **r["knobs"]},
                 events=[{"when": e["when"], "chip": fx["chips"][e["chip"]], "plan": fx["plans"][e["plan"]]}
                         for e in r["events"]]) for r in fx["rows"]]


def main():
    args = dict(a.split("=", 1) for a in sys.argv[1:])
    out = args.get("out", FIXTURE)
    if "plans" in args or "chips" in args:
        build_fixture(args["plans"], args["chips"], out)
        return
    log = args.get("log") or os.path.join(tempfile.mkdtemp(), "launch_plans.log")
    record(args.get("library_path"), log)
    if "log" not in args:
        build_fixture(log, log, out)


if __name__ == "__main__":
    main()
