"""Host-side logic and the C-ABI surface, no GPU needed (no compute call is made)."""
import ast
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import gym_trading_env_amd as gte
from gym_trading_env_amd import _abi, spaces, staging
from gym_trading_env_amd.config import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    hdr = open(os.path.join(ROOT, "include", "gte.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(gte_[a-z_0-9]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    names = _declared_functions()
    assert len(names) >= 18 and "gte_step" in names and "gte_reset" in names
    lib = _abi.load_library()
    assert sorted(_abi.SYMBOLS) == names, "ctypes table and include/gte.h disagree"
    for n in names:
        assert hasattr(lib, n), f"libgte.so does not export {n}"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = set(re.findall(r" T (gte_[a-z_0-9]+)", out))
    assert set(names) <= exported
    assert lib.gte_abi_version() == _abi.GTE_ABI_VERSION


def test_library_contains_gfx950_code_object_only():
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o",
                          f"--input={_abi.LIB_PATH}"], capture_output=True, text=True)
    if out.returncode == 0 and out.stdout.strip():
        targets = [t for t in out.stdout.split() if "amdgcn" in t]
        assert targets and all("gfx950" in t for t in targets), targets


def test_struct_layout_matches_the_c_header(oracle_mod):
    # the oracle is compiled against include/gte.h and rejects a config whose
    # struct_bytes differs from its sizeof(gte_config)
    cfg = make_config(n_envs=3, n_static=2)
    assert cfg.struct_bytes == C.sizeof(_abi.GteConfig)
    env = oracle_mod.OracleEnv(cfg, [(np.zeros((10, 4), np.float32), np.ones(10))])
    env.close()


@pytest.mark.skipif(_abi.load_library().gte_device_count() > 0, reason="host has a GPU")
def test_no_cpu_fallback_fails_loudly():
    """On a GPU-less host the product refuses to run instead of falling back."""
    from gym_trading_env_amd.batched import BatchedTradingEnv
    feat = np.zeros((50, 3), np.float32)
    with pytest.raises(gte.GteError) as ei:
        BatchedTradingEnv((feat, np.ones(50)), num_envs=4, output="numpy")
    assert ei.value.status == _abi.GTE_ERR_NO_DEVICE
    assert "no CPU fallback" in str(ei.value)


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(ImportError, match="no CPU fallback"):
        _abi.load_library(str(tmp_path / "libgte.so"))


def test_config_mirrors_reference_constructor_checks():
    # environments.py:106
    with pytest.raises(AssertionError, match="initial_position"):
        make_config(n_envs=1, n_static=1, positions=[0, 1], initial_position=0.5)
    cfg = make_config(n_envs=1, n_static=1, positions=[-1, 0, 1], initial_position=0,
                      portfolio_initial_value=5)
    assert cfg.initial_position_index == 1
    assert cfg.portfolio_initial_value == 5.0 and isinstance(cfg.portfolio_initial_value, float)  # :104
    assert make_config(n_envs=1, n_static=1).initial_position_index == -1  # 'random'
    assert make_config(n_envs=1, n_static=1).max_episode_duration == 0  # 'max'
    assert make_config(n_envs=1, n_static=1, windows=None).window == 0
    assert list(make_config(n_envs=1, n_static=1).positions[:2]) == [0.0, 1.0]  # default [0, 1] (:81)
    c = make_config(n_envs=1, n_static=1, reward_function=("clipped_log_return", 1.0, -0.002, 0.005))
    assert (c.reward_kind, c.reward_param1, c.reward_param2) == (_abi.REWARD_CLIPPED_LOG_RETURN, -0.002, 0.005)
    with pytest.raises(ValueError, match="unknown reward spec"):
        make_config(n_envs=1, n_static=1, reward_function="sharpe")
    with pytest.raises(ValueError, match="unknown dynamic feature"):
        make_config(n_envs=1, n_static=1, dynamic_feature_functions=["momentum"])


def test_callables_are_recognised_by_identity_never_by_name():
    """Only THIS package's default objects (and explicit string / tuple specs) map to the device
    enums.  A user's function that merely shares a default's NAME is the user's code: it must be
    evaluated (host / vectorised path), not silently replaced by the device built-in."""
    from gym_trading_env_amd import config, defaults

    def basic_reward_function(history):  # same name as the default, different semantics
        return 0.25

    def dynamic_feature_real_position(history):
        return 7.0

    def log_return(history):
        return -1.0

    assert config.resolve_reward(defaults.basic_reward_function)[0] == _abi.REWARD_LOG_RETURN
    assert config.resolve_reward("basic_reward_function")[0] == _abi.REWARD_LOG_RETURN
    for f in (basic_reward_function, log_return, lambda h: 0.0):
        assert config.resolve_reward(f)[0] == config.HOST_CALLABLE
    assert config.resolve_dynamic_features(
        [defaults.dynamic_feature_last_position_taken, defaults.dynamic_feature_real_position,
         "real_position", 0]) == [_abi.DYN_LAST_POSITION, _abi.DYN_REAL_POSITION,
                                  _abi.DYN_REAL_POSITION, _abi.DYN_LAST_POSITION]
    assert config.resolve_dynamic_features([dynamic_feature_real_position, lambda h: 0.0]) == \
        [config.HOST_CALLABLE, config.HOST_CALLABLE]
    # the public names of the package ARE the default objects
    import gym_trading_env_amd as g
    assert g.basic_reward_function is defaults.basic_reward_function
    assert g.dynamic_feature_real_position is defaults.dynamic_feature_real_position
    # make_config keeps a device placeholder for a user's callable (its value is overwritten
    # after every launch); the struct itself never names a host callable
    c = make_config(n_envs=1, n_static=1, reward_function=basic_reward_function,
                    dynamic_feature_functions=[dynamic_feature_real_position])
    assert c.reward_kind == _abi.REWARD_LOG_RETURN and c.n_dyn == 1
    with pytest.raises(TypeError):
        config.resolve_reward(3.5)


def _df(T=30):
    idx = pd.date_range("2021-01-01", periods=T, freq="h")
    rng = np.random.default_rng(0)
    return pd.DataFrame({"open": rng.random(T) + 1, "high": rng.random(T) + 2, "low": rng.random(T),
                         "close": rng.random(T) + 1, "volume": rng.random(T),
                         "feature_b": rng.random(T), "my_feature_a": rng.random(T)}, index=idx)


def test_stage_dataframe_follows_set_df():
    df = _df()
    s = staging.stage_dataframe(df, n_dyn=2)
    # :130 every column whose name CONTAINS "feature", DataFrame order
    assert s.feature_columns == ["feature_b", "my_feature_a", "dynamic_feature__0", "dynamic_feature__1"]
    assert s.feat.dtype == np.float32 and s.feat.shape == (30, 4) and s.feat.flags.c_contiguous
    np.testing.assert_array_equal(s.feat[:, 0], df["feature_b"].to_numpy().astype(np.float32))
    np.testing.assert_array_equal(s.feat[:, 2:], 0)                 # :135-138
    assert s.close.dtype == np.float64
    np.testing.assert_array_equal(s.close, df["close"].to_numpy())  # :143
    assert set(s.info_columns) == {"open", "high", "low", "close", "volume"}  # :131
    assert s.info_array.shape == (30, 5) and s.T == 30 and s.n_obs == 4
    with pytest.raises(KeyError):
        staging.stage_dataframe(df.drop(columns=["close"]))


def test_stage_arrays_and_geometry_checks():
    s = staging.stage_arrays(np.ones((20, 3)), np.arange(1, 21), n_dyn=1)
    assert s.feat.shape == (20, 4) and s.feat[:, 3].sum() == 0
    with pytest.raises(ValueError):
        staging.stage_arrays(np.ones((20, 3)), np.arange(19))
    staging.check_episode_geometry(100, 5, 50)
    with pytest.raises(ValueError, match="low >= high"):   # np.random.randint(low, high) (:174)
        staging.check_episode_geometry(60, 5, 55)
    with pytest.raises(ValueError, match="too short"):
        staging.check_episode_geometry(5, 5, "max")


def test_spaces():
    d = spaces.Discrete(3)
    assert d.n == 3 and d.contains(d.sample()) and not d.contains(3)
    b = spaces.Box(-np.inf, np.inf, shape=[4, 7])
    assert tuple(b.shape) == (4, 7) and b.dtype == np.float32
    md = spaces.MultiDiscrete([3] * 5)
    assert md.contains(md.sample())


def test_golden_fixtures_are_data_only():
    import replay
    names = replay.golden_names()
    assert len(names) >= 10
    for n in names:
        z = np.load(os.path.join(replay.GOLDEN_DIR, n + ".npz"), allow_pickle=False)
        assert "obs" in z.files and "cfg_json" in z.files
    z = np.load(os.path.join(replay.GOLDEN_DIR, "portfolio_random.npz"), allow_pickle=False)
    assert z["inputs"].shape == (3000, 9) and z["outputs"].shape == (3000, 6)


def _resource_usage(source):
    """VGPRs / scratch / occupancy per kernel from hipcc's resource-usage remarks (gfx950)."""
    import re
    import shutil
    import subprocess
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                            "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
                            "-c", os.path.join(csrc, source), "-o", os.path.join(tmp, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for block in r.stderr.split("Function Name:")[1:]:
        get = lambda key: int(re.search(key + r":\s*(\d+)", block).group(1))
        out.append({"name": block.split()[0], "vgprs": get("VGPRs"),
                    "scratch": get(r"ScratchSize \[bytes/lane\]"),
                    "occupancy": get(r"Occupancy \[waves/SIMD\]")})
    assert out, r.stderr[-2000:]
    return out


@pytest.mark.parametrize("source,min_occupancy", [("gte_hot.hip", 6), ("gte_hot_nt.hip", 6),
                                                  ("gte_rollout.hip", 4), ("gte_backtest.hip", 3)])
def test_kernel_register_budget(source, min_occupancy):
    """The step kernel's speed hangs on its register allocation: one occupancy step costs
    10+ us per step, and scratch use doubles the store traffic.  A change to the
    shared device code that pushes the hot instantiations over their budget fails here, on the
    CPU, before anything is measured.  gte_backtest.hip: its two from-registers kernels carry an env
    and its statistics record through all fused steps (142 and 153 VGPRs, 3 waves/SIMD); written as
    a plain loop body the compiler kept the env's registers in scratch memory."""
    kernels = _resource_usage(source)
    for k in kernels:
        assert k["scratch"] == 0, k
        assert k["occupancy"] >= min_occupancy, k
    if source == "gte_backtest.hip":
        _assert_kernels_found(kernels, ("gte_backtest_kernel", "gte_backtest_signal_kernel"), 3)


def _assert_kernels_found(kernels, names, min_occupancy):
    """each from-registers backtest kernel is in the unit it is looked for in, by name, without scratch and at
    the occupancy it had before csrc/gte_summary_body.h held its body"""
    for name in names:
        found = [k for k in kernels if re.search(rf"_ZN3gte\d+{name}E", k["name"])]
        assert len(found) == 1, (name, [k["name"] for k in kernels])
        assert found[0]["scratch"] == 0 and found[0]["occupancy"] >= min_occupancy, found[0]


def test_features_compiled_out_of_the_hot_translation_units_are_guarded():
    """The isolated hot instantiations (GTE_HOT_ONLY) leave features out of phase A.  Every such
    block must name the Params field it depends on, that field must be tested by
    `hot_tu_covers` (gte_device.h), `gte_step` must pick the kernel with that predicate, and every
    launcher of a GTE_HOT_ONLY translation unit must refuse a launch it does not cover — so a
    launch predicate cannot drift from a compiled-out feature again (round 2: `final_info` read
    records the kernel never wrote)."""
    csrc = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
    read = lambda f: open(os.path.join(csrc, f)).read()
    dev = read("gte_device.h")
    body = re.search(r"inline bool hot_tu_covers\(const Params& p\) \{(.*?)\}", dev, re.S).group(1)
    # every block, in whichever file, carries `// p.<field>:` (the shared device code lives in headers:
    # no block merely fences off what an including file must not get)
    blocks = [b for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))
              for b in re.findall(r"^#ifndef GTE_HOT_ONLY(.*)", read(f), re.M)]
    fields = [re.match(r"\s*//\s*p\.([a-z_]+)", b) for b in blocks]
    named = [m.group(1) for m in fields if m]
    assert len(blocks) >= 4 and len(blocks) - len(named) == 0, "an #ifndef GTE_HOT_ONLY block does not name its field"
    assert sorted(set(named)) == ["final_rec", "log"]
    for f in set(named):
        assert re.search(rf"p\.{f}\b", body), f"hot_tu_covers does not test p.{f}"
    api = read("gte_api.hip")
    assert re.search(r"const bool hot = [^;]*gte::hot_tu_covers\(p\)", api)
    # (the two hot units are macro definitions plus the include of their launcher)
    for tu, holds_launcher in (("gte_hot.hip", "gte_hot_body.h"), ("gte_hot_nt.hip", "gte_hot_body.h"),
                               ("gte_rollout.hip", "gte_rollout.hip")):
        assert "#define GTE_HOT_ONLY 1" in read(tu)
        assert holds_launcher == tu or f'#include "{holds_launcher}"' in read(tu)
        src = read(holds_launcher)
        launchers = re.findall(r"hipError_t (?:GTE_HOT_NAME\()?(launch_[a-z_]+)\)?\(const Params& p.*?\n\}", src, re.S)
        assert launchers
        for m in re.finditer(r"hipError_t (?:GTE_HOT_NAME\()?launch_[a-z_]+\)?\(const Params& p.*?\n\}", src, re.S):
            assert "if (!hot_tu_covers(p)) return hipErrorInvalidValue;" in m.group(0), m.group(0)[:80]


def _csrc_sources():
    """name -> text of every .hip / .h under csrc/, comments removed"""
    csrc = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
    strip = lambda s: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))
    return {n: strip(open(os.path.join(csrc, n)).read()) for n in sorted(os.listdir(csrc))
            if n.endswith((".hip", ".h"))}


def _namespace_spans(text, namespace):
    """(start, end) of the text between the braces of every `namespace <namespace> {` block that opens at column 0"""
    spans = []
    for m in re.finditer(rf"^namespace {namespace} \{{", text, re.M):
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            i += 1
        spans.append((m.end(), i - 1))
    return spans


def _outside_namespace(text, namespace):
    for a, b in reversed(_namespace_spans(text, namespace)):
        text = text[:a] + text[b:]
    return text


def _signatures(text, namespace="gte"):
    """`ret name(params)` of every function declared or defined at column 0 inside `namespace <namespace>`
    (every block of it the text has, each to its closing brace)
    that is not static / inline / a template / device code -> {name: (signature, is_definition)},
    white space normalised.  GTE_HOT_NAME(x) stands for x and x_nt (gte_hot.hip is compiled twice).

    Known limits — this reads the way csrc/ is written, it is no C++ parser: the return type and the
    name stand on ONE line that starts at column 0; a `template <...>` head is on the line above;
    an attribute or a macro in front of the return type is not understood.  A function written
    otherwise is not seen at all, which test_cross_file_functions_are_declared_once_in_gte_launch_h
    reports as "declares a function no file defines" (or misses, for a function that is not declared
    either: then it cannot be called across files).  Parameter NAMES are compared as well as types:
    stricter than the compiler, on purpose — the header is the one place a reader looks them up."""
    out = {}
    inside = "\n".join(text[a:b] for a, b in _namespace_spans(text, namespace))
    skip = r"static\b|template\b|inline\b|__global__|__device__|struct\b|typedef\b|enum\b|constexpr\b|using\b|return\b"
    for m in re.finditer(rf"^(?!{skip})([A-Za-z_][\w \*&:<>]*?[\s\*&])(GTE_HOT_NAME\(\w+\)|\w+)\(", inside, re.M):
        if re.search(r"^template\b[^\n]*\n\Z", inside[:m.start()], re.M):
            continue  # (the line above opens a template)
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(inside[i], 0)
            i += 1
        after = inside[i:].lstrip()[:1]
        if after not in "{;":
            continue
        ret, name, params = " ".join(m.group(1).split()), m.group(2), " ".join(inside[m.end():i - 1].split())
        names = [name]
        if name.startswith("GTE_HOT_NAME("):
            names = [name[13:-1], name[13:-1] + "_nt"]
        for n in names:
            assert n not in out, f"{n} appears twice"
            out[n] = (f"{ret} {n}({params})", after == "{")
    return out


def test_every_struct_under_csrc_is_defined_in_exactly_one_file():
    """A struct that crosses a translation-unit boundary by value (RolloutArgs, StateSoA, LogPack:
    kernel arguments) has ONE body, in gte_launch.h: with a copy per file, a member added on one side
    still links and the kernel reads garbage."""
    seen = {}
    for name, src in _csrc_sources().items():
        for s in re.findall(r"^\s*struct\s+(?:alignas\(\d+\)\s+)?(\w+)\s*\{", src, re.M):
            seen.setdefault(s, []).append(name)
    assert {"RolloutArgs", "StateSoA", "LogPack", "Params", "EnvRec", "LaunchPlan"} <= set(seen)
    assert {s: f for s, f in seen.items() if len(f) != 1} == {}
    for s in ("RolloutArgs", "StateSoA", "LogPack"):
        assert seen[s] == ["gte_launch.h"]
    for s in ("LaunchPlan", "Shape", "Knobs", "Chip"):  # the planner's (tests/plan_check.cpp compiles them with g++)
        assert seen[s] == ["gte_plan.h"]


def _host_units():
    """the host side's translation units: the gte_api*.hip of the Makefile's SRCS (gte_comm.hip, which holds the
    RCCL wrappers of `namespace gte` as well as its entry points, is added where a test says so)"""
    units = [u for u in _makefile_srcs() if re.fullmatch(r"gte_api\w*\.hip", u)]
    assert units == ["gte_api.hip", "gte_api_backtest.hip", "gte_api_leaderboard.hip", "gte_api_read.hip"], units
    return units


def _host_files():
    return _host_units() + ["gte_host.h"]


_DEFINITION = re.compile(r"^(?![ \t#}/])(?!(?:struct|namespace|extern|using|typedef|enum|static_assert|template)\b)"
                         r"[^\n;{}()=]*?\b(\w+)\(", re.M)


def _defined_functions(text):
    """names of the functions defined at column 0 (static or not, in a namespace block or an extern "C" block or
    outside): `... name(params) {`, the head on one line as everywhere in csrc/"""
    out = []
    for m in _DEFINITION.finditer(text):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        if text[i:].lstrip()[:1] == "{":
            out.append(m.group(1))
    return out


def test_gte_api_declares_no_gte_function_itself():
    """The host side takes every kernel-side prototype from gte_launch.h, through gte_host.h: no host unit opens a
    `namespace gte` or has a function declaration at file scope (the hand-copied block gte_api.hip had was checked
    against nothing).  The only prototypes of the host side are those of `namespace gte_host` in gte_host.h."""
    src = _csrc_sources()
    assert '#include "gte_launch.h"' in src["gte_host.h"]
    assert '#include "gte_host.h"' in src["gte_comm.hip"]
    for name in _host_files():
        text = src[name]
        assert name == "gte_host.h" or '#include "gte_host.h"' in text, name
        assert not re.search(r"namespace gte\b", text), name  # (`namespace gte_host` is another word)
        protos = re.findall(r"^(?!static_assert)[A-Za-z_][^\n;{}]*\([^;{}]*\)\s*;",
                            _outside_namespace(text, "gte_host"), re.M)
        assert protos == [], (name, protos)
        assert _signatures(text) == {}, name
        if name != "gte_host.h":  # a unit defines gte_host functions, it declares none
            assert all(is_def for _, is_def in _signatures(text, "gte_host").values()), name


def test_host_functions_that_cross_units_are_declared_once_in_gte_host_h():
    """Every function of `namespace gte_host` is declared in gte_host.h and defined in exactly one unit with the
    same signature, parameter names included (the reader of the gte_launch.h test, told the namespace)."""
    src = _csrc_sources()
    declared = _signatures(src["gte_host.h"], "gte_host")
    assert not any(is_def for _, is_def in declared.values())
    assert sorted(declared) == ["backtest_entry", "fail", "launch_lookup", "publish_period_row", "publish_signal_table",
                                "trade_list_on"]
    defined = {}
    for name in _host_units() + ["gte_comm.hip"]:
        for fn, (sig, is_def) in _signatures(src[name], "gte_host").items():
            assert is_def, f"{name} declares {fn} itself"
            assert fn not in defined, f"{fn} is defined in {name} and in {defined[fn]}"
            defined[fn] = name
            assert fn in declared, f"{name}: {fn} is not declared in gte_host.h"
            assert declared[fn][0] == sig, f"{name}: {sig}  !=  {declared[fn][0]}"
    assert sorted(declared) == sorted(defined), "gte_host.h declares a function no unit defines"
    # the step path stays within one unit, backtest()'s per-step loop with it: nothing that launches a step per
    # call crosses a unit boundary (enqueue_step and what it needs are static there, as they always were)
    assert defined["fail"] == defined["backtest_entry"] == "gte_api.hip"
    for fn in ("enqueue_step", "own_targets", "age_order", "report_rollout_path", "backtest"):
        assert re.search(rf"^static [^\n]*\b{fn}\(", src["gte_api.hip"], re.M), fn
    assert src["gte_api.hip"].count("thread_local") == 1 and "extern thread_local std::string g_err;" in src["gte_host.h"]
    for name in _host_units()[1:] + ["gte_comm.hip"]:  # ONE error string: no unit has a thread-local of its own
        assert "thread_local" not in src[name], name


def test_no_host_function_is_defined_twice_and_every_entry_point_once():
    """Copying a helper into a second unit is how the copies come back: no function name is defined, static or
    not, in two files of the host side.  Every gte_* function of include/gte.h and include/gte_mc.h is defined at
    column 0 in exactly one unit; struct gte_env has one body, in gte_host.h."""
    src = _csrc_sources()
    where = {}
    for name in _host_files() + ["gte_comm.hip"]:
        for fn in set(_defined_functions(src[name])):
            where.setdefault(fn, []).append(name)
    assert len(where) >= 150 and where["dev_alloc"] == ["gte_host.h"] and where["backtest"] == ["gte_api.hip"]
    assert {fn: files for fn, files in where.items() if len(files) != 1} == {}
    entry_points = _declared_functions()
    assert len(entry_points) >= 70
    for fn in entry_points:
        units = [u for u in _makefile_srcs() if re.search(rf"^[A-Za-z_][\w \*]*[ \*]{fn}\(", src[u], re.M)
                 and fn in _defined_functions(src[u])]
        assert len(units) == 1, (fn, units)
        assert units[0] in _host_units() + ["gte_comm.hip"], (fn, units)
    assert [n for n, t in src.items() if re.search(r"^\s*struct\s+gte_env\s*\{", t, re.M)] == ["gte_host.h"]


def test_replaceable_memory_has_one_owner_type_and_gte_destroy_names_no_feature():
    """hipMalloc, hipFree, hipHostMalloc and hipHostFree are called in gte_host.h only (dev_alloc, the
    allocate-and-report step and the HIP bindings of gte_own.h's owner), and gte_destroy names no member of a
    feature struct: a buffer the env may replace is an owner inside its feature's struct, released by `delete E`,
    so a feature cannot forget its line there."""
    src = _csrc_sources()
    for name in _host_units() + ["gte_comm.hip"]:
        for call in ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree("):
            assert call not in src[name], (name, call)
    for call in ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree("):
        assert call in src["gte_host.h"], call
    env = re.search(r"^struct gte_env \{\n(.*?)^\};", src["gte_host.h"], re.M | re.S).group(1)
    features = re.findall(r"^  (\w+State) (\w+);", env, re.M)
    assert [m for _, m in features] == ["backtest", "trades", "periods", "signals", "rank", "comm", "readback"]
    for struct, _ in features:
        assert re.search(rf"^struct {struct} \{{", src["gte_host.h"], re.M), struct
    body = re.search(r"^void gte_destroy\(gte_env\* E\) \{\n(.*?)^\}", src["gte_api.hip"], re.M | re.S).group(1)
    for _, member in features:
        assert not re.search(rf"E->{member}\b", body), member
    for owner in re.findall(r"\b(?:DeviceBlock|PinnedBlock)>? ([^;]+);", env):  # the owners gte_env holds flat
        for member in re.findall(r"\w+", re.sub(r"\[\d+\]", "", owner)):
            assert member not in body, member
    for kept in ("hipSetDevice(", "gte_comm_destroy(E)", "E->allocs", "hipEventDestroy(", "hipStreamDestroy(",
                 "ledger().forget(E)", "delete E;"):
        assert kept in body, kept
    assert body.count("hipStreamSynchronize(") == 2


def test_error_channel_is_one_string_for_every_host_unit():
    """fail() is defined in gte_api.hip and called from five units: the message of a refusal in any of them is what
    gte_last_error() returns.  One entry point per unit whose first check is the NULL env; none touches a device."""
    lib = _abi.load_library()
    calls = (  # unit, call, message
        ("gte_api.hip", lambda: lib.gte_step(None, None, 0), "env is NULL"),
        ("gte_api_backtest.hip", lambda: lib.gte_backtest(None, None, 1, 0, None), "env is NULL"),
        ("gte_api_leaderboard.hip", lambda: lib.gte_cscv(None, None, 1, 1, None, 2, None, None, 1, 0, None), "env is NULL"),
        ("gte_api_read.hip", lambda: lib.gte_get_log(None, None), "NULL argument"),
        ("gte_comm.hip", lambda: lib.gte_comm_init(None, None, 0, 1), "NULL argument"),
    )
    src = _csrc_sources()
    for (unit, call, message), fn in zip(calls, ("gte_step", "gte_backtest", "gte_cscv", "gte_get_log", "gte_comm_init")):
        assert fn in _defined_functions(src[unit]), (unit, fn)
    for unit, call, message in calls:
        # first the OTHER message, through gte_api.hip (whose unit gte_last_error reads): a unit that wrote to a
        # string of its own would leave this one in place
        if message == "env is NULL":
            assert lib.gte_get_schedule(None, None) == _abi.GTE_ERR_INVALID
        else:
            assert lib.gte_synchronize(None) == _abi.GTE_ERR_INVALID
        assert lib.gte_last_error().decode() in ("env is NULL", "NULL argument")
        assert lib.gte_last_error().decode() != message
        assert call() == _abi.GTE_ERR_INVALID, unit
        assert lib.gte_last_error().decode() == message, (unit, lib.gte_last_error())


def test_gte_api_keeps_no_ledger_of_its_own():
    """What a sparse flag store and a slide step rely on is proved in gte_ledger.h, behind its mutex: the
    host side keeps no lock and no validity bit of its own."""
    read = lambda f: open(os.path.join(ROOT, "gym-trading-env_amd", "csrc", f)).read()
    assert '#include "gte_ledger.h"' in read("gte_host.h")
    for name in _host_files() + ["gte_comm.hip"]:
        for gone in ("std::mutex", "lock_guard", "flags_sparse_ok", "slide_valid"):
            assert gone not in read(name), (name, gone)


def test_gte_api_plans_nothing_itself():
    """The launch rules are in gte_plan.h, fed with values: the host side asks the device for its properties once,
    in require_device (whose CU count the planner's Chip hands on), reads the planner's environment switches only
    where it fills Knobs (debug_geometry / read_knobs), and stands no placeholder pointer in for a Shape bool.
    Counted over all host units and gte_host.h together."""
    api = "\n".join(_csrc_sources()[name] for name in _host_files())
    once = api.split("static int require_device(")[1].split("\n}\n")[0]
    assert once.count("hipGetDeviceProperties") == 1 and api.count("hipGetDeviceProperties") == 1
    assert "multiProcessorCount <= 0" in once  # gte_create refuses a device without compute units
    knobs = api.split("static bool debug_geometry()")[1].split("static gte_plan::Knobs read_knobs(")[1].split("\n}\n")[0]
    names = ("GTE_SLIDE_FULL_WINDOWS", "GTE_SLIDE_AB", "GTE_SLIDE_STORE", "GTE_AFFINITY_BINS", "GTE_RESIDENT_EPB")
    for name in names:
        assert knobs.count(f'getenv("{name}")') == 1 and api.count(f'"{name}"') == 1, name
    assert api.count('"GTE_DEBUG_GEOMETRY"') == 1
    assert 'static bool debug_geometry() { return getenv("GTE_DEBUG_GEOMETRY") != nullptr; }' in api
    assert "(float*)(uintptr_t)16" not in api and "uintptr_t)16" not in api
    for rule in ("step_geometry", "slide_store_policy", "setup_affinity", "choose_resident_epb(gte_env",
                 "choose_rollout_epw(gte_env"):
        assert f"static void {rule}" not in api and f"static int {rule}" not in api, rule
    plan = _csrc_sources()["gte_plan.h"]  # (comments removed)
    assert "getenv" not in plan and "hipGetDeviceProperties" not in plan


def _makefile_srcs():
    makefile = open(os.path.join(ROOT, "gym-trading-env_amd", "csrc", "Makefile")).read()
    return re.search(r"^SRCS = (.*)$", makefile, re.M).group(1).split()


def _included(src, name):
    """every file of csrc/ that `name` includes, directly or through another"""
    seen, todo = set(), [name]
    while todo:
        for inc in re.findall(r'^#include "([^"/]+)"', src[todo.pop()], re.M):
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    return seen


def test_device_code_is_shared_through_headers_only():
    """No translation unit doubles as the header of another: nothing includes a .hip, every .hip under
    csrc/ is a unit the Makefile builds, and the macro that fenced gte_kernels.hip's own kernels off from
    an including file is gone with the include."""
    csrc = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
    texts = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc))
             if n.endswith((".hip", ".h")) or n == "Makefile"}
    for name, text in texts.items():
        assert not re.search(r'#\s*include\s*"[^"]*\.hip"', text), f"{name} includes a .hip file"
        assert "GTE_PHASE_A_ONLY" not in text, name
    assert sorted(n for n in texts if n.endswith(".hip")) == sorted(_makefile_srcs())


def test_cross_file_functions_are_declared_once_in_gte_launch_h():
    """Every non-static gte:: function a translation unit of the Makefile's SRCS defines (itself, or in a
    header that holds its body: gte_hot_body.h) is declared in gte_launch.h with the same signature —
    and the defining file includes that header (directly or through another), so the compiler checks
    the return type as well."""
    src = _csrc_sources()
    declared = _signatures(src["gte_launch.h"])
    assert len(declared) >= 30 and not any(is_def for _, is_def in declared.values())
    units = [u for u in _makefile_srcs() if u not in _host_units()]  # (the host units: the gte_host.h tests)
    assert "gte_backtest.hip" in units and "gte_hot_nt.hip" in units and len(units) >= 7
    # gte_hot.hip and gte_hot_nt.hip compile one body under two names: GTE_HOT_NAME(x) = x and x_nt
    assert [u for u in units if "gte_hot_body.h" in _included(src, u)] == ["gte_hot.hip", "gte_hot_nt.hip"]
    assert "#define GTE_HOT_NAME(x) x\n" in src["gte_hot.hip"] and "#define GTE_HOT_NAME(x) x##_nt\n" in src["gte_hot_nt.hip"]
    assert not any(d.endswith(".hip") for d in src if d not in _makefile_srcs())
    defined = {}
    for name in units + sorted(h for h in src if h.endswith(".h") and h not in ("gte_launch.h", "gte_host.h")):
        text = src[name]
        # (gte_ledger.h and gte_own.h: host bookkeeping only, no device code and no cross-file gte:: function;
        # gte_members.h: forceinline and inline rules only, compiled for the host by tests/test_strategy_records_cpu.py)
        no_launch_h = ("gte_device.h", "gte_ledger.h", "gte_plan.h", "gte_members.h", "gte_own.h")
        assert name in no_launch_h or "gte_launch.h" in _included(src, name), name
        for fn, (sig, is_def) in _signatures(text).items():
            assert is_def, f"{name} declares {fn} itself"
            assert fn not in defined, f"{fn} is defined in {name} and in {defined[fn]}"
            defined[fn] = name
            assert fn in declared, f"{name}: {fn} is not declared in gte_launch.h"
            assert declared[fn][0] == sig, f"{name}: {sig}  !=  {declared[fn][0]}"
    assert "launch_step_hot_nt" in defined and "rccl_load" in defined and "launch_pack_log" in defined
    assert defined["launch_step_hot"] == defined["hot_blocks_per_cu_nt"] == "gte_hot_body.h"
    for fn in ("launch_backtest_begin", "launch_backtest_summary", "launch_backtest_fold",
               "launch_signal_actions", "launch_signal_summary"):
        assert defined.get(fn) == "gte_backtest.hip", fn
        assert f"gte::{fn}(" in src["gte_api.hip"], fn  # (backtest() and launch_lookup: the unit of enqueue_step)
    assert sorted(declared) == sorted(defined), "gte_launch.h declares a function no file defines"
    # gte_backtest.hip runs phase A with the terminal-record store compiled in
    assert "#define GTE_HOT_ONLY" not in src["gte_backtest.hip"]
    makefile = open(os.path.join(ROOT, "gym-trading-env_amd", "csrc", "Makefile")).read()
    hdrs = re.search(r"^HDRS = (.*)$", makefile, re.M).group(1).split()
    assert sorted(h for h in src if h.endswith(".h")) == sorted(h for h in hdrs if "/" not in h)
    # the ledger, the planner and the owner type stand alone (tests/ledger_check.cpp, tests/plan_check.cpp and
    # tests/own_check.cpp compile them with g++): nothing of csrc/, nothing of HIP; the planner takes include/gte.h
    # for the GTE_KV_* names
    for alone, own in (("gte_ledger.h", ()), ("gte_plan.h", ('"../../include/gte.h"',)), ("gte_own.h", ())):
        includes = re.findall(r'#\s*include\s*([<"][^>"]+[>"])', src[alone])
        assert includes and not any((i.startswith('"') and i not in own) or "hip" in i.lower() for i in includes), includes
        assert "__global__" not in src[alone] and "__device__" not in src[alone]
        assert alone in hdrs
    # the limits the kernels share with the planner have one definition each, in gte_plan.h
    for const in ("LEAN_MAX_ROWS", "ROLLOUT_WAVES", "RES_NEW", "RES_OWNERS", "RES_LDS_MAX"):
        assert [n for n, t in src.items() if re.search(rf"constexpr \w+ {const}\b", t)] == ["gte_plan.h"], const
    for macro in ("GTE_WAVES", "GTE_LEAN_U"):
        assert [n for n, t in src.items() if re.search(rf"#\s*define {macro}\b", t)] == ["gte_plan.h"], macro


def test_the_fused_backtest_step_is_written_once():
    """The from-registers backtest kernels (three action sources x three trackers) are one body, summary_body() of
    gte_summary_body.h, called with two policies — with ONE hand-written exception, gte_backtest_exit_kernel in
    gte_exits.hip, which measured about 1 % slower through the shared body ("One body for the nine fused
    backtest kernels").  So the fused step exists twice, in the header and in that kernel, and nowhere else: a
    further hand-copied kernel fails here before anything runs.  (gte_exit_actions_kernel, the lookup outside a
    fused launch, has an exit_decide of its own.)"""
    src = _csrc_sources()
    units = ("gte_backtest.hip", "gte_exits.hip", "gte_trades.hip", "gte_periods.hip")
    body = "gte_summary_body.h"
    count = lambda needle: {n: src[n].count(needle) for n in units + (body,) if needle in src[n]}
    kernel = lambda name: re.search(rf"void {name}\(.*?\n\}}\n", src["gte_exits.hip"], re.S).group(0)
    by_hand = kernel("gte_backtest_exit_kernel")
    assert count("phase_a<MODE_STEP>(") == {body: 1, "gte_exits.hip": 1} and by_hand.count("phase_a<MODE_STEP>(") == 1
    assert count("exit_decide(") == {body: 1, "gte_exits.hip": 2}
    assert by_hand.count("exit_decide(") == 1 and kernel("gte_exit_actions_kernel").count("exit_decide(") == 1
    # the other eight kernels are calls of the body, in the files they always had
    assert count("summary_body(") == {body: 1, "gte_backtest.hip": 2, "gte_trades.hip": 3, "gte_periods.hip": 3}
    csrc = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
    for name in sorted(os.listdir(csrc)):  # (comments and the Makefile too)
        if os.path.isfile(os.path.join(csrc, name)) and not name.endswith(".so"):
            assert "GTE_SIGNAL_BYTE_LOAD" not in open(os.path.join(csrc, name), errors="replace").read(), name


_HOLDS_VARIANT = re.compile(r"(?i:variant)|^kv$|^DENSE$|^ROLLOUT")  # names of things that hold kernel_variant bits


def _bare_variant_literals(text):
    """(line, value) of every non-zero integer literal of a Python source that stands where a
    kernel_variant is expected.  Such places are recognised by NAME: the value assigned to, or looped
    over by, a name that matches _HOLDS_VARIANT (containers searched throughout: `ROLLOUT_MODES =
    {"gather": (256, True)}`); a keyword argument or a dict entry of such a name; a positional
    argument of a function of the same file whose parameter has such a name; the column of such a
    name in a `parametrize` list; either side of `&` / `|` with such a name or a `KV_*` constant."""
    tree = ast.parse(text)
    ident = lambda n: n.id if isinstance(n, ast.Name) else n.attr if isinstance(n, ast.Attribute) else None
    named = lambda s: isinstance(s, str) and bool(_HOLDS_VARIANT.search(s))
    params = {f.name: [a.arg for a in f.args.args if a.arg not in ("self", "cls")]
              for f in ast.walk(tree) if isinstance(f, ast.FunctionDef)}
    holds = []
    for n in ast.walk(tree):
        if isinstance(n, (ast.Assign, ast.AnnAssign)):
            if any(named(ident(t)) for t in (n.targets if isinstance(n, ast.Assign) else [n.target])):
                holds.append(n.value)
        elif isinstance(n, (ast.For, ast.comprehension)) and named(ident(n.target)):
            holds.append(n.iter)
        elif isinstance(n, ast.Dict):
            holds += [v for k, v in zip(n.keys, n.values) if isinstance(k, ast.Constant) and named(k.value)]
        elif isinstance(n, ast.BinOp) and isinstance(n.op, (ast.BitAnd, ast.BitOr)):
            if any(named(ident(s)) or str(ident(s)).startswith("KV_") for s in (n.left, n.right)):
                holds += [n.left, n.right]
        elif isinstance(n, ast.Call):
            holds += [k.value for k in n.keywords if named(k.arg)]
            holds += [a for a, p in zip(n.args, params.get(ident(n.func), [])) if named(p)]
            if ident(n.func) == "parametrize" and isinstance(n.args[0], ast.Constant) \
                    and isinstance(n.args[1], (ast.List, ast.Tuple)):
                names = [s.strip() for s in n.args[0].value.split(",")]
                for case in n.args[1].elts:
                    row = case.args if isinstance(case, ast.Call) else case.elts if len(names) > 1 else [case]
                    holds += [v for v, s in zip(row, names) if named(s)]
    return sorted({(c.lineno, c.value) for h in holds if h is not None for c in ast.walk(h)
                   if isinstance(c, ast.Constant) and type(c.value) is int and c.value != 0})


def test_kernel_variant_bits_have_one_set_of_names():
    """`_abi.KV_*` mirror `enum gte_kernel_variant` of include/gte.h, and nobody passes or tests a
    bit as a bare number: not plan_create (gte_plan.h), not a test, not a Python tool (see
    _bare_variant_literals for what counts; the forms this project used to write are tried first)."""
    hdr = open(os.path.join(ROOT, "include", "gte.h")).read()
    body = re.search(r"typedef enum gte_kernel_variant \{(.*?)\} gte_kernel_variant;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    enum = {k: int(v) for k, v in re.findall(r"\bGTE_(KV_[A-Z_0-9]+)\s*=\s*(\d+)", body)}
    mirror = {k: v for k, v in vars(_abi).items() if k.startswith("KV_")}
    assert enum == mirror
    assert sorted(enum.values()) == [1, 2, 4, 64, 128, 256, 1024, 2048, 4096, 8192, 16384]
    planner = open(os.path.join(ROOT, "gym-trading-env_amd", "csrc", "gte_plan.h")).read()
    assert planner.count("kernel_variant;") == 1  # (besides the Shape member's declaration, which ends `= 0,`)
    plan = planner.split("inline LaunchPlan plan_create(const Shape& p, const Knobs& k, Chip& chip) {")[1].split("\n}\n")[0]
    assert plan.count("kernel_variant") == 1  # read once, into `kv`; every use of `kv` tests named bits
    uses = re.findall(r"\bkv\b\s*([^\n]{0,10})", re.sub(r"//[^\n]*", "", plan).split("kv = p.kernel_variant;")[1])
    assert len(uses) >= 10 and all(re.match(r"&\s*\(?GTE_KV_", u) for u in uses), uses

    head = "import pytest\n"
    for bad, n in (('_KERNEL_VARIANT = {"variant64": 64, "variant1": 1}', 2), ("DENSE = 16384", 1),
                   ("VARIANTS = [1, 2, 64, 4096, 8192]", 5), ("for variant in (1024, 2048): pass", 2),
                   ('ROLLOUT_MODES = {"resident": (0, True), "gather": (256, True)}', 1),
                   ('@pytest.mark.parametrize("variant,store", [(0, 1), (64, 2), (1 | 2, 1)])\ndef t(): pass', 3),
                   ('@pytest.mark.parametrize("kernel_variant", [0, 1024])\ndef t(): pass', 1),
                   ("Env(kernel_variant=128)", 1), ('kw = {**kw, "kernel_variant": 128}', 1),
                   ("def case(o, kernel_variant): pass\ncase(o, 1024)", 1), ("if kv & 128: pass", 1),
                   ("x = _abi.KV_SHARED_TU | 2", 1)):
        assert len(_bare_variant_literals(head + bad)) == n, bad
    for good in ('@pytest.mark.parametrize("variant,store", [(0, 1), (_abi.KV_SHARED_TU, 2)])\ndef t(): pass',
                 "Env(kernel_variant=_abi.KV_LOG_SEPARATE | _abi.KV_SHARED_TU, envs_per_wave=4)",
                 "def case(o, kernel_variant): pass\ncase(1024, 0)"):
        assert _bare_variant_literals(head + good) == [], good
    for folder in ("tests", "tools"):
        for name in sorted(os.listdir(os.path.join(ROOT, folder))):
            if name.endswith(".py"):
                text = open(os.path.join(ROOT, folder, name)).read()
                assert _bare_variant_literals(text) == [], f"{folder}/{name}"


def test_inline_asm_wide_stores_carry_their_wait_states():
    """A VMEM store of more than 64 bits keeps reading its data VGPRs for a couple of cycles after
    it issues; hipcc pads its own stores but does not look inside inline asm, so an asm
    `global_store_dwordx3/x4` must end with `s_nop 1` INSIDE its string — otherwise the compiler's
    next VALU instruction may overwrite the data before the store has read it (round 3: the lean
    copy loop stored address words in place of x, y until this was added; the generic loop had
    been getting away with it by luck of scheduling)."""
    csrc = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
    found = 0
    for name in os.listdir(csrc):
        if not name.endswith((".hip", ".h")):
            continue
        src = open(os.path.join(csrc, name)).read()
        for m in re.finditer(r'asm\s+volatile\(\s*"([^"]*(?:"\s*"[^"]*)*)"', src):
            text = m.group(1)
            if re.search(r"(global|buffer|flat)_store_dwordx[34]", text):
                found += 1
                assert re.search(r"_store_dwordx[34][^\\]*\\n\\ts_nop 1", text), (name, text)
    assert found >= 1


def test_integration_md_stub_matches_the_abi():
    """The ctypes stub INTEGRATION.md shows a maintainer of the reference is not prose: its
    gte_config must have the fields, order and size of the real one."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    code = text.split("```python")[1].split("```")[0]
    code = code.split('lib = C.CDLL("libgte.so")')[0]  # the struct, not the load
    scope = {}
    exec(compile(code, "INTEGRATION.md", "exec"), scope)  # our own document
    stub = scope["gte_config"]
    assert [f[0] for f in stub._fields_] == [f[0] for f in _abi.GteConfig._fields_]
    assert C.sizeof(stub) == C.sizeof(_abi.GteConfig)
    for (name, a), (_, b) in zip(stub._fields_, _abi.GteConfig._fields_):
        assert C.sizeof(a) == C.sizeof(b), name


def test_stage_dataframe_equals_the_reference_set_df():
    """tests/golden/set_df.npz: what the reference's `_set_df` made of an awkward DataFrame
    (feature columns = name contains 'feature', case-sensitive; the rest is info)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "set_df.npz"), allow_pickle=False)
    cols = [str(c) for c in z["columns"]]
    df = pd.DataFrame(z["values"], columns=cols,
                      index=pd.date_range("2021-03-01", periods=len(z["values"]), freq="h"))
    s = staging.stage_dataframe(df, n_dyn=2)
    assert s.feature_columns == [str(c) for c in z["features_columns"]]
    assert s.n_obs == int(z["nb_features"]) and s.n_static == int(z["nb_static_features"])
    np.testing.assert_array_equal(s.feat, z["obs_array"])
    np.testing.assert_array_equal(s.close, z["price_array"])
    ref_info = [str(c) for c in z["info_columns"]]  # a set difference: order is arbitrary there
    assert sorted(s.info_columns) == sorted(ref_info)
    for j, c in enumerate(ref_info):
        np.testing.assert_array_equal(np.asarray(s.info_array[:, s.info_columns.index(c)], np.float64),
                                      z["info_array"][:, j])


@pytest.mark.parametrize("modern", [True, False])
def test_gymnasium_registration_with_a_stand_in(monkeypatch, modern):
    """register_gymnasium_ids() (the reference's __init__.py:3-14: same ids, same flags) against
    an in-memory stand-in of `gymnasium.envs.registration` — gymnasium itself is not installed
    here.  Gymnasium >= 1.0 also gets a vector entry point (gym.make_vec -> one batched env);
    an older register() without that keyword is called the reference's way."""
    import sys
    import types
    import gym_trading_env_amd as gte
    calls = []

    def register_modern(id, entry_point=None, vector_entry_point=None, disable_env_checker=False,
                        order_enforce=True, **kw):
        calls.append(dict(id=id, entry_point=entry_point, vector_entry_point=vector_entry_point,
                          disable_env_checker=disable_env_checker, order_enforce=order_enforce))

    def register_old(id, entry_point=None, disable_env_checker=False, order_enforce=True):
        calls.append(dict(id=id, entry_point=entry_point, vector_entry_point=None,
                          disable_env_checker=disable_env_checker, order_enforce=order_enforce))

    reg = types.ModuleType("gymnasium.envs.registration")
    reg.register = register_modern if modern else register_old
    reg.registry = {}
    gym = types.ModuleType("gymnasium")
    envs_mod = types.ModuleType("gymnasium.envs")
    envs_mod.registration = reg
    gym.envs = envs_mod
    for name, mod in (("gymnasium", gym), ("gymnasium.envs", envs_mod),
                      ("gymnasium.envs.registration", reg)):
        monkeypatch.setitem(sys.modules, name, mod)
    assert gte.register_gymnasium_ids() is True
    assert [c["id"] for c in calls] == ["TradingEnv", "MultiDatasetTradingEnv"]
    from gym_trading_env_amd import envs
    assert calls[0]["entry_point"] is envs.TradingEnv and calls[1]["entry_point"] is envs.MultiDatasetTradingEnv
    assert all(c["disable_env_checker"] is True and c["order_enforce"] is False for c in calls)
    assert all((c["vector_entry_point"] is not None) == modern for c in calls)


def _build_c_demo(tmp_path):
    import subprocess
    exe = str(tmp_path / "c_abi_demo")
    csrc = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "c_abi_demo.c"), "-L", csrc, "-lgte",
                           f"-Wl,-rpath,{csrc}", "-lm", "-o", exe])
    return exe


def test_c_program_binds_the_abi_and_fails_loudly_without_a_gpu(tmp_path):
    """examples/c_abi_demo.c: a plain C host (gcc, include/gte.h, -lgte; no Python, no torch)
    compiles against the boundary; on a host without a gfx950 device it stops at gte_create with
    GTE_ERR_NO_DEVICE — there is no CPU fallback to fall into."""
    import subprocess
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the C demo runs for real in tests/test_gpu_examples.py")
    exe = _build_c_demo(tmp_path)
    r = subprocess.run([exe, "64", "5"], capture_output=True, text=True)
    assert r.returncode == 3
    assert "no CPU fallback" in r.stderr and "gte_create" in r.stderr
