"""csrc/gte_plan.h on the CPU: tests/plan_check.cpp (its own main) replays every plan recorded in
tests/golden/launch_plans.json against a Chip that answers from the recording, and checks what the rules guarantee
over a few thousand fixed-seed shapes with a synthetic Chip.  Built with g++ against the header alone, under
ASan + UBSan, and run as a child process: nothing is loaded into Python and no GPU is touched."""
import json
import os
import re
import subprocess

import pytest

from gym_trading_env_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "plan_check.cpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_plans.json")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    # (the sanitizers' runtimes are linked statically, for the reason test_ledger_cpu.py gives)
    out = str(tmp_path_factory.mktemp("plan") / "plan_check_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SOURCE, "-o", out],
                   check=True, cwd=ROOT)
    return out


def _run(binary, *args):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([binary, *args], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def rows():
    """the fixture's rows in full (it keeps what differs from `base` and names chip questions and plans by index)"""
    fx = json.load(open(FIXTURE))
    return [dict(r, shape={**fx["base"]["shape"], **r["shape"]}, knobs={**fx["base"]["knobs"], **r["knobs"]},
                 events=[{"when": e["when"], "chip": fx["chips"][e["chip"]], "plan": fx["plans"][e["plan"]]}
                         for e in r["events"]]) for r in fx["rows"]]


def test_the_planner_replays_every_recorded_plan(binary, rows):
    out = _run(binary, "replay", FIXTURE)
    assert re.findall(r"^replayed (\S+)$", out, re.M) == [r["name"] for r in rows]
    assert f"replay ok: {len(rows)} rows" in out


def test_what_the_rules_guarantee_over_random_shapes(binary):
    out = _run(binary, "model")
    assert "model ok" in out
    counts = dict(zip(*[iter(re.search(r"^shapes (.*)$", out, re.M).group(0).split())] * 2))
    print(counts)
    # (no empty exercise: every kind of plan the asserts are about occurs in numbers)
    assert int(counts["shapes"]) >= 2000
    for kind in ("slid", "lean", "ordered", "resident"):
        assert int(counts[kind]) >= 50, counts


def _ceil(a, b):
    return -(-a // b)


def _branches(row):
    """The branches of plan_create a row went through, told from its Shape, its recorded chip answers and its
    recorded plan (not from the planner)."""
    s, ev = row["shape"], row["events"][0]
    assert ev["when"] == "create"
    p, chip = ev["plan"], ev["chip"]
    out = {f"stage {p['stage']}", f"store {p['store']}", f"slide_store {p['slide_store']}"}
    vpe = s["W"] * s["Fobs"] // p["vec"]
    searched = s["envs_per_wave"] == 0 and any(q[0] == "hot_per_cu" for q in chip[:3])
    if searched and p["hot_per_cu"] > 0:
        n_cu = chip[0][-1]
        busiest = _ceil(p["blocks"], n_cu)
        lean_epw = [c for c in range(1, 17) if c * vpe % 256 == 0 and c * s["W"] <= 512]
        if busiest <= p["hot_per_cu"] and busiest * 4 >= 16:
            out.add("one round")
        elif s["kernel_variant"] & _abi.KV_GENERIC_COPY or not lean_epw:
            out.add("streaming")
        else:
            out.add("lean")
            c = lean_epw[0]
            while c * 2 <= 16 and c * vpe < 1280 and c * 2 * s["W"] <= 512:
                c *= 2
            if s["N"] >= 200000 and p["epw"] == 2 * c:
                out.add("lean doubled")
    e = s["envs_per_wave"]
    if e and e * vpe > 1 << 20 and p["epw"] < e:
        out.add("shrunk for the index range")
    while e > 1 and e * vpe > 1 << 20:
        e >>= 1
    if e and e * 4 * s["W"] * max(s["nd"], 1) * 4 > 32 * 1024 and p["epw"] < e:
        out.add("shrunk for LDS")
    for later in row["events"][1:]:
        out |= {"resident_epb > 0" for v in later["plan"]["resident_epb"] if v > 0}
        out |= {"resident_epb -1" for v in later["plan"]["resident_epb"] if v == -1}
        if later["when"] == "finalize" and later["plan"]["affinity_period"] != p["affinity_period"]:
            out.add("order off after the upload")
    return out


def test_the_fixture_reaches_every_branch(rows):
    reached = {}
    for row in rows:
        for b in _branches(row):
            reached.setdefault(b, []).append(row["name"])
    print({b: len(v) for b, v in sorted(reached.items())})
    need = ["one round", "streaming", "lean", "lean doubled", "shrunk for the index range", "shrunk for LDS",
            "stage 0", "stage 1", "stage 2", "store 0", "store 1", "store 2", "slide_store 0", "slide_store 1",
            "slide_store 2", "resident_epb > 0", "resident_epb -1", "order off after the upload"]
    assert [b for b in need if b not in reached] == []
    # (the table of tools/record_launch_plans.py has 64 rows)
    assert len(rows) >= 60 and os.path.getsize(FIXTURE) < 128 * 1024
