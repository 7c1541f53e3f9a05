"""The library's launch plans against tests/golden/launch_plans.json: every row of the fixture is created through
the C ABI with GTE_DEBUG_GEOMETRY set (and, up to 65 536 envs, taken through upload, reset and its rollout, as
tools/record_launch_plans.py does), and the `[gte] plan:` and `[gte] chip:` lines it prints equal the recorded
ones.  A changed chip answer means the kernels' resource use moved; a changed plan, that a rule did: either way
the fixture is re-recorded on purpose.  Needs an MI355X.
"""
import ctypes as C
import importlib.util
import os

import pytest

from gym_trading_env_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_launch_plans", os.path.join(ROOT, "tools", "record_launch_plans.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)
FIXTURE = {r["name"]: r for r in rec.load_fixture()}


def test_the_fixture_holds_the_recorders_table():
    assert list(FIXTURE) == list(rec.rows())
    for name, over in rec.rows().items():
        shape, knobs = rec.shape_and_knobs(over)
        assert (FIXTURE[name]["shape"], FIXTURE[name]["knobs"]) == (shape, knobs), name


@pytest.mark.parametrize("name", list(FIXTURE))
def test_plan_and_chip_answers_equal_the_fixture(name, capfd):
    lib = _abi.load_library()
    row, over = FIXTURE[name], rec.rows()[name]
    full = row["shape"]["N"] <= 65536  # (beyond that: create alone, which allocates no observation buffer)
    info = {}

    def launch_info(E):
        v = [C.c_int32() for _ in range(4)]
        _abi.check(lib, lib.gte_get_launch_info(E, *[C.byref(x) for x in v]))
        info.update(zip(("epw", "threads", "blocks", "vector_bytes"), (x.value for x in v)))

    capfd.readouterr()
    rec.run_row(lib, over, full=full, inspect=launch_info)
    events = rec.parse(capfd.readouterr().err)
    want = row["events"] if full else row["events"][:1]
    assert [e["when"] for e in events] == [e["when"] for e in want]
    for got, exp in zip(events, want):
        assert got["plan"] == exp["plan"], (name, got["when"])
        assert got["chip"] == exp["chip"], (name, got["when"])
    # gte_get_launch_info, as batched.py's launch_info() decodes it, agrees with the printed plan
    p = events[0]["plan"]
    assert (info["epw"], info["threads"], info["blocks"]) == (p["epw"], p["threads"], p["blocks"])
    assert info["vector_bytes"] == p["vec"] * 4 + 1000 * (p["coop"] + 2 * p["stage"] + 16 * p["store"] +
                                                        64 * (p["hot_per_cu"] & 15) + 1024 * p["store"])
