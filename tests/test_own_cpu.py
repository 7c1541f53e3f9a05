"""csrc/gte_own.h on the CPU: tests/own_check.cpp (its own main) binds the owner of a replaceable block to
malloc / free plus a counter and checks by count that a block is released exactly once, and that the three growth
rules give the sizes the host units always allocated.  Built with g++ against the header alone under ASan + UBSan
and run as a child process: nothing is loaded into Python and no GPU is touched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "own_check.cpp")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    # (the sanitizer's runtime is linked into the program itself, as in test_ledger_cpu.py)
    out = str(tmp_path_factory.mktemp("own") / "own_check_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SOURCE, "-o", out],
                   check=True, cwd=ROOT)
    return out


def _run(binary, *args):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    return subprocess.run([binary, *args], capture_output=True, text=True, env=env, timeout=120)


def test_owner_releases_every_block_exactly_once_and_grows_by_the_three_rules(binary):
    """replace releases the old block once and adopts the new one; reset on an empty owner and a second reset
    release nothing; the destructor releases a held block; a moved-from owner releases nothing; exact,
    need + need / 2 and max(need, 2 * have) at (0, 1), (100, 100), (100, 101), (100, 250).  No report of ASan, UBSan
    or LeakSanitizer: a block the type forgot would be one."""
    r = _run(binary)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "owner ok" in r.stdout and "growth ok" in r.stdout, r.stdout


def test_a_block_nobody_releases_is_reported(binary):
    """The clean run above proves something only if a forgotten block is seen: `leak` forgets one on purpose."""
    r = _run(binary, "leak")
    assert "leaked one block" in r.stdout
    assert r.returncode != 0 and "LeakSanitizer" in r.stderr, (r.returncode, r.stderr[-2000:])
