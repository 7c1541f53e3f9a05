"""csrc/gte_ledger.h on the CPU: tests/ledger_check.cpp (its own main) drives the ledger and a byte-by-byte
model of a 256-byte address space together and asserts soundness after every operation, liveness on
scripted sequences.  Built with g++ against the header alone, under ASan + UBSan and once under TSan, and run
as a child process: nothing is loaded into Python and no GPU is touched."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-trading-env_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "ledger_check.cpp")


def _build(out, sanitizers):
    # The sanitizer's runtime is linked into the program itself.  A dynamically linked ASan runtime refuses to
    # start ("does not come first in initial library list") wherever the environment preloads any library of
    # its own into every process, and this test neither sets nor clears LD_PRELOAD; the static archives come
    # with the compiler's sanitizer packages.
    static = [f"-static-lib{s}" for s in {"address,undefined": ("asan", "ubsan"), "thread": ("tsan",)}[sanitizers]]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", f"-fsanitize={sanitizers}", *static, "-Wall", "-Wextra",
                    "-Werror", "-pthread", "-I", CSRC, SOURCE, "-o", out], check=True, cwd=ROOT)
    return out


def _run(binary, mode):
    # (any report is fatal, so that the exit status alone tells)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1:exitcode=66")
    r = subprocess.run([binary, mode], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def asan_binary(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("ledger") / "ledger_check_asan"), "address,undefined")


def test_ledger_is_sound_and_live_against_the_byte_model(asan_binary):
    """Soundness after every operation of the fixed-seed random sequences (3 envs, overlapping and disjoint
    buffers, every entry point of the table in gte_ledger.h), liveness on the scripted ones; and the random
    sequences are no empty exercise: at least one step query in five is granted, for each kind."""
    out = _run(asan_binary, "model")
    assert "scripted ok" in out and "model ok" in out, out
    for kind in ("flags", "window"):
        granted, asked = map(int, re.search(rf"^{kind} granted (\d+) / asked (\d+)$", out, re.M).groups())
        print(f"{kind}: {granted} of {asked} step queries granted")
        assert asked >= 1000 and 5 * granted >= asked, (kind, granted, asked)


def test_ledger_threads_under_asan(asan_binary):
    assert "threads ok" in _run(asan_binary, "threads")


def test_ledger_is_race_free_under_tsan(tmp_path):
    """4 threads, an env each, overlapping ranges, the process-wide ledger: TSan reports nothing."""
    binary = _build(str(tmp_path / "ledger_check_tsan"), "thread")
    assert "threads ok" in _run(binary, "threads")
