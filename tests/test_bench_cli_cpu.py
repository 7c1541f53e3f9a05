"""bench.py's command line, as far as it can be checked without a GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv],
                          capture_output=True, text=True, timeout=300)


def test_full_is_an_option():
    r = _bench("--help")
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout


def test_plain_run_starts_no_counter_passes():
    """A plain run goes straight to the GPU: no rocprofv3 child pass is attempted in front of it
    (without a GPU each would fail and say so before the run itself refuses to start)."""
    r = _bench("--gpus", "1", "--steps", "1", "--warmup", "0")
    assert "live PMC pass" not in r.stderr
    if r.returncode != 0:  # no GPU on this host: there is no CPU fallback
        assert "bench.py needs an MI355X" in r.stderr
        assert '{"metric"' not in r.stdout
