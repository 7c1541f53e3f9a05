"""bench.py as a command: a plain run does only what its headline figure needs, everything
else it measures sits behind --full."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 20, 5
HEADLINE = {"metric": "env-steps/sec", "unit": "env-steps/s", "higher_is_better": True, "dtype": "f64"}


def _bench(*extra, timeout):
    """One bench.py run in a new process -> (its JSON line, seconds from start to exit)."""
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", str(STEPS), "--warmup", str(WARMUP), *extra],
                       capture_output=True, text=True, timeout=timeout)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    for k, v in HEADLINE.items():
        assert out[k] == v
    assert out["steps"] == STEPS and out["warmup"] == WARMUP
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(out["config"]["envs_per_gpu"] / (out["ms_per_step"] * 1e-3))
    return out, wall


def test_plain_run_is_lean(tmp_path):
    """Set-up, warm-up, the timed steps, --dump-outputs and the line, nothing else: no CPU
    baseline, no second size, no counter passes of its own, and at most 30 s from start to exit
    outside its (steps + warmup) x ms_per_step."""
    out, wall = _bench("--dump-outputs", str(tmp_path / "dump"), timeout=300)
    outside = wall - (STEPS + WARMUP) * out["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.1f} s from start to exit, {outside:.1f} s outside its steps")
    assert out["full"] is False
    assert "cpu_baseline" not in out
    assert "hbm_regime" not in out["roofline"]
    assert not str(out["roofline"].get("traffic_source", "recorded")).startswith("live")
    assert out["roofline"]["kernel_us_per_launch"] > 0
    assert out["config"]["episodes_finished"] > 0
    for name in ("obs", "reward", "terminated", "truncated", "env_ids", "info_idx"):
        assert (tmp_path / "dump" / (name + ".npy")).exists()
    assert outside <= 30.0


def test_full_run_keeps_every_other_measurement():
    """--full: the CPU baseline and the 262 144-env leg are measured and reported as before, the
    headline fields mean the same, and the run ends well within 10 minutes."""
    out, wall = _bench("--full", timeout=600)
    print(f"--full run: {wall:.1f} s from start to exit")
    assert out["full"] is True
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["unit"] == "env-steps/s"
    hbm = out["roofline"]["hbm_regime"]
    assert hbm["envs"] == 262_144 and hbm["env_steps_per_s"] > 0
    assert wall < 600
