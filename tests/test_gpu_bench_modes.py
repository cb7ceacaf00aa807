"""GPU (-m gpu): bench.py's two modes, each in a fresh child process.  A plain run prints the headline and its roofline and
nothing that takes runs of its own; ``--full`` adds the CPU baseline and the end-to-end cycles (the other configs run at the
headline's shape only, which this small shape is not).  The numbers mean nothing."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "2", "--warmup", "1", "--verts", "20000", "--frames", "256", "--comps", "32"]


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SMALL, *extra], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-4000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "snapshots/s" and d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["steps"] == 2 and d["warmup"] == 1 and d["config"]["K"] == 32
    assert "step" in d["roofline"]
    return d


def test_plain_run_prints_the_headline_only():
    d = _bench()
    assert not {"cpu_baseline", "end_to_end", "other_configs"} & set(d)


def test_full_run_adds_baseline_and_end_to_end():
    d = _bench("--full", "--cpu-budget", "1")
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["unit"] == "snapshots/s"
    e = d["end_to_end"]
    assert e["total_ms"] > 0 and e["cold"]["basis_download_ms"] > 0 and e["basis_bytes"] == 32 * 20000 * 3 * 8
    assert "other_configs" not in d
