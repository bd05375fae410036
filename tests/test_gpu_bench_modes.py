"""bench.py with and without --full on cuda:0.

A plain run (`--gpus 1 --steps N --warmup W`) sets up, warms up, times its steps, writes --dump-outputs and prints its
line: no serialised roofline, power, host-fed, exact-f32, PMC, rehearsal or CPU pass.  `--full` runs those passes
(here all but the PMC children, the rehearsal and the CPU baseline, which take minutes) and reports them in the line."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

EXTRA_PASS_LOGS = ("serialised roofline pass", "power pass", "host-fed pass", "exact-f32 pass", "pmc:", "cpu baseline")


def _bench(tmp_path, *extra):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--details", str(tmp_path / "details.json"), *extra],
                       capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    logs = [ln for ln in r.stderr.splitlines() if ln.startswith("[bench +")]
    return json.loads(lines[0]), logs


def test_plain_run_is_the_headline_pass_alone(tmp_path):
    d, logs = _bench(tmp_path, "--dump-outputs", str(tmp_path / "out"))
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 5 and d["warmup"] == 2 and d["dtype"] == "f16x3"
    assert d["roofline"] is None and d["value_exact_f32"] is None and d["value_host_fed"] is None
    assert d["cpu_baseline"] is None and "power" not in d and "host_rehearsal" not in d
    assert not [ln for ln in logs if any(m in ln for m in EXTRA_PASS_LOGS)], logs
    assert (tmp_path / "out" / "segmentation.npy").exists() and (tmp_path / "out" / "embeddings.npy").exists()


def test_full_run_reports_the_other_passes(tmp_path):
    d, logs = _bench(tmp_path, "--full", "--pmc", "off", "--no-rehearsal", "--no-cpu-baseline", "--power-seconds", "0")
    assert d["value"] > 0 and d["value_exact_f32"] > 0 and d["value_host_fed"] > 0
    assert d["roofline"]["serialised"] is True and d["roofline"]["kernel"]
    assert any("serialised roofline pass" in ln for ln in logs) and any("exact-f32 pass" in ln for ln in logs)
