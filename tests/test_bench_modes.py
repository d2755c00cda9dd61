"""bench.py's two kinds of run: a plain run does only what the headline needs (set up, warm up, time, dump, one JSON line);
`--full` adds every extra leg and check (per-kernel pass, roofline, spread, cold clock, CPU baseline, `verified`, ...)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
EXTRAS = ("roofline", "value_spread", "cold_clock", "small_batch", "scaling_anchor", "config5", "per_column_grid",
          "in_process_all_gpus", "dropin", "dropin_value", "cpu_baseline", "verified_detail")


def _run(*argv):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH] + list(argv), capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0]


def test_full_is_an_option():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "--full" in r.stdout


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone():
    line = _run("--gpus", "1", "--cols", "2048", "--steps", "5", "--warmup", "1")
    assert line["full"] is False and line["verified"] is None
    assert line["steps"] == 5 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["unit"] == "column-exchanges/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert not [k for k in EXTRAS if k in line]


@pytest.mark.gpu
def test_full_run_measures_and_checks_the_rest():
    line = _run("--gpus", "1", "--cols", "2048", "--steps", "5", "--warmup", "1", "--full", "--cpu-seconds", "1",
                "--no-cpu-multicore", "--no-small-batch", "--no-dropin", "--multi-devices", "none")
    assert line["full"] is True and line["verified"] is True, line.get("verified_detail")
    for k in ("roofline", "value_spread", "cold_clock", "cpu_baseline"):
        assert k in line, k
    assert line["roofline"]["avg_launch_us"] > 0 and line["cpu_baseline"]["value"] > 0
