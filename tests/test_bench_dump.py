"""bench.py --dump-outputs: what the last timed step computed, written as DIR/<name>.npy (float32 / float64, at most
bench.DUMP_BYTES in all, a fixed seeded row sample when the outputs do not fit) so that two builds can be compared
output for output.  CPU: the row sample and the writer on stand-in plans.  GPU: a real bench.py run whose dump equals the
plain-C oracle on the inputs of the batch its last timed step launched."""
import json
import os
import subprocess
import sys
import types

import numpy
import pytest
import torch

import bench
from sp_coupler_amd import synthetic
from tests import oracle_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD = ("f_u", "f_v", "f_thl", "f_qt", "f_ql", "ql_ref", "f_ps", "idx")
BWD = ("f_T", "f_SH", "f_QL", "f_QI", "f_U", "f_V", "f_A")


def _plans(n, nG, nL, dtype, seed=5):
    """stand-ins with the outputs of Engine.plan_exchange: K1's six [n x nL] arrays, f_ps, the int32 index map in a
    padded column pitch (a view, as the engine allocates it), K3's seven [n x nG] tendencies"""
    g = torch.Generator().manual_seed(seed)
    f = {k: torch.randn(n, nL, generator=g, dtype=torch.float64).to(dtype) for k in FWD[:6]}
    f["f_ps"] = torch.randn(n, generator=g, dtype=torch.float64).to(dtype)
    f["idx"] = torch.randint(0, nL, (n, nG + 3), generator=g, dtype=torch.int32)[:, :nG]
    b = {k: torch.randn(n, nG, generator=g, dtype=torch.float64).to(dtype) for k in BWD}
    return types.SimpleNamespace(outputs=f), types.SimpleNamespace(outputs=b)


def test_dump_rows_fit_the_budget_and_are_the_same_every_time():
    for n, nG, nL in ((35718, 91, 160), (88838, 137, 512), (348528, 91, 160)):       # configs 3, 5, 4
        row_bytes = 8 * (6 * nL + 1 + nG + 7 * nG)
        rows = bench.dump_rows(n, row_bytes, 15)
        assert len(rows) * row_bytes + 256 * 15 <= bench.DUMP_BYTES
        assert len(rows) > 1000 and rows[0] == 0 and rows[-1] == n - 1
        assert (numpy.diff(rows) > 0).all()
        assert numpy.array_equal(rows, bench.dump_rows(n, row_bytes, 15))
    assert numpy.array_equal(bench.dump_rows(1024, 13512, 15), numpy.arange(1024))   # config 2 fits whole


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dump_writes_every_output_of_both_plans_on_a_row_sample(tmp_path, dtype):
    n, nG, nL = 500, 91, 160
    fp, bp = _plans(n, nG, nL, dtype)
    budget = 150 * 1000
    info = bench.dump_outputs(str(tmp_path), fp, bp, budget=budget)
    names = set(FWD + BWD)
    assert set(info["arrays"]) == names and {f[:-4] for f in os.listdir(tmp_path)} == names
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) == info["bytes"] <= budget
    m = info["rows"]
    assert 1 < m < n and info["rows_in_block"] == n
    esize = torch.empty(0, dtype=dtype).element_size()
    rows = bench.dump_rows(n, esize * (6 * nL + 1 + 7 * nG) + 8 * nG, len(names), budget)
    assert len(rows) == m and rows[0] == 0 and rows[-1] == n - 1
    want_type = numpy.float64 if dtype == torch.float64 else numpy.float32
    for k, t in list(fp.outputs.items()) + list(bp.outputs.items()):
        a = numpy.load(tmp_path / (k + ".npy"))
        assert a.dtype == (numpy.float64 if k == "idx" else want_type), k
        assert numpy.array_equal(a, t.numpy()[rows]), k


def test_dump_writes_every_row_when_they_fit(tmp_path):
    fp, bp = _plans(40, 19, 32, torch.float64)
    info = bench.dump_outputs(str(tmp_path / "new" / "dir"), fp, bp)
    assert info["rows"] == 40 and info["row_sample"] is None
    assert numpy.array_equal(numpy.load(tmp_path / "new" / "dir" / "f_T.npy"), bp.outputs["f_T"].numpy())


def test_dump_needs_a_timed_step():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dump-outputs", "x"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr


@pytest.mark.gpu
def test_bench_dump_is_what_the_last_timed_step_computed(tmp_path):
    """5 timed steps over 3 rotating batches: the last one launches batch 4 % 3 = 1 (not batch 0, not batch 5 % 3), whose
    inputs are config 3's seed + 1; all 2048 rows fit, and they equal the plain-C oracle (f_thl within 8 ulp of thl / dt)"""
    n, steps, rotate = 2048, 5, 3
    out = tmp_path / "dump"
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cols", str(n), "--rotate", str(rotate),
                        "--steps", str(steps), "--warmup", "1", "--cpu-seconds", "0", "--no-kernel-events", "--no-dropin",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")][-1]
    assert line["steps"] == steps and line["dump_outputs"]["batch"] == 1 and line["dump_outputs"]["rows"] == n
    F = {k: numpy.load(out / (k + ".npy")) for k in FWD}
    B = {k: numpy.load(out / (k + ".npy")) for k in BWD}
    assert all(a.dtype == numpy.float64 for a in list(F.values()) + list(B.values()))
    gcm, zf, zh, prof = synthetic.make_batch(n, 91, 160, synthetic.CONFIGS[3][3] + 1, couple_surface=False)
    ref_f = oracle_c.forward(gcm, zf, zh, prof, 1.0, 900.0, couple_surface=False)
    ref_b = oracle_c.backward(gcm, None, zf, prof, 1.0, 900.0)
    bad, _ = bench.compare_with_oracle(F, B, ref_f, ref_b, 1.0, 900.0)
    assert not bad, bad
