#!/usr/bin/env python3
"""Engine.les_moments (K20) timed on the GPU at 256 LES of 8 x 8 x 160 and at 16 LES of 64 x 64 x 160, float64 and float32, with
the fields of statistics.FIELDS (W at the faces) and the pairs of statistics.PAIRS, all four kinds of output: HIP events around a
window of launches after pre-heating the clocks, five windows of at least 0.2 s per case, the minimum and the spread (max - min)
reported.  Two yardsticks from the same process:
  - the eager torch composition of the same statement on the same tensors (the face average, a mean, the deviations kept and
    used for the variance and for every covariance, a sqrt; not checked for equal bits here, only to 1e-9 (f32: 1e-3) of the spreads):
    the only other way this tree could do it on the device;
  - Engine.slab_means (K10) of the same fields: one walk and one chain per level, the floor of a kernel that must walk twice.
--pmc adds one ``rocprofv3 --pmc FETCH_SIZE`` run per size (a child of its own, no tracing beside it) of three launches of K10 and
three of K20 in float64: the counter of K20 over the counter of K10, whose launch reads every field exactly once, is the number
of times K20's reads reached the HBM.
--resusage heads the log with the register counts and scratch bytes of every instantiation (tools/resusage.py moments: a
compilation, which needs no GPU).
Each size runs as a child process of its own under a time limit; nothing is started after a failure.
Usage: python tools/les_moments_bench.py [--resusage] [--pmc] [--out profiles/les_moments_bench.log]"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.les_micro_bench import _events, _preheat      # noqa: E402

SIZES = ((256, 8, 8, 160), (16, 64, 64, 160))
WINDOWS = 5


def _windows(fn):
    t1 = _events(fn, 5)
    reps = int(max(10, min(20000, 0.2 / max(t1, 1e-7))))
    ts = [_events(fn, reps) for _ in range(WINDOWS)]
    return min(ts), max(ts) - min(ts), reps


def torch_moments(fields, pairs, face):
    """the statement of include/spc.h as torch operations on whole tensors"""
    import torch
    x = dict(fields)
    if face is not None:
        w = x[face]
        x[face] = 0.5 * (torch.cat([torch.zeros_like(w[..., :1]), w[..., :-1]], dim=-1) + w)
    mean = {k: v.mean(dim=(1, 2)) for k, v in x.items()}
    d = {k: v - mean[k][:, None, None, :] for k, v in x.items()}
    var = {k: (v * v).mean(dim=(1, 2)) for k, v in d.items()}
    std = {k: torch.sqrt(v) for k, v in var.items()}
    cov = {(a, b): (d[a] * d[b]).mean(dim=(1, 2)) for a, b in pairs}
    return {"mean": mean, "var": var, "std": std, "cov": cov}


def _fields(eng, n, itot, jtot, ktot):
    import torch
    from sp_coupler_amd import statistics as st
    gen = torch.Generator(device=eng.device).manual_seed(n)
    base = {"U": 5.0, "V": -2.0, "W": 0.0, "THL": 290.0, "QT": 8e-3, "QL": 1e-4, "QR": 1e-5}
    spread = {"U": 1.0, "V": 1.0, "W": 0.5, "THL": 0.5, "QT": 4e-4, "QL": 1e-4, "QR": 1e-5}
    return {k: (base[k] + spread[k] * torch.randn((n, itot, jtot, ktot), dtype=torch.float64, device=eng.device, generator=gen)).to(eng.dtype)
            for k in st.FIELDS}


def section_size(index):
    import torch
    from sp_coupler_amd import statistics as st
    from sp_coupler_amd.engine import Engine
    n, itot, jtot, ktot = SIZES[index]
    _preheat()
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        eng = Engine("cuda:0", dtype=dtype)
        fields = _fields(eng, n, itot, jtot, ktot)
        out = eng.les_moments(fields, st.PAIRS, std=True, face=st.FACE)
        want = torch_moments(fields, st.PAIRS, st.FACE)
        torch.cuda.synchronize()
        for kind, d in want.items():
            for key, v in d.items():
                sd = lambda k: float(want["std"][k].max())                                             # noqa: E731
                scale = sd(key[0]) * sd(key[1]) if kind == "cov" else (float(v.abs().max()) + sd(key)) if kind == "mean" else float(v.max())
                assert float((out[kind][key] - v).abs().max()) <= (1e-3 if dtype == torch.float32 else 1e-9) * scale, (kind, key)
        means = eng.slab_means(fields)
        t, spread, reps = _windows(lambda _r: eng.les_moments(fields, st.PAIRS, std=True, face=st.FACE, out=out))
        tk, kspread, kreps = _windows(lambda _r: eng.slab_means(fields, out=means))
        tt, tspread, treps = _windows(lambda _r: torch_moments(fields, st.PAIRS, st.FACE))
        nbytes = len(fields) * n * itot * jtot * ktot * dtype.itemsize
        print("les_moments %s n=%-4d %d x %d x %d  %d fields, %d pairs: %9.4f ms per launch (min of %d windows of %d; spread %.4f ms)  %7.1f GB/s of ONE read "
              "of the fields (%.1f MB) | torch composition %9.4f ms (windows of %d; spread %.4f ms)  K20 / torch %.4f  faster beyond both spreads: %s"
              " | slab_means (K10) %9.4f ms (windows of %d; spread %.4f ms)  K20 / K10 %.2f"
              % (name, n, itot, jtot, ktot, len(fields), len(st.PAIRS), t * 1e3, WINDOWS, reps, spread * 1e3, nbytes / t / 1e9, nbytes / 1e6,
                 tt * 1e3, treps, tspread * 1e3, t / tt, t + spread < tt - tspread, tk * 1e3, kreps, kspread * 1e3, t / tk), flush=True)
        del fields, out, want
        torch.cuda.empty_cache()


def section_pmc(index):
    """the workload of the counter run: three launches of K10 and three of K20, float64"""
    import torch
    from sp_coupler_amd import statistics as st
    from sp_coupler_amd.engine import Engine
    eng = Engine("cuda:0")
    fields = _fields(eng, *SIZES[index])
    for _ in range(3):
        eng.slab_means(fields)
        torch.cuda.synchronize()
    for _ in range(3):
        eng.les_moments(fields, st.PAIRS, std=True, face=st.FACE)
        torch.cuda.synchronize()


def pmc(index):
    """one counter run of its own -> a line of the log"""
    n, itot, jtot, ktot = SIZES[index]
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--pmc-section", str(index)]
        r = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True)
        if r.returncode != 0:
            return r.returncode, "# the counter run of size %s ended with status %d\n%s" % (SIZES[index], r.returncode, r.stderr[-2000:])
        got = {}
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if row.get("Counter_Name") == "FETCH_SIZE":
                        for k in ("k_slab_means", "k_les_moments"):
                            if k in row["Kernel_Name"]:
                                got.setdefault(k, []).append(float(row["Counter_Value"]))
    if not got.get("k_slab_means") or not got.get("k_les_moments"):
        return 1, "# the counter run of size %s named neither kernel" % (SIZES[index],)
    k10, k20 = min(got["k_slab_means"]), min(got["k_les_moments"])
    from sp_coupler_amd import statistics as st
    nbytes = len(st.FIELDS) * n * itot * jtot * ktot * 8
    return 0, ("les_moments f64 n=%-4d %d x %d x %d  FETCH_SIZE (rocprofv3 --pmc, its own run, the least of three launches): K20 %.0f KiB, K10 %.0f KiB "
               "(K10 reads the %.1f MB of the fields once)  K20 / K10 %.2f reads of the fields from the HBM"
               % (n, itot, jtot, ktot, k20, k10, nbytes / 1e6, k20 / k10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pmc", action="store_true", help="one rocprofv3 --pmc FETCH_SIZE run per size after the timings")
    ap.add_argument("--resusage", action="store_true", help="head the log with tools/resusage.py moments (compiles the library's source)")
    ap.add_argument("--section", type=int, default=None, help="(internal) run one size in this process")
    ap.add_argument("--pmc-section", type=int, default=None, help="(internal) the workload of one counter run")
    args = ap.parse_args()
    if args.section is not None:
        return section_size(args.section)
    if args.pmc_section is not None:
        return section_pmc(args.pmc_section)
    lines, failed = [], False
    if args.resusage:
        r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "resusage.py"), "moments"], cwd=HERE, capture_output=True, text=True)
        lines, failed = ["# " + x for x in r.stdout.splitlines()], r.returncode != 0
        print("\n".join(lines), flush=True)
    for index in range(len(SIZES)) if not failed else ():
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--section", str(index)]
        r = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True)
        lines += r.stdout.splitlines()
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append("# size %s ended with status %d; nothing further was started" % (SIZES[index], r.returncode))
            print(lines[-1] + "\n" + r.stderr[-3000:], flush=True)
            failed = True
            break
    for index in range(len(SIZES)) if args.pmc and not failed else ():
        rc, line = pmc(index)
        lines.append(line)
        print(line, flush=True)
        if rc:
            failed = True
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("# Engine.les_moments (K20), the fields and pairs of sp_coupler_amd/statistics.py\n" + "\n".join(lines) + "\n")
    return 1 if failed or not lines else 0


if __name__ == "__main__":
    sys.exit(main())
