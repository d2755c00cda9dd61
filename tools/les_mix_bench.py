#!/usr/bin/env python3
"""Engine.les_mix (K24: k_les_eddy and k_les_hmix, two launches) timed on the GPU at 256 LES of 8 x 8 x 160 and at 16 LES of
64 x 64 x 160, float64 and float32, five fields (U, V, THL, QT, QR): HIP events around a window of calls after pre-heating the
clocks, three windows per case, the minimum and the spread (max - min) reported.  Next to it, measured in the same process:
  - the torch composition of the same rule on the same tensors (torch.roll for the neighbours, slices along k; not checked for
    equal bits): the only way to do this on the device without the kernels;
  - the time of 4 + 1 + 2 NF = 15 field passes (u, v and theta read, km written; km read again, five fields read and five
    written) at the rate the stream copy of tools/libspc_tools.so reaches on the same number of bytes.
No ratio is asked for in advance: each line states both ratios and whether K24 beats the torch composition by more than the two
spreads.  The share of cells the cap binds in is that of a step of ``DT`` seconds on a grid of ``DX`` m, the ensemble's defaults.
--pmc adds one ``rocprofv3 --pmc FETCH_SIZE`` run per case (a child of its own, no tracing beside it) of three float64 calls: the
bytes both kernels fetched from the HBM against one read of their inputs.
Each case runs as a child process of its own under a time limit; nothing is started after a failure.
Usage: python tools/les_mix_bench.py [--cases 256x8x8,16x64x64] [--pmc] [--out profiles/les_mix_bench.log]"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.les_micro_bench import WINDOWS, _windows, _copy_rate, _preheat      # noqa: E402

KTOT = 160
NAMES = ("U", "V", "THL", "QT", "QR")
PASSES = 4 + 1 + 2 * len(NAMES)
DT = 900.0
DX = 200.0


def torch_rule(fields, u, v, theta, gx, gy, gz, bz, l2, kcap, coef):
    """the rule of include/spc.h as torch operations on whole tensors; returns (km, kmax, dict name -> the mixed field)"""
    import torch
    L = lambda a: a[:, None, None, None]                                                   # noqa: E731
    P = lambda a: a[:, None, None, :]                                                      # noqa: E731
    dz = lambda x: torch.cat([x[..., 1:], x[..., -1:]], 3) - torch.cat([x[..., :1], x[..., :-1]], 3)          # noqa: E731
    ux, vx = (torch.roll(u, -1, 1) - torch.roll(u, 1, 1)) * L(gx), (torch.roll(v, -1, 1) - torch.roll(v, 1, 1)) * L(gx)
    uy, vy = (torch.roll(u, -1, 2) - torch.roll(u, 1, 2)) * L(gy), (torch.roll(v, -1, 2) - torch.roll(v, 1, 2)) * L(gy)
    uz, vz = dz(u) * P(gz), dz(v) * P(gz)
    a, sh = ux * ux + vy * vy, uy + vx
    d = (a + a) + sh * sh + (uz * uz + vz * vz) - dz(theta) * P(bz)
    kk = P(l2) * torch.sqrt(torch.clamp_min(d, 0.0))
    km = torch.minimum(kk, L(kcap))
    kw, ke = torch.roll(km, 1, 1) + km, km + torch.roll(km, -1, 1)
    ks, kn = torch.roll(km, 1, 2) + km, km + torch.roll(km, -1, 2)
    out = {}
    for k, x in fields.items():
        ax, ay = L(coef[k][0]), L(coef[k][1])
        fw, fe = kw * ax * (x - torch.roll(x, 1, 1)), ke * ax * (torch.roll(x, -1, 1) - x)
        fs, fn = ks * ay * (x - torch.roll(x, 1, 2)), kn * ay * (torch.roll(x, -1, 2) - x)
        out[k] = x + ((fe - fw) + (fn - fs))
    return km, kk.amax(dim=(1, 2, 3)), out


def _case(eng, n, itot, jtot):
    """the tensors of one case on the engine's device: a sheared, weakly stable flow with noise on every field"""
    import numpy
    import torch
    from sp_coupler_amd import mixing as mix
    dtype = eng.dtype
    shape = (n, itot, jtot, KTOT)
    gen = torch.Generator(device=eng.device).manual_seed(n)
    up = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device, dtype)             # noqa: E731
    rnd = lambda: torch.rand(shape, dtype=dtype, device=eng.device, generator=gen)                # noqa: E731
    k = numpy.arange(KTOT, dtype=numpy.float64)
    zh = numpy.cumsum(20.0 + 0.25 * k) - 20.0
    zf = zh + 0.5 * (20.0 + 0.25 * k)
    gx, gy, wind, scalar = mix.coefficients(DT, DX, DX, n=n)
    kcap = up(mix.cap(wind, scalar))
    gz, bz, l2 = (up(a) for a in mix.profiles(zf, zh, DX, DX, n=n))
    wind, scalar = tuple(up(a) for a in wind), tuple(up(a) for a in scalar)
    f = {"U": rnd().mul_(2.0).add_(4.0), "V": rnd().mul_(2.0).sub_(3.0), "THL": rnd().sub_(0.5).add_(up(290.0 + 10.0 * k / KTOT)),
         "QT": rnd().mul_(0.1).add_(0.95).mul_(up(8e-3 * numpy.exp(-k / KTOT))), "QR": rnd().mul_(1e-5)}
    coef = {name: wind if name in ("U", "V") else scalar for name in NAMES}
    return f, up(gx), up(gy), gz, bz, l2, kcap, coef


def _call(eng, f, gx, gy, gz, bz, l2, kcap, coef, out, km, kmax):
    return eng.les_mix(f, out, f["U"], f["V"], f["THL"], gx, gy, gz, bz, l2, kcap, km, {k: coef[k][0] for k in f}, {k: coef[k][1] for k in f},
                       kmax=kmax)


def section_case(n, itot, jtot):
    import torch
    from sp_coupler_amd.engine import Engine
    _preheat()
    cells = n * itot * jtot * KTOT
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        eng = Engine("cuda:0", dtype=dtype)
        nbytes = PASSES * cells * dtype.itemsize
        copy = _copy_rate(nbytes)
        f, gx, gy, gz, bz, l2, kcap, coef = _case(eng, n, itot, jtot)
        out, km = {k: torch.empty_like(x) for k, x in f.items()}, torch.empty_like(f["U"])
        kmax = torch.empty(n, dtype=dtype, device=eng.device)
        launch = lambda _r: _call(eng, f, gx, gy, gz, bz, l2, kcap, coef, out, km, kmax)               # noqa: E731
        launch(0)
        torch.cuda.synchronize()
        capped = float((km == kcap[:, None, None, None]).double().mean())
        top = float(kmax.max())
        t, spread, reps = _windows(launch)
        rate = nbytes / t / 1e9
        floor = nbytes / (copy * 1e9)
        loop = lambda _r: torch_rule(f, f["U"], f["V"], f["THL"], gx, gy, gz, bz, l2, kcap, coef)      # noqa: E731
        want = loop(0)
        torch.cuda.synchronize()
        scale = float(want[2]["U"].abs().max())
        tol = 1e-3 if dtype == torch.float32 else 1e-7              # (the same rule; a sqrt near zero differs most)
        assert float((want[2]["U"] - out["U"]).abs().max()) <= tol * scale
        del want
        tt, tspread, treps = _windows(loop)
        print("les_mix %s %4d LES of %d x %d x %d strip %s %d fields, dt %g s dx %g m: largest kk %.3g m2/s, kcap %.3g m2/s, %.1f %% of the cells capped"
              " %9.3f ms per call of two launches (min of %d windows of %d; spread %.3f ms)  %7.1f GB/s of %d passes | %d passes at the copy rate"
              " %.0f GB/s on the same bytes %8.3f ms  K24 / passes %.3f | torch composition %10.3f ms (windows of %d; spread %.3f ms)"
              "  K24 / torch %.4f  faster beyond both spreads: %s"
              % (name, n, itot, jtot, KTOT, eng.advect_strip(n, itot, jtot, KTOT), len(NAMES), DT, DX, top, float(kcap.min()), 100.0 * capped, t * 1e3,
                 WINDOWS, reps, spread * 1e3, rate, PASSES, PASSES, copy, floor * 1e3, t / floor, tt * 1e3, treps, tspread * 1e3, t / tt,
                 t + spread < tt - tspread), flush=True)
        del f, out, km
        torch.cuda.empty_cache()


def section_pmc(n, itot, jtot):
    """the workload of the counter run: three float64 calls"""
    import torch
    from sp_coupler_amd.engine import Engine
    eng = Engine("cuda:0")
    f, gx, gy, gz, bz, l2, kcap, coef = _case(eng, n, itot, jtot)
    out, km = {k: torch.empty_like(x) for k, x in f.items()}, torch.empty_like(f["U"])
    for _ in range(3):
        _call(eng, f, gx, gy, gz, bz, l2, kcap, coef, out, km, True)
        torch.cuda.synchronize()


def pmc(case):
    """one counter run of its own -> (status, a line of the log)"""
    n, itot, jtot = (int(x) for x in case.split("x"))
    got = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--pmc-section", case]
        r = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True)
        if r.returncode != 0:
            return r.returncode, "# the counter run of case %s ended with status %d\n%s" % (case, r.returncode, r.stderr[-2000:])
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if row.get("Counter_Name") == "FETCH_SIZE":
                        for k in ("k_les_eddy", "k_les_hmix"):
                            if k in row["Kernel_Name"]:
                                got.setdefault(k, []).append(float(row["Counter_Value"]))
    if not got.get("k_les_eddy") or not got.get("k_les_hmix"):
        return 1, "# the counter run of case %s named neither kernel" % case
    field = n * itot * jtot * KTOT * 8 / 1024.0
    eddy, hmix = min(got["k_les_eddy"]), min(got["k_les_hmix"])
    return 0, ("les_mix f64 %4d LES of %d x %d x %d  FETCH_SIZE (rocprofv3 --pmc, its own run, the least of three calls): k_les_eddy %.0f KiB = %.2f reads"
               " of its three input fields, k_les_hmix %.0f KiB = %.2f reads of km and its %d fields (one field: %.0f KiB)"
               % (n, itot, jtot, KTOT, eddy, eddy / (3 * field), hmix, hmix / ((1 + len(NAMES)) * field), len(NAMES), field))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="256x8x8,16x64x64", help="n x itot x jtot of every case; ktot is %d" % KTOT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pmc", action="store_true", help="one rocprofv3 --pmc FETCH_SIZE run per case after the timings")
    ap.add_argument("--section", default=None, help="(internal) run one case in this process")
    ap.add_argument("--pmc-section", default=None, help="(internal) the workload of one counter run")
    args = ap.parse_args()
    if args.section:
        return section_case(*(int(x) for x in args.section.split("x")))
    if args.pmc_section:
        return section_pmc(*(int(x) for x in args.pmc_section.split("x")))
    lines, failed = [], False
    cases = [c for c in args.cases.split(",") if c]
    for case in cases:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--section", case]
        r = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True)
        lines += r.stdout.splitlines()
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append("# case %s ended with status %d; nothing further was started" % (case, r.returncode))
            print(lines[-1] + "\n" + r.stderr[-3000:], flush=True)
            failed = True
            break
    for case in cases if args.pmc and not failed else ():
        rc, line = pmc(case)
        lines.append(line)
        print(line, flush=True)
        if rc:
            failed = True
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("# Engine.les_mix (K24), LES of %d levels, U, V, THL, QT and QR\n" % KTOT + "\n".join(lines) + "\n")
    return 1 if failed or not lines else 0


if __name__ == "__main__":
    sys.exit(main())
