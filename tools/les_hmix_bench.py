#!/usr/bin/env python3
"""Engine.les_hmix (K26: k_les_hline along i, then along j, two launches) timed on the GPU at 256 LES of 8 x 8 x 160 and at 16 LES
of 64 x 64 x 160, float64 and float32, five fields (U, V, THL, QT, QR) on the fields and the coefficients of tools/les_mix_bench.py
(dt 900 s, dx 200 m) by the UNCAPPED viscosity of those fields: HIP events around a window of calls after pre-heating the clocks,
three windows per case, the minimum and the spread (max - min) reported.  Next to it, measured in the same process:
  (a) ONE les_mix call (K24, both launches, five fields, capped), and ceil(kmax / kcap) of them: the substeps the explicit
      scheme needs to mix by the same viscosity, kmax the largest kk of the bench fields;
  (b) the time of the 2 x NF x 7 = 70 field passes of K26's shape (per sweep and field: km read, the field read and written three
      times each) at the rate the stream copy of tools/libspc_tools.so reaches (on at most 2 GiB each way);
  (c) the launch the implicit mode shares with the explicit one: les_mix without fields (k_les_eddy alone) under a cap that never
      binds.
An eager torch composition of the cyclic solve was not written: it would be a Python loop over the cells of a line.
No ratio is asked for in advance: each line states the ratios with the spreads beside them.
--resusage puts the register and scratch lines of tools/resusage.py (hline) at the head of the log (needs hipcc).
Each case runs as a child process of its own under a time limit; nothing is started after a failure.
Usage: python tools/les_hmix_bench.py [--cases 256x8x8,16x64x64] [--resusage] [--out profiles/les_hmix_bench.log]"""
import argparse
import math
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.les_micro_bench import WINDOWS, _windows, _copy_rate, _preheat      # noqa: E402
from tools.les_mix_bench import DT, DX, KTOT, NAMES, _call, _case              # noqa: E402

PASSES = 2 * len(NAMES) * 7


def section_case(n, itot, jtot):
    import torch
    from sp_coupler_amd import horizontal_mixing as hm
    from sp_coupler_amd.engine import Engine
    _preheat()
    cells = n * itot * jtot * KTOT
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        eng = Engine("cuda:0", dtype=dtype)
        nbytes = PASSES * cells * dtype.itemsize
        copy = _copy_rate(nbytes)
        f, gx, gy, gz, bz, l2, kcap, coef = _case(eng, n, itot, jtot)
        keep = {k: x.clone() for k, x in f.items()}
        out, km = {k: torch.empty_like(x) for k, x in f.items()}, torch.empty_like(f["U"])
        kmax = torch.empty(n, dtype=dtype, device=eng.device)
        huge = torch.full((n,), torch.finfo(dtype).max, dtype=dtype, device=eng.device)
        kh2 = torch.from_numpy(hm.bound(n)).to(eng.device, dtype)
        ax, ay = {k: coef[k][0] for k in f}, {k: coef[k][1] for k in f}
        probe = lambda _r: eng.les_mix({}, {}, f["U"], f["V"], f["THL"], gx, gy, gz, bz, l2, huge, km, {}, {}, kmax=kmax)       # noqa: E731
        probe(0)                                                     # km: the closure's own viscosity of the bench fields
        torch.cuda.synchronize()
        top, lowest = float(kmax.max()), float(kcap.min())
        steps = int(math.ceil(top / lowest))

        def fresh():                                                 # (a step is in place: without this the fields would relax to constants)
            for k, x in f.items():
                x.copy_(keep[k])
        new = lambda _r: eng.les_hmix(f, km, ax, ay, kh2)                                          # noqa: E731
        new(0)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(x).all()) for x in f.values())
        moved = float((f["U"] - keep["U"]).abs().max())
        drift = max(abs(float(f[k].double().sum() - keep[k].double().sum())) / float(keep[k].double().abs().sum()) for k in f)
        fresh()
        t, spread, reps = _windows(new)
        floor = nbytes / (copy * 1e9)
        fresh()
        kcapped = torch.empty_like(km)
        old = lambda _r: _call(eng, f, gx, gy, gz, bz, l2, kcap, coef, out, kcapped, kmax)             # noqa: E731
        old(0)
        told, oldspread, oldreps = _windows(old)
        tp, pspread, preps = _windows(probe)
        print("les_hmix %s %4d LES of %d x %d x %d, lines per workgroup %d along i and %d along j, %d fields, dt %g s dx %g m:"
              " largest kk %.3g m2/s against kcap %.3g m2/s; one step moved U by up to %.3g m/s and the field sums by %.2g of sum|x|"
              " %9.3f ms per call of two launches (min of %d windows of %d; spread %.3f ms)  %7.1f GB/s of %d passes"
              " | (b) %d passes at the copy rate %.0f GB/s %8.3f ms  K26 / passes %.3f"
              " | (a) one les_mix call (K24, capped) %9.3f ms (windows of %d; spread %.3f ms)  K26 / K24 %.3f;"
              " ceil(kmax / kcap) = %d explicit substeps %9.3f ms  K26 / substeps %.4f"
              " | (c) the probe of the uncapped viscosity (k_les_eddy alone) %9.3f ms (windows of %d; spread %.3f ms) = %.3f of a K26 call"
              % (name, n, itot, jtot, KTOT, eng.hmix_lines_per_block(itot), eng.hmix_lines_per_block(jtot), len(NAMES), DT, DX, top, lowest,
                 moved, drift, t * 1e3, WINDOWS, reps, spread * 1e3, nbytes / t / 1e9, PASSES, PASSES, copy, floor * 1e3, t / floor,
                 told * 1e3, oldreps, oldspread * 1e3, t / told, steps, steps * told * 1e3, t / (steps * told),
                 tp * 1e3, preps, pspread * 1e3, tp / t), flush=True)
        del f, keep, out, km, kcapped
        torch.cuda.empty_cache()


def resusage():
    r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "resusage.py"), "hline"], cwd=HERE, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    if r.returncode:
        lines.append("# tools/resusage.py hline ended with status %d" % r.returncode)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="256x8x8,16x64x64", help="n x itot x jtot of every case; ktot is %d" % KTOT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resusage", action="store_true", help="the lines of tools/resusage.py hline at the head of the log")
    ap.add_argument("--section", default=None, help="(internal) run one case in this process")
    args = ap.parse_args()
    if args.section:
        return section_case(*(int(x) for x in args.section.split("x")))
    head = resusage() if args.resusage else []
    print("\n".join(head), flush=True)
    lines, failed = [], False
    for case in [c for c in args.cases.split(",") if c]:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--section", case]
        r = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True)
        lines += r.stdout.splitlines()
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append("# case %s ended with status %d; nothing further was started" % (case, r.returncode))
            print(lines[-1] + "\n" + r.stderr[-3000:], flush=True)
            failed = True
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(head + ["# Engine.les_hmix (K26), LES of %d levels, U, V, THL, QT and QR" % KTOT] + lines) + "\n")
    return 1 if failed or not lines else 0


if __name__ == "__main__":
    sys.exit(main())
