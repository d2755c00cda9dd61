#!/usr/bin/env python3
"""Engine.les_buoyancy (K21: k_les_hydrostatic and k_les_pgrad, two launches) timed on the GPU at 256 LES of 8 x 8 x 160 and at 16
LES of 64 x 64 x 160, float64 and float32: HIP events around a window of calls after pre-heating the clocks, three windows per
case, the minimum and the spread (max - min) reported.  Next to it, measured in the same process:
  - the torch composition of the same rule on the same tensors (a flipped torch.cumsum for the chain, torch.roll for the
    neighbours; not checked for equal bits): the only way to do this on the device without the kernels;
  - the time of nine field passes (thl, qt and ql read, phi written, phi read again, u and v read and written) at the rate
    the stream copy of tools/libspc_tools.so reaches on the same number of bytes.
Each case runs as a child process of its own under a time limit; nothing is started after a failure.
Usage: python tools/les_buoyancy_bench.py [--cases 256x8x8,16x64x64] [--out profiles/les_buoyancy_bench.log]"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.les_micro_bench import WINDOWS, _windows, _copy_rate, _preheat      # noqa: E402

KTOT = 160
PASSES = 9                                                     # read 3, write phi, re-read phi, read and write u and v
DT = 6.0


def torch_rule(thl, qt, ql, u, v, hx, hy, t0, lex, s, c1, c2):
    """the rule of include/spc.h as torch operations on whole tensors; u and v updated in place; returns (phi, amax)"""
    import torch
    b_ = lambda a: a[:, None, None, :]                                                     # noqa: E731
    tl = thl + b_(lex) * ql
    m = (1.0 + c1 * qt) - c2 * ql
    b = (tl * m - b_(t0)) * b_(s)
    del tl, m
    above = torch.flip(torch.cumsum(torch.flip(b, (3,)), dim=3), (3,))                     # the sum of b from k to the lid
    phi = b - 2.0 * above                                                                  # -(2 sum above k) - b[k]
    del b, above
    du = hx[:, None, None, None] * (torch.roll(phi, -1, 1) - torch.roll(phi, 1, 1))
    dv = hy[:, None, None, None] * (torch.roll(phi, -1, 2) - torch.roll(phi, 1, 2))
    u.sub_(du)
    v.sub_(dv)
    return phi, (du.abs() + dv.abs()).amax(dim=(1, 2, 3))


def section_case(n, itot, jtot):
    import numpy
    import torch
    from sp_coupler_amd import advection as adv
    from sp_coupler_amd import buoyancy as buo
    from sp_coupler_amd.engine import Engine
    _preheat()
    shape = (n, itot, jtot, KTOT)
    cells = n * itot * jtot * KTOT
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        eng = Engine("cuda:0", dtype=dtype)
        nbytes = PASSES * cells * dtype.itemsize
        copy = _copy_rate(nbytes)
        gen = torch.Generator(device=eng.device).manual_seed(n)
        up = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device, dtype)             # noqa: E731
        rnd = lambda: torch.rand(shape, dtype=dtype, device=eng.device, generator=gen)                # noqa: E731
        k = numpy.arange(KTOT, dtype=numpy.float64)
        zh = numpy.cumsum(20.0 + 0.25 * k) - 20.0
        thm = numpy.tile(290.0 + 10.0 * k / KTOT, (n, 1))
        qtm = numpy.tile(8e-3 * numpy.exp(-k / KTOT), (n, 1))
        qlm = numpy.tile(numpy.where((k >= 60) & (k < 70), 2e-4, 0.0), (n, 1))
        presf = 1e5 * numpy.exp(-(zh + 10.0) / 8000.0) * numpy.ones((n, 1))
        t0, lex, s = (up(a) for a in buo.profiles(thm, qtm, qlm, presf, zh))
        hx, hy = (up(a) for a in adv.coefficients(DT, 200.0, 200.0, n=n))
        thl = rnd().sub_(0.5).add_(up(thm)[:, None, None, :])
        qt = rnd().mul_(0.1).add_(0.95).mul_(up(qtm)[:, None, None, :])
        ql = rnd().mul_(2.0).mul_(up(qlm)[:, None, None, :])
        u, v = rnd().mul_(2.0).add_(4.0), rnd().mul_(2.0).sub_(3.0)
        phi = torch.empty_like(thl)
        amax = torch.empty(n, dtype=dtype, device=eng.device)
        launch = lambda _r: eng.les_buoyancy(thl, qt, ql, u, v, hx, hy, t0, lex, s, phi, amax=amax)     # noqa: E731
        launch(0)
        torch.cuda.synchronize()
        change = float(amax.max())
        t, spread, reps = _windows(launch)
        rate = nbytes / t / 1e9
        floor = nbytes / (copy * 1e9)
        loop = lambda _r: torch_rule(thl, qt, ql, u, v, hx, hy, t0, lex, s, buo.C1, buo.C2)             # noqa: E731
        loop(0)
        torch.cuda.synchronize()
        tt, tspread, treps = _windows(loop)
        print("les_buoyancy %s %4d LES of %d x %d x %d cols %d strip %s largest wind change %.3g m/s %9.3f ms per call of two launches"
              " (min of %d windows of %d; spread %.3f ms)  %7.1f GB/s of %d passes | nine passes at the copy rate %.0f GB/s on the same bytes"
              " %8.3f ms  K21 / nine passes %.3f | torch composition %10.3f ms (windows of %d; spread %.3f ms)  K21 / torch %.4f"
              % (name, n, itot, jtot, KTOT, eng.buoyancy_cols_per_block(KTOT), eng.advect_strip(n, itot, jtot, KTOT), change, t * 1e3, WINDOWS, reps,
                 spread * 1e3, rate, PASSES, copy, floor * 1e3, t / floor, tt * 1e3, treps, tspread * 1e3, t / tt), flush=True)
        del thl, qt, ql, u, v, phi
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="256x8x8,16x64x64", help="n x itot x jtot of every case; ktot is %d" % KTOT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--section", default=None, help="(internal) run one case in this process")
    args = ap.parse_args()
    if args.section:
        return section_case(*(int(x) for x in args.section.split("x")))
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
            f.write("# Engine.les_buoyancy (K21), LES of %d levels, liquid water at the levels 60 ... 69\n" % KTOT + "\n".join(lines) + "\n")
    return 1 if failed or not lines else 0


if __name__ == "__main__":
    sys.exit(main())
