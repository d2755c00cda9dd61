#!/usr/bin/env python3
"""Engine.les_radiate (K18) timed on the GPU at LES of 64 x 64 x 160 with a cloud deck of about 10 levels, float64 and float32:
HIP events around a window of launches after pre-heating the clocks, three windows per case, the minimum and the spread
(max - min) reported.  The algorithmic bytes of a launch (ql read, thl read and written; the profiles, f0, f1 and the table
are noise, flux is not written) per second are set against the stream copy of the same process on the same number of bytes
(tools/libspc_tools.so, read + write).  Next to it the launch that also writes flux, and the torch composition of the same rule
on the same tensors (torch.cumsum and a flipped cumsum for the optical depths, torch.exp for the table; not checked for equal
bits): the only way to do this on the device without the kernel.  The ``ensemble`` section times
DeviceLESEnsemble.evolve_model_batched without and with enable_radiation().
Each size runs as a child process of its own under a time limit; nothing is started after a failure.
Usage: python tools/les_radiate_bench.py [--sizes 2,16,256,1024] [--ensemble 256] [--out profiles/les_radiate_bench.log]"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.les_micro_bench import SHAPE, CELLS, WINDOWS, _windows, _copy_rate, _preheat      # noqa: E402

PASSES = 3                                                     # ql read, thl read and written
DT = 60.0
DECK = (60, 70)                                                # the levels of the cloud deck


def torch_rule(ql, thl, w, c, f0, f1):
    """the rule of include/spc.h as torch operations on whole tensors; thl updated in place"""
    import torch
    t = w[:, None, None, :] * ql
    B = torch.cumsum(t, dim=3)                                 # the depth below the upper face of every cell
    A = torch.flip(torch.cumsum(torch.flip(t, (3,)), dim=3), (3,))     # the depth above the lower face
    del t
    zero = torch.zeros_like(A[..., :1])
    b0, b1 = f0[:, None, None, None], f1[:, None, None, None]
    lo = b0 * torch.exp(-A) + b1 * torch.exp(-torch.cat([zero, B[..., :-1]], dim=3))
    hi = b0 * torch.exp(-torch.cat([A[..., 1:], zero], dim=3)) + b1 * torch.exp(-B)
    del A, B
    thl.sub_(c[:, None, None, :] * (hi - lo))
    return hi


def deck(n, dtype, device, gen):
    """ql with 3e-4 ... 7e-4 kg/kg in the levels DECK of every column, the edges of the deck ragged by one level"""
    import torch
    ql = torch.zeros((n,) + SHAPE, dtype=dtype, device=device)
    ql[..., DECK[0]:DECK[1]] = torch.rand((n,) + SHAPE[:2] + (DECK[1] - DECK[0],), dtype=dtype, device=device, generator=gen) * 4e-4 + 3e-4
    ql[..., DECK[1] - 1] *= (torch.rand((n,) + SHAPE[:2], dtype=dtype, device=device, generator=gen) < 0.5)
    return ql


def section_size(n):
    import numpy
    import torch
    from sp_coupler_amd import radiation as rad
    from sp_coupler_amd.engine import Engine
    _preheat()
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        eng = Engine("cuda:0", dtype=dtype)
        nbytes = PASSES * n * CELLS * dtype.itemsize
        copy = _copy_rate(nbytes)
        gen = torch.Generator(device=eng.device).manual_seed(n)
        up = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device, dtype)             # noqa: E731
        k = numpy.arange(SHAPE[2], dtype=numpy.float64)
        zh = numpy.cumsum(20.0 + 0.25 * k) - 20.0
        rho = numpy.tile(1.15 * numpy.exp(-k / 400.0), (n, 1))
        w, c = (up(a) for a in rad.profiles(rho, zh, 1e5 * numpy.exp(-zh / 8000.0) * numpy.ones((n, 1)), DT))
        f0, f1 = up(numpy.full(n, rad.F0)), up(numpy.full(n, rad.F1))
        ql = deck(n, dtype, eng.device, gen)
        thl = torch.rand((n,) + SHAPE, dtype=dtype, device=eng.device, generator=gen).mul_(10.0).add_(285.0)
        launch = lambda _r: eng.les_radiate(ql, thl, w, c, f0, f1)                                    # noqa: E731
        launch(0)
        torch.cuda.synchronize()
        t, spread, reps = _windows(launch)
        flux = torch.empty_like(thl)
        both = lambda _r: eng.les_radiate(ql, thl, w, c, f0, f1, flux=flux)                           # noqa: E731
        both(0)
        torch.cuda.synchronize()
        depth = float((w[:, None, None, DECK[0]:DECK[1]] * ql[..., DECK[0]:DECK[1]]).sum(dim=3).mean())
        tf, fspread, freps = _windows(both)
        del flux
        torch.cuda.empty_cache()
        rate = nbytes / t / 1e9
        loop = lambda _r: torch_rule(ql, thl, w, c, f0, f1)                                           # noqa: E731
        loop(0)
        torch.cuda.synchronize()
        tt, tspread, treps = _windows(loop)
        print("les_radiate %s n=%-4d cols %d mean optical depth %.2f %9.3f ms per launch (min of %d windows of %d; spread %.3f ms)  %7.1f GB/s of %d passes"
              "  %5.1f %% of the copy rate %.0f GB/s on the same bytes | with flux %8.3f ms (windows of %d; spread %.3f ms)"
              " | torch composition %10.3f ms (windows of %d; spread %.3f ms)  K18 / torch %.4f"
              % (name, n, eng.radiate_cols_per_block(SHAPE[2]), depth, t * 1e3, WINDOWS, reps, spread * 1e3, rate, PASSES, 100 * rate / copy, copy,
                 tf * 1e3, freps, fspread * 1e3, tt * 1e3, treps, tspread * 1e3, t / tt), flush=True)
        del ql, thl
        torch.cuda.empty_cache()


def section_ensemble(n):
    import numpy
    import torch
    from sp_coupler_amd import models, spcpl
    from sp_coupler_amd.engine import Engine
    _preheat()
    nL = SHAPE[2]
    for radiate in (False, True):
        eng = Engine("cuda:0")
        spcpl.set_engine(eng)
        gen = torch.Generator(device=eng.device).manual_seed(n)
        rnd = lambda: torch.rand((n,) + SHAPE, dtype=torch.float64, device=eng.device, generator=gen)       # noqa: E731
        gcm = models.BatchedSyntheticGCM(n + 4, 91, 1)
        ens = models.DeviceLESEnsemble.for_gcm(gcm, numpy.arange(1, n + 1), nL=nL, seed=2, itot=SHAPE[0], jtot=SHAPE[1], engine=eng)
        ens.set_fields_batched("THL", rnd().mul_(10.0).add_(285.0))
        qsat = rnd().mul_(1e-3).add_(8e-3)
        ens.set_fields_batched("QT", qsat - 2e-4 + deck(n, torch.float64, eng.device, gen))
        ens.set_fields_batched("Qsat", qsat)
        del qsat
        if radiate:
            ens.enable_radiation()
        rng = numpy.random.default_rng(3)
        for k, s in (("THL", 1e-5), ("QT", 1e-9)):
            ens.tend[k] = rng.standard_normal((n, nL)) * s
        clock = [float(ens.model_time)]

        def step(_r):
            clock[0] += DT
            ens.evolve_model_batched(clock[0])
        for _ in range(3):
            step(0)
        torch.cuda.synchronize()
        t, spread, reps = _windows(step)
        print("evolve_model_batched n=%-4d radiation=%-5s %9.3f ms per call (min of %d windows of %d calls; spread %.3f ms)  dt %g s"
              % (n, radiate, t * 1e3, WINDOWS, reps, spread * 1e3, DT), flush=True)
        del ens
        spcpl.set_engine(None)
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2,16,256,1024")
    ap.add_argument("--ensemble", type=int, default=256, help="LES of the evolve_model_batched section (0: skip it)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--section", default=None, help="(internal) run one section in this process")
    ap.add_argument("--n", type=int, default=0)
    args = ap.parse_args()
    if args.section == "size":
        return section_size(args.n)
    if args.section == "ensemble":
        return section_ensemble(args.n)
    jobs = [("size", int(s)) for s in args.sizes.split(",") if s] + ([("ensemble", args.ensemble)] if args.ensemble else [])
    lines, failed = [], False
    for section, n in jobs:
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--section", section, "--n", str(n)]
        r = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True)
        lines += r.stdout.splitlines()
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append("# %s n=%d ended with status %d; nothing further was started" % (section, n, r.returncode))
            print(lines[-1] + "\n" + r.stderr[-3000:], flush=True)
            failed = True
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("# Engine.les_radiate (K18), %d x %d x %d LES, a cloud deck at the levels %d ... %d\n" % (SHAPE + (DECK[0], DECK[1] - 1))
                    + "\n".join(lines) + "\n")
    return 1 if failed or not lines else 0


if __name__ == "__main__":
    sys.exit(main())
