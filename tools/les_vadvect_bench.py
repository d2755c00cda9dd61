#!/usr/bin/env python3
"""Engine.les_vadvect (K17) timed on the GPU at LES of 64 x 64 x 160, four fields (U, V, THL, QT; U and V are the winds and
fields at once), float64 and float32: HIP events around a window of launches after pre-heating the clocks, three windows per
case, the minimum and the spread (max - min) reported.  The algorithmic bytes of a launch (four reads and four writes of one
field; the profiles, hx, hy and cmax are noise, mtop is not written) per second are set against the stream copy of the same
process on the same number of bytes (tools/libspc_tools.so, read + write).  Next to it K16 on the same fields and the torch
composition of the same rule on the same tensors (torch.roll for the faces, a loop over the levels for M; not checked for equal
bits here): the only way to do this on the device without the kernel.  The ``ensemble`` section times
DeviceLESEnsemble.evolve_model_batched with enable_advection() and with enable_advection(vertical=True).
Each size runs as a child process of its own under a time limit; nothing is started after a failure.
Usage: python tools/les_vadvect_bench.py [--sizes 2,16,256,1024] [--ensemble 256] [--out profiles/les_vadvect_bench.log]"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.les_micro_bench import SHAPE, CELLS, WINDOWS, _windows, _copy_rate, _preheat      # noqa: E402

NAMES = ("U", "V", "THL", "QT")
PASSES = 2 * len(NAMES)                                        # one read and one write per field; the winds are two of them
DT = 10.0


def torch_rule(fields, out, u, v, hx, hy, g, r):
    """the rule of include/spc.h as torch operations on whole tensors (one rounding per operation); returns cmax"""
    import torch
    bx, by = hx[:, None, None, None], hy[:, None, None, None]
    zero = torch.zeros((), dtype=u.dtype, device=u.device)
    cw, ce = (torch.roll(u, 1, 1) + u) * bx, (u + torch.roll(u, -1, 1)) * bx
    cs, cn = (torch.roll(v, 1, 2) + v) * by, (v + torch.roll(v, -1, 2)) * by
    e = g[:, None, None, :] * ((ce - cw) + (cn - cs))
    del cw, ce, cs, cn
    ktot = u.shape[3]
    M = torch.zeros(u.shape[:3] + (ktot + 1,), dtype=u.dtype, device=u.device)
    for k in range(ktot):                                      # the serial chain: one launch per level
        torch.sub(M[..., k], e[..., k], out=M[..., k + 1])
    rr = r[:, None, None, :]
    cb, ct = M[..., :-1] * rr, M[..., 1:] * rr
    pb, pt = torch.where(cb > 0, cb, zero), torch.where(ct < 0, -ct, zero)
    del e, M, cb, ct
    new = {}
    for k, x in fields.items():
        xm = torch.cat([x[..., :1], x[..., :-1]], dim=3)
        xp = torch.cat([x[..., 1:], x[..., -1:]], dim=3)
        new[k] = (x + pb * (xm - x)) + pt * (xp - x)
    for k, y in new.items():                                   # (every field is read before any is written)
        out[k].copy_(y)
    return (pb + pt).flatten(1).amax(dim=1)


def section_size(n):
    import numpy
    import torch
    from sp_coupler_amd import advection as adv
    from sp_coupler_amd.engine import Engine
    _preheat()
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        eng = Engine("cuda:0", dtype=dtype)
        nbytes = PASSES * n * CELLS * dtype.itemsize
        copy = _copy_rate(nbytes)
        gen = torch.Generator(device=eng.device).manual_seed(n)
        rnd = lambda: torch.rand((n,) + SHAPE, dtype=dtype, device=eng.device, generator=gen)       # noqa: E731
        up = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device, dtype)             # noqa: E731
        hx, hy = (up(a) for a in adv.coefficients(DT, n=n))
        k = numpy.arange(SHAPE[2], dtype=numpy.float64)
        g, r = (up(a) for a in adv.vertical_profiles(numpy.tile(1.15 * numpy.exp(-k / 400.0) * (20.0 + 0.25 * k), (n, 1))))
        fields = {"U": rnd().mul_(10.0).sub_(5.0), "V": rnd().mul_(10.0).sub_(5.0), "THL": rnd().mul_(10.0).add_(285.0), "QT": rnd().mul_(0.02)}
        out = {k: torch.empty_like(x) for k, x in fields.items()}
        cmax = torch.empty(n, dtype=dtype, device=eng.device)
        launch = lambda _r: eng.les_vadvect(fields, out, fields["U"], fields["V"], hx, hy, g, r, cmax=cmax)      # noqa: E731
        launch(0)
        torch.cuda.synchronize()
        c = float(cmax.max())
        t, spread, reps = _windows(launch)
        probe = lambda _r: eng.les_vadvect({}, {}, fields["U"], fields["V"], hx, hy, g, r, cmax=cmax)            # noqa: E731
        tp, pspread, preps = _windows(probe)
        k16 = lambda _r: eng.les_advect(fields, out, fields["U"], fields["V"], hx, hy, cmax=cmax)                # noqa: E731
        k16(0)
        th, hspread, hreps = _windows(k16)
        rate = nbytes / t / 1e9
        loop = lambda _r: torch_rule(fields, out, fields["U"], fields["V"], hx, hy, g, r)                       # noqa: E731
        loop(0)
        torch.cuda.synchronize()
        tt, tspread, treps = _windows(loop)
        print("les_vadvect %s n=%-4d cols %d cmax %.3f %9.3f ms per launch (min of %d windows of %d; spread %.3f ms)  %7.1f GB/s of %d passes"
              "  %5.1f %% of the copy rate %.0f GB/s on the same bytes | probe %8.3f ms (windows of %d; spread %.3f ms)"
              " | K16 %8.3f ms (windows of %d; spread %.3f ms)  K17 / K16 %.2f"
              " | torch composition %10.3f ms (windows of %d; spread %.3f ms)  K17 / torch %.4f"
              % (name, n, eng.vadvect_cols_per_block(SHAPE[2]), c, t * 1e3, WINDOWS, reps, spread * 1e3, rate, PASSES, 100 * rate / copy, copy,
                 tp * 1e3, preps, pspread * 1e3, th * 1e3, hreps, hspread * 1e3, t / th, tt * 1e3, treps, tspread * 1e3, t / tt), flush=True)
        del fields, out
        torch.cuda.empty_cache()


def section_ensemble(n):
    import numpy
    import torch
    from sp_coupler_amd import models, spcpl
    from sp_coupler_amd.engine import Engine
    _preheat()
    nL = SHAPE[2]
    for vertical in (False, True):
        eng = Engine("cuda:0")
        spcpl.set_engine(eng)
        gen = torch.Generator(device=eng.device).manual_seed(n)
        rnd = lambda: torch.rand((n,) + SHAPE, dtype=torch.float64, device=eng.device, generator=gen)       # noqa: E731
        gcm = models.BatchedSyntheticGCM(n + 4, 91, 1)
        ens = models.DeviceLESEnsemble.for_gcm(gcm, numpy.arange(1, n + 1), nL=nL, seed=2, itot=SHAPE[0], jtot=SHAPE[1], engine=eng)
        for k in ("U", "V"):
            ens.set_fields_batched(k, rnd().mul_(10.0).sub_(5.0))
        ens.set_fields_batched("THL", rnd().mul_(10.0).add_(285.0))
        ens.set_fields_batched("QT", rnd().mul_(0.02))
        ens.set_fields_batched("Qsat", rnd().mul_(0.02))
        ens.enable_advection(vertical=vertical)
        rng = numpy.random.default_rng(3)
        for k, s in (("U", 1e-4), ("V", 1e-4), ("THL", 1e-5), ("QT", 1e-9)):
            ens.tend[k] = rng.standard_normal((n, nL)) * s
        clock = [float(ens.model_time)]

        def step(_r):
            clock[0] += DT
            ens.evolve_model_batched(clock[0])
        for _ in range(3):
            step(0)
        torch.cuda.synchronize()
        t, spread, reps = _windows(step)
        print("evolve_model_batched n=%-4d advection vertical=%-5s %9.3f ms per call (min of %d windows of %d calls; spread %.3f ms)"
              "  dt %g s, dx = dy = 200 m: n_sub %d, Courant sum of a substep %.3f%s"
              % (n, vertical, t * 1e3, WINDOWS, reps, spread * 1e3, DT, ens.advect_substeps, ens.advect_courant,
                 ", vertical %.3f" % ens.advect_courant_z if vertical else ""), flush=True)
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
            f.write("# Engine.les_vadvect (K17), %d x %d x %d LES, %d fields\n" % (SHAPE + (len(NAMES),)) + "\n".join(lines) + "\n")
    return 1 if failed or not lines else 0


if __name__ == "__main__":
    sys.exit(main())
