#!/usr/bin/env python3
"""Engine.les_vmix (K25: k_les_speed and k_les_vmix, two launches) timed on the GPU at 256 LES of 8 x 8 x 160 and at 16 LES of
64 x 64 x 160, float64 and float32, five fields (U, V, THL, QT, QR) with the drag on U and V and the fluxes into THL and QT: HIP
events around a window of calls after pre-heating the clocks, three windows per case, the minimum and the spread (max - min)
reported.  Next to it, measured in the same process:
  (a) the path K25 replaces, enable_mixing(vertical=True): K10's slab means of km, then K15 on four fields (U, V, THL, QT) -- the
      device time of the two launches, and separately the wall time of the whole path with the copy of the means to the host, the
      float64 elimination in NumPy and the upload of a, m and cp between the two kernels;
  (b) the time of 3 NF + 1 = 16 field passes (per field: km read, the field read and written; the speed plane is a 160th of a
      field) at the rate the stream copy of tools/libspc_tools.so reaches on the same number of bytes;
  (c) the extra launch of a step where K24's cap binds: les_mix without fields (k_les_eddy alone) under a cap that never binds.
No ratio is asked for in advance: each line states the ratios with the spreads beside them.
--resusage puts the register and scratch lines of tools/resusage.py (speed, vmix) at the head of the log (needs hipcc).
Each case runs as a child process of its own under a time limit; nothing is started after a failure.
Usage: python tools/les_vmix_bench.py [--cases 256x8x8,16x64x64] [--resusage] [--out profiles/les_vmix_bench.log]"""
import argparse
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.les_micro_bench import WINDOWS, _windows, _copy_rate, _preheat      # noqa: E402

KTOT = 160
NAMES = ("U", "V", "THL", "QT", "QR")
WINDS = ("U", "V")
OLD = ("U", "V", "THL", "QT")                                      # what K15 diffuses
PASSES = 3 * len(NAMES) + 1
DT = 900.0
DX = 200.0
Z0M = 0.05


def _case(eng, n, itot, jtot):
    """the tensors of one case on the engine's device: a sheared flow with noise on every field and a km that is zero in a third of
    the cells and reaches a few m2/s in the others"""
    import numpy
    import torch
    from sp_coupler_amd import mixing as mix
    from sp_coupler_amd import vertical_mixing as vm
    dtype = eng.dtype
    shape = (n, itot, jtot, KTOT)
    gen = torch.Generator(device=eng.device).manual_seed(n)
    up = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device, dtype)             # noqa: E731
    rnd = lambda: torch.rand(shape, dtype=dtype, device=eng.device, generator=gen)                # noqa: E731
    k = numpy.arange(KTOT, dtype=numpy.float64)
    dz = 20.0 + 0.25 * k
    zh = numpy.cumsum(dz) - dz
    zf = zh + 0.5 * dz
    rhobf = numpy.broadcast_to(1.2 * numpy.exp(-zf / 8000.0), (n, KTOT))
    wind, scalar, s0 = vm.coefficients(zh, zf, rhobf, DT)
    kb, kv2 = vm.background(n, KTOT)
    c = dict(wind=tuple(up(a) for a in wind), scalar=tuple(up(a) for a in scalar), s0=up(s0), kb=up(kb), kv2=up(kv2),
             dr=up(vm.drag(numpy.full(n, Z0M), zf, dz, DT)), wt=up(numpy.full(n, 0.12)), wq=up(numpy.full(n, 6e-5)),
             zh=zh, zf=zf, rhobf=rhobf)
    f = {"U": rnd().mul_(2.0).add_(4.0), "V": rnd().mul_(2.0).sub_(3.0), "THL": rnd().sub_(0.5).add_(up(290.0 + 10.0 * k / KTOT)),
         "QT": rnd().mul_(0.1).add_(0.95).mul_(up(8e-3 * numpy.exp(-k / KTOT))), "QR": rnd().mul_(1e-5)}
    km = torch.clamp_min(rnd().mul_(6.0).sub_(2.0), 0.0)
    # what the probe of (c) needs
    gx, gy, mwind, mscalar = mix.coefficients(DT, DX, DX, n=n)
    c["probe"] = (up(gx), up(gy)) + tuple(up(a) for a in mix.profiles(zf, zh, DX, DX, n=n))
    c["huge"] = torch.full((n,), torch.finfo(dtype).max, dtype=dtype, device=eng.device)
    return f, km, c


def _vmix(eng, f, km, c, speed):
    coef = {k: c["wind"] if k in WINDS else c["scalar"] for k in f}
    eng.les_vmix(f, km, {k: coef[k][0] for k in f}, {k: coef[k][1] for k in f}, c["kb"], c["kv2"], s0=c["s0"],
                 flux={"THL": c["wt"], "QT": c["wq"]}, drag={"U": c["dr"], "V": c["dr"]}, u=f["U"], v=f["V"], speed=speed)


def section_case(n, itot, jtot):
    import numpy
    import torch
    from sp_coupler_amd import diffusion as df
    from sp_coupler_amd import mixing as mix
    from sp_coupler_amd.engine import Engine
    _preheat()
    cells = n * itot * jtot * KTOT
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        eng = Engine("cuda:0", dtype=dtype)
        nbytes = PASSES * cells * dtype.itemsize
        copy = _copy_rate(nbytes)
        f, km, c = _case(eng, n, itot, jtot)
        keep = {k: x.clone() for k, x in f.items()}
        speed = torch.empty((n, itot, jtot), dtype=dtype, device=eng.device)

        def fresh():                                                 # (a step is in place: without this the fields would relax to constants)
            for k, x in f.items():
                x.copy_(keep[k])
        new = lambda _r: _vmix(eng, f, km, c, speed)                                              # noqa: E731
        new(0)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(x).all()) for x in f.values())
        fresh()
        t, spread, reps = _windows(new)
        floor = nbytes / (copy * 1e9)
        # (a) the slab-mean path: K10 of km, the elimination on the host, K15 on four fields
        old_fields = {k: f[k] for k in OLD}
        flux = {"THL": c["wt"], "QT": c["wq"]}
        up = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device, dtype)         # noqa: E731

        def host_part():
            m = eng.slab_means({"km": km})["km"].cpu().numpy().astype(numpy.float64)
            return [up(a) for a in df.profiles(c["zh"], c["zf"], c["rhobf"], DT, kd=mix.face_diffusivity(m, df.K_BG))]
        a, m, cp, s0 = host_part()

        def old_device(_r):
            eng.slab_means({"km": km})
            eng.les_diffuse(old_fields, a, m, cp, s0=s0, flux=flux)
        fresh()
        told, oldspread, oldreps = _windows(old_device)
        walls = []
        for _ in range(WINDOWS):
            fresh()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                pa, pm, pcp, ps0 = host_part()
                eng.les_diffuse(old_fields, pa, pm, pcp, s0=ps0, flux=flux)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) / 5)
        wall, wallspread = min(walls), max(walls) - min(walls)
        fresh()
        torch.cuda.synchronize()
        walls = []
        for _ in range(WINDOWS):
            t0 = time.perf_counter()
            for _ in range(5):
                new(0)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) / 5)
        newwall, newwallspread = min(walls), max(walls) - min(walls)
        # (c) the probe of the uncapped viscosity
        gx, gy, gz, bz, l2 = c["probe"]
        kv = torch.empty_like(km)
        probe = lambda _r: eng.les_mix({}, {}, f["U"], f["V"], f["THL"], gx, gy, gz, bz, l2, c["huge"], kv, {}, {}, kmax=False)     # noqa: E731
        probe(0)
        tp, pspread, preps = _windows(probe)
        print("les_vmix %s %4d LES of %d x %d x %d, %d columns per workgroup, %d fields with drag and fluxes, dt %g s:"
              " %9.3f ms per call of two launches (min of %d windows of %d; spread %.3f ms)  %7.1f GB/s of %d passes"
              " | (b) %d passes at the copy rate %.0f GB/s on the same bytes %8.3f ms  K25 / passes %.3f"
              " | (a) K10 of km + K15 on %d fields, device %9.3f ms (windows of %d; spread %.3f ms)  K25 / that %.3f;"
              " wall with the host elimination and the upload %9.3f ms (min of %d times 5 calls; spread %.3f ms), K25 wall %9.3f ms (spread %.3f ms)"
              "  K25 wall / that wall %.4f"
              " | (c) the probe of the uncapped viscosity (k_les_eddy alone) %9.3f ms (windows of %d; spread %.3f ms) = %.3f of a K25 call"
              % (name, n, itot, jtot, KTOT, eng.vmix_cols_per_block(KTOT), len(NAMES), DT, t * 1e3, WINDOWS, reps, spread * 1e3, nbytes / t / 1e9, PASSES,
                 PASSES, copy, floor * 1e3, t / floor, len(OLD), told * 1e3, oldreps, oldspread * 1e3, t / told, wall * 1e3, WINDOWS, wallspread * 1e3,
                 newwall * 1e3, newwallspread * 1e3, newwall / wall, tp * 1e3, preps, pspread * 1e3, tp / t), flush=True)
        del f, keep, km, kv
        torch.cuda.empty_cache()


def resusage():
    lines = []
    for entry in ("speed", "vmix"):
        r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "resusage.py"), entry], cwd=HERE, capture_output=True, text=True)
        lines += r.stdout.splitlines()
        if r.returncode:
            lines.append("# tools/resusage.py %s ended with status %d" % (entry, r.returncode))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="256x8x8,16x64x64", help="n x itot x jtot of every case; ktot is %d" % KTOT)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resusage", action="store_true", help="the lines of tools/resusage.py speed / vmix at the head of the log")
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
            f.write("\n".join(head + ["# Engine.les_vmix (K25), LES of %d levels, U, V, THL, QT and QR" % KTOT] + lines) + "\n")
    return 1 if failed or not lines else 0


if __name__ == "__main__":
    sys.exit(main())
