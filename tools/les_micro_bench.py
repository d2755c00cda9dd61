#!/usr/bin/env python3
"""Engine.les_microphysics (K14) timed on the GPU at LES of 64 x 64 x 160, float64 and float32: HIP events around a window of
launches after pre-heating the clocks, three windows per case, the minimum and the spread (max - min) reported.  The bytes of
a launch (qt, ql, qr, thl, temp read; qt, thl, qr_new written: 5 + 3 passes over one field; rain, the means and the profiles
are noise) per second are set against the stream copy of the same process on the same number of bytes (tools/libspc_tools.so,
read + write).  Next to it the torch composition of the same rule on the same tensors, with K10's slab means of the four
fields: the only way to do this on the device without the kernel.  The ``ensemble`` section times
DeviceLESEnsemble.evolve_model_batched with and without enable_microphysics(), with and without enable_thermo().
Each size runs as a child process of its own under a time limit; nothing is started after a failure.
``--rows 2`` / ``--rows 4`` time the kernels with that many rows per batch at every size instead of the library's choice.
Usage: python tools/les_micro_bench.py [--sizes 2,16,256,1024] [--ensemble 256] [--rows 2|4] [--out profiles/les_micro_bench.log]"""
import argparse
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (64, 64, 160)
CELLS = SHAPE[0] * SHAPE[1] * SHAPE[2]
WINDOWS = 3
PASSES = 8                                                     # 5 reads + 3 writes per cell with THL and temp


def _events(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for r in range(reps):
        fn(r)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def _windows(fn):
    t1 = _events(fn, 2)
    reps = int(max(3, min(200, 0.3 / max(t1, 1e-6))))
    ts = [_events(fn, reps) for _ in range(WINDOWS)]
    return min(ts), max(ts) - min(ts), reps


def _copy_rate(nbytes):
    """GB/s (read + write) of a stream copy that moves ``nbytes`` in all (half of them read, half written)"""
    import torch
    from tools import spc_tools
    half = max(1 << 20, min(nbytes // 2, 2 << 30))             # (at most 2 GiB each way)
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    s = torch.cuda.current_stream()
    for _ in range(3):
        spc_tools.stream_copy(dst, src, s)
    t, _, _ = _windows(lambda r: spc_tools.stream_copy(dst, src, s))
    return 2 * half / t / 1e9


def _preheat():
    import torch
    t_end = time.perf_counter() + 2.0
    heat = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    while time.perf_counter() < t_end:
        heat.add_(1)
        torch.cuda.synchronize()


def torch_rule(eng, qt, ql, qr, qr_new, so, si, lc, w, dt, thl, temp, rain):
    """the rule of include/spc.h as torch operations (one rounding per operation, not checked for equal bits here) and K10"""
    import torch
    from sp_coupler_amd import microphysics as mp
    T = lambda v: torch.tensor(v, dtype=qt.dtype, device=qt.device)                        # noqa: E731
    b = lambda a: a[:, None, None, :]                                                      # noqa: E731
    ka, kc, tu, td = T(mp.K_AUTO) * T(dt), T(mp.K_ACC) * T(dt), T(mp.T_UP), T(mp.T_DN)
    up = torch.zeros_like(qr)
    up[..., :-1] = qr[..., 1:]
    out = b(so) * qr
    qs = (qr - out) + b(si) * up
    d = ql - T(mp.QC0)
    x = torch.where(d > 0, d, torch.where(d != d, d, T(0.0)))
    s = ka * x + (kc * ql) * qs
    s = torch.where(s > ql, ql, s)
    qt.sub_(s)
    thl.add_(b(lc) * s)
    torch.add(qs, s, out=qr_new)
    rain.add_((so[:, 0, None, None] * qr[..., 0]) * w[:, 0, None, None])
    fi = torch.where(temp >= tu, T(0.0), torch.where(temp <= td, T(1.0), (tu - temp) / (tu - td)))
    qi = (ql - s) * fi
    return eng.slab_means({"QT": qt, "THL": thl, "QR": qr_new, "QI": qi})


def section_size(n):
    import numpy
    import torch
    from sp_coupler_amd import microphysics as mp
    from sp_coupler_amd.engine import Engine
    _preheat()
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        eng = Engine("cuda:0", dtype=dtype)
        nbytes = PASSES * n * CELLS * dtype.itemsize
        copy = _copy_rate(nbytes)
        gen = torch.Generator(device=eng.device).manual_seed(n)
        shape = (n,) + SHAPE
        rnd = lambda: torch.rand(shape, dtype=dtype, device=eng.device, generator=gen)       # noqa: E731
        zh = numpy.arange(SHAPE[2]) * 25.0
        zf = zh + 12.5
        rhobf = numpy.tile(1.2 * numpy.exp(-zf / 9000.0), (n, 1))
        presf = numpy.tile(1e5 * numpy.exp(-zf / 8000.0), (n, 1))
        so, si, lc, w = (torch.from_numpy(a).to(eng.device, dtype) for a in mp.profiles(zh, zf, rhobf, presf, 10.0))
        qt = rnd().mul_(4e-3).add_(8e-3)
        ql = torch.where(rnd() < 0.3, rnd().mul_(2e-3), torch.zeros((), dtype=dtype, device=eng.device))
        qr = torch.where(rnd() < 0.3, rnd().mul_(1e-3), torch.zeros((), dtype=dtype, device=eng.device))
        thl, temp = rnd().mul_(10.0).add_(285.0), rnd().mul_(40.0).add_(240.0)
        qr_new = torch.empty_like(qt)
        rain = torch.zeros(shape[:3], dtype=dtype, device=eng.device)
        means = {k: torch.empty((n, SHAPE[2]), dtype=dtype, device=eng.device) for k in ("QT", "QR", "THL", "QI")}
        launch = lambda _r: eng.les_microphysics(qt, ql, qr, qr_new, so, si, lc, w, 10.0, thl=thl, temp=temp, rain=rain, means=means)   # noqa: E731
        launch(0)
        torch.cuda.synchronize()
        t, spread, reps = _windows(launch)
        rate = nbytes / t / 1e9
        composed = lambda _r: torch_rule(eng, qt, ql, qr, qr_new, so, si, lc, w, 10.0, thl, temp, rain)      # noqa: E731
        composed(0)
        torch.cuda.synchronize()
        tt, tspread, treps = _windows(composed)
        print("les_microphysics %s n=%-4d %9.3f ms per launch (min of %d windows of %d; spread %.3f ms)  %7.1f GB/s of %d passes"
              "  %5.1f %% of the copy rate %.0f GB/s on the same bytes | torch composition + K10 %9.3f ms (windows of %d; spread %.3f ms)"
              "  K14 / torch %.3f" % (name, n, t * 1e3, WINDOWS, reps, spread * 1e3, rate, PASSES, 100 * rate / copy, copy, tt * 1e3, treps,
                                      tspread * 1e3, t / tt), flush=True)
        del qt, ql, qr, thl, temp, qr_new, rain
        torch.cuda.empty_cache()


def section_ensemble(n):
    import numpy
    import torch
    from sp_coupler_amd import models, spcpl
    from sp_coupler_amd.engine import Engine
    _preheat()
    nL = SHAPE[2]
    for thermo in (False, True):
        for micro in (False, True):
            eng = Engine("cuda:0")
            spcpl.set_engine(eng)
            gen = torch.Generator(device=eng.device).manual_seed(n)
            rnd = lambda: torch.rand((n,) + SHAPE, dtype=torch.float64, device=eng.device, generator=gen)       # noqa: E731
            gcm = models.BatchedSyntheticGCM(n + 4, 91, 1)
            ens = models.DeviceLESEnsemble.for_gcm(gcm, numpy.arange(1, n + 1), nL=nL, seed=2, itot=SHAPE[0], jtot=SHAPE[1], engine=eng)
            for k in ("U", "V"):
                ens.set_fields_batched(k, rnd())
            ens.set_fields_batched("THL", rnd().mul_(10.0).add_(285.0))
            ens.set_fields_batched("QT", rnd().mul_(0.02))
            if thermo:
                ens.enable_thermo()
            else:
                ens.set_fields_batched("Qsat", rnd().mul_(0.02))
            if micro:
                ens.enable_microphysics()
            rng = numpy.random.default_rng(3)
            for k, s in (("U", 1e-4), ("V", 1e-4), ("THL", 1e-5), ("QT", 1e-9)):
                ens.tend[k] = rng.standard_normal((n, nL)) * s
            clock = [float(ens.model_time)]

            def step(_r):
                clock[0] += 10.0
                ens.evolve_model_batched(clock[0])
            for _ in range(3):
                step(0)
            torch.cuda.synchronize()
            t, spread, reps = _windows(step)
            print("evolve_model_batched n=%-4d thermo=%-5s microphysics=%-5s %9.3f ms per call (min of %d windows of %d calls; spread %.3f ms)"
                  % (n, thermo, micro, t * 1e3, WINDOWS, reps, spread * 1e3), flush=True)
            del ens
            spcpl.set_engine(None)
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2,16,256,1024")
    ap.add_argument("--ensemble", type=int, default=256, help="LES of the evolve_model_batched section (0: skip it)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=0, choices=(0, 2, 4),
                    help="force the kernels with 2 or 4 rows per batch at every size (through SPC_CUS: the library picks them by "
                         "the waves per SIMD of the launch); 0: the library's choice")
    ap.add_argument("--section", default=None, help="(internal) run one section in this process")
    ap.add_argument("--n", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    if args.section == "size":
        return section_size(args.n)
    if args.section == "ensemble":
        return section_ensemble(args.n)
    jobs = [("size", int(s)) for s in args.sizes.split(",") if s] + ([("ensemble", args.ensemble)] if args.ensemble else [])
    lines, failed = [], False
    for section, n in jobs:
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--section", section, "--n", str(n)]
        env = dict(os.environ)
        if args.rows:
            env["SPC_CUS"] = "1" if args.rows == 2 else "1000000"
        r = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True, env=env)
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
            f.write("# Engine.les_microphysics (K14), %d x %d x %d LES%s\n" % (SHAPE + ((", %d rows per batch forced" % args.rows) if args.rows else "",))
                    + "\n".join(lines) + "\n")
    return 1 if failed or not lines else 0


if __name__ == "__main__":
    sys.exit(main())
