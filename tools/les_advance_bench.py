#!/usr/bin/env python3
"""models.DeviceLESEnsemble.evolve_model_batched timed on the GPU (LES of 64 x 64 x 160 float64; U, V, THL, QT stepped,
QL = max(QT - Qsat, 0), five slab means): HIP events around a window of calls after pre-heating the clocks, three windows
per size, the minimum and the spread (max - min) reported.  Only the public ensemble call is used, so the same script times
another checkout of the library (--root: the parent commit, whose step is torch ops + K10) next to this one in one visit.
Where the engine has ``les_advance`` (K11) the launch alone is timed too, and its bytes (5 fields read, 5 written) per second
are set against the stream copy of the same visit (tools/libspc_tools.so, read + write).
Each size runs as a child process of its own under a time limit; nothing is started after a failure.
Usage: python tools/les_advance_bench.py [--root DIR] [--label NAME] [--sizes 2,16,256] [--min-les N] [--out profiles/les_advance_bench.log]
       (--out appends, so that two trees share one log)"""
import argparse
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (64, 64, 160)
FIELD_BYTES = SHAPE[0] * SHAPE[1] * SHAPE[2] * 8
WINDOWS = 3


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


def section_copybw():
    import torch
    from tools import spc_tools
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    s = torch.cuda.current_stream()
    for _ in range(5):
        spc_tools.stream_copy(dst, src, s)
    t = _events(lambda r: spc_tools.stream_copy(dst, src, s), 20)
    print("copybw %.1f GB/s (read + write, 1 GiB stream copy)" % (2 * src.numel() / t / 1e9))


def section_size(n, label, copy_gbs, min_les=None):
    import numpy
    import torch
    from sp_coupler_amd import models, spcpl
    from sp_coupler_amd.engine import Engine
    if min_les is not None and hasattr(models.DeviceLESEnsemble, "FUSED_MIN_LES"):
        models.DeviceLESEnsemble.FUSED_MIN_LES = min_les           # (locating the threshold: the fused path at every size)
    eng = Engine("cuda:0")
    spcpl.set_engine(eng)
    nL = SHAPE[2]
    gen = torch.Generator(device=eng.device).manual_seed(n)
    rnd = lambda: torch.rand((n,) + SHAPE, dtype=torch.float64, device=eng.device, generator=gen)       # noqa: E731
    gcm = models.BatchedSyntheticGCM(n + 4, 91, 1)
    ens = models.DeviceLESEnsemble.for_gcm(gcm, numpy.arange(1, n + 1), nL=nL, seed=2, itot=SHAPE[0], jtot=SHAPE[1], engine=eng)
    for k in ("U", "V", "THL"):
        ens.set_fields_batched(k, rnd())
    qt = rnd().mul_(0.02)
    ens.set_fields_batched("QT", qt)
    ens.set_fields_batched("Qsat", rnd().mul_(0.02))
    rng = numpy.random.default_rng(3)
    for k, s in (("U", 1e-4), ("V", 1e-4), ("THL", 1e-5), ("QT", 1e-9)):
        ens.tend[k] = rng.standard_normal((n, nL)) * s
    clock = [float(ens.model_time)]

    def step(_r):
        clock[0] += 10.0
        ens.evolve_model_batched(clock[0])
    t_end = time.perf_counter() + 2.0
    while time.perf_counter() < t_end:                             # pre-heat the clocks
        step(0)
        torch.cuda.synchronize()
    t, spread, reps = _windows(step)
    fused = bool(getattr(ens, "fused_advance", False)) and hasattr(eng, "les_advance") and n >= getattr(ens, "FUSED_MIN_LES", 0)
    print("%-8s evolve_model_batched n=%-4d %9.3f ms per call (min of %d windows of %d calls; spread %.3f ms) path=%s"
          % (label, n, t * 1e3, WINDOWS, reps, spread * 1e3, "fused K11" if fused else "torch ops + K10"), flush=True)
    if hasattr(eng, "les_advance"):
        f = {k: ens.fields3d[k] for k in ("U", "V", "THL", "QT")}
        tend = {k: torch.from_numpy(ens.tend[k]).to(eng.device) for k in f}
        means = {k: torch.empty((n, nL), dtype=torch.float64, device=eng.device) for k in list(f) + ["QL"]}
        launch = lambda _r: eng.les_advance(f, tend, 10.0, qsat=ens.fields3d["Qsat"], sat="QT", ql=ens.fields3d["QL"], means=means)   # noqa: E731
        launch(0)
        t, spread, reps = _windows(launch)
        rate = 10 * n * FIELD_BYTES / t / 1e9
        print("%-8s les_advance launch   n=%-4d %9.3f ms per launch (spread %.3f ms)  %8.1f GB/s read + write  %5.1f %% of the copy bandwidth"
              % (label, n, t * 1e3, spread * 1e3, rate, 100 * rate / copy_gbs if copy_gbs else float("nan")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE, help="the checkout whose sp_coupler_amd is timed (default: this one)")
    ap.add_argument("--label", default="this")
    ap.add_argument("--sizes", default="2,16,256")
    ap.add_argument("--out", default=None)
    ap.add_argument("--section", default=None, help="(internal) run one section in this process")
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--copy-gbs", type=float, default=0.0)
    ap.add_argument("--min-les", type=int, default=None, help="override DeviceLESEnsemble.FUSED_MIN_LES (0: fused at every size)")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    if args.section == "copybw":
        return section_copybw()
    if args.section == "size":
        return section_size(args.n, args.label, args.copy_gbs, args.min_les)
    lines, copy_gbs, failed = [], 0.0, False
    for section, n, limit in [("copybw", 0, 120)] + [("size", int(s), 300) for s in args.sizes.split(",")]:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--section", section, "--n", str(n),
               "--root", root, "--label", args.label, "--copy-gbs", str(copy_gbs)]
        if args.min_les is not None:
            cmd += ["--min-les", str(args.min_les)]
        r = subprocess.run(cmd, cwd=root, capture_output=True, text=True)
        lines += r.stdout.splitlines()
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append("# %s: section %s n=%d ended with status %d; nothing further was started" % (args.label, section, n, r.returncode))
            print(lines[-1] + "\n" + r.stderr[-3000:], flush=True)
            failed = True
            break
        if section == "copybw":
            copy_gbs = float(r.stdout.split()[1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("# %s: DeviceLESEnsemble.evolve_model_batched, %d x %d x %d float64 LES\n" % ((args.label,) + SHAPE) + "\n".join(lines) + "\n")
    return 1 if failed or not lines else 0


if __name__ == "__main__":
    sys.exit(main())
