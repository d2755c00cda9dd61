#!/usr/bin/env python3
"""K10 and the device-resident LES fields, timed on the GPU (64 x 64 x 160 LES, float64).

1. copy bandwidth of this visit (tools/libspc_tools.so stream copy, 1 GiB, read + write bytes over HIP-event time);
2. Engine.slab_means with F = 8 fields for 2, 16, 256, 1 024 LES: time per launch (HIP events around a window of launches,
   clocks pre-heated, inputs rotated through more sets than the 256 MiB Infinity Cache holds where one set fits it) and
   bytes read / time as a fraction of the copy bandwidth; Engine.slab_cloud_fraction (91 layers) likewise;
3. spcpl.variability_nudge_ensemble and spcpl.set_les_state_batched at 256 LES on an ensemble with host fields (the path of
   the parent commit, unchanged here) and on models.DeviceLESEnsemble, alternating, best of the repeats, host clock around
   calls that end with their results on the host; the nudged QT of both must be bit-equal.
Each section runs as a child process of its own under a time limit; nothing is started after a failure.
Usage: python tools/slab_bench.py [--out profiles/slab_bench.log] [--sizes 2,16,256,1024] [--les 256]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = (64, 64, 160)
FIELD_BYTES = SHAPE[0] * SHAPE[1] * SHAPE[2] * 8


def _events(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for r in range(reps):
        fn(r)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


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


def section_k10(sizes, copy_gbs):
    import torch
    from sp_coupler_amd.engine import Engine
    eng = Engine("cuda:0")
    names = ["U", "V", "THL", "QT", "QL", "QL_ice", "QR", "T"]
    heat = {k: torch.rand((16,) + SHAPE, dtype=torch.float64, device=eng.device) for k in names}
    t_end = time.perf_counter() + 2.0
    while time.perf_counter() < t_end:                          # pre-heat the clocks
        eng.slab_means(heat)
        torch.cuda.synchronize()
    del heat
    for n in sizes:
        set_bytes = 8 * n * FIELD_BYTES
        nsets = max(1, min(4, -(-(512 << 20) // set_bytes)))     # rotate through >= 512 MiB where one set is smaller
        sets = [{k: torch.rand((n,) + SHAPE, dtype=torch.float64, device=eng.device) for k in names} for _ in range(nsets)]
        out = {k: torch.empty((n, SHAPE[2]), dtype=torch.float64, device=eng.device) for k in names}
        for s in sets:
            eng.slab_means(s, out=out)
        torch.cuda.synchronize()
        t1 = _events(lambda r: eng.slab_means(sets[r % nsets], out=out), 3)
        reps = int(max(5, min(400, 0.4 / max(t1, 1e-6))))
        t = _events(lambda r: eng.slab_means(sets[r % nsets], out=out), reps)
        rate = set_bytes / t / 1e9
        print("slab_means     n=%-5d F=8  %10.3f ms per launch  %8.1f GB/s read  %5.1f %% of the copy bandwidth (%d input sets, %d launches)"
              % (n, t * 1e3, rate, 100 * rate / copy_gbs, nsets, reps), flush=True)
        ql = [s["QL"] for s in sets]
        for q in ql:
            q.sub_(0.97).clamp_min_(0.0)                         # 3 % of the cells cloudy
        idx = torch.linspace(0, SHAPE[2], 92, device=eng.device)[1:].to(torch.int32).repeat(n, 1).contiguous()
        A = torch.empty((n, 91), dtype=torch.float64, device=eng.device)
        eng.slab_cloud_fraction(ql[0], idx, out=A)
        torch.cuda.synchronize()
        t1 = _events(lambda r: eng.slab_cloud_fraction(ql[r % nsets], idx, out=A), 3)
        reps = int(max(5, min(400, 0.4 / max(t1, 1e-6))))
        t = _events(lambda r: eng.slab_cloud_fraction(ql[r % nsets], idx, out=A), reps)
        rate = n * FIELD_BYTES / t / 1e9
        print("cloud_fraction n=%-5d nG=91 %9.3f ms per call    %8.1f GB/s read  %5.1f %% of the copy bandwidth (3 launches per call)"
              % (n, t * 1e3, rate, 100 * rate / copy_gbs), flush=True)
        del sets, ql, out
        torch.cuda.empty_cache()


def section_paths(n):
    import numpy
    import torch
    from sp_coupler_amd import models, spcpl
    from sp_coupler_amd.engine import Engine

    class HostEns(models.SyntheticLESEnsemble):
        """host fields of SHAPE: the per-column faces report the field extents"""
        def __getitem__(self, i):
            row = super().__getitem__(i)
            if not isinstance(i, slice):
                row.get_itot, row.get_jtot = (lambda: SHAPE[0]), (lambda: SHAPE[1])
            return row

    spcpl.set_engine(Engine("cuda:0"))
    itot, jtot, nL = SHAPE
    rng = numpy.random.default_rng(1)
    z = (numpy.arange(nL) + 0.5) / nL
    qsat_p = 0.016 * numpy.exp(-3.0 * z)
    qt_p = qsat_p * (0.75 + 0.3 * numpy.exp(-((z - 0.35) / 0.15) ** 2))
    noise = lambda: (rng.random((n,) + SHAPE, dtype=numpy.float32) - 0.5).astype(numpy.float64) * 3.46       # noqa: E731
    fields = {"QT": qt_p + 0.04 * qt_p * (0.2 + z) * noise(), "Qsat": qsat_p * (1 + 0.01 * noise())}
    fields["QL"] = numpy.maximum(fields["QT"] - fields["Qsat"], 0.0)
    ql_av = numpy.stack([f.mean(axis=(0, 1)) for f in fields["QL"]])
    qt_av = numpy.stack([f.mean(axis=(0, 1)) for f in fields["QT"]])
    ql_ref = ql_av * rng.uniform(0.5, 2.0, (n, nL))
    presf = numpy.tile(1e5 * numpy.exp(-0.5 * z), (n, 1))
    gcm = models.BatchedSyntheticGCM(n + 4, 91, 1)
    prof4 = [rng.normal(m, 1.0, (n, nL)) for m in (5.0, -3.0, 300.0)] + [rng.uniform(0, 0.02, (n, nL))]

    def make(cls):
        ens = cls.for_gcm(gcm, numpy.arange(1, n + 1), nL=nL, seed=2)
        ens.attach_fields(fields)
        ens.p["presf"] = presf.copy()
        if cls is HostEns:
            ens.p["QL"], ens.p["QT"] = ql_av.copy(), qt_av.copy()
        ens.ql_ref, ens.model_time = ql_ref, 900.0
        return ens

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    best = {"host": float("inf"), "device": float("inf")}
    qt_after = {}
    for rep in range(3):
        for name, cls in (("host", HostEns), ("device", models.DeviceLESEnsemble)):
            ens = make(cls)
            numpy.random.seed(7)
            best[name] = min(best[name], timed(lambda: spcpl.variability_nudge_ensemble(ens, 900.0, False, write=False)))
            if rep == 0:
                q = ens.fields3d["QT"]
                qt_after[name] = q[:2].cpu().numpy() if isinstance(q, torch.Tensor) else q[:2].copy()
            del ens
    same = numpy.array_equal(qt_after["host"], qt_after["device"])
    ratio = best["device"] / best["host"]
    print("variability_nudge_ensemble n=%d: host fields (the parent commit's path) %.1f ms, device fields %.1f ms, ratio %.3f "
          "(condition: <= 0.2: %s), nudged QT bit-equal=%s" % (n, best["host"] * 1e3, best["device"] * 1e3, ratio,
                                                               "met" if ratio <= 0.2 else "NOT met", same), flush=True)
    if not same:
        sys.exit("slab_bench: the nudged QT of the two paths differ")
    best = {"host": float("inf"), "device": float("inf")}
    for rep in range(2):
        for name, cls in (("host", HostEns), ("device", models.DeviceLESEnsemble)):
            ens = cls.for_gcm(gcm, numpy.arange(1, n + 1), nL=nL, seed=2)
            if cls is not HostEns:
                ens.itot, ens.jtot = itot, jtot
            numpy.random.seed(7)
            best[name] = min(best[name], timed(lambda: spcpl.set_les_state_batched(ens, *prof4)))
            del ens
    print("set_les_state_batched      n=%d: host fields %.1f ms, device fields %.1f ms, ratio %.3f (no threshold)"
          % (n, best["host"] * 1e3, best["device"] * 1e3, best["device"] / best["host"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="2,16,256,1024")
    ap.add_argument("--les", type=int, default=256)
    ap.add_argument("--section", default=None, help="(internal) run one section in this process")
    ap.add_argument("--copy-gbs", type=float, default=0.0)
    args = ap.parse_args()
    if args.section == "copybw":
        return section_copybw()
    if args.section == "k10":
        return section_k10([int(s) for s in args.sizes.split(",")], args.copy_gbs)
    if args.section == "paths":
        return section_paths(args.les)
    lines, copy_gbs = [], 0.0
    for section, limit in (("copybw", 120), ("k10", 400), ("paths", 500)):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--section", section, "--sizes", args.sizes,
               "--les", str(args.les), "--copy-gbs", str(copy_gbs)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines += r.stdout.splitlines()
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append("# section %s ended with status %d; nothing further was started" % (section, r.returncode))
            print(lines[-1] + "\n" + r.stderr[-3000:], flush=True)
            break
        if section == "copybw":
            copy_gbs = float(r.stdout.split()[1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# K10 and device-resident LES fields, %d x %d x %d float64 LES\n" % SHAPE + "\n".join(lines) + "\n")
    return 0 if lines and not lines[-1].startswith("# section") else 1


if __name__ == "__main__":
    sys.exit(main())
