#!/usr/bin/env python3
"""K13 timed on the GPU (64 x 64 x 160 LES): Engine.les_water_paths with 1 field and with 3 fields plus the cloud outputs (top,
cover), float64 and float32, at 2, 16, 256 and 1 024 LES.

Per case: HIP events around a window of launches after the clocks were pre-heated, the inputs rotated through more sets than
the 256 MiB Infinity Cache holds where one set fits it; the MINIMUM of three windows with their spread; the bytes read per
time as a share of the stream-copy rate (tools/libspc_tools.so, 1 GiB, read + write bytes) measured in the SAME process just
before.  For scale, the time of ``torch.sum(q * w[:, None, None, :], dim=3)`` for every field on the same tensors: the unfused
alternative, which writes and re-reads the product and is not bit-equal to NumPy.
One child process under a time limit does all of it.
Usage: python tools/les_water_paths_bench.py [--out profiles/les_water_paths_bench.log] [--sizes 2,16,256,1024]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = (64, 64, 160)


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
    """(minimum, maximum) of three windows of launches, seconds per launch"""
    t1 = _events(fn, 3)
    reps = int(max(5, min(400, 0.3 / max(t1, 1e-6))))
    ts = [_events(fn, reps) for _ in range(3)]
    return min(ts), max(ts), reps


def section(sizes):
    import torch
    from sp_coupler_amd.engine import Engine
    from tools import spc_tools
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    s = torch.cuda.current_stream()
    for _ in range(5):
        spc_tools.stream_copy(dst, src, s)
    t = _events(lambda r: spc_tools.stream_copy(dst, src, s), 20)
    copy_gbs = 2 * src.numel() / t / 1e9
    print("copybw %.1f GB/s (read + write, 1 GiB stream copy, this process)" % copy_gbs, flush=True)
    del src, dst
    for dtype, tag, esize in ((torch.float64, "f64", 8), (torch.float32, "f32", 4)):
        eng = Engine("cuda:0", dtype=dtype)
        heat = {"QL": torch.rand((16,) + SHAPE, dtype=dtype, device=eng.device)}
        hw = torch.rand((16, SHAPE[2]), dtype=dtype, device=eng.device)
        t_end = time.perf_counter() + 2.0
        while time.perf_counter() < t_end:                          # pre-heat the clocks
            eng.les_water_paths(heat, hw)
            torch.cuda.synchronize()
        del heat, hw
        for n in sizes:
            for names in (("QL",), ("QL", "QT", "QR")):
                F = len(names)
                set_bytes = F * n * SHAPE[0] * SHAPE[1] * SHAPE[2] * esize
                nsets = max(1, min(4, -(-(512 << 20) // set_bytes)))     # rotate through >= 512 MiB where one set is smaller
                sets = [{k: torch.rand((n,) + SHAPE, dtype=dtype, device=eng.device) for k in names} for _ in range(nsets)]
                for st in sets:
                    st["QL"].sub_(0.97).clamp_min_(0.0)                  # 3 % of the cells cloudy
                w = torch.rand((n, SHAPE[2]), dtype=dtype, device=eng.device) + 1.0
                out = {k: torch.empty((n,) + SHAPE[:2], dtype=dtype, device=eng.device) for k in names}
                cloud = F > 1
                top = torch.empty((n,) + SHAPE[:2], dtype=torch.int32, device=eng.device) if cloud else False
                cover = torch.empty((n,), dtype=dtype, device=eng.device) if cloud else False
                run = lambda r: eng.les_water_paths(sets[r % nsets], w, cloud="QL" if cloud else None, out=out, top=top, cover=cover)   # noqa: E731
                run(0)
                torch.cuda.synchronize()
                lo, hi, reps = _windows(run)
                rate = set_bytes / lo / 1e9
                wb = w[:, None, None, :]
                ref = lambda r: [torch.sum(sets[r % nsets][k] * wb, dim=3) for k in names]                      # noqa: E731
                ref(0)
                torch.cuda.synchronize()
                tlo, thi, _ = _windows(ref)
                print("les_water_paths %s n=%-5d F=%d%s %10.3f ms per call (max of 3 windows %10.3f)  %8.1f GB/s read  %5.1f %% of the copy "
                      "bandwidth (%d input sets, %d calls per window) | torch.sum(q * w, dim=3) x %d: %10.3f ms (max %10.3f), ratio %.2f"
                      % (tag, n, F, " + top, cover" if cloud else "             ", lo * 1e3, hi * 1e3, rate, 100 * rate / copy_gbs, nsets, reps,
                         F, tlo * 1e3, thi * 1e3, lo / tlo), flush=True)
                del sets, out, w, wb
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="2,16,256,1024")
    ap.add_argument("--section", action="store_true", help="(internal) run the measurements in this process")
    args = ap.parse_args()
    if args.section:
        return section([int(s) for s in args.sizes.split(",")])
    cmd = ["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--section", "--sizes", args.sizes]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    print(r.stdout, end="", flush=True)
    if r.returncode != 0:
        lines.append("# the measurements ended with status %d" % r.returncode)
        print(lines[-1] + "\n" + r.stderr[-3000:], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# K13, %d x %d x %d LES\n" % SHAPE + "\n".join(lines) + "\n")
    return 0 if r.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
