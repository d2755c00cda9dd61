#!/usr/bin/env python3
"""Engine.les_thermo (K12) timed on the GPU at LES of 64 x 64 x 160, float64 and float32, with the saturation-pressure table
staged in LDS and read from global memory: HIP events around a window of launches after pre-heating the clocks, three windows
per case, the minimum and the spread (max - min) reported.  The bytes of a launch (thl and qt read, qsat and ql written; the
means and the profiles are noise) per second are set against the stream copy of the same visit on the same number of bytes
(tools/libspc_tools.so, read + write, as tools/copybw.py measures it).
Each size runs as a child process of its own under a time limit; nothing is started after a failure.
Usage: python tools/les_thermo_bench.py [--sizes 16,256,1024] [--n-iter N] [--temp] [--out profiles/les_thermo_bench.log]"""
import argparse
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (64, 64, 160)
CELLS = SHAPE[0] * SHAPE[1] * SHAPE[2]
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


def section_size(n, n_iter, want_temp):
    import torch
    from sp_coupler_amd import _abi, thermo
    from sp_coupler_amd.engine import Engine
    n_iter = thermo.DEFAULT_N_ITER if n_iter is None else n_iter
    streams = 5 if want_temp else 4
    t_end = time.perf_counter() + 2.0
    heat = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    while time.perf_counter() < t_end:                             # pre-heat the clocks
        heat.add_(1)
        torch.cuda.synchronize()
    del heat
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        eng = Engine("cuda:0", dtype=dtype)
        nbytes = streams * n * CELLS * dtype.itemsize
        copy = _copy_rate(nbytes)
        gen = torch.Generator(device=eng.device).manual_seed(n)
        shape = (n,) + SHAPE
        presf = (1e5 - torch.linspace(0.0, 4e4, SHAPE[2], dtype=torch.float64, device=eng.device)).repeat(n, 1)
        ex = ((presf / 1e5) ** (287.04 / 1004.)).to(dtype)
        presf = presf.to(dtype)
        thl = torch.randn(shape, dtype=dtype, device=eng.device, generator=gen).mul_(4.0).add_(292.0)
        qt = torch.rand(shape, dtype=dtype, device=eng.device, generator=gen).mul_(1.2e-2).add_(2e-3)    # about half of the cells cloudy
        qsat, ql = torch.empty_like(thl), torch.empty_like(thl)
        temp = torch.empty_like(thl) if want_temp else None
        means = {k: torch.empty((n, SHAPE[2]), dtype=dtype, device=eng.device) for k in ("QL", "T")}
        for mode, label in ((_abi.THERMO_TABLE_LDS, "table in LDS"), (_abi.THERMO_TABLE_GLOBAL, "table in global memory")):
            launch = lambda _r: eng.les_thermo(thl, qt, presf, ex, n_iter=n_iter, qsat=qsat, ql=ql, temp=temp, means=means, table_mode=mode)   # noqa: E731
            launch(0)
            torch.cuda.synchronize()
            t, spread, reps = _windows(launch)
            rate = nbytes / t / 1e9
            print("les_thermo %s n=%-4d n_iter=%d %-22s %9.3f ms per launch (min of %d windows of %d; spread %.3f ms)  %7.1f GB/s of %d streams"
                  "  %5.1f %% of the copy rate %.0f GB/s on the same bytes  cloudy %.2f"
                  % (name, n, n_iter, label, t * 1e3, WINDOWS, reps, spread * 1e3, rate, streams, 100 * rate / copy, copy,
                     float((ql[:1] > 0).double().mean())), flush=True)
        del thl, qt, qsat, ql, temp
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,256,1024")
    ap.add_argument("--n-iter", type=int, default=None)
    ap.add_argument("--temp", action="store_true", help="write the temp field too (a fifth stream)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--section", default=None, help="(internal) run one section in this process")
    ap.add_argument("--n", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    if args.section == "size":
        return section_size(args.n, args.n_iter, args.temp)
    lines, failed = [], False
    for n in (int(s) for s in args.sizes.split(",")):
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--section", "size", "--n", str(n)]
        cmd += (["--n-iter", str(args.n_iter)] if args.n_iter is not None else []) + (["--temp"] if args.temp else [])
        r = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True)
        lines += r.stdout.splitlines()
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append("# n=%d ended with status %d; nothing further was started" % (n, r.returncode))
            print(lines[-1] + "\n" + r.stderr[-3000:], flush=True)
            failed = True
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("# Engine.les_thermo (K12), %d x %d x %d LES\n" % SHAPE + "\n".join(lines) + "\n")
    return 1 if failed or not lines else 0


if __name__ == "__main__":
    sys.exit(main())
