#!/usr/bin/env python3
"""Engine.les_qt_local (K19) timed on the GPU at 256 LES of 8 x 8 x 160 and at 16 LES of 64 x 64 x 160, float64 and float32: HIP
events around a window of launches after pre-heating the clocks, five windows of at least 0.2 s per case, the minimum and the
spread (max - min) reported.  The forcing acts on the levels 30 ... 89 (a of random sign, 1e-9 in size so that thousands of
launches in place leave every cell on its side of the thresholds); the levels below and above are skipped, as above a cloud layer.
Two yardsticks from the same process:
  - the eager torch composition of the same rule on the same tensors (compare, count, two quotients, two masked updates; not
    checked for equal bits here): the only other way this tree could do it on the device;
  - the algorithmic bytes of the case, counted from the counts the launch returns: one field read for the count on the levels
    with a != 0, one (a > 0) or two (a < 0) reads and one write on the mixed ones, nothing on the skipped ones; per second, as a
    share of the 8 TB/s peak of the HBM (K11 at 256 LES of 64 x 64 x 160: 3 835 GB/s, 48 %: profiles/les_advance_bench.log).
Where the library would split the planes over several workgroups the forced split 1 (the fused launch) is timed beside it.
Each size runs as a child process of its own under a time limit; nothing is started after a failure.
Usage: python tools/les_qt_local_bench.py [--out profiles/les_qt_local_bench.log]"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.les_micro_bench import _events, _preheat      # noqa: E402

SIZES = ((256, 8, 8, 160), (16, 64, 64, 160))
ACTIVE = (30, 90)
WINDOWS = 5
PEAK = 8000.0                                                   # GB/s, the HBM's datasheet peak


def _windows(fn):
    t1 = _events(fn, 5)
    reps = int(max(20, min(20000, 0.2 / max(t1, 1e-7))))
    ts = [_events(fn, reps) for _ in range(WINDOWS)]
    return min(ts), max(ts) - min(ts), reps


def torch_rule(qt, ql, A, QTM):
    """the rule of include/spc.h as torch operations on whole tensors; qt updated in place, the counts returned"""
    import torch
    N = qt.shape[1] * qt.shape[2]
    a, m = A[:, None, None, :], QTM[:, None, None, :]
    wet = torch.where(a > 0, qt > m, (a < 0) & (ql > 0))
    c = wet.sum(dim=(1, 2))
    signed = (A > 0) | (A < 0)
    act = signed & (c > 0) & (c < N)
    s = A * N
    dw, dd = s / c.to(qt.dtype), s / (N - c).to(qt.dtype)
    new = torch.where(wet, qt + dw[:, None, None, :], qt - dd[:, None, None, :])
    qt.copy_(torch.where(act[:, None, None, :], new, qt))
    return torch.where(signed, c, torch.zeros_like(c))


def section_size(index):
    import torch
    from sp_coupler_amd.engine import Engine
    n, itot, jtot, ktot = SIZES[index]
    N = itot * jtot
    _preheat()
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        eng = Engine("cuda:0", dtype=dtype)
        gen = torch.Generator(device=eng.device).manual_seed(n)
        rnd = lambda *s: torch.rand(s, dtype=torch.float64, device=eng.device, generator=gen)       # noqa: E731
        base = 8e-3 * (1.0 - 0.5 * torch.arange(ktot, dtype=torch.float64, device=eng.device) / ktot)
        qt = (base + 2e-4 * (rnd(n, itot, jtot, ktot) - 0.5)).to(dtype)
        qsat = (base + 1e-4 * (rnd(n, 1, 1, ktot) - 0.5)).to(dtype)
        ql = (qt - qsat).clamp_min_(0.0)
        A = torch.zeros(n, ktot, dtype=torch.float64, device=eng.device)
        A[:, ACTIVE[0]:ACTIVE[1]] = 1e-9 * torch.where(rnd(n, ACTIVE[1] - ACTIVE[0]) < 0.5, -1.0, 1.0)
        A = A.to(dtype)
        QTM = eng.slab_means({"QT": qt})["QT"]
        start = qt.clone()
        count = eng.les_qt_local(qt, ql, A, QTM)
        torch.cuda.synchronize()
        mixed = (count > 0) & (count < N)
        cells = int((A != 0).sum()) + 2 * int((mixed & (A > 0)).sum()) + 3 * int((mixed & (A < 0)).sum())
        nbytes = cells * N * dtype.itemsize
        chosen = eng.qt_local_split(n, itot, jtot, ktot)
        qt.copy_(start)
        want = torch_rule(qt.clone(), ql, A, QTM)
        assert torch.equal(want.to(torch.int32), count), "the torch composition counts other cells"
        cases = [("library split %d" % chosen, 0)] + ([("forced split 1", 1)] if chosen != 1 else [])
        times = {}
        for tag, split in cases:
            qt.copy_(start)
            launch = lambda _r: eng.les_qt_local(qt, ql, A, QTM, count=count, split=split)          # noqa: E731
            launch(0)
            torch.cuda.synchronize()
            times[tag] = _windows(launch)
        qt.copy_(start)
        loop = lambda _r: torch_rule(qt, ql, A, QTM)                                                # noqa: E731
        loop(0)
        torch.cuda.synchronize()
        tt, tspread, treps = _windows(loop)
        assert bool(((eng.les_qt_local(qt, ql, A, QTM) > 0) == (count > 0)).all())                  # (the levels kept their classes)
        for tag, (t, spread, reps) in times.items():
            rate = nbytes / t / 1e9
            print("les_qt_local %s n=%-4d %d x %d x %d  %s: %9.4f ms per launch (min of %d windows of %d; spread %.4f ms)  levels a != 0: %d, mixed: %d"
                  "  %7.1f GB/s of the algorithmic bytes (%.1f MB)  %5.2f %% of the %.0f GB/s peak | torch composition %9.4f ms (windows of %d; spread"
                  " %.4f ms)  K19 / torch %.4f  faster beyond both spreads: %s"
                  % (name, n, itot, jtot, ktot, tag, t * 1e3, WINDOWS, reps, spread * 1e3, int((A != 0).sum()), int(mixed.sum()), rate, nbytes / 1e6,
                     100 * rate / PEAK, PEAK, tt * 1e3, treps, tspread * 1e3, t / tt, t + spread < tt - tspread), flush=True)
        del qt, ql, start
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--section", type=int, default=None, help="(internal) run one size in this process")
    args = ap.parse_args()
    if args.section is not None:
        return section_size(args.section)
    lines, failed = [], False
    for index in range(len(SIZES)):
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--section", str(index)]
        r = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True)
        lines += r.stdout.splitlines()
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append("# size %s ended with status %d; nothing further was started" % (SIZES[index], r.returncode))
            print(lines[-1] + "\n" + r.stderr[-3000:], flush=True)
            failed = True
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("# Engine.les_qt_local (K19), the forcing on the levels %d ... %d of 160\n" % (ACTIVE[0], ACTIVE[1] - 1) + "\n".join(lines) + "\n")
    return 1 if failed or not lines else 0


if __name__ == "__main__":
    sys.exit(main())
