#!/usr/bin/env python3
"""Engine.les_transport (K22) timed on the GPU against what it replaces, K16 followed by K17 (Engine.les_advect into spare
buffers, then Engine.les_vadvect on those with the winds K16 produced, as DeviceLESEnsemble runs them), at 256 LES of
8 x 8 x 160 and 16 LES of 64 x 64 x 160, five fields (U, V, THL, QT, QR; U and V are the winds and fields at once), float64 and
float32, all in ONE process: HIP events around a window of launches after pre-heating the clocks, three windows per case, the
minimum and the spread (max - min) reported.  K17 and K22 write mtop, K22 writes ftop as well, every launch writes cmax: what
the ensemble asks of them.  The floor is the stream copy of the same process (tools/libspc_tools.so, read + write) on the
bytes of 2 + 2 NF passes over one field; the pair moves 4 + 4 NF.  The probe (n_fields == 0 with cmax) is timed next to
them.  Exit status 1 where K22 takes longer than the pair at any case.
Usage: python tools/les_transport_bench.py [--out profiles/les_transport_bench.log]"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.les_micro_bench import WINDOWS, _windows, _copy_rate, _preheat      # noqa: E402

NAMES = ("U", "V", "THL", "QT", "QR")
PASSES = 2 + 2 * len(NAMES)
SHAPES = ((256, 8, 8, 160), (16, 64, 64, 160))
DT = 10.0


def case(shape, dtype, name):
    """one line of the log and whether K22 was no slower than the pair"""
    import numpy
    import torch
    from sp_coupler_amd import advection as adv
    from sp_coupler_amd.engine import Engine
    eng = Engine("cuda:0", dtype=dtype)
    n, ktot = shape[0], shape[3]
    cells = shape[0] * shape[1] * shape[2] * shape[3]
    nbytes = PASSES * cells * dtype.itemsize
    copy = _copy_rate(nbytes)
    gen = torch.Generator(device=eng.device).manual_seed(n)
    rnd = lambda: torch.rand(shape, dtype=dtype, device=eng.device, generator=gen)                  # noqa: E731
    up = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device, dtype)             # noqa: E731
    hx, hy = (up(a) for a in adv.coefficients(DT, n=n))
    k = numpy.arange(ktot, dtype=numpy.float64)
    g, r = (up(a) for a in adv.vertical_profiles(numpy.tile(1.15 * numpy.exp(-k / 400.0) * (20.0 + 0.25 * k), (n, 1))))
    fields = {"U": rnd().mul_(10.0).sub_(5.0), "V": rnd().mul_(10.0).sub_(5.0), "THL": rnd().mul_(10.0).add_(285.0), "QT": rnd().mul_(0.02),
              "QR": rnd().mul_(1e-4)}
    mid = {k: torch.empty_like(x) for k, x in fields.items()}
    out = {k: torch.empty_like(x) for k, x in fields.items()}
    mtop = torch.empty_like(fields["U"])
    ftop = torch.empty((len(NAMES),) + shape[:3], dtype=dtype, device=eng.device)
    cmax = torch.empty(n, dtype=dtype, device=eng.device)
    k22 = lambda _r: eng.les_transport(fields, out, fields["U"], fields["V"], hx, hy, g, r, cmax=cmax, mtop=mtop, ftop=ftop)      # noqa: E731

    def pair(_r):
        eng.les_advect(fields, mid, fields["U"], fields["V"], hx, hy, cmax=cmax)
        eng.les_vadvect(mid, out, mid["U"], mid["V"], hx, hy, g, r, cmax=cmax, mtop=mtop)
    k22(0)
    torch.cuda.synchronize()
    c = float(cmax.max())
    t, spread, reps = _windows(k22)
    pair(0)
    torch.cuda.synchronize()
    tp, pspread, preps = _windows(pair)
    t2, spread2, _ = _windows(k22)                                 # (again after the pair: the order of the two is not what is measured)
    if t2 < t:
        t, spread = t2, spread2
    probe = lambda _r: eng.les_transport({}, {}, fields["U"], fields["V"], hx, hy, g, r, cmax=cmax)                              # noqa: E731
    tq, qspread, qreps = _windows(probe)
    floor = nbytes / (copy * 1e9)
    line = ("les_transport %s %d x %d x %d x %d cols %d cmax %.3f | K22 %8.3f ms (min of 2 x %d windows of %d; spread %.3f ms)"
            " | K16 + K17 %8.3f ms (windows of %d; spread %.3f ms)  K22 / pair %.3f"
            " | copy floor of %d passes %8.3f ms at %.0f GB/s  K22 / floor %.2f"
            " | probe (the winds alone: phases 1 and 2 and the Courant sums) %8.3f ms (windows of %d; spread %.3f ms)"
            % ((name,) + tuple(shape) + (eng.transport_cols_per_block(ktot), c, t * 1e3, WINDOWS, reps, spread * 1e3, tp * 1e3, preps, pspread * 1e3,
                                         t / tp, PASSES, floor * 1e3, copy, t / floor, tq * 1e3, qreps, qspread * 1e3)))
    del fields, mid, out, mtop, ftop
    torch.cuda.empty_cache()
    return line, t <= tp


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _preheat()
    lines, ok = ["# Engine.les_transport (K22) against K16 + K17 on %s, %d fields" % (torch.cuda.get_device_name(0), len(NAMES))], True
    for shape in SHAPES:
        for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
            line, fine = case(shape, dtype, name)
            print(line, flush=True)
            lines.append(line)
            ok = ok and fine
    lines.append("# not measured: more than one device, other field counts, the ensemble's step; K22 %s the pair at every case"
                 % ("is no slower than" if ok else "IS SLOWER THAN"))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
