#!/usr/bin/env python3
"""Engine.les_transport2 (K23) with both limiters timed on the GPU against K22 (Engine.les_transport), the first-order step it
replaces in the ensemble, at 256 LES of 8 x 8 x 160 and 16 LES of 64 x 64 x 160, five fields (U, V, THL, QT, QR; U and V are the
winds and fields at once), float64 and float32, all in ONE process: HIP events around a window of launches after pre-heating
the clocks, three windows per kernel and round, two rounds in which the three kernels ALTERNATE (MC, none, K22, then again), the
minimum and the spread (max - min) reported.  Every launch writes cmax, mtop and ftop, what the ensemble asks for.  The floor is
the stream copy of the same process (tools/libspc_tools.so, read + write) on the bytes of 2 + 2 NF passes over one field.  No
ratio is fixed in advance: the yardstick is K22 in the same run, the exit status is 0.
Usage: python tools/les_transport2_bench.py [--out profiles/les_transport2_bench.log]"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.les_micro_bench import WINDOWS, _windows, _copy_rate, _preheat      # noqa: E402

NAMES = ("U", "V", "THL", "QT", "QR")
PASSES = 2 + 2 * len(NAMES)
SHAPES = ((256, 8, 8, 160), (16, 64, 64, 160))
ROUNDS = 2
DT = 10.0


def case(shape, dtype, name):
    """one line of the log"""
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
    out = {k: torch.empty_like(x) for k, x in fields.items()}
    mtop = torch.empty_like(fields["U"])
    ftop = torch.empty((len(NAMES),) + shape[:3], dtype=dtype, device=eng.device)
    cmax = torch.empty(n, dtype=dtype, device=eng.device)
    kernels = {
        "K23 mc": lambda _r: eng.les_transport2(fields, out, fields["U"], fields["V"], hx, hy, g, r, limiter="mc", cmax=cmax, mtop=mtop, ftop=ftop),
        "K23 none": lambda _r: eng.les_transport2(fields, out, fields["U"], fields["V"], hx, hy, g, r, limiter="none", cmax=cmax, mtop=mtop, ftop=ftop),
        "K22": lambda _r: eng.les_transport(fields, out, fields["U"], fields["V"], hx, hy, g, r, cmax=cmax, mtop=mtop, ftop=ftop)}
    best = {}
    for fn in kernels.values():
        fn(0)
    torch.cuda.synchronize()
    c = float(cmax.max())
    for _ in range(ROUNDS):                                        # the kernels alternate: none of them has the warmer clocks
        for tag, fn in kernels.items():
            t, spread, reps = _windows(fn)
            if tag not in best or t < best[tag][0]:
                best[tag] = (t, spread, reps)
    floor = nbytes / (copy * 1e9)
    t22 = best["K22"][0]
    line = "les_transport2 %s %d x %d x %d x %d cols %d cmax %.3f" % ((name,) + tuple(shape) + (eng.transport2_cols_per_block(ktot), c))
    for tag in kernels:
        t, spread, reps = best[tag]
        line += " | %s %8.3f ms (min of %d x %d windows of %d; spread %.3f ms)" % (tag, t * 1e3, ROUNDS, WINDOWS, reps, spread * 1e3)
    line += " | K23 mc / K22 %.2f  K23 none / K22 %.2f" % (best["K23 mc"][0] / t22, best["K23 none"][0] / t22)
    line += " | copy floor of %d passes %8.3f ms at %.0f GB/s  K23 mc / floor %.2f  K23 none / floor %.2f  K22 / floor %.2f" % (
        PASSES, floor * 1e3, copy, best["K23 mc"][0] / floor, best["K23 none"][0] / floor, t22 / floor)
    del fields, out, mtop, ftop
    torch.cuda.empty_cache()
    return line


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _preheat()
    lines = ["# Engine.les_transport2 (K23, both limiters) against Engine.les_transport (K22) on %s, %d fields" % (torch.cuda.get_device_name(0), len(NAMES))]
    for shape in SHAPES:
        for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
            line = case(shape, dtype, name)
            print(line, flush=True)
            lines.append(line)
    lines.append("# not measured: more than one device, other field counts, the ensemble's step, where inside the kernel the time goes")
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
