#!/usr/bin/env python3
"""Times the initial LES state (K9: spcpl.set_les_state_batched / Engine.les_state) against the host loop of the reference
(spcpl.set_les_state per LES) for 16 / 256 / 1 024 LES of 64 x 64 x 160.  Clocks are pre-heated by repeated launches
first.  Reports, per size: the device call (Engine.les_state: jump rounds + generation, fields left in HBM; host clock around
a call that ends in a stream synchronise) with its write rate against HBM (4 float64 fields per LES), the whole
set_les_state_batched call (fields to the host, set_field on LES that discard them), and the host loop (timed at 16 LES;
at the larger sizes it is that per-LES time times n, marked as such).  Every timed result is checked bit for bit against
the host loop on the first LES.  Usage: python tools/les_state_bench.py [--out FILE] [--sizes 16,256,1024]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine

SHAPE = (64, 64, 160)
HBM_PEAK = 8.0e12          # MI355X spec (MI355X_MICROARCH: ~6.3 TB/s achievable)


class NullLES:
    def __init__(self, keep=False):
        self.keep, self.got = keep, []

    def get_itot(self):
        return SHAPE[0]

    def get_jtot(self):
        return SHAPE[1]

    def get_ktot(self):
        return SHAPE[2]

    def set_field(self, name, values):
        if self.keep:
            self.got.append(numpy.array(values))

    def set_surface_pressure(self, ps):
        pass


def profiles(n):
    rng = numpy.random.default_rng(1)
    k = SHAPE[2]
    return [rng.normal(5.0, 1.0, (n, k)), rng.normal(-3.0, 1.0, (n, k)), rng.normal(300.0, 5.0, (n, k)), rng.uniform(0, 0.02, (n, k))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="16,256,1024")
    ap.add_argument("--device-only", action="store_true", help="only the device calls (for a rocprofv3 --kernel-trace run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("les_state_bench: needs a GPU (no CPU fallback)")
    eng = Engine("cuda:0")
    spcpl.set_engine(eng)
    sizes = [int(s) for s in args.sizes.split(",")]
    V = SHAPE[0] * SHAPE[1] * SHAPE[2]
    lines = ["# initial LES state, %d x %d x %d per LES, on %s (torch %s, numpy %s)" % (SHAPE + (torch.cuda.get_device_name(0),
             torch.__version__, numpy.__version__))]

    # the host loop at 16 LES (the reference's arithmetic: numpy.random.uniform + scale + add, 4 fields per LES)
    n0 = 16
    host_per_les = None
    if not args.device_only:
        u, v, thl, qt = profiles(n0)
        numpy.random.seed(42)
        t0 = time.perf_counter()
        host_les = [NullLES(keep=(l == 0)) for l in range(n0)]
        for l, les in enumerate(host_les):
            spcpl.set_les_state(les, u[l], v[l], thl[l], qt[l])
        host_per_les = (time.perf_counter() - t0) / n0
        lines.append("host loop: %.1f ms per LES (one host core, measured at %d LES)" % (host_per_les * 1e3, n0))
        print(lines[-1], flush=True)

    # pre-heat: device launches for ~2 s
    n_heat = min(sizes[0], 256) if args.device_only else 256
    u, v, thl, qt = profiles(n_heat)
    t_end = time.perf_counter() + 2.0
    while time.perf_counter() < t_end:
        eng.les_state([SHAPE] * n_heat, u, v, thl, qt, numpy.random.get_state())
    for n in sizes:
        u, v, thl, qt = profiles(n)
        st = numpy.random.get_state()
        reps = 5 if n <= 256 else 2
        best = float("inf")
        for _ in range(reps):
            fields = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fields, _ = eng.les_state([SHAPE] * n, u, v, thl, qt, st)
            best = min(best, time.perf_counter() - t0)
            del fields
        nbytes = 4 * 8 * V * n
        lines.append("n=%-5d device call (Engine.les_state, fields stay in HBM) %9.2f ms  %.2f TB/s written (%.0f %% of 8 TB/s)"
                     % (n, best * 1e3, nbytes / best / 1e12, 100 * nbytes / best / HBM_PEAK))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
        if n <= 256 and not args.device_only:
            numpy.random.seed(42)
            les = [NullLES(keep=(l == 0)) for l in range(n)]
            t0 = time.perf_counter()
            spcpl.set_les_state_batched(les, u, v, thl, qt)
            dt = time.perf_counter() - t0
            numpy.random.seed(42)
            ref = NullLES(keep=True)
            spcpl.set_les_state(ref, u[0], v[0], thl[0], qt[0])
            same = all(numpy.array_equal(a, b) for a, b in zip(les[0].got, ref.got))
            host = host_per_les * n
            lines.append("n=%-5d set_les_state_batched (fields to the host) %9.2f ms  host loop %s %9.1f ms  -> %.1fx  bit-equal=%s"
                         % (n, dt * 1e3, "measured" if n == n0 else "16-LES rate x n", host * 1e3, host / dt, same))
            print(lines[-1], flush=True)
            if not same:
                sys.exit("les_state_bench: batched fields differ from the host loop")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
