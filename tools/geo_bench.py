#!/usr/bin/env python3
"""Times sputils.get_mask_indices (K8: k_point_in_polygon / k_haversine) at the column counts of T159 (35 718), T511
(348 528) and TCo1279 (6 599 680) for three masks: the infinite box (spmaster.py --all), a 2 000-vertex polygon and 8 points.
Reports ms per call (host clock around calls that end in a device synchronise, after warm-up) and, for the polygon,
point x edge tests per second (2 images per point).  For context: the NumPy oracle (tests/geo_ref.py) on one host core at
the smallest size.  Usage: python tools/geo_bench.py [--out FILE] [--reps N]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch

from sp_coupler_amd import geometry, spcpl, sputils
from sp_coupler_amd.engine import Engine

SIZES = (35718, 348528, 6599680)


def grid(n):
    """n points on latitude rings, fewer towards the poles (reduced-Gaussian-like), longitudes 0 ... 360"""
    n_lat = int(numpy.sqrt(n / 1.3))
    lats = numpy.linspace(89.5, -89.5, n_lat)
    counts = numpy.maximum(4, numpy.cos(numpy.radians(lats)) * 2.6 * n_lat)
    counts = numpy.floor(counts * n / counts.sum()).astype(int)
    counts[n_lat // 2] += n - counts.sum()
    lon = numpy.concatenate([numpy.arange(c) * (360.0 / c) for c in counts])
    lat = numpy.concatenate([numpy.full(c, la) for c, la in zip(counts, lats)])
    return numpy.stack([lon, lat], axis=1)


def star(nv):
    k = numpy.arange(nv)
    r = numpy.where(k % 2 == 0, 40.0, 25.0)
    a = 2 * numpy.pi * k / nv
    return list(zip((10.0 + r * numpy.cos(a)).tolist(), (0.9 * r * numpy.sin(a)).tolist()))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("geo_bench: needs a GPU (no CPU fallback)")
    spcpl.set_engine(Engine("cuda:0"))
    poly = geometry.Polygon(star(2000))
    masks = {"infinite box": [geometry.box(-float("inf"), -float("inf"), float("inf"), float("inf"))],
             "polygon 2000 vertices": [poly],
             "8 points": [geometry.Point((15.0 * k, 40.0 - 10.0 * k)) for k in range(8)]}
    lines = ["# sputils.get_mask_indices on %s (torch %s); host ms per call incl. upload of the points and list(set()) of the result"
             % (torch.cuda.get_device_name(0), torch.__version__)]
    for n in SIZES:
        pts = grid(n)
        dev = torch.from_numpy(pts).cuda()
        for name, m in masks.items():
            for form, arg in (("host array", pts), ("device tensor", dev)):
                ms = timed(lambda: sputils.get_mask_indices(arg, m), args.reps)
                sel = len(sputils.get_mask_indices(arg, m))
                extra = ""
                if name.startswith("polygon"):
                    tests = 2.0 * n * (len(poly.exterior.coords) - 1)
                    extra = "  %.3g point x edge tests/s" % (tests / (ms * 1e-3))
                lines.append("n=%-8d %-22s %-13s %9.3f ms  selected %8d%s" % (n, name, form, ms, sel, extra))
                print(lines[-1], flush=True)
    from tests import geo_ref
    pts = grid(SIZES[0])
    vx, vy, start, role, rp, npoly = geometry.pack(*geometry.as_mask(poly))
    t0 = time.perf_counter()
    geo_ref.locations(pts[:, 0], pts[:, 1], vx, vy, start, role, rp, npoly)
    ms = (time.perf_counter() - t0) * 1e3
    lines.append("n=%-8d %-22s %-13s %9.1f ms  (NumPy oracle tests/geo_ref.py, one host core: context only)" % (SIZES[0], "polygon 2000 vertices", "host", ms))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
