"""Loader of tests/golden/ref_*.npz -- what the reference's own functions returned (tests/golden/make_reference_goldens.py) --
and the comparisons tests/test_reference_pins_cpu.py and tests/test_reference_pins_gpu.py share.  Reads tests/golden/ only.

A ``Tally`` counts, per family, how many recorded arrays a test compared and how many of them needed a tolerance."""
import glob
import os

import numpy

from tests.gpu_util import assert_bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXCHANGE = ("edge", "geo19", "geo137", "runtime")
THICK_NL = (240, 480, 960, 2000)
GCM_VARS = ["U", "V", "T", "SH", "QL", "QI", "Pfull", "Phalf", "A", "Zgfull", "Zghalf"]
FWD_BITS = ("f_u", "f_v", "f_qt", "f_ql", "f_ps", "ql_ref", "z0m", "z0h", "wqt", "Zf", "Zh", "u", "v", "qt", "ps")   # no pow()
FWD_POW = ("thl", "f_thl", "wthl")                                                                                    # through iexner
TEND = ("f_T", "f_SH", "f_QL", "f_QI", "f_U", "f_V", "f_A")
_cache = {}


def load(stem):
    if stem not in _cache:
        with numpy.load(os.path.join(GOLDEN, stem + ".npz"), allow_pickle=False) as z:
            _cache[stem] = {k: z[k] for k in z.files}
    return _cache[stem]


def stems(family):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "ref_%s_*.npz" % family)))


def exchange(family):
    """(gcm, zf, zh, prof, factor, dt, ref) of a column-exchange family, its files joined along the column axis; the arrays
    are read-only"""
    key = "exchange:" + family
    if key not in _cache:
        parts = [load(s) for s in stems(family)]
        assert parts and [int(p["in_first_column"]) for p in parts] == list(numpy.cumsum([0] + [p["in_gcm_T"].shape[0] for p in parts[:-1]]))
        per_col = parts[0]["in_zf"].ndim == 2
        joined = {}
        for k in parts[0]:
            if k.startswith("meta_") or k in ("in_factor", "in_dt", "in_first_column") or (k in ("in_zf", "in_zh") and not per_col):
                joined[k] = parts[0][k]
                assert all(numpy.array_equal(p[k], parts[0][k]) for p in parts) or k == "in_first_column"
            else:
                joined[k] = numpy.ascontiguousarray(numpy.concatenate([p[k] for p in parts]))
        for v in joined.values():
            v.setflags(write=False)
        gcm = {k[7:]: v for k, v in joined.items() if k.startswith("in_gcm_")}
        prof = {k[7:]: v for k, v in joined.items() if k.startswith("in_les_")}
        ref = {k: v for k, v in joined.items() if not k.startswith(("in_", "meta_"))}
        _cache[key] = (gcm, joined["in_zf"], joined["in_zh"], prof, float(joined["in_factor"]), float(joined["in_dt"]), ref)
    return _cache[key]


def thick(nL):
    d = load("ref_thick_%d" % nL)
    gcm = {k[7:]: v for k, v in d.items() if k.startswith("in_gcm_")}
    prof = {k[7:]: v for k, v in d.items() if k.startswith("in_les_")}
    ref = {k: v for k, v in d.items() if not k.startswith(("in_", "meta_"))}
    return gcm, d["in_zf"], d["in_zh"], prof, float(d["in_factor"]), float(d["in_dt"]), d["in_integral_ab"], ref


class Tally:
    """compares and counts: ``bits`` (tests.gpu_util.assert_bits: NaN positions and the sign of zero included) and ``close``
    (|got - want| <= tol * scale where the reference is finite, equal bits where it is not)"""

    def __init__(self, family):
        self.family, self.n_bits, self.n_tol = family, 0, 0

    def bits(self, name, got, want):
        assert_bits("%s %s" % (self.family, name), got, want)
        self.n_bits += 1

    def close(self, name, got, want, tol, scale=None):
        got, want = numpy.asarray(got), numpy.asarray(want)
        name = "%s %s" % (self.family, name)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        fin = numpy.isfinite(want)
        assert numpy.array_equal(numpy.isfinite(got), fin), name + ": non-finite positions differ"
        assert_bits(name + " (non-finite)", got[~fin], want[~fin])
        if scale is None:
            scale = numpy.abs(want[fin]).max()
        err = numpy.abs(got[fin] - want[fin]).max() if fin.any() else 0.0
        assert err <= tol * scale, "%s: max abs err %.3e > %.3e (tol %.1e x scale %.3e)" % (name, err, tol * scale, tol, scale)
        self.n_tol += 1

    def rel(self, name, got, want, tol, keep=None):
        """|got - want| <= tol * |want| element by element (where ``keep``)"""
        got, want = numpy.asarray(got), numpy.asarray(want)
        assert got.shape == want.shape, (self.family, name, got.shape, want.shape)
        keep = numpy.ones(want.shape, dtype=bool) if keep is None else keep
        with numpy.errstate(invalid="ignore"):               # inf - inf outside ``keep``
            rel = numpy.abs(got - want)[keep] / numpy.maximum(numpy.abs(want[keep]), 1e-300)
        assert rel.max() <= tol, "%s %s: max rel err %.3e > %.1e" % (self.family, name, rel.max(), tol)
        self.n_tol += 1

    def report(self):
        print("reference pins %-8s: %3d arrays compared, %d of them with a tolerance" % (self.family, self.n_bits + self.n_tol, self.n_tol))


def finite_max(a):
    a = numpy.asarray(a)
    return numpy.abs(a[numpy.isfinite(a)]).max()
