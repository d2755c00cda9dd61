"""K6, the variability nudge, at the edges of its kernels (sp_coupler_amd/csrc/spc_vnudge.hpp, spc_vnudge2.hpp,
spc_vnudge_host.hpp): the inputs as NumPy arrays (tests/test_vnudge_edges_cpu.py states on the CPU that the reference alone
reaches what each body claims) and the bodies of the GPU tests, each taking an engine (tests/test_vnudge_edges_gpu.py hands
them Engine("cuda:0", dtype); tools/mutation_control.py --vnudge hands them the engines of its mutant libraries).  A helper
module, not collected.

A body builds FieldLES objects, runs spcpl.variability_nudge_batched(les, 900.0, constantT, write=False) on the engine --
both constantT values, the device routes of tests/test_vnudge.py::test_kernel_matches_the_numpy_scipy_oracle chosen through
the environment, which vnudge_impl reads at every launch -- and compares with oracle/vnudge_oracle.py (float64) or
tests/vnudge_f32_ref.py (float32), R from vo.make_R under the same numpy.random.seed: status, beta, a, alpha, the updated qt
and qt_std value for value (NaN where the reference has NaN, everything else bit for bit, the signs of zeros and infinities
included); thl under constantT within the bounds of the two existing files (8 ulp of float64, THL_ULP of float32) where the
reference is not NaN, and NaN where it is.

The old matrix (old_matrix) is the shape matrix of test_kernel_matches_the_numpy_scipy_oracle and of its float32 copy: the
two tests call it with their own assertions, the mutation control calls it on every mutant library ("old guard")."""
import contextlib
import os

import numpy
import torch

from oracle import vnudge_oracle as vo
from tests import vnudge_f32_ref as v32
from tests.les_harness import DTYPES, NP, run_bodies  # noqa: F401  (DTYPES: for the tests)
from tests.test_vnudge import FieldLES, make_les_fields

BODIES = ("designed_levels", "tall", "std_many_workgroups", "small_trees", "chunk_edges", "ragged_columns")
EPS64, EPS32 = float(numpy.finfo(numpy.float64).eps), float(numpy.finfo(numpy.float32).eps)
THL_ULP = {torch.float64: 8, torch.float32: 4}      # the bounds of tests/test_vnudge.py and tests/test_vnudge_f32_gpu.py (THL_ULP)

#: device routes of the solve: the environment of vnudge_impl (spc_vnudge_host.hpp)
ROUTES = {"default": {}, "pair": {"SPC_VN_PAIR": "2"}, "strided": {"SPC_VN_TRANSPOSE": "0"}, "global": {"SPC_VN_GLOBAL": "1"}}
TWO_ROUTES, FOUR_ROUTES = ("default", "global"), ("default", "pair", "strided", "global")


@contextlib.contextmanager
def route(name):
    """the environment of one device route, restored afterwards (no monkeypatch: the mutation control runs without pytest)"""
    env = dict({"SPC_VN_GLOBAL": "0", "SPC_VN_PAIR": "1", "SPC_VN_TRANSPOSE": "1"}, **ROUTES[name])
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# -- the host's arithmetic, restated (spc_vnudge_host.hpp, spc_vnudge.hpp) ---------------------------------------------------
def leaf_sizes(n):
    """the leaves of numpy's pairwise sum over n elements, chunk by chunk: [[leaf lengths of chunk 0], ...] (vn_build_tree)"""
    def split(m):
        if m <= 128:
            return [m]
        n2 = m // 2
        n2 -= n2 % 8
        return split(n2) + split(m - n2)
    return [split(min(8192, n - c0)) for c0 in range(0, n, 8192)]


def std_workgroups(n_cols, ktot):
    """(workgroups of k_vnudge_std, its ROWS): 16 levels per workgroup; 512 rows up to 256 workgroups, 256 beyond"""
    wg = (ktot + 15) // 16 * n_cols
    return wg, (512 if wg <= 256 else 256)


def argmax_segment(nij, TL):
    """elements per lane of the argmax scan of a level that has TL threads (k_vnudge_solve)"""
    return (nij + TL - 1) // TL


# -- inputs: the twelve designed levels --------------------------------------------------------------------------------------
#: the statuses the twelve levels are built for (VN_MULT 1, VN_UNSAT 2, VN_ADD 4, VN_ADD_SKIPPED 8, VN_NO_BRACKET 16)
DESIGNED_STATUS = (0, 2, 1, 0, 2, 2, 10, 24, 1, 5, 2, 1)
DESIGNED_PLANES = ((9, 7), (2, 3), (1, 1), (1, 8), (3, 3), (64, 64), (92, 92))


def designed_dropped(nij):
    """levels a plane of nij points is too small for (they stay clear): the tie needs two points; the additive search of level
    9 needs a noise plane that is not zero (R of a single point is R - R = 0); level 10 needs three points"""
    return tuple(k for k, need in ((4, 2), (9, 2), (10, 3)) if nij < need)


def tie_points(nij):
    """the two points of the tie level: 9 and 54 of a 9 x 7 plane.  They lie 5 nij / 7 apart: in different segments of the
    argmax for every number of threads per level (a segment has ceil(nij / TL) <= ceil(nij / 32) elements)"""
    return nij // 7, (6 * nij) // 7


def designed_les(itot, jtot, dtype, seed):
    """One LES of twelve levels, every number formed in ``dtype`` (numpy.float64 or numpy.float32) and returned as float64
    (exactly), so that what is exact is exact on a float32 engine too.  qt_av is the nominal value the planes are built around
    (a profile the kernel is handed, like ql_av), not the sample mean: planes of one point can then reach every branch.
      0 clear; 1 ql_ref = 1e-9 (not "> 1e-9": barely unsaturated, beta in (0, 1)); 2 ql_ref = nextafter(1e-9, 1): brentq;
      3 ql_av == ql_ref = 5e-10 over a plane that has cloud: no branch; 4 bit-equal maxima of qt - qsat at tie_points and at
      the point behind the first of them, each with another beta: the first wins; 5 wettest point with qt > qt_av > qsat:
      beta < 0 -> 1; 6 wettest point below the mean, qsat six times further below: beta = 6 >= 5 with ql_ref = 0 <= ql_av:
      2 | 8; 7 mean state saturated beyond ql_ref, ql_ref <= ql_av: 16 | 8; 8 ql_ref = the mean of get_ql_diff(0)'s plane, in the reference's own expression: f(0) == 0, brentq
      returns 0 at once, alpha = -inf; 9 the same at 5: beta == 5.0 >= 5, the additive search runs; 10 a large finite excess at
      point 0, NaN in qt at nij - 2 and in qsat at nij - 1: argmax takes the first NaN, beta is NaN, the plane becomes NaN;
      11 an ordinary brentq level.  Levels of designed_dropped(nij) are left clear.  ql is 33/32 of max(qt - qsat, 0), so
      that the thl correction of constantT changes the levels that are touched but not applied (6 and 7)."""
    dt = NP.get(dtype, dtype)
    nij, K = itot * jtot, 12
    rng = numpy.random.default_rng(seed)
    dropped = designed_dropped(nij)
    av = (0.007 + 1e-4 * numpy.arange(K)).astype(dt)
    nq, ns = rng.normal(size=(nij, K)).astype(dt), rng.normal(size=(nij, K)).astype(dt)
    qsat = av[None, :] + dt(8e-4) + dt(5e-5) * ns
    qt = numpy.minimum(av[None, :] + dt(2e-4) * nq, qsat - dt(1e-5))          # clear: qt < qsat everywhere
    p, p2 = nij // 2, nij // 3
    for k in (1, 3):                                                           # one cloudy point, qt > qsat > qt_av
        qsat[p, k], qt[p, k] = av[k] + dt(3e-4), av[k] + dt(5e-4)
    for k in (2, 9, 11):                                                       # a point that is cloudy at beta = 5: a bracket
        qt[p2, k], qsat[p2, k] = av[k] + dt(4e-4), av[k] + dt(8e-4)
    if 4 not in dropped:
        i1, i2 = tie_points(nij)
        b = dt(2.0 ** -7)
        qsat[i1, 4], qt[i1, 4] = b, b + dt(2.0 ** -12)
        qsat[i2, 4], qt[i2, 4] = b + dt(2.0 ** -9), b + dt(2.0 ** -9) + dt(2.0 ** -12)
        if i1 + 1 < i2:                      # a third one next to the first: the same lane's segment on the larger planes
            qsat[i1 + 1, 4], qt[i1 + 1, 4] = b + dt(2.0 ** -8), b + dt(2.0 ** -8) + dt(2.0 ** -12)
    qsat[p, 5], qt[p, 5] = av[5] - dt(1e-4), av[5] + dt(2e-4)
    qt[p, 6], qsat[p, 6] = av[6] - dt(1e-4), av[6] - dt(6e-4)
    qsat[:, 7] = av[7] - dt(1e-3) + dt(5e-5) * ns[:, 7]
    sat = numpy.arange(nij) % 3 == 0                                           # level 8: every third point saturated at the mean
    qsat[sat, 8] = av[8] - dt(1e-5) - dt(2e-4) * numpy.abs(ns[sat, 8])         # and above the mean, so that f(5) >= f(0)
    qt[sat, 8] = av[8] + numpy.abs(qt[sat, 8] - av[8])
    if 10 not in dropped:
        qt[0, 10], qsat[0, 10] = av[10] + dt(1e-3), av[10] + dt(1e-4)
        qt[nij - 2, 10] = numpy.nan
        qsat[nij - 1, 10] = numpy.nan
    qt, qsat = qt.reshape(itot, jtot, K), qsat.reshape(itot, jtot, K)
    assert qt.dtype == dt and qsat.dtype == dt
    ql = numpy.maximum(qt - qsat, 0) * dt(1.03125)       # the LES's own ql, not the one of the nudge: dQL != 0 at untouched qt
    ql_av = ql.mean(axis=(0, 1)).astype(dt)
    ql_av[3] = dt(5e-10)
    if 10 not in dropped:
        ql_av[10] = dt(1e-6)                                                    # (the mean of a plane with NaN is NaN)

    def plane_mean(b, k):                                                      # spcpl.py:646-648 without "- ql_ref[k]"
        return numpy.maximum((b * (qt[:, :, k] - av[k]) + av[k] - qsat[:, :, k]), 0).sum() / (itot * jtot)

    ql_ref = numpy.zeros(K, dtype=dt)
    ql_ref[1] = dt(1e-9)
    ql_ref[2] = numpy.nextafter(dt(1e-9), dt(1))
    ql_ref[3] = dt(5e-10)
    ql_ref[7] = dt(5e-4)
    ql_ref[8] = plane_mean(0, 8)
    if 9 not in dropped:
        ql_ref[9] = plane_mean(5, 9)
    ql_ref[11] = plane_mean(3, 11)
    assert ql_ref.dtype == dt and ql_av.dtype == dt
    z = (numpy.arange(K) + 0.5) / K
    f = dict(qt=qt, qsat=qsat, ql=ql, thl=(290.0 + 10 * z[None, None, :] + 0.1 * rng.normal(size=(itot, jtot, K))).astype(dt),
             ql_av=ql_av, qt_av=av, presf=(1e5 * numpy.exp(-0.5 * z)).astype(dt), ql_ref=ql_ref)
    return {k: v.astype(numpy.float64) for k, v in f.items()}


def designed_status(nij):
    return tuple(0 if k in designed_dropped(nij) else s for k, s in enumerate(DESIGNED_STATUS))


# -- inputs: levels of four kinds --------------------------------------------------------------------------------------------
def edge_fields(itot, jtot, kinds, seed):
    """One LES whose level k is of kind kinds[k]: "c" clear (no cloud, ql_ref = 0: untouched), "m" multiplicative (ql_ref =
    the cloud the plane has at a beta drawn from [1.5, 4.5]: brentq finds a root below 5), "a" additive (ql_ref = 5e-4, more
    than five times the variability gives: no bracket, then the noise search), "u" barely unsaturated (ql_ref = 0 under a
    plane with a few cloudy points above the mean).  qt_av and ql_av are the planes' means."""
    kinds = numpy.array(list(kinds))
    K, nij = len(kinds), itot * jtot
    rng = numpy.random.default_rng(seed)
    av = 0.007 + 4e-3 * (numpy.arange(K) + 0.5) / K
    qsat = av[None, :] + 8e-4 + 5e-5 * rng.normal(size=(nij, K))
    qt = numpy.minimum(av[None, :] + 2e-4 * rng.normal(size=(nij, K)), qsat - 1e-5)
    cols = numpy.arange(K)
    m = kinds == "m"
    qt[rng.integers(nij, size=K)[m], cols[m]] = av[m] + 6e-4                   # a point that is cloudy from beta = 1.5 on
    qt[nij - 1, m] = av[m] + 6e-4                                              # and the LAST point: the end of the last chunk counts
    cloudy = rng.random((nij, K)) < 0.05
    cloudy[rng.integers(nij, size=K), cols] = True
    cloudy &= (kinds == "u")[None, :]
    qsat[cloudy] = numpy.broadcast_to(av[None, :] + 3e-4, qsat.shape)[cloudy]
    qt[cloudy] = qsat[cloudy] + 1e-4 * (1 + rng.random(int(cloudy.sum())))
    qt, qsat = qt.reshape(itot, jtot, K), qsat.reshape(itot, jtot, K)
    ql = numpy.maximum(qt - qsat, 0)
    ql_av, qt_av = ql.mean(axis=(0, 1)), qt.mean(axis=(0, 1))
    x0 = rng.uniform(1.5, 4.5, K)
    ql_ref = numpy.where(m, numpy.maximum(x0 * (qt - qt_av) + qt_av - qsat, 0).mean(axis=(0, 1)), 0.0)
    ql_ref[kinds == "a"] = 5e-4
    z = (numpy.arange(K) + 0.5) / K
    return dict(qt=qt, qsat=qsat, ql=ql, thl=290.0 + 10 * z[None, None, :] + 0.1 * rng.normal(size=(itot, jtot, K)),
                ql_av=ql_av, qt_av=qt_av, presf=1e5 * numpy.exp(-0.5 * z), ql_ref=ql_ref)


def random_kinds(ktot, seed, p_clear, forced=()):
    """kinds of ktot levels: clear with probability p_clear, else "m", "a" or "u"; ``forced``: (first level, kinds) runs"""
    rng = numpy.random.default_rng(seed)
    kinds = numpy.where(rng.random(ktot) < p_clear, "c", rng.choice(list("mau"), ktot))
    for k0, run in forced:
        kinds[k0:k0 + len(run)] = list(run)
    return "".join(kinds)


def sparse_kinds(ktot, i):
    """all clear but four levels whose places depend on the LES i"""
    kinds = ["c"] * ktot
    for j, kind in enumerate("maum"):
        kinds[(7 * i + 61 * j + 3) % ktot] = kind
    return "".join(kinds)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def launches(body, dtype):
    """the launches of a body: [(name, [fields of every LES], routes)]; one launch has one plane geometry.  The fields depend on
    ``dtype`` (a torch dtype) for designed_levels only.  Built once and shared (nothing changes them: FieldLES hands out copies)."""
    def make():
        if body == "designed_levels":
            return [("designed %d x %d" % pl, [designed_les(pl[0], pl[1], dtype, 100 + n)], FOUR_ROUTES) for n, pl in enumerate(DESIGNED_PLANES)]
        if body == "tall":
            mid = [(252, "cmamuamuc")]                                          # levels 253 ... 259: both sides of k = 256
            return [("tall 9 x 7 x 300", [edge_fields(9, 7, random_kinds(300, 1, 0.6, mid + [(297, "mau")]), 11)], TWO_ROUTES),
                    ("tall 16 x 16 x 513", [edge_fields(16, 16, random_kinds(513, 2, 0.6, mid + [(510, "amu")]), 12)], TWO_ROUTES)]
        if body == "std_many_workgroups":
            return [("std 17 x (16 x 16 x 257)", [edge_fields(16, 16, sparse_kinds(257, i), 20 + i) for i in range(17)], TWO_ROUTES),
                    ("std 19 x (24 x 24 x 225)", [edge_fields(24, 24, sparse_kinds(225, i), 40 + i) for i in range(19)], TWO_ROUTES)]
        if body == "small_trees":
            return [("trees %d x %d" % pl, [edge_fields(pl[0], pl[1], "cmaumuam", 60 + n)], TWO_ROUTES)
                    for n, pl in enumerate(SMALL_TREE_PLANES)]
        if body == "chunk_edges":
            return [("chunks %d x %d" % pl, [edge_fields(pl[0], pl[1], "cmaum", 70 + n)], TWO_ROUTES) for n, pl in enumerate(CHUNK_PLANES)]
        if body == "ragged_columns":
            return [("ragged 3 x (64 x 64 x 21)", [edge_fields(64, 64, random_kinds(21, 80 + i, 0.4), 80 + i) for i in range(3)], TWO_ROUTES),
                    ("ragged 37 x (9 x 7 x 23)", [edge_fields(9, 7, random_kinds(23, 90 + i, 0.4), 90 + i) for i in range(37)], TWO_ROUTES)]
        raise KeyError(body)
    return _cached(("launch", body, dtype if body == "designed_levels" else None), make)


SMALL_TREE_PLANES = ((16, 16), (32, 16), (17, 8), (25, 8))        # 256: two leaves; 512: four balanced; 136: 64 + 72; 200: 96 + 104
CHUNK_PLANES = ((128, 64), (3, 2731), (8, 1025))                  # 8192: one full chunk; 8193: a second chunk of 1; 8200: one of 8
SEED = 42


def reference(body, n, dtype, constantT):
    """the references of launch n of a body, one per LES, computed once: R in les order from numpy's global generator"""
    def make():
        fs = launches(body, dtype)[n][1]
        fn = vo.variability_nudge if dtype == torch.float64 else v32.variability_nudge
        numpy.random.seed(SEED)
        with numpy.errstate(all="ignore"):
            return [fn(f["qt"], f["qsat"], f["ql_av"], f["qt_av"], f["presf"], f["ql_ref"], vo.make_R(*f["qt"].shape[:2]), 900.0,
                       constantT, thl=f["thl"], ql=f["ql"]) for f in fs]
    return _cached(("ref", body, n, dtype, constantT), make)


# -- comparison --------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """equal value for value: NaN where b has NaN (payloads are not compared), every other element bit for bit"""
    a, b = numpy.asarray(a), numpy.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not numpy.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
        return False
    if a.dtype.kind != "f":
        return True
    u = {8: numpy.uint64, 4: numpy.uint32}[a.dtype.itemsize]
    keep = ~numpy.isnan(a)
    return numpy.array_equal(a[keep].view(u), b[keep].view(u))


def compare(g, r, m, constantT, dtype, what):
    assert r["error"] is None, what
    assert numpy.array_equal(g["status"], r["status"]), (what, g["status"], r["status"])
    for key in ("beta", "a", "alpha", "qt_std"):
        assert same_bits(g[key], r[key]), (what, key, g[key], r[key])
    assert same_bits(m.fields.QT, r["qt"]), (what, "qt", numpy.argwhere(~((m.fields.QT == r["qt"]) | numpy.isnan(r["qt"])))[:5])
    if not constantT:
        assert not hasattr(m.fields, "THL"), what
        return
    got, ref = m.fields.THL, r["thl"]
    assert got.dtype == ref.dtype, what
    got, ref = got.astype(numpy.float64), ref.astype(numpy.float64)
    keep = ~numpy.isnan(ref)
    assert numpy.array_equal(numpy.isnan(got), ~keep), (what, "thl: NaN in other places")
    if keep.any():
        err = numpy.abs(got - ref)[keep].max()
        assert err <= THL_ULP[dtype] * (EPS64 if dtype == torch.float64 else EPS32) * numpy.abs(ref[keep]).max(), (what, "thl", err)


def check_body(eng, body):
    """every launch of the body on the engine: both constantT values, every route of the launch"""
    from sp_coupler_amd import spcpl
    spcpl.set_engine(eng)
    try:
        for n, (name, fs, routes) in enumerate(launches(body, eng.dtype)):
            for constantT in (False, True):
                refs = reference(body, n, eng.dtype, constantT)
                for rt in routes:
                    les = [FieldLES(f, f["ql_ref"].copy(), grid_index=i + 1) for i, f in enumerate(fs)]
                    numpy.random.seed(SEED)
                    try:
                        with route(rt), numpy.errstate(all="ignore"):
                            got = spcpl.variability_nudge_batched(les, 900.0, constantT, write=False)
                    except (ValueError, RuntimeError) as e:                 # scipy's exceptions where the reference raised none
                        raise AssertionError((name, rt, constantT, e))
                    for i, (m, g, r) in enumerate(zip(les, got, refs)):
                        compare(g, r, m, constantT, eng.dtype, (name, rt, "constantT=%s" % constantT, "LES %d" % i))
    finally:
        spcpl.set_engine(None)


def check_designed_levels(eng):
    """the twelve hand-built levels of designed_les on planes of 9 x 7, 2 x 3, 1 x 1, 1 x 8, 3 x 3, 64 x 64 (the noise plane in
    registers, full leaves) and 92 x 92 (two chunks) points, on all four routes (92 x 92 in double is the largest plane that
    is loaded without the workspace).  Dropped: levels 4, 9 and 10 on 1 x 1 (designed_dropped); none on the other planes."""
    check_body(eng, "designed_levels")


def check_tall(eng):
    """9 x 7 x 300 and 16 x 16 x 513: the second and third trip of k_vnudge_update's staging loop; multiplicative, additive
    and unsaturated levels on both sides of k = 256 and at the very top"""
    check_body(eng, "tall")


def check_std_many_workgroups(eng):
    """more than 256 workgroups of qt.std (k_vnudge_std<T, 256>): 17 LES of 16 x 16 x 257 (289 workgroups; a plane is one full
    tile) and 19 LES of 24 x 24 x 225 (285; two full tiles and a ragged one of 64 rows); four active levels per LES"""
    check_body(eng, "std_many_workgroups")


def check_small_trees(eng):
    """planes of 256 (two leaves), 512 (four balanced leaves), 136 (64 + 72) and 200 (96 + 104) points"""
    check_body(eng, "small_trees")


def check_chunk_edges(eng):
    """128 x 64 = 8192 (one full chunk), 3 x 2731 = 8193 (a second chunk of one point), 8 x 1025 = 8200 (one of eight), ktot = 5"""
    check_body(eng, "chunk_edges")


def check_ragged_columns(eng):
    """3 LES of 64 x 64 x 21 (11 tiles in groups of 8: the last group of every column is ragged) and 37 LES of 9 x 7 x 23 (74
    groups on 80 workgroups; streamed: 23 tiles in groups of 16), every LES with its own seed and pattern of active levels"""
    check_body(eng, "ragged_columns")


def jobs(eng, names=BODIES):
    return [(name, lambda name=name: globals()["check_" + name](eng)) for name in names]


def check_everything(eng, names=BODIES):
    """the bodies on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the names that failed."""
    return run_bodies(names, jobs(eng, names))


# -- the old matrix ----------------------------------------------------------------------------------------------------------
OLD_SHAPES = [(16, 12, 40, 3), (9, 7, 23, 4), (64, 64, 160, 5), (96, 96, 12, 6), (32, 32, 24, 7), (64, 32, 21, 8), (90, 90, 12, 10),
              (92, 92, 12, 11), (128, 128, 12, 12), (200, 170, 5, 13)]
OLD_GROUPS = ([0, 1], [2], [3], [4], [5], [6], [7], [8], [9])      # one launch per extent (a launch has one plane geometry)
OLD_ROUTES = {"1": "default", "pair": "pair", "strided": "strided", "global": "global"}


def old_matrix(spcpl, constantT, lds, f32, check):
    """The shape matrix of tests/test_vnudge.py::test_kernel_matches_the_numpy_scipy_oracle (``f32``: of its copy in
    tests/test_vnudge_f32_gpu.py) on the engine spcpl holds, on the device route ``lds`` ("1", "pair", "strided", "global"):
    92 x 92 = 8464 points is the LDS path with TWO chunks of numpy's 8192-element blocking; 96 x 96, 128 x 128 and 200 x 170
    (4 chunks + a ragged last one) do not fit the LDS in double (in float 128 x 128 does): one workgroup per level streams the
    planes from the transposed workspace; without a workspace ("strided") they are refused, so those are left out.  Calls
    check(g, r, m, f) for every LES: g what the drop-in returned, r the reference (computed once per shape), m the FieldLES."""
    def fields(group):
        fs = [make_les_fields(*OLD_SHAPES[g][:3], seed=OLD_SHAPES[g][3]) for g in group]
        if len(group) == 2:                             # same geometry needed inside one launch: pad the second to the first
            fs[1] = make_les_fields(*OLD_SHAPES[group[0]][:3], seed=OLD_SHAPES[group[1]][3])
        return fs

    def refs(fs):
        numpy.random.seed(42)
        fn = v32.variability_nudge if f32 else vo.variability_nudge
        return [fn(f["qt"], f["qsat"], f["ql_av"], f["qt_av"], f["presf"], f["ql_ref"], vo.make_R(*f["qt"].shape[:2]), 900.0, constantT,
                   thl=f["thl"], ql=f["ql"]) for f in fs]

    with route(OLD_ROUTES[lds]):
        for group in OLD_GROUPS:
            if lds == "strided" and OLD_SHAPES[group[0]][0] * OLD_SHAPES[group[0]][1] > (18000 if f32 else 9000):
                continue
            fs = _cached(("old", tuple(group)), lambda: fields(group))
            les = [FieldLES(f, f["ql_ref"].copy(), grid_index=i + 1) for i, f in enumerate(fs)]
            numpy.random.seed(42)
            got = spcpl.variability_nudge_batched(les, 900.0, constantT, write=False)
            for m, f, g, r in zip(les, fs, got, _cached(("oldref", tuple(group), f32, constantT), lambda: refs(fs))):
                check(g, r, m, f)


def old_guard(eng):
    """the old matrix on one engine with the assertions of the two tests that own it; returns the cases that failed"""
    from sp_coupler_amd import spcpl
    f32 = eng.dtype == torch.float32

    def check(g, r, m, f):
        assert r["error"] is None
        assert numpy.array_equal(g["status"], r["status"])
        assert m.ktot < 12 or ((r["status"] & 1).any() and (r["status"] & 4).any())
        assert numpy.array_equal(g["beta"], r["beta"]) and numpy.array_equal(g["a"], r["a"])
        assert numpy.array_equal(m.fields.QT, r["qt"])
        assert numpy.array_equal(g["qt_std"], r["qt_std"]) and numpy.array_equal(g["alpha"], r["alpha"])
        if constantT:
            err = numpy.abs(m.fields.THL.astype(numpy.float64) - r["thl"]).max()
            assert err <= THL_ULP[eng.dtype] * (EPS32 if f32 else EPS64) * numpy.abs(r["thl"]).max()
            assert not numpy.array_equal(m.fields.THL, f["thl"].astype(m.fields.THL.dtype))

    failed = []
    spcpl.set_engine(eng)
    try:
        for constantT in (False, True):
            for lds in OLD_ROUTES:
                try:
                    old_matrix(spcpl, constantT, lds, f32, check)
                except (AssertionError, ValueError, RuntimeError):
                    failed.append("%s-%s" % (constantT, lds))
    finally:
        spcpl.set_engine(None)
    return failed
