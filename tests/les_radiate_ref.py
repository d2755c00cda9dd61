"""NumPy oracle of K18 (include/spc.h: spc_les_radiate_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_radiate_gpu.py (each takes an engine: tools/mutation_control.py --radiate hands them the engines of its mutant
libraries), the host twins of models.DeviceLESEnsemble's radiation mode and an oracle-backed engine with ``les_radiate`` for the
CPU suite.

The oracle spells the rule out one operation per NumPy call in the element type, vectorised over the columns, Python loops
over k for both running sums, so nothing fuses.  Every device array of the bodies is the LEADING part of a poisoned buffer
(tests/les_harness.Poisoned); the bytes behind it (and in front of a view off the 16-byte grid) are checked after the launch."""

import numpy
import torch

from sp_coupler_amd import _abi, models
from sp_coupler_amd import radiation as rad
from tests import les_diffuse_ref as ldr
from tests import les_micro_ref as lmr
from tests import les_thermo_ref as ltr
from tests import les_vadvect_ref as lvr
from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, cols_table, ensemble_case, fill_args, host_of, np_of, on_both, run_bodies,
    with_tail)

#: one column per LES (1 x 1: a tile holds many LES), tiles that straddle LES (2 x 3), a tile that is exactly one LES (8 x 8)
PLANES = [(1, 1), (2, 3), (8, 8)]
#: no chain (1), one add (2), shorter than one chunk of 8 levels (7), the flagship's 160 (whole chunks) and 161 (one more)
KTOTS = [1, 2, 7, 160, 161]
NS = [1, 2, 5]
OUT_FILL = -7.0
DT = 60.0


# -- the rule --------------------------------------------------------------------------------------------------------------
def lookup(x, etab, inv_step=rad.INV_STEP):
    """E(x) of the rule: the table ``etab`` interpolated at x clamped to [0, x_hi], in the dtype of x"""
    T = x.dtype.type
    assert etab.dtype == x.dtype
    n_tab = etab.shape[0]
    x_hi = T(float(n_tab - 1) / float(inv_step))
    with numpy.errstate(all="ignore"):
        xc = numpy.where(x < 0, T(0), numpy.where(x > x_hi, x_hi, x))
        s = xc * T(inv_step)
        m = numpy.minimum(numpy.where(s >= 0, s, T(0)).astype(numpy.int64), n_tab - 2)      # NaN: m = 0, fr stays NaN
        fr = s - m.astype(x.dtype)
        e0 = etab[m]
        d = etab[m + 1] - e0
        t = fr * d
        e = e0 + t
    assert e.dtype == x.dtype
    return e


def optical_depths(ql, w):
    """(A, B) [n x itot x jtot x (ktot + 1)]: the optical depth above and below every face"""
    ktot = ql.shape[-1]
    with numpy.errstate(all="ignore"):
        t = w[:, None, None, :] * ql
        A = numpy.zeros(ql.shape[:3] + (ktot + 1,), dtype=ql.dtype)
        B = numpy.zeros_like(A)
        for k in range(ktot):
            B[..., k + 1] = B[..., k] + t[..., k]
        for k in range(ktot - 1, -1, -1):
            A[..., k] = A[..., k + 1] + t[..., k]
    return A, B


def fluxes(ql, w, f0, f1, etab, inv_step=rad.INV_STEP):
    """F [n x itot x jtot x (ktot + 1)]: the net upward flux at every face"""
    A, B = optical_depths(ql, w)
    with numpy.errstate(all="ignore"):
        fa = f0[:, None, None, None] * lookup(A, etab, inv_step)
        fb = f1[:, None, None, None] * lookup(B, etab, inv_step)
        F = fa + fb
    assert F.dtype == ql.dtype
    return F


def les_radiate(ql, thl, w, c, f0, f1, etab, inv_step=rad.INV_STEP):
    """(the new thl, flux, fsfc), new arrays: ql, thl [n x itot x jtot x ktot] of dtype T, w, c [n x ktot], f0, f1 [n], etab
    [n_tab] of the same T"""
    T = ql.dtype
    assert all(a.dtype == T for a in (thl, w, c, f0, f1, etab))
    F = fluxes(ql, w, f0, f1, etab, inv_step)
    with numpy.errstate(all="ignore"):
        dF = F[..., 1:] - F[..., :-1]
        t = c[:, None, None, :] * dF
        new = thl - t
    assert new.dtype == T
    return new, numpy.ascontiguousarray(F[..., 1:]), numpy.ascontiguousarray(F[..., 0])


# -- inputs ------------------------------------------------------------------------------------------------------------------
def grid(n, ktot, rng):
    """(rhobf, zh, zf, presf, kappa) of LES with layers of 20 ... 30 m: another grid, density, pressure and kappa per LES"""
    dz = 20.0 + 10.0 * rng.random((n, ktot))
    if ktot > 1:
        dz[:, -1] = dz[:, -2]
    zh = numpy.concatenate([numpy.zeros((n, 1)), numpy.cumsum(dz, axis=1)[:, :-1]], axis=1)
    zf = zh + 0.5 * dz
    scale = 7000.0 + 3000.0 * rng.random((n, 1))
    rhobf = (1.0 + 0.3 * rng.random((n, 1))) * numpy.exp(-zf / scale)
    presf = 1e5 * (1.0 - 0.03 * rng.random((n, 1))) * numpy.exp(-zf / scale)
    kappa = rad.KAPPA * (1.0 + 0.05 * numpy.arange(n))
    return rhobf, zh, zf, presf, kappa


def cloud(shape, kind, rng):
    """float64 ql of ``shape``: "clear"; one cloudy cell per column at the "bottom", the "top" or in the "middle"; a "deck" of
    several levels in every column; "mixed": two columns in three hold a deck of another base, depth and water each"""
    n, itot, jtot, ktot = shape
    ql = numpy.zeros(shape)
    water = 2e-4 + 6e-4 * rng.random(shape)
    if kind == "bottom":
        ql[..., 0] = water[..., 0]
    elif kind == "top":
        ql[..., ktot - 1] = water[..., ktot - 1]
    elif kind == "middle":
        ql[..., ktot // 2] = water[..., ktot // 2]
    elif kind in ("deck", "mixed"):
        k = numpy.arange(ktot)
        base = rng.integers(0, max(1, ktot - 1), shape[:3] + (1,)) if kind == "mixed" else numpy.full(shape[:3] + (1,), ktot // 3)
        depth = rng.integers(1, max(2, min(12, ktot)), shape[:3] + (1,)) if kind == "mixed" else max(1, min(10, ktot // 3))
        there = (k >= base) & (k < base + depth)
        if kind == "mixed":
            there &= rng.random(shape[:3] + (1,)) < 2.0 / 3.0
        ql = numpy.where(there, water, 0.0)
    else:
        assert kind == "clear", kind
    return ql


def case(shape, dtype, seed=0, kind="mixed", dt=DT):
    """dict of the arguments in ``dtype``: ql, thl, w, c, f0, f1, etab (radiation.exp_table: what an engine uploads)"""
    dtype = numpy.dtype(dtype).type
    n, itot, jtot, ktot = shape
    rng = numpy.random.default_rng(8000 + seed + 7 * ktot + itot * jtot + 31 * n)
    rhobf, zh, zf, presf, kappa = grid(n, ktot, rng)
    w, c = rad.profiles(rhobf, zh, presf, dt, kappa, zf=zf)
    ql = cloud(shape, kind, rng)
    thl = 290.0 + 10.0 * numpy.arange(ktot) / 160.0 + 0.5 * rng.standard_normal(shape)
    f0 = rad.F0 * (1.0 + 0.1 * numpy.arange(n))
    f1 = rad.F1 * (1.0 + 0.2 * numpy.arange(n))
    return dict(ql=ql.astype(dtype), thl=thl.astype(dtype), w=numpy.ascontiguousarray(w.astype(dtype)), c=numpy.ascontiguousarray(c.astype(dtype)),
                f0=f0.astype(dtype), f1=f1.astype(dtype), etab=rad.exp_table(dtype), inv_step=rad.INV_STEP)


def oracle(c):
    return les_radiate(c["ql"], c["thl"], c["w"], c["c"], c["f0"], c["f1"], c["etab"], c["inv_step"])


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one launch through ``eng.les_radiate`` with every array inside a poisoned buffer; ``check`` compares thl, flux and fsfc
    with the oracle bit for bit, the read-only inputs with what was uploaded, and looks at the bytes around every array.
    ``leads``: elements in front of (ql, thl, flux); ``pad``: elements between the rows of w and c (pitched profiles)"""

    def __init__(self, eng, c, leads=(0, 0, 0), pad=0, flux=True, fsfc=True):
        self.eng, self.c, self.pad = eng, c, pad
        self.mem = Poisoned(eng)
        assert numpy.array_equal(c["etab"], rad.exp_table(c["ql"].dtype)) and c["inv_step"] == rad.INV_STEP     # (the engine's table)

        put = self.mem.put
        prof = lambda tag, a: self.mem.rows(tag, a, 1e30, pad=pad)                          # noqa: E731
        self.dql = put("ql", c["ql"], float("nan"), leads[0])
        self.dthl = put("thl", c["thl"], float("nan"), leads[1])
        self.dw, self.dc = prof("w", c["w"]), prof("c", c["c"])
        self.df0, self.df1 = put("f0", c["f0"], 1e30), put("f1", c["f1"], 1e30)
        self.dflux = put("flux", numpy.full_like(c["ql"], OUT_FILL), 1e30, leads[2]) if flux else None
        self.dfsfc = put("fsfc", numpy.full(c["ql"].shape[:3], OUT_FILL, dtype=c["ql"].dtype), 1e30) if fsfc else None
        self.got = eng.les_radiate(self.dql, self.dthl, self.dw, self.dc, self.df0, self.df1, flux=self.dflux, fsfc=self.dfsfc)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def check(self, what=""):
        c = self.c
        thl, flux, fsfc = oracle(c)
        assert self.got is None
        assert_bits("%s thl" % what, self.dthl.cpu().numpy(), thl)
        if self.dflux is not None:
            assert_bits("%s flux" % what, self.dflux.cpu().numpy(), flux)
        if self.dfsfc is not None:
            assert_bits("%s fsfc" % what, self.dfsfc.cpu().numpy(), fsfc)
        for tag, t, a in (("ql", self.dql, c["ql"]), ("w", self.dw, c["w"]), ("c", self.dc, c["c"]), ("f0", self.df0, c["f0"]), ("f1", self.df1, c["f1"])):
            assert Poisoned.read_only(t, a), (what, tag, "read only")
        self.mem.check_around(what)
        return thl, flux, fsfc


PTRS = ("ql", "thl", "w", "c", "f0", "f1", "etab", "flux", "fsfc")


def raw_launch(eng, c, alias=None, extents=None, null=(), flux=True, fsfc=True):
    """spc_les_radiate_* itself with the case's own table: (rc, host thl, host flux or None, host fsfc or None).  ``alias``:
    (member, key) pairs that replace a pointer member by that of tensor ``key``; ``extents``: overrides of the scalar members;
    ``null``: members set to NULL.  The table is the leading part of a NaN-poisoned buffer."""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    n, itot, jtot, ktot = c["ql"].shape
    t = {k: dev(c[k]) for k in ("ql", "thl", "w", "c", "f0", "f1")}
    t["etab"] = with_tail(eng, c["etab"], float("nan"), tail_elems=64)[0]
    t["flux"] = dev(numpy.full_like(c["ql"], OUT_FILL))
    t["fsfc"] = dev(numpy.full(c["ql"].shape[:3], OUT_FILL, dtype=c["ql"].dtype))
    a = _abi.LesRadiateArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_tab, a.pitch_prof, a.inv_step = n, itot, jtot, ktot, c["etab"].shape[0], ktot, c["inv_step"]
    fill_args(a, t, [k for k in PTRS if (k != "flux" or flux) and (k != "fsfc" or fsfc)], alias, extents, null)
    rc = abi_call(eng, "spc_les_radiate", a)
    assert Poisoned.read_only(t["ql"], c["ql"]) and Poisoned.read_only(t["etab"], c["etab"])
    return rc, t["thl"].cpu().numpy(), t["flux"].cpu().numpy() if flux else None, t["fsfc"].cpu().numpy() if fsfc else None


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, n=3):
    """mixed columns (clear ones and decks of another base, depth and water) against the oracle; the answer is not the input"""
    c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
    c["ql"][0, 0, 0, :] = np_of(eng)(5e-4) * (numpy.arange(ktot) >= ktot // 2)            # (at least one cloudy column)
    thl, flux, fsfc = Run(eng, c).check("n %d plane %s ktot %d" % (n, plane, ktot))
    assert (thl != c["thl"]).any() and (thl[0, 0, 0, ktot - 1] < c["thl"][0, 0, 0, ktot - 1])
    assert (flux[0, 0, 0, -1] > fsfc[0, 0, 0]) if ktot > 1 else True


def check_rows(eng, ktot):
    """n = 1, 2, 5 at 2 x 3: w, c, f0 and f1 differ per LES, so a wrong l shows; then the same with pitched profiles"""
    for n in NS:
        for pad in (0, 3):
            c = case((n, 2, 3, ktot), np_of(eng), seed=1, kind="deck")
            if n > 1:
                assert not numpy.array_equal(c["w"][0], c["w"][1]) and c["f0"][0] != c["f0"][1] and c["f1"][0] != c["f1"][1]
            Run(eng, c, pad=pad).check("rows n %d ktot %d pad %d" % (n, ktot, pad))


def check_tiles(eng):
    """for every C of spc_les_radiate_cols_per_block: C - 1, C, C + 1 and 2 C + 1 columns, as one LES of 1 x cols columns (a
    tile ends inside a row), as cols LES of one column (l per lane) and as LES of 1 x 3 (a tile ends inside an LES); ktot on
    both sides of every change of C; 17 columns at the last supported ktot; the first unsupported ktot refused"""
    dtype = np_of(eng)
    first, changes, bad = cols_table(eng.radiate_cols_per_block)
    assert sorted(first) == [16, 32, 64] and len(changes) == 2
    for C, k0 in first.items():
        ktot = 7 if C == 64 else k0
        assert eng.radiate_cols_per_block(ktot) == C
        for cols in (C - 1, C, C + 1, 2 * C + 1):
            shapes = [(1, 1, cols, ktot), (cols, 1, 1, ktot)] + ([(cols // 3, 1, 3, ktot)] if cols % 3 == 0 else [])
            for shape in shapes:
                Run(eng, case(shape, dtype, seed=3)).check("tiles %s C %d" % (shape, C))
    for ktot in changes:
        for k in (ktot - 1, ktot):
            Run(eng, case((2, 2, 3, k), dtype, seed=4)).check("change at ktot %d: %d" % (ktot, k))
    Run(eng, case((1, 1, 17, bad - 1), dtype, seed=5)).check("17 columns at the last ktot %d" % (bad - 1))
    try:
        Run(eng, case((1, 1, 2, bad), dtype, seed=5))
    except _abi.SpcError as e:
        assert e.code == _abi.SPC_ERR_UNSUPPORTED and str(bad - 1) in str(e), str(e)
    else:
        raise AssertionError("ktot %d was not refused" % bad)
    return first, changes, bad


def check_outputs(eng):
    """with and without flux and fsfc: thl does not depend on them, and what is not asked for is not written"""
    for ktot in (2, 65):
        c = case((2, 2, 3, ktot), np_of(eng), seed=6, kind="deck")
        for flux in (True, False):
            for fsfc in (True, False):
                Run(eng, c, flux=flux, fsfc=fsfc).check("flux %s fsfc %s ktot %d" % (flux, fsfc, ktot))
    want = oracle(c)
    rc, thl, flux, fsfc = raw_launch(eng, c)
    assert rc == 0
    for tag, got, w in zip(("thl", "flux", "fsfc"), (thl, flux, fsfc), want):
        assert_bits("raw " + tag, got, w)


def check_alignment(eng, leads, ktot=65, pad=0):
    """views off the 16-byte grid: all equally (the 16-byte mover with a head and a tail) or each on its own (single elements)"""
    c = case((3, 2, 3, ktot), np_of(eng), seed=sum(leads) + 10 * pad)
    Run(eng, c, leads=leads, pad=pad).check("leads %s pad %d ktot %d" % (leads, pad, ktot))


COLTILE_KTOTS = (1, 2, 7, 8, 9, 17)


def coltile_leads(V, arrays):
    """leads of ``arrays`` 4-D arrays: all equal, 0 ... V - 1 (the 16-byte walk with a head and a tail), then one array at a time
    1 ... V - 1 off the others, and all different (vec == 0: single elements)"""
    equal = [(lead,) * arrays for lead in range(V)]
    one = [tuple(lead if a == b else 0 for b in range(arrays)) for a in range(arrays) for lead in range(1, V)]
    return equal + one + [tuple((a + 1) % V for a in range(arrays))]


def check_coltile(eng):
    """the cases of the column tile (spc_coltile.hpp) together: 3 LES of 3 x 5 (one partial tile that spans three LES, more than
    DIF_STAGE) and 6 of them (a whole 64-column tile that spans five LES, then a partial one); ktot 1, 2, 7, 8, 9 and 17, and at
    n = 3 the last ktot of every C and the first of the next; ql, thl and flux led by 0 ... V - 1 elements, equally and each on its own (coltile_leads);
    the bytes around every array are looked at by Run.check"""
    dtype = np_of(eng)
    V = 16 // numpy.dtype(dtype).itemsize
    for n in (3, 6):
        for ktot in COLTILE_KTOTS:
            for leads in coltile_leads(V, 3):
                Run(eng, case((n, 3, 5, ktot), dtype, seed=11 + sum(leads)), leads=leads).check("coltile n %d ktot %d leads %s" % (n, ktot, leads))
    first, changes, bad = cols_table(eng.radiate_cols_per_block)
    for ktot in [k for c in changes for k in (c - 1, c)] + [bad - 1]:
        for leads in ((0, 0, 0), (1, 1, 1), (1, 0, 0)):
            Run(eng, case((3, 3, 5, ktot), dtype, seed=12), leads=leads).check("coltile C %d ktot %d leads %s" % (eng.radiate_cols_per_block(ktot), ktot, leads))


def check_clouds(eng):
    """a clear sky keeps every bit of thl (-0.0 included) and F = f0 + f1 everywhere; one cloudy cell at the bottom, at the top
    and in the middle and a deck: the topmost cloudy cell cools; with f0 = 0 and cloud from k0 up the cells below k0 keep
    their bits, cell k0 warms and no cell cools"""
    dtype = np_of(eng)
    for ktot in (2, 7, 64):
        c = case((2, 2, 3, ktot), dtype, seed=7, kind="clear")
        c["thl"][0, 0, 0, :] = -0.0
        c["thl"][1, 1, 2, ::2] = -0.0
        thl, flux, fsfc = Run(eng, c).check("clear ktot %d" % ktot)
        assert_bits("a clear sky keeps thl", thl, c["thl"])
        with numpy.errstate(all="ignore"):
            total = c["f0"] * dtype(1) + c["f1"] * dtype(1)
        assert_bits("a clear sky: flux", flux, numpy.broadcast_to(total[:, None, None, None], flux.shape))
        assert_bits("a clear sky: fsfc", fsfc, numpy.broadcast_to(total[:, None, None], fsfc.shape))
        for kind in ("bottom", "top", "middle", "deck"):
            c = case((2, 2, 3, ktot), dtype, seed=8, kind=kind)
            thl = Run(eng, c).check("%s ktot %d" % (kind, ktot))[0]
            top = (ktot - 1) - numpy.argmax(c["ql"][..., ::-1] > 0, axis=3)
            pick = lambda a: numpy.take_along_axis(a, top[..., None], axis=3)[..., 0]         # noqa: E731
            assert (pick(c["ql"]) > 0).all() and (pick(thl) < pick(c["thl"])).all(), (kind, ktot, "the cloud top cools")
        k0 = max(1, ktot // 3)
        c = case((2, 2, 3, ktot), dtype, seed=9, kind="clear")
        c["ql"][..., k0:] = dtype(4e-4)
        c["f0"][:] = 0
        thl = Run(eng, c).check("base ktot %d" % ktot)[0]
        assert_bits("below the base", thl[..., :k0], c["thl"][..., :k0])
        assert (thl[..., k0] > c["thl"][..., k0]).all() and (thl >= c["thl"]).all()


def node_case(dtype, ktot=9):
    """w = 64 and ql = j / 4096: every t, A and B is a table node exactly (fr == +0).  Column (0, 0, 1) holds 0.5 - 2 ** -16 in
    one cell (an optical depth of 32 - 2 ** -10, just below x_hi = 32), column (0, 1, 0) 1000 in one cell (far beyond: the
    clamp), column (0, 1, 1) adds up to x_hi exactly"""
    c = case((2, 2, 3, ktot), dtype, seed=10, kind="clear")
    c["w"][:] = 64
    rng = numpy.random.default_rng(3)
    c["ql"][...] = (rng.integers(0, 40, c["ql"].shape) / 4096.0).astype(dtype)
    c["ql"][0, 0, 1, :] = 0
    c["ql"][0, 0, 1, ktot // 2] = dtype(0.5 - 2.0 ** -16)
    c["ql"][0, 1, 0, ktot - 2] = 1000
    c["ql"][0, 1, 1, :] = 0
    c["ql"][0, 1, 1, :2] = 0.25
    return c


def coarse_case(dtype, ktot=5):
    """a table of FIVE nodes at a step of 2 that is not smooth, handed in through the C ABI: x_hi = 8; column (0, 0, 0) adds up
    to 8 exactly, (0, 0, 1) lies beyond it, the others inside.  e0 + 1 * (e1 - e0) of the last segment is not e1."""
    c = case((1, 2, 2, ktot), dtype, seed=11, kind="clear")
    c["w"][:] = 1
    c["etab"] = numpy.array([1.0, 0.6, 0.3, 1.0, 1e-30], dtype=dtype)
    c["inv_step"] = 0.5
    c["f1"][:] = 0                                                 # (F = f0 E(A): nothing hides the last segment's rounding)
    c["ql"][0, 0, 0, :2] = 4
    c["ql"][0, 0, 1, 1] = 50
    c["ql"][0, 1, 0, :] = 0.75
    c["ql"][0, 1, 1, 2] = 7.5
    return c


def check_lookup(eng):
    """optical depths exactly on table nodes, one just below x_hi, one far beyond it (the clamp); a coarse table of the caller's"""
    dtype = np_of(eng)
    c = node_case(dtype)
    A, B = optical_depths(c["ql"], c["w"])
    assert ((A[1] * 64) % 1 == 0).all() and A[0, 0, 1, 0] == dtype(32 - 2.0 ** -10) and A[0, 1, 0, 0] > 1e4 and A[0, 1, 1, 0] == 32
    Run(eng, c).check("nodes")
    c = coarse_case(dtype)
    want = oracle(c)
    assert optical_depths(c["ql"], c["w"])[0][0, 0, 0, 0] == 8 and want[2][0, 0, 0] == 0 != c["f0"][0] * dtype(1e-30)
    rc, thl, flux, fsfc = raw_launch(eng, c)
    assert rc == 0
    for tag, got, w in zip(("thl", "flux", "fsfc"), (thl, flux, fsfc), want):
        assert_bits("coarse table " + tag, got, w)


def special_case(dtype, ktot=7):
    """(clean case, the same with one cell each of ql and of thl set to -0.0, NaN, +inf, -inf and ql to a negative value, the
    columns (l, i, j) that hold them)"""
    c = case((3, 3, 4, ktot), dtype, seed=12, kind="deck")
    s = dict(c, ql=c["ql"].copy(), thl=c["thl"].copy())
    planted = {"ql": {(0, 0, 1): -0.0, (0, 1, 2): numpy.nan, (1, 0, 0): numpy.inf, (1, 2, 3): -numpy.inf, (2, 1, 1): -3e-4},
               "thl": {(0, 2, 0): -0.0, (1, 1, 1): numpy.nan, (2, 0, 2): numpy.inf, (2, 2, 3): -numpy.inf}}
    for key, cells in planted.items():
        for (l, i, j), v in cells.items():
            s[key][l, i, j, ktot // 2] = v
    return c, s, [col for cells in planted.values() for col in cells]


def check_special(eng):
    """a negative ql, NaN, +-inf and -0.0 in one ql cell and in one thl cell each: they act on their own column as the oracle
    says (a NaN in ql makes every thl of its column NaN), and every other column is bit-equal to the run without them"""
    dtype = np_of(eng)
    for ktot in (7, 64):
        c, s, cols = special_case(dtype, ktot)
        clean = Run(eng, c).check("clean ktot %d" % ktot)
        r = Run(eng, s)
        want = r.check("special ktot %d" % ktot)
        others = numpy.ones(c["ql"].shape[:3], dtype=bool)
        for col in cols:
            others[col] = False
        for tag, t, k in (("thl", r.dthl, 0), ("flux", r.dflux, 1), ("fsfc", r.dfsfc, 2)):
            assert_bits("the other columns: " + tag, t.cpu().numpy()[others], clean[k][others])
        assert numpy.isnan(want[0][0, 1, 2]).all() and numpy.isnan(want[1][0, 1, 2]).all() and numpy.isnan(want[2][0, 1, 2])
        assert numpy.isnan(want[0][1, 1, 1]).sum() == 1 and numpy.isfinite(want[1][1, 1, 1]).all()


def check_refusals(eng):
    """n = 0 is a no-op; n_tab < 2, inv_step <= 0 (and NaN), pitch_prof < ktot, and thl, flux or fsfc equal to an input or to
    each other are refused by the library; the engine refuses the same aliases and bad shapes; no refused call writes"""
    dtype = np_of(eng)
    c = case((2, 2, 3, 8), dtype, seed=13, kind="deck")
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    t = {k: dev(c[k]) for k in ("ql", "thl", "w", "c", "f0", "f1")}
    assert eng.les_radiate(t["ql"][:0], t["thl"][:0], t["w"][:0], t["c"][:0], t["f0"][:0], t["f1"][:0]) is None
    rc, thl, flux, fsfc = raw_launch(eng, c, extents=dict(n_les=0))
    assert rc == 0 and (flux == OUT_FILL).all() and (fsfc == OUT_FILL).all()
    assert_bits("n = 0", thl, c["thl"])
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    bad = [(dict(extents=dict(n_tab=1)), b"n_tab"), (dict(extents=dict(inv_step=0.0)), b"inv_step"), (dict(extents=dict(inv_step=-64.0)), b"inv_step"),
           (dict(extents=dict(inv_step=float("nan"))), b"inv_step"), (dict(extents=dict(pitch_prof=7)), b"pitch_prof")]
    bad += [(dict(alias=((out, key),)), b"also an input") for out in ("thl", "flux", "fsfc") for key in ("ql", "w", "c", "f0", "f1", "etab")]
    bad += [(dict(alias=(("flux", "thl"),)), b"same array"), (dict(alias=(("fsfc", "thl"),)), b"same array"), (dict(alias=(("fsfc", "flux"),)), b"same array")]
    bad += [(dict(null=(k,)), b"required pointer " + k.encode()) for k in ("ql", "thl", "w", "c", "f0", "f1", "etab")]
    for kw, text in bad:
        rc, thl, flux, fsfc = raw_launch(eng, c, **kw)
        assert rc == E and text in eng.lib.spc_last_error(), (kw, rc, eng.lib.spc_last_error())
        if "thl" not in dict(kw.get("alias", ())) and "thl" not in kw.get("null", ()):
            assert_bits("refused: thl", thl, c["thl"])
        assert (flux == OUT_FILL).all() and (fsfc == OUT_FILL).all()
    flux, fsfc = torch.empty_like(t["thl"]), torch.empty_like(t["thl"][..., 0])
    like = lambda p: p.view(2, 1, 1, 8)                                                      # noqa: E731
    other = torch.float64 if eng.dtype == torch.float32 else torch.float32
    args = (t["ql"], t["thl"], t["w"], t["c"], t["f0"], t["f1"])
    for call in (lambda: eng.les_radiate(t["ql"], t["ql"], *args[2:]),
                 lambda: eng.les_radiate(*args, flux=t["thl"]),
                 lambda: eng.les_radiate(*args, flux=t["ql"]),
                 lambda: eng.les_radiate(like(t["w"]), like(t["c"]), t["w"], t["c"], t["f0"], t["f1"]),
                 lambda: eng.les_radiate(*args, flux=flux, fsfc=flux[..., 0]),
                 lambda: eng.les_radiate(*args, fsfc=fsfc[:1]),
                 lambda: eng.les_radiate(*args[:3], t["c"][:, :4], *args[4:]),
                 lambda: eng.les_radiate(*args[:4], t["f0"][:1], t["f1"]),
                 lambda: eng.les_radiate(t["ql"], t["thl"][..., ::2], *args[2:]),
                 lambda: eng.les_radiate(t["ql"], t["thl"].to(other), *args[2:]),
                 lambda: eng.les_radiate(t["ql"].cpu(), *args[1:])):
        try:
            call()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad call was not refused")
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    assert_bits("refused: thl", t["thl"].cpu().numpy(), c["thl"])
    assert_bits("refused: ql", t["ql"].cpu().numpy(), c["ql"])


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    c = case((n, 2, 3, 40), np_of(one), seed=n, kind="deck")
    want = oracle(c)
    for tag, eng, up in on_both(one, multi, n):
        t = {k: up(c[k]) for k in ("ql", "thl", "w", "c", "f0", "f1")}
        flux, fsfc = up(numpy.full_like(c["ql"], OUT_FILL)), up(numpy.full(c["ql"].shape[:3], OUT_FILL, dtype=c["ql"].dtype))
        assert eng.les_radiate(t["ql"], t["thl"], t["w"], t["c"], t["f0"], t["f1"], flux=flux, fsfc=fsfc) is None
        multi.synchronize()
        for k, got, w in (("thl", t["thl"], want[0]), ("flux", flux, want[1]), ("fsfc", fsfc, want[2])):
            assert_bits("%s %s" % (tag, k), host_of(got), w)
    return blocks_of(t["thl"], multi, n)


BODIES = ("parity", "rows", "tiles", "coltile", "outputs", "alignment", "clouds", "lookup", "special", "refusals")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in (1, 2, 7, 161)]),
            ("rows", lambda: [check_rows(eng, k) for k in (2, 65)]),
            ("tiles", lambda: check_tiles(eng)),
            ("coltile", lambda: check_coltile(eng)),
            ("outputs", lambda: check_outputs(eng)),
            ("alignment", lambda: [check_alignment(eng, *a) for a in (((1, 1, 1), 65, 0), ((1, 0, 3), 64, 0), ((3, 3, 3), 7, 5))]),
            ("clouds", lambda: check_clouds(eng)),
            ("lookup", lambda: check_lookup(eng)),
            ("special", lambda: check_special(eng)),
            ("refusals", lambda: check_refusals(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_radiate (CPU suite) ------------------------------------------------------------------------
class RadiateOracleEngine(lvr.VadvectOracleEngine):
    """tests/les_vadvect_ref.VadvectOracleEngine with ``les_radiate`` by the NumPy oracle above: thl updated in place, flux and
    fsfc written whole into the caller's tensors, as the HIP engine does"""

    def les_radiate(self, ql, thl, w, c, f0, f1, *, flux=None, fsfc=None, **kw):
        written = [t.data_ptr() for t in (thl, flux, fsfc) if t is not None]
        if ql.shape[0] and (len(set(written)) != len(written) or set(written) & {t.data_ptr() for t in (ql, w, c, f0, f1)}):
            raise ValueError("thl, flux or fsfc is an input or another of them")
        new, F, F0 = les_radiate(ql.numpy(), thl.numpy(), numpy.ascontiguousarray(w.numpy()), numpy.ascontiguousarray(c.numpy()),
                                 f0.numpy(), f1.numpy(), rad.exp_table(ql.numpy().dtype))
        thl.copy_(torch.from_numpy(new))
        if flux is not None:
            flux.copy_(torch.from_numpy(F))
        if fsfc is not None:
            fsfc.copy_(torch.from_numpy(F0))


# -- the host twins of models.DeviceLESEnsemble after enable_radiation() ---------------------------------------------------------
class _HostRadiate:
    """NumPy fields: the executable definition of what evolve_model_batched does after enable_radiation(), on top of any of
    the other modes: the step, the advection, the diffusion, QL and the means of those fields, K18 on THL with that QL, QL and
    the means again, the microphysics, the tail"""

    radiate_par = None
    _flux = None

    def enable_radiation(self, f0=None, f1=None, kappa=None):
        if self.nL == 1 or "THL" not in self.fields3d or not (self.THERMO or "Qsat" in self.fields3d):
            raise ValueError("the radiation (K18) needs a THL field, more than one level and a Qsat field or enable_thermo()")
        full = lambda v, d: numpy.array(numpy.broadcast_to(numpy.asarray(d if v is None else v, dtype=numpy.float64), (self.n,)))      # noqa: E731
        self.radiate_par = {"f0": full(f0, rad.F0), "f1": full(f1, rad.F1), "kappa": full(kappa, rad.KAPPA)}

    def _follow(self):
        f = self.fields3d
        if self.THERMO:
            self._stale = True
            self._ensure_ql()
        elif "QL" in f or ("QT" in f and "Qsat" in f):
            f["QL"] = numpy.maximum(f["QT"] - f["Qsat"], 0.0)
        self._slab_means()

    def get_radiative_flux_batched(self):
        return self._flux

    def evolve_model_batched(self, t):
        from sp_coupler_amd import thermo
        dt = float(t) - self.model_time
        if dt <= 0:
            return
        if self.radiate_par is None:
            return super().evolve_model_batched(t)
        f, p, par = self.fields3d, self.p, self.radiate_par
        self._step(dt)
        if "PS" in self.tend:
            p["PS"] = p["PS"] + dt * self.tend["PS"]
        if self.advect_par is not None:
            self._advect(dt)
        if self.diffuse_par is not None:
            a, m, cp, s0 = (self._r(x) for x in ldr.df.profiles(self.zh_cache, self.zf_cache, p["Rhobf"], dt, **self.diffuse_par))
            for key, slot in (("U", None), ("V", None), ("THL", "wt"), ("QT", "wq")):
                if key in f:
                    flux = self._r(numpy.asarray(self.tend[slot], dtype=numpy.float64).reshape(self.n)) if slot in self.tend else None
                    f[key] = ldr.les_diffuse(f[key], a, m, cp, s0 if flux is not None else None, flux)
        self._follow()
        w, c = (self._r(x) for x in rad.profiles(p["Rhobf"], self.zh_cache, p["presf"], dt, par["kappa"]))
        f["THL"], self._flux, _ = les_radiate(f["QL"], f["THL"], w, c, self._r(par["f0"]), self._r(par["f1"]), rad.exp_table(self.dtype))
        self._follow()
        if self.micro_par is not None and self.THERMO:
            presf = numpy.asarray(p["presf"], dtype=numpy.float64)
            self._micro_step(dt, ltr.les_thermo(f["THL"], f["QT"], self._r(presf), self._r(thermo.exner(presf)), self.n_iter)["temp"])
            self._stale = True
            self._ensure_ql()
        elif self.micro_par is not None:
            self._micro_step(dt, None)
            f["QL"] = numpy.maximum(f["QT"] - f["Qsat"], 0.0)
            p["QL"] = self._w(slab_ref.slab_means(f["QL"]))
        p["QL_ice"] = numpy.minimum(p["QL_ice"], p["QL"])
        if not self.THERMO:
            p["T"] = p["THL"] * (p["presf"] / 1e5) ** (287.04 / 1004.) + 2.53e6 * p["QL"] / 1004.
        if self.micro_par is None:
            p["Rain"] = p["Rain"] + 1e-6 * dt
        self.model_time = float(t)


class HostRadiateLESEnsemble(_HostRadiate, lvr.HostVadvectLESEnsemble):
    """without enable_thermo(): QL = max(QT - Qsat, 0)"""


class HostThermoRadiateLESEnsemble(_HostRadiate, lvr.HostThermoVadvectLESEnsemble):
    """after enable_thermo(): K12's oracle before and after K18"""


VARIANTS = {"plain": dict(), "diffuse": dict(diffuse=True), "all": dict(diffuse=True, thermo=True, micro=True, vertical=True)}


def ensemble_run(engine, n, device, radiate=True, thermo=False, micro=False, diffuse=False, vertical=False, itot=4, jtot=5, nL=20, steps=3):
    """an ensemble with attached U, V, THL, QT (and Qsat, or thermo; QR with the microphysics) and enable_radiation() with
    another f0, f1 and kappa per LES (``radiate`` None: never called) through ``steps`` calls of evolve_model_batched and one
    variability nudge (constantT) before the last; after each of them every profile, the fields and the flux.  Returns (ens,
    list of records)"""
    def record(ens, rec):
        if radiate:
            flux = ens.get_radiative_flux_batched()
            rec["flux"] = numpy.zeros((n, itot, jtot, nL)) if flux is None else numpy.array(host_of(flux))

    def before(ens):
        assert not radiate or ens.get_radiative_flux_batched() is None
    return ensemble_case(engine, n, models.DeviceLESEnsemble if device else (HostThermoRadiateLESEnsemble if thermo else HostRadiateLESEnsemble),
                         thermo=thermo, micro=micro, diffuse=diffuse, edit=lvr.raise_u if vertical else None,
                         advection=dict(dx=lvr.DX, dy=1.5 * lvr.DX, vertical=True) if vertical else None,
                         radiation=radiation_of(n, "f0", "f1", "kappa") if radiate else None, record=record, before=before,
                         itot=itot, jtot=jtot, nL=nL, steps=steps)


def radiation_of(n, *names):
    """the arguments ``names`` of enable_radiation of the ensemble runs: another f0, f1 and kappa per LES"""
    par = {"f0": rad.F0 * (1.0 + 0.05 * numpy.arange(n)), "f1": rad.F1 * (1.0 + 0.1 * (numpy.arange(n) % 3)),
           "kappa": rad.KAPPA * (1.0 + 0.02 * (numpy.arange(n) % 5))}
    return {k: par[k] for k in names}


def check_ensemble(one, engines, n, variant):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``; THL at the cloud top of the twin's
    first step differs from the same run without enable_radiation(), whose device run is bit-equal to its twin as well"""
    kw = VARIANTS[variant]
    host = ensemble_run(one, n, False, **kw)[1]
    plain = ensemble_run(one, n, False, radiate=None, **kw)[1]
    ql = host[1]["field QL"]
    cloudy = (ql > 0).any(axis=3)
    assert cloudy.any()
    top = (ql.shape[3] - 1) - numpy.argmax(ql[..., ::-1] > 0, axis=3)
    a = numpy.take_along_axis(host[1]["field THL"], top[..., None], axis=3)[..., 0]
    b = numpy.take_along_axis(plain[1]["field THL"], top[..., None], axis=3)[..., 0]
    assert (a[cloudy] != b[cloudy]).any() and (host[1]["flux"] > 0).all()
    if variant == "plain":
        assert (a[cloudy] < b[cloudy]).all()                      # (nothing else touches THL between the step and K18)
    for engine in engines:
        lmr.same_logs(host, ensemble_run(engine, n, True, **kw)[1])
    lmr.same_logs(plain, ensemble_run(engines[0], n, True, radiate=None, **kw)[1])
    return host
