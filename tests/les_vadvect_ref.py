"""NumPy oracle of K17 (include/spc.h: spc_les_vadvect_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_vadvect_gpu.py (each takes an engine: tools/mutation_control.py --vadvect hands them the engines of its mutant
libraries), the host twins of models.DeviceLESEnsemble's enable_advection(vertical=True) and an oracle-backed engine with
``les_vadvect`` for the CPU suite.

The oracle spells the rule out one operation per NumPy call in the element type, the neighbours by numpy.roll, the mass flux by
a Python loop over the levels, so nothing fuses.  Every device array of the bodies is the LEADING part of a poisoned buffer
(tests/les_harness.Poisoned); the bytes behind it (and in front of a view off the 16-byte grid) are checked after the launch,
the inputs against what was uploaded."""

import numpy
import torch

from sp_coupler_amd import _abi, models
from sp_coupler_amd import advection as adv
from tests import les_advect_ref as lar
from tests import les_micro_ref as lmr
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, cols_table, ensemble_case, fill_args, host_of, np_of, on_both, run_bodies)

PLANES = lar.PLANES
KTOTS = lar.KTOTS
NS = lar.NS
NAMES = lar.NAMES
ALL_NAMES = lar.ALL_NAMES
OUT_FILL = lar.OUT_FILL
field_like = lar.field_like


# -- the rule --------------------------------------------------------------------------------------------------------------
def courant_faces(u, v, hx, hy):
    """K16's face Courant numbers (cw, ce, cs, cn) of winds [n x itot x jtot x ktot] of dtype T and hx, hy [n] of the same T"""
    T = u.dtype
    assert v.dtype == T and hx.dtype == T and hy.dtype == T
    bx, by = hx[:, None, None, None], hy[:, None, None, None]
    with numpy.errstate(all="ignore"):
        aw = numpy.roll(u, 1, axis=1) + u
        ae = u + numpy.roll(u, -1, axis=1)
        as_ = numpy.roll(v, 1, axis=2) + v
        an = v + numpy.roll(v, -1, axis=2)
        return aw * bx, ae * bx, as_ * by, an * by


def mass_flux(u, v, hx, hy, g):
    """M [n x itot x jtot x ktot + 1]: the mass through the lower face of every level and, last, through the lid"""
    T = u.dtype
    assert g.dtype == T and g.shape == (u.shape[0], u.shape[3])
    cw, ce, cs, cn = courant_faces(u, v, hx, hy)
    with numpy.errstate(all="ignore"):
        dx = ce - cw
        dy = cn - cs
        d = dx + dy
        e = g[:, None, None, :] * d
        M = numpy.zeros(u.shape[:3] + (u.shape[3] + 1,), dtype=T)
        for k in range(u.shape[3]):                                # sequential from the ground
            M[..., k + 1] = M[..., k] - e[..., k]
    assert e.dtype == T
    return M


def face_numbers(M, r):
    """(pb, pt, s) of the mass flux M and r = 1 / g [n x ktot]"""
    T = M.dtype
    zero = T.type(0)
    rr = r[:, None, None, :]
    with numpy.errstate(all="ignore"):
        cb = M[..., :-1] * rr
        ct = M[..., 1:] * rr
        pb = numpy.where(cb > 0, cb, zero)
        pt = numpy.where(ct < 0, -ct, zero)
        s = pb + pt
    assert all(a.dtype == T for a in (pb, pt, s))
    return pb, pt, s


def les_vadvect(fields, u, v, hx, hy, g, r):
    """(dict name -> the new field (a new array), cmax [n], mtop): fields, u, v [n x itot x jtot x ktot] of dtype T, hx, hy [n],
    g, r [n x ktot]"""
    M = mass_flux(u, v, hx, hy, g)
    pb, pt, s = face_numbers(M, r)
    n = u.shape[0]
    cmax = s.reshape(n, -1).max(axis=1) if n else numpy.zeros(0, dtype=u.dtype)
    out = {}
    with numpy.errstate(all="ignore"):
        for k, x in fields.items():
            assert x.dtype == u.dtype and x.shape == u.shape
            xm = numpy.concatenate([x[..., :1], x[..., :-1]], axis=3)
            xp = numpy.concatenate([x[..., 1:], x[..., -1:]], axis=3)
            t = xm - x
            t = pb * t
            y = x + t
            t = xp - x
            t = pt * t
            y = y + t
            assert y.dtype == x.dtype
            out[k] = y
    return out, cmax, numpy.ascontiguousarray(M[..., 1:])


# -- inputs ------------------------------------------------------------------------------------------------------------------
def profiles(n, ktot, dtype):
    """g = rho dz and r = 1 / g [n x ktot] of dtype: another density and another stretched grid per LES"""
    k = numpy.arange(ktot, dtype=numpy.float64)
    rho = 1.15 * numpy.exp(-k / 400.0)[None, :] * (1.0 + 0.05 * numpy.arange(n))[:, None]
    dz = (20.0 + 0.25 * k)[None, :] * (1.0 + 0.1 * numpy.arange(n) % 0.35)[:, None]
    g, r = adv.vertical_profiles(rho * dz)
    return g.astype(dtype), r.astype(dtype)


def case(shape, dtype, seed=0, dt=1.0, names=NAMES):
    """tests/les_advect_ref.case (u, v, fields, hx, hy) with g and r: Courant sums below and above 1"""
    c = lar.case(shape, dtype, seed=seed, dt=dt, names=names)
    c["g"], c["r"] = profiles(shape[0], shape[3], numpy.dtype(dtype).type)
    return c


def oracle(c):
    return les_vadvect(c["fields"], c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one launch through ``eng.les_vadvect`` with every array inside a poisoned buffer; ``check`` compares the outputs, cmax
    and mtop with the oracle bit for bit, the inputs with what was uploaded, and looks at the bytes around every array.
    ``pad``: elements between the rows of g and r (a pitched profile)"""

    def __init__(self, eng, c, lead=0, cmax=True, mtop=True, pad=0):
        self.eng, self.c = eng, c
        self.mem = Poisoned(eng)
        put = lambda tag, a, poison: self.mem.put(tag, a, poison, lead)                    # noqa: E731
        prof = lambda tag, a: self.mem.rows(tag, a, 1e30, lead, pad)                        # noqa: E731
        self.du, self.dv = put("u", c["u"], float("nan")), put("v", c["v"], float("nan"))
        self.dev = {k: (self.du if x is c["u"] else self.dv if x is c["v"] else put(k, x, float("nan"))) for k, x in c["fields"].items()}
        self.out = {k: put("out " + k, numpy.full_like(x, OUT_FILL), 1e30) for k, x in c["fields"].items()}
        self.dhx, self.dhy = put("hx", c["hx"], 1e30), put("hy", c["hy"], 1e30)
        self.dg, self.dr = prof("g", c["g"]), prof("r", c["r"])
        self.dcmax = put("cmax", numpy.full_like(c["hx"], -5.0), 1e30) if cmax else None
        self.dmtop = put("mtop", numpy.full_like(c["u"], OUT_FILL), 1e30) if mtop else None
        self.got = eng.les_vadvect(self.dev, self.out, self.du, self.dv, self.dhx, self.dhy, self.dg, self.dr,
                                   cmax=self.dcmax if cmax else False, mtop=self.dmtop)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def check(self, what=""):
        c = self.c
        want, cmax, mtop = oracle(c)
        for k in c["fields"]:
            assert_bits("%s out %s" % (what, k), self.out[k].cpu().numpy(), want[k])
        if self.dcmax is None:
            assert self.got is None
        else:
            assert self.got is self.dcmax
            assert_bits("%s cmax" % what, self.dcmax.cpu().numpy(), cmax)
        if self.dmtop is not None:
            assert_bits("%s mtop" % what, self.dmtop.cpu().numpy(), mtop)
        for tag, t, a in [("u", self.du, c["u"]), ("v", self.dv, c["v"]), ("hx", self.dhx, c["hx"]), ("hy", self.dhy, c["hy"]),
                          ("g", self.dg, c["g"]), ("r", self.dr, c["r"])] + [(k, self.dev[k], x) for k, x in c["fields"].items()]:
            assert Poisoned.read_only(t, a), (what, tag, "read only")
        self.mem.check_around(what)
        return want, cmax, mtop


def raw_launch(eng, c, names=None, cmax=True, mtop=True, alias=None, extents=None, null=()):
    """spc_les_vadvect_* itself: (rc, dict name -> host output, host cmax or None, host mtop or None).  ``alias``: (slot, key)
    pairs that replace out[slot] (slot "mtop" / "cmax": that output) by the pointer of tensor ``key`` ("u", "v", "hx", "hy",
    "g", "r", "cmax", "mtop", a field name, or "out <name>"); ``extents``: overrides of n_les, itot, jtot, ktot, pitch_prof;
    ``null``: members set to NULL"""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    names = list(c["fields"]) if names is None else list(names)
    n, itot, jtot, ktot = c["u"].shape
    t = {"u": dev(c["u"]), "v": dev(c["v"]), "hx": dev(c["hx"]), "hy": dev(c["hy"]), "g": dev(c["g"]), "r": dev(c["r"]),
         "cmax": dev(numpy.full_like(c["hx"], -5.0)), "mtop": dev(numpy.full_like(c["u"], OUT_FILL))}
    for k in names:
        x = c["fields"][k]
        t[k] = t["u"] if x is c["u"] else t["v"] if x is c["v"] else dev(x)
        t["out " + k] = dev(numpy.full_like(x, OUT_FILL))
    a = _abi.LesVadvectArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.pitch_prof = n, itot, jtot, ktot, len(names), ktot
    a.u, a.v, a.hx, a.hy, a.g, a.r = (t[k].data_ptr() for k in ("u", "v", "hx", "hy", "g", "r"))
    if cmax:
        a.cmax = t["cmax"].data_ptr()
    if mtop:
        a.mtop = t["mtop"].data_ptr()
    for f, k in enumerate(names):
        a.fields[f], a.out[f] = t[k].data_ptr(), t["out " + k].data_ptr()
    for slot, key in (alias or ()):
        if slot in ("mtop", "cmax"):
            setattr(a, slot, t[key].data_ptr())
        else:
            a.out[slot] = t[key].data_ptr()
    fill_args(a, t, (), extents=extents, null=null)
    rc = abi_call(eng, "spc_les_vadvect", a)
    return rc, {k: t["out " + k].cpu().numpy() for k in names}, t["cmax"].cpu().numpy() if cmax else None, t["mtop"].cpu().numpy() if mtop else None


def split(ncols):
    """(n, itot, jtot) with n * itot * jtot == ncols, n and itot as large as 5 / 3 allow"""
    n = next(q for q in (5, 3, 2, 1) if ncols % q == 0)
    itot = next(q for q in (3, 2, 1) if (ncols // n) % q == 0)
    return n, itot, ncols // n // itot


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, n=3):
    """U, V (the winds themselves), THL and QT against the oracle, cmax and mtop included; the answer is not the input where the
    plane has a divergence"""
    c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
    want, cmax, mtop = Run(eng, c).check("n %d plane %s ktot %d" % (n, plane, ktot))
    assert (cmax >= 0).all() and not numpy.signbit(cmax).any()
    if min(plane) > 2 and ktot > 1:
        assert (cmax > 0).all() and all((want[k] != c["fields"][k]).any() for k in NAMES)


def check_rows(eng, ktot):
    """n = 1, 2, 5 at 3 x 5: hx, hy, g and r differ per LES, so a wrong l or a swapped profile shows"""
    for n in NS:
        c = case((n, 3, 5, ktot), np_of(eng), seed=1)
        assert (c["hx"] != c["hy"]).all() and (n == 1 or (c["hx"][0] != c["hx"][1] and (c["g"][0] != c["g"][1]).all() and (c["r"][0] != c["r"][1]).all()))
        Run(eng, c).check("rows n %d ktot %d" % (n, ktot))


def check_tiles(eng):
    """every boundary of the workgroups: n * itot * jtot of C - 1, C, C + 1 and 2 C + 1 columns for every C the dtype gets (a
    tile ends inside a row, inside an LES, and is one column), ktot on both sides of every change of
    spc_les_vadvect_cols_per_block, and one tall case of 17 columns at the last supported ktot; the first unsupported ktot is
    refused (SPC_ERR_UNSUPPORTED) and writes nothing"""
    first, changes, bad = cols_table(eng.vadvect_cols_per_block)
    assert sorted(first) == [16, 32, 64] and len(changes) == 2, (first, changes)
    for C, ktot in first.items():
        for ncols in (C - 1, C, C + 1, 2 * C + 1):
            n, itot, jtot = split(ncols)
            assert eng.vadvect_cols_per_block(ktot) == C
            Run(eng, case((n, itot, jtot, ktot), np_of(eng), seed=2, names=("U", "QT"))).check("C %d: %d x %d x %d x %d" % (C, n, itot, jtot, ktot))
    for k in changes:
        for ktot in (k - 1, k):
            Run(eng, case((1, 3, 23, ktot), np_of(eng), seed=3, names=("THL",))).check("change at %d: ktot %d" % (k, ktot))
    Run(eng, case((1, 1, 17, bad - 1), np_of(eng), seed=4, names=("V", "QT"))).check("tall: 17 columns of %d" % (bad - 1))
    rc, got, cmax, mtop = raw_launch(eng, case((1, 1, 2, bad), np_of(eng), seed=4, names=("QT",)))
    assert rc == _abi.SPC_ERR_UNSUPPORTED and b"levels" in eng.lib.spc_last_error()
    assert (got["QT"] == OUT_FILL).all() and (cmax == -5.0).all() and (mtop == OUT_FILL).all()
    return first, changes, bad


def check_fields(eng):
    """0 to 6 fields with U and V among them, 1 to 6 without, with and without cmax and mtop, a pitched g / r, and the C ABI"""
    dtype = np_of(eng)
    for nf in range(0, 7):
        Run(eng, case((2, 3, 5, 65), dtype, seed=3, names=ALL_NAMES[:nf])).check("%d fields with the winds" % nf)
        if nf:
            c = case((2, 3, 5, 65), dtype, seed=4, names=ALL_NAMES[:nf])
            rng = numpy.random.default_rng(nf)
            c["fields"] = {("F%d" % i): field_like(k, c["u"].shape, dtype, rng) for i, k in enumerate(ALL_NAMES[:nf])}  # none is u or v
            Run(eng, c).check("%d fields without the winds" % nf)
    for cmax in (True, False):
        for mtop in (True, False):
            Run(eng, case((2, 3, 5, 9), dtype, seed=5), cmax=cmax, mtop=mtop).check("cmax %s mtop %s" % (cmax, mtop))
    Run(eng, case((5, 3, 5, 33), dtype, seed=6), pad=3).check("pitched g and r")
    rc, got, cmax, mtop = raw_launch(eng, case((2, 3, 5, 9), dtype, seed=5))
    want = oracle(case((2, 3, 5, 9), dtype, seed=5))
    assert rc == 0
    for k in NAMES:
        assert_bits("raw %s" % k, got[k], want[0][k])
    assert_bits("raw cmax", cmax, want[1])
    assert_bits("raw mtop", mtop, want[2])


def check_probe(eng):
    """n_fields == 0 with cmax and / or mtop: bit-equal to those of a full launch and to the oracle's"""
    dtype = np_of(eng)
    for shape in ((1, 1, 1, 1), (2, 3, 5, 64), (5, 9, 9, 161)):
        c = case(shape, dtype, seed=6)
        _, want, mwant = oracle(c)
        full = Run(eng, c)
        full.check("full %s" % (shape,))
        for cmax, mtop in ((True, True), (True, False), (False, True)):
            probe = Run(eng, dict(c, fields={}), cmax=cmax, mtop=mtop)
            probe.check("probe %s" % (shape,))
            if cmax:
                assert_bits("probe == full", probe.dcmax.cpu().numpy(), full.dcmax.cpu().numpy())
                assert_bits("probe == oracle", probe.dcmax.cpu().numpy(), want)
            if mtop:
                assert_bits("probe mtop == full", probe.dmtop.cpu().numpy(), full.dmtop.cpu().numpy())
                assert_bits("probe mtop == oracle", probe.dmtop.cpu().numpy(), mwant)


def check_alignment(eng, lead, ktot=65):
    """views one (or more) elements off the 16-byte grid"""
    Run(eng, case((3, 3, 5, ktot), np_of(eng), seed=10 + lead), lead=lead).check("lead %d ktot %d" % (lead, ktot))


def column_winds(c, sign, level=None):
    """u of case ``c`` made convergent (sign +1: air rises everywhere in column (1, j)) or divergent (-1) around row i = 1 at
    every level, or at ``level`` only; v uniform per level"""
    n, itot, jtot, ktot = c["u"].shape
    T = c["u"].dtype.type
    c["u"][...] = T(2.0)
    c["v"][...] = (numpy.arange(ktot) % 3).astype(T)[None, None, None, :]
    ks = slice(None) if level is None else slice(level, level + 1)
    c["u"][:, 0, :, ks] = T(2.0 + sign)
    c["u"][:, 2, :, ks] = T(2.0 - sign)
    return c


def check_columns(eng):
    """all-convergent and all-divergent columns (pb alone or pt alone carries a column), a divergence at one level only (M is
    constant above it), winds uniform per level (M = 0: cmax = +0, every field keeps its bits) and exact zeros"""
    dtype = np_of(eng)
    for sign in (1, -1):
        c = column_winds(case((2, 4, 3, 9), dtype, seed=8, names=("THL", "QT")), sign)
        want, cmax, mtop = Run(eng, c).check("sign %d" % sign)
        assert (mtop[:, 1, :, :] * sign > 0).all() and (mtop[:, 3, :, :] * sign < 0).all() and (mtop[:, 0, :, :] == 0).all() and (cmax > 0).all()
        assert (want["THL"][:, 1] != c["fields"]["THL"][:, 1]).any()
        assert_bits("no divergence keeps THL", want["THL"][:, 0], c["fields"]["THL"][:, 0])
        c = column_winds(case((2, 4, 3, 9), dtype, seed=8, names=("THL", "QT")), sign, level=4)
        want, cmax, mtop = Run(eng, c).check("sign %d at level 4" % sign)
        assert (mtop[..., :4] == 0).all() and (mtop[:, 1, :, 4:] == mtop[:, 1, :, 4:5]).all() and (mtop[:, 1, :, 4] != 0).all()
    c = case((2, 3, 5, 9), dtype, seed=8, names=("THL", "QT"))
    c["u"][...] = (numpy.arange(9) - 4.0).astype(dtype)[None, None, None, :]
    c["v"][...] = dtype(3.0)
    r = Run(eng, c)
    _, cmax, mtop = r.check("uniform per level")
    assert not cmax.any() and not numpy.signbit(cmax).any() and not mtop.any()
    for k, x in c["fields"].items():
        assert_bits("uniform winds keep " + k, r.out[k].cpu().numpy(), x)
    c = case((2, 3, 5, 9), dtype, seed=8, names=("THL", "QT"))
    c["u"][...] = 0.0
    c["v"][...] = -0.0
    c["fields"]["QT"][...] = 0.0
    r = Run(eng, c)
    _, cmax, mtop = r.check("zeros")
    assert not cmax.any() and not r.out["QT"].cpu().numpy().any()


def special_case(dtype, ktot=7):
    """(clean case with fields that are not the winds, the same with NaN, +inf, -inf and -0.0 planted in one cell each of THL,
    the mask of the cells within one level of a planted value)"""
    c = case((3, 9, 9, ktot), dtype, seed=9, names=("THL", "QT"))
    s = dict(c, fields={k: x.copy() for k, x in c["fields"].items()})
    planted = {(0, 0, 0, 1): numpy.nan, (0, 4, 8, 2): numpy.inf, (1, 8, 3, 0): -numpy.inf, (1, 2, 6, ktot - 1): -0.0}
    mask = numpy.zeros(c["u"].shape, dtype=bool)
    for (l, i, j, k), val in planted.items():
        s["fields"]["THL"][l, i, j, k] = val
        mask[l, i, j, max(k - 1, 0):k + 2] = True
    return c, s, mask


def check_special(eng):
    """NaN, +-inf and -0.0 planted in single cells of a field: every output is the oracle's and the cells further than one
    level away hold the bits of a run without them.  A NaN in one wind cell u[l][i][j][k]: every cell outside the columns
    (i - 1 ... i + 1, j) at the levels >= k is bit-equal to the run without it, and cmax stays finite.  A constant field keeps
    its bits under any winds"""
    dtype = np_of(eng)
    c, s, mask = special_case(dtype)
    clean, _, clean_mtop = Run(eng, c).check("clean")
    r = Run(eng, s)
    want, cmax, _ = r.check("special")
    assert_bits("the cells further away", r.out["THL"].cpu().numpy()[~mask], clean["THL"][~mask])
    assert_bits("QT never sees THL", r.out["QT"].cpu().numpy(), clean["QT"])
    assert numpy.isnan(want["THL"][0, 0, 0, :3]).any() and numpy.isfinite(cmax).all()
    w = dict(c, u=c["u"].copy())
    w["u"][2, 0, 4, 3] = numpy.nan
    r = Run(eng, w)
    want, cmax, mtop = r.check("NaN wind")
    mask = numpy.zeros(c["u"].shape, dtype=bool)
    for i in (8, 0, 1):
        mask[2, i, 4, 3:] = True
    for k in ("THL", "QT"):
        assert_bits("outside the NaN's columns, " + k, r.out[k].cpu().numpy()[~mask], clean[k][~mask])
    assert_bits("mtop outside the NaN's columns", mtop[~mask], clean_mtop[~mask])
    assert numpy.isnan(mtop[mask]).all() and numpy.isfinite(cmax).all()
    k = case((2, 3, 5, 9), dtype, seed=10, names=("THL", "QT"))
    k["fields"]["THL"][...] = dtype(287.3)
    k["fields"]["QT"][...] = dtype(-1e-3)
    r = Run(eng, k)
    r.check("constants")
    for name in ("THL", "QT"):
        assert_bits("a constant keeps its bits: " + name, r.out[name].cpu().numpy(), k["fields"][name])


def elsewhere(eng, t):
    """``t`` on another device than the engine's: the host for an engine on a GPU, the meta device for a stand-in on the host"""
    return t.cpu() if eng.device.type == "cuda" else t.to("meta")


def bad_calls(eng, t, o, u, v, hx, hy, g, r, m):
    """the calls of ``Engine.les_vadvect`` that are refused, as callables: ``check_refusals`` makes them on a device,
    tests/test_engine_les_args_cpu.py on a stand-in that launches nothing, where it pins their texts"""
    many = {("F%d" % i): t["QT"].clone() for i in range(7)}
    other = torch.float64 if eng.dtype == torch.float32 else torch.float32
    V = eng.les_vadvect
    return [lambda: V({}, {}, u, v, hx, hy, g, r, cmax=False),
            lambda: V({}, {}, u, v, hx, hy, g, r, cmax=None, mtop=None),
            lambda: V(t, dict(o, QT=t["THL"]), u, v, hx, hy, g, r),
            lambda: V(t, dict(o, QT=u), u, v, hx, hy, g, r),
            lambda: V(t, dict(o, QT=o["THL"]), u, v, hx, hy, g, r),
            lambda: V(t, o, u, v, hx, hy, g, r, mtop=o["QT"]),
            lambda: V(t, o, u, v, hx, hy, g, r, mtop=u),
            lambda: V(t, o, u, v, hx, hy, g, r, mtop=m[:, :1]),
            lambda: V(t, {k: x for k, x in o.items() if k != "QT"}, u, v, hx, hy, g, r),
            lambda: V(many, {k: torch.empty_like(x) for k, x in many.items()}, u, v, hx, hy, g, r),
            lambda: V(t, o, u, v[:, :1], hx, hy, g, r),
            lambda: V(t, o, u, v, hx[:1], hy, g, r),
            lambda: V(t, o, u, v, hx, hy, g[:1], r),
            lambda: V(t, o, u, v, hx, hy, g, r[:, :7]),
            lambda: V(t, o, u, v, hx, hy, g, None),
            lambda: V(t, o, u, v, hx, hy, g, r, cmax=hx),
            lambda: V(t, o, u, v, hx, hy, g, r, cmax=torch.empty(3, dtype=eng.dtype, device=eng.device)),
            lambda: V({"QT": t["QT"][..., ::2]}, {"QT": o["QT"][..., ::2]}, u, v, hx, hy, g, r),
            lambda: V({"QT": t["QT"].to(other)}, {"QT": o["QT"]}, u, v, hx, hy, g, r),
            lambda: V({"QT": elsewhere(eng, t["QT"])}, {"QT": o["QT"]}, u, v, hx, hy, g, r)]


def check_refusals(eng):
    """n = 0 is a no-op; nothing to do, a NULL g or r, pitch_prof < ktot, an output that is an input or another output and an
    extent below 1 are refused by the library and by the engine, and no refused call touches anything"""
    dtype = np_of(eng)
    c = case((2, 2, 3, 8), dtype, seed=11)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    for kw, text in ((dict(names=(), cmax=False, mtop=False), b"nothing to do"), (dict(null=("g",)), b"g is NULL"), (dict(null=("r",)), b"r is NULL"),
                     (dict(extents={"pitch_prof": 7}), b"pitch_prof"), (dict(alias=((2, "u"),)), b"also an input"),
                     (dict(alias=((2, "QT"),)), b"also an input"), (dict(alias=((3, "THL"),)), b"also an input"),
                     (dict(alias=((2, "hy"),)), b"also an input"), (dict(alias=((2, "g"),)), b"also an input"), (dict(alias=((3, "r"),)), b"also an input"),
                     (dict(alias=((3, "cmax"),)), b"same array"), (dict(alias=((3, "mtop"),)), b"same array"), (dict(alias=((3, "out U"),)), b"same array"),
                     (dict(alias=(("mtop", "v"),)), b"also an input"), (dict(alias=(("mtop", "THL"),)), b"also an input"),
                     (dict(alias=(("mtop", "out QT"),)), b"same array"), (dict(alias=(("cmax", "hx"),)), b"also an input"),
                     (dict(alias=(("cmax", "mtop"),)), b"same array"), (dict(extents={"itot": 0}), b">= 1"),
                     (dict(extents={"jtot": 0}), b">= 1"), (dict(extents={"ktot": -1}), b">= 1"), (dict(extents={"n_les": -1}), b"< 0")):
        rc, got, cmax, mtop = raw_launch(eng, c, **kw)
        assert rc == E and text in eng.lib.spc_last_error(), (kw, rc, eng.lib.spc_last_error())
        assert all((v == OUT_FILL).all() for v in got.values()) and (cmax is None or (cmax == -5.0).all()), kw
        assert mtop is None or (mtop == OUT_FILL).all(), kw
    rc, got, cmax, mtop = raw_launch(eng, c, extents={"n_les": 0})
    assert rc == 0 and all((v == OUT_FILL).all() for v in got.values()) and (cmax == -5.0).all() and (mtop == OUT_FILL).all()
    u, v, hx, hy, g, r = (dev(c[k]) for k in ("u", "v", "hx", "hy", "g", "r"))
    t = {"U": u, "V": v, "THL": dev(c["fields"]["THL"]), "QT": dev(c["fields"]["QT"])}
    o = {k: torch.full_like(x, OUT_FILL) for k, x in t.items()}
    m = torch.full_like(u, OUT_FILL)
    got = eng.les_vadvect({k: x[:0] for k, x in t.items()}, {k: x[:0] for k, x in o.items()}, u[:0], v[:0], hx[:0], hy[:0], g[:0], r[:0], mtop=m[:0])
    assert tuple(got.shape) == (0,)
    for bad in bad_calls(eng, t, o, u, v, hx, hy, g, r, m):
        try:
            bad()
        except (ValueError, TypeError):
            pass
        else:
            raise AssertionError("a bad call was not refused")
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    for k, x in o.items():
        assert bool((x == OUT_FILL).all()), k
    assert bool((m == OUT_FILL).all())
    for k, x in c["fields"].items():
        assert_bits("refused: " + k, t[k].cpu().numpy(), x)


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle, cmax and mtop included"""
    c = case((n, 3, 5, 40), np_of(one), seed=n)
    want, cmax, mtop = oracle(c)
    for tag, eng, up in on_both(one, multi, n):
        u, v = up(c["u"]), up(c["v"])
        t = {k: (u if x is c["u"] else v if x is c["v"] else up(x)) for k, x in c["fields"].items()}
        o = {k: up(numpy.full_like(x, OUT_FILL)) for k, x in c["fields"].items()}
        m = up(numpy.full_like(c["u"], OUT_FILL))
        prof = [up(c[k]) for k in ("hx", "hy", "g", "r")]
        got = eng.les_vadvect(t, o, u, v, *prof, mtop=m)
        multi.synchronize()
        for k in NAMES:
            assert_bits("%s %s" % (tag, k), host_of(o[k]), want[k])
        assert_bits("%s cmax" % tag, host_of(got), cmax)
        assert_bits("%s mtop" % tag, host_of(m), mtop)
        probe = eng.les_vadvect({}, {}, u, v, *prof)
        multi.synchronize()
        assert_bits("%s probe" % tag, host_of(probe), cmax)
    return blocks_of(o["QT"], multi, n)


BODIES = ("parity", "rows", "tiles", "fields", "probe", "alignment", "columns", "special", "refusals")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in (1, 3, 64, 161)]),
            ("rows", lambda: [check_rows(eng, k) for k in (1, 65)]),
            ("tiles", lambda: check_tiles(eng)),
            ("fields", lambda: check_fields(eng)),
            ("probe", lambda: check_probe(eng)),
            ("alignment", lambda: [check_alignment(eng, lead) for lead in (1, 3)]),
            ("columns", lambda: check_columns(eng)),
            ("special", lambda: check_special(eng)),
            ("refusals", lambda: check_refusals(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_vadvect (CPU suite) ------------------------------------------------------------------------
class VadvectOracleEngine(lar.AdvectOracleEngine):
    """tests/les_advect_ref.AdvectOracleEngine with ``les_vadvect`` by the NumPy oracle above: the outputs written whole into
    the caller's tensors, as the HIP engine does"""

    def les_vadvect(self, fields, out, u, v, hx, hy, g, r, cmax=True, mtop=None, **kw):
        want = cmax is not None and cmax is not False
        if sorted(fields) != sorted(out) or (not fields and not want and mtop is None):
            raise ValueError("out does not match the fields, or nothing to do")
        read = {t.data_ptr() for t in [u, v] + list(fields.values())}
        written = [t.data_ptr() for t in out.values()] + ([mtop.data_ptr()] if mtop is not None else [])
        if u.shape[0] and (len(set(written)) != len(written) or set(written) & read):
            raise ValueError("an output is an input or another output")
        res, c, m = les_vadvect({k: t.numpy() for k, t in fields.items()}, u.numpy(), v.numpy(), hx.numpy(), hy.numpy(),
                                numpy.ascontiguousarray(g.numpy()), numpy.ascontiguousarray(r.numpy()))
        for k, t in out.items():
            t.copy_(torch.from_numpy(res[k]))
        if mtop is not None:
            mtop.copy_(torch.from_numpy(m))
        if not want:
            return None
        c = torch.from_numpy(c)
        return c if cmax is True else cmax.copy_(c)


# -- the host twins of models.DeviceLESEnsemble after enable_advection(vertical=True) --------------------------------------------
class _HostVadvect:
    """NumPy fields: the executable definition of what evolve_model_batched does after enable_advection(vertical=True): K16's
    and K17's probes with the coefficients of the whole step, then per substep K16 and K17 on the winds K16 produced"""

    advect_vertical = False
    advect_courant_z = None
    _mtop = _mtop_dt = None

    def enable_advection(self, dx=None, dy=None, cfl=None, max_substeps=None, vertical=False):
        super().enable_advection(dx=dx, dy=dy, cfl=cfl, max_substeps=max_substeps)
        self.advect_vertical = bool(vertical)

    def _advect(self, dt):
        if not self.advect_vertical:
            return super()._advect(dt)
        f, par = self.fields3d, self.advect_par
        T = f["U"].dtype
        g, r = (a.astype(T) for a in adv.vertical_profiles(self.water_path_weights()))
        hx, hy = (a.astype(T) for a in adv.coefficients(dt, par["dx"], par["dy"], n=self.n))
        c = float(lar.faces(f["U"], f["V"], hx, hy)[4].max())
        c = max(c, float(face_numbers(mass_flux(f["U"], f["V"], hx, hy, g), r)[2].max()))
        n_sub = adv.substeps(c, par["cfl"], par["max_substeps"])
        hx, hy = (a.astype(T) for a in adv.coefficients(dt / n_sub, par["dx"], par["dy"], n=self.n))
        worst = worst_z = 0.0
        for _ in range(n_sub):
            new, cmax = lar.les_advect({k: f[k] for k in self.KEYS if k in f}, f["U"], f["V"], hx, hy)
            f.update(new)
            worst = max(worst, float(cmax.max()))
            new, cmax, self._mtop = les_vadvect({k: f[k] for k in self.KEYS if k in f}, f["U"], f["V"], hx, hy, g, r)
            f.update(new)
            worst_z = max(worst_z, float(cmax.max()))
        self.advect_substeps, self.advect_courant, self.advect_courant_z, self._mtop_dt = n_sub, worst, worst_z, dt / n_sub

    def get_vertical_wind_batched(self):
        if self._mtop is None:
            return None
        rho = numpy.asarray(self.p["Rhobf"], dtype=numpy.float64)
        face = 0.5 * (rho + numpy.concatenate([rho[:, 1:], rho[:, -1:]], axis=1))
        # (float64 from the T mass flux, rounded once: within 3 roundings of the device's expression in T, bound of check_w: 4)
        return (self._mtop / (face * self._mtop_dt)[:, None, None, :]).astype(self.dtype)


class HostVadvectLESEnsemble(_HostVadvect, lar.HostAdvectLESEnsemble):
    """without enable_thermo()"""


class HostThermoVadvectLESEnsemble(_HostVadvect, lar.HostThermoAdvectLESEnsemble):
    """after enable_thermo()"""


RAISED = (1, 3)                                                   # the column (i, j) whose U is raised
DX = 30000.0                                                      # the vertical Courant sums of the first step (0.7 ... 0.9) ask for 2 substeps


def ensemble_run(engine, n, thermo, device, micro=False, diffuse=False, vertical=True, dx=DX, itot=4, jtot=5, nL=20, steps=3):
    """tests/les_advect_ref.ensemble_run with U raised by 2 m/s in the column RAISED of every LES (air converges on one side
    of it and diverges on the other) and enable_advection(vertical=...): after every step every profile, the fields, the
    substeps, both Courant sums and W.  Returns (ens, list of records)"""
    def before(ens):
        assert not vertical or ens.get_vertical_wind_batched() is None
    # (``vertical`` None: the call as it was before K17)
    return ensemble_case(engine, n, models.DeviceLESEnsemble if device else (HostThermoVadvectLESEnsemble if thermo else HostVadvectLESEnsemble),
                         thermo=thermo, micro=micro, diffuse=diffuse, edit=raise_u,
                         advection=dict(dx=dx, dy=1.5 * numpy.asarray(dx), **({} if vertical is None else {"vertical": vertical})),
                         record=lambda ens, rec: lar.record_substeps(ens, rec, z=vertical), before=before, itot=itot, jtot=jtot, nL=nL, steps=steps)


def raise_u(fields):
    fields["U"][:, RAISED[0], RAISED[1], :] += 2.0


def check_w(ens, twin):
    """the device W against the twin's: a torch expression, so within a few roundings (4 eps of the largest |W|)"""
    w, want = host_of(ens.get_vertical_wind_batched()), twin.get_vertical_wind_batched()
    assert w.shape == want.shape and numpy.isfinite(want).all() and numpy.abs(want).max() > 0
    assert w.dtype == want.dtype and numpy.abs(w - want).max() <= 4 * numpy.finfo(want.dtype).eps * numpy.abs(want).max()


def check_ensemble(one, engines, n, thermo, micro=False, diffuse=False, **kw):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``; the vertical wind carries the
    fields: THL in and next to the raised column differs from the same run with vertical=False, which is bit-equal to the run
    of enable_advection() without the argument.  Returns the twin's substeps of the first step"""
    twin, host = ensemble_run(one, n, thermo, False, micro=micro, diffuse=diffuse, **kw)
    flat = ensemble_run(one, n, thermo, False, micro=micro, diffuse=diffuse, vertical=False, **kw)[1]
    i, j = RAISED
    assert all((host[1]["field THL"][:, i + di, j, 1:] != flat[1]["field THL"][:, i + di, j, 1:]).any() for di in (-1, 0, 1))
    n_sub = int(host[1]["substeps"][0])
    assert n_sub in (2, 3), n_sub
    assert 0 < host[1]["courant"][0] <= 0.5 and 0 < host[1]["courant z"][0] and numpy.isfinite(host[-1]["courant z"][0])
    for engine in engines:
        ens, log = ensemble_run(engine, n, thermo, True, micro=micro, diffuse=diffuse, **kw)
        lmr.same_logs(host, log)
        check_w(ens, twin)
        lmr.same_logs(flat, ensemble_run(engine, n, thermo, True, micro=micro, diffuse=diffuse, vertical=False, **kw)[1])
        if engine is engines[0]:
            lmr.same_logs(flat, ensemble_run(engine, n, thermo, True, micro=micro, diffuse=diffuse, vertical=None, **kw)[1])
    return n_sub
