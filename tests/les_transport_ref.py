"""NumPy oracle of K22 (include/spc.h: spc_les_transport_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_transport_gpu.py (each takes an engine: tools/mutation_control.py --transport hands them the engines of its
mutant libraries), the host twins of DeviceLESEnsemble's enable_advection(vertical=True, conservative=True) and an
oracle-backed engine with ``les_transport`` for the CPU suite.

The oracle spells the rule out in the statement order of include/spc.h, one operation per NumPy call in the element type, the
neighbours by numpy.roll, the mass flux by a Python loop over the levels (tests/les_vadvect_ref.mass_flux), so nothing fuses.
Every device array of the bodies is the LEADING part of a poisoned buffer (tests/les_harness.Poisoned); the bytes behind it
(and in front of a view off the 16-byte grid) are checked after the launch, the inputs against what was uploaded."""
import ctypes

import numpy
import torch

from sp_coupler_amd import _abi, models
from sp_coupler_amd import advection as adv
from sp_coupler_amd import buoyancy as buo
from tests import les_advect_ref as lar
from tests import les_buoyancy_ref as lbr
from tests import les_micro_ref as lmr
from tests import les_radiate_ref as lrr
from tests import les_vadvect_ref as lvr
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, cols_table, ensemble_case, fill_args, host_of, np_of, on_both, run_bodies)

#: a cell that is its own four neighbours, one extent of 1 either way, both neighbours the same cell, itot < jtot, a plane of
#: exactly 64 columns, and a row longer than a wave
PLANES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (8, 8), (5, 33)]
KTOTS = [1, 2, 3, 63, 64, 65, 160]
NS = lar.NS
NAMES = lar.NAMES
ALL_NAMES = lar.ALL_NAMES
OUT_FILL = lar.OUT_FILL
MAX_CELLS = 130 * 4 * 5 * 20                                       # no case is larger
field_like = lar.field_like
derived_cols = lbr.derived_cols
split = lvr.split
profiles = lvr.profiles
case = lvr.case


# -- the rule --------------------------------------------------------------------------------------------------------------
def parts(c):
    """(p, q) of face numbers c: p = c > 0 ? c : 0, q = c < 0 ? c : 0 (a NaN gives +0 twice)"""
    zero = c.dtype.type(0)
    with numpy.errstate(all="ignore"):
        return numpy.where(c > 0, c, zero), numpy.where(c < 0, c, zero)


def face_numbers(u, v, hx, hy, g, r):
    """dict of the twelve face numbers pw, qw, ..., pt, qt, the outflow Courant sum s and M [.. x ktot + 1]"""
    T = u.dtype
    cw, ce, cs, cn = lvr.courant_faces(u, v, hx, hy)
    M = lvr.mass_flux(u, v, hx, hy, g)
    n = {"M": M}
    n["pw"], n["qw"] = parts(cw)
    n["pe"], n["qe"] = parts(ce)
    n["ps"], n["qs"] = parts(cs)
    n["pn"], n["qn"] = parts(cn)
    n["pb"], n["qb"] = parts(M[..., :-1])
    n["pt"], n["qt"] = parts(M[..., 1:])
    rr = r[:, None, None, :]
    with numpy.errstate(all="ignore"):
        sx = n["pe"] - n["qw"]
        sy = n["pn"] - n["qs"]
        sh = sx + sy
        sz = n["pt"] - n["qb"]
        sv = rr * sz
        n["s"] = sh + sv
    assert all(a.dtype == T for a in n.values())
    return n


def fluxes(x, n):
    """(Fw, Fe, Fs, Fn, Fb, Ft) of the field x and the face numbers n"""
    with numpy.errstate(all="ignore"):
        xw, xe = numpy.roll(x, 1, axis=1), numpy.roll(x, -1, axis=1)
        xs, xn = numpy.roll(x, 1, axis=2), numpy.roll(x, -1, axis=2)
        xm = numpy.concatenate([x[..., :1], x[..., :-1]], axis=3)
        xp = numpy.concatenate([x[..., 1:], x[..., -1:]], axis=3)
        w1, w2 = n["pw"] * xw, n["qw"] * x
        e1, e2 = n["pe"] * x, n["qe"] * xe
        s1, s2 = n["ps"] * xs, n["qs"] * x
        n1, n2 = n["pn"] * x, n["qn"] * xn
        b1, b2 = n["pb"] * xm, n["qb"] * x
        t1, t2 = n["pt"] * x, n["qt"] * xp
        return w1 + w2, e1 + e2, s1 + s2, n1 + n2, b1 + b2, t1 + t2


def les_transport(fields, u, v, hx, hy, g, r):
    """(dict name -> the new field (a new array), cmax [n], mtop, dict name -> ftop [n x itot x jtot]): fields, u, v
    [n x itot x jtot x ktot] of dtype T, hx, hy [n], g, r [n x ktot]"""
    nums = face_numbers(u, v, hx, hy, g, r)
    n = u.shape[0]
    cmax = nums["s"].reshape(n, -1).max(axis=1) if n else numpy.zeros(0, dtype=u.dtype)
    rr = r[:, None, None, :]
    out, ftop = {}, {}
    with numpy.errstate(all="ignore"):
        for k, x in fields.items():
            assert x.dtype == u.dtype and x.shape == u.shape
            Fw, Fe, Fs, Fn, Fb, Ft = fluxes(x, nums)
            hi = Fe - Fw
            hj = Fn - Fs
            h = hi + hj
            dz = Ft - Fb
            z = rr * dz
            y = x - h
            y = y - z
            assert y.dtype == x.dtype and Ft.dtype == x.dtype
            out[k] = y
            ftop[k] = numpy.ascontiguousarray(Ft[..., -1])
    return out, cmax, numpy.ascontiguousarray(nums["M"][..., 1:]), ftop


def oracle(c):
    return les_transport(c["fields"], c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])


def split_pair(fields, u, v, hx, hy, g, r):
    """what the split pair does with the same arguments: K16, then K17 on the winds and fields K16 produced (the winds are
    transported only where they are among the fields, as in the ensemble).  Returns the new fields"""
    new, _ = lar.les_advect(fields, u, v, hx, hy)
    u2 = next((new[k] for k, x in fields.items() if x is u), u)
    v2 = next((new[k] for k, x in fields.items() if x is v), v)
    return lvr.les_vadvect(new, u2, v2, hx, hy, g, r)[0]


def scaled(c, target=0.9):
    """case ``c`` with its winds rescaled to a largest outflow Courant sum of ``target`` (s is linear in the winds); the fields
    that are the winds follow"""
    T = c["u"].dtype.type
    unit = float(face_numbers(c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])["s"].max())
    assert unit > 0
    k = T(target / unit)
    u, v = c["u"] * k, c["v"] * k
    fields = {name: (u if x is c["u"] else v if x is c["v"] else x) for name, x in c["fields"].items()}
    return dict(c, u=u, v=v, fields=fields)


def closed_cell(dtype, n=1, itot=8, jtot=8, ktot=40, courant=0.34):
    """the closed overturning cell: u = 4 sin(2 pi i / itot) a(k) with sum_k g a = 0 (made exact to rounding by correcting the
    top level), v = 0, so nothing passes the lid up to rounding; hx is chosen for a largest outflow Courant sum of ``courant``.
    One QT-like field"""
    T = numpy.dtype(dtype).type
    g, r = profiles(n, ktot, numpy.float64)
    a = numpy.cos(numpy.pi * (numpy.arange(ktot) + 0.5) / ktot)[None, :] * numpy.ones((n, 1))
    a[:, -1] -= (g * a).sum(axis=1) / g[:, -1]
    i = numpy.arange(itot)
    u = (4.0 * numpy.sin(2.0 * numpy.pi * i / itot)[None, :, None, None] * a[:, None, None, :] * numpy.ones((1, 1, jtot, 1))).astype(T)
    v = numpy.zeros_like(u)
    rng = numpy.random.default_rng(40)
    c = dict(u=u, v=v, fields={"QT": field_like("QT", u.shape, T, rng)}, hx=numpy.full(n, 1e-3, dtype=T), hy=numpy.full(n, 1e-3, dtype=T),
             g=g.astype(T), r=r.astype(T))
    unit = float(face_numbers(c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])["s"].max())
    c["hx"] = (c["hx"].astype(numpy.float64) * courant / unit).astype(T)
    return c


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one launch through ``eng.les_transport`` with every array inside a poisoned buffer; ``check`` compares the outputs, cmax,
    mtop and ftop with the oracle bit for bit, the inputs with what was uploaded, and looks at the bytes around every array.
    ``pad``: elements between the rows of g and r (a pitched profile)"""

    def __init__(self, eng, c, lead=0, cmax=True, mtop=True, ftop=True, pad=0):
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
        nf = len(c["fields"])
        self.dftop = put("ftop", numpy.full((nf,) + c["u"].shape[:3], OUT_FILL, dtype=c["u"].dtype), 1e30) if ftop and nf else None
        self.got = eng.les_transport(self.dev, self.out, self.du, self.dv, self.dhx, self.dhy, self.dg, self.dr,
                                     cmax=self.dcmax if cmax else False, mtop=self.dmtop, ftop=self.dftop)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def check(self, what=""):
        c = self.c
        want, cmax, mtop, ftop = oracle(c)
        for k in c["fields"]:
            assert_bits("%s out %s" % (what, k), self.out[k].cpu().numpy(), want[k])
        if self.dcmax is None:
            assert self.got is None
        else:
            assert self.got is self.dcmax
            assert_bits("%s cmax" % what, self.dcmax.cpu().numpy(), cmax)
        if self.dmtop is not None:
            assert_bits("%s mtop" % what, self.dmtop.cpu().numpy(), mtop)
        if self.dftop is not None:
            got = self.dftop.cpu().numpy()
            for q, k in enumerate(c["fields"]):
                assert_bits("%s ftop %s" % (what, k), got[q], ftop[k])
        for tag, t, a in [("u", self.du, c["u"]), ("v", self.dv, c["v"]), ("hx", self.dhx, c["hx"]), ("hy", self.dhy, c["hy"]),
                          ("g", self.dg, c["g"]), ("r", self.dr, c["r"])] + [(k, self.dev[k], x) for k, x in c["fields"].items()]:
            assert Poisoned.read_only(t, a), (what, tag, "read only")
        self.mem.check_around(what)
        return want, cmax, mtop, ftop


def raw_launch(eng, c, names=None, cmax=True, mtop=True, ftop=True, alias=None, extents=None, null=()):
    """spc_les_transport_* itself: (rc, dict name -> host output, host cmax or None, host mtop or None, host ftop or None).
    ``alias``: (slot, key) pairs that replace out[slot] (slot "mtop" / "cmax" / "ftop": that output) by the pointer of tensor
    ``key`` ("u", "v", "hx", "hy", "g", "r", "cmax", "mtop", "ftop", a field name, or "out <name>"); ``extents``: overrides of
    n_les, itot, jtot, ktot, pitch_prof, n_fields; ``null``: members set to NULL"""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    names = list(c["fields"]) if names is None else list(names)
    n, itot, jtot, ktot = c["u"].shape
    t = {"u": dev(c["u"]), "v": dev(c["v"]), "hx": dev(c["hx"]), "hy": dev(c["hy"]), "g": dev(c["g"]), "r": dev(c["r"]),
         "cmax": dev(numpy.full_like(c["hx"], -5.0)), "mtop": dev(numpy.full_like(c["u"], OUT_FILL)),
         "ftop": dev(numpy.full((max(len(names), 1), n, itot, jtot), OUT_FILL, dtype=c["u"].dtype))}
    for k in names:
        x = c["fields"][k]
        t[k] = t["u"] if x is c["u"] else t["v"] if x is c["v"] else dev(x)
        t["out " + k] = dev(numpy.full_like(x, OUT_FILL))
    a = _abi.LesTransportArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.pitch_prof = n, itot, jtot, ktot, len(names), ktot
    a.u, a.v, a.hx, a.hy, a.g, a.r = (t[k].data_ptr() for k in ("u", "v", "hx", "hy", "g", "r"))
    for flag, slot in ((cmax, "cmax"), (mtop, "mtop"), (ftop, "ftop")):
        if flag:
            setattr(a, slot, t[slot].data_ptr())
    for f, k in enumerate(names):
        a.fields[f], a.out[f] = t[k].data_ptr(), t["out " + k].data_ptr()
    for slot, key in (alias or ()):
        if slot in ("mtop", "cmax", "ftop"):
            setattr(a, slot, t[key].data_ptr())
        else:
            a.out[slot] = t[key].data_ptr()
    fill_args(a, t, (), extents=extents, null=null)
    rc = abi_call(eng, "spc_les_transport", a)
    host = lambda flag, k: t[k].cpu().numpy() if flag else None                             # noqa: E731
    return rc, {k: t["out " + k].cpu().numpy() for k in names}, host(cmax, "cmax"), host(mtop, "mtop"), host(ftop, "ftop")


def _n_for(plane, ktot, n=3):
    """n LES, or 1 where n of them would be larger than MAX_CELLS"""
    return n if n * plane[0] * plane[1] * ktot <= MAX_CELLS else 1


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, n=3):
    """U, V (the winds themselves), THL and QT against the oracle, cmax, mtop and ftop included; mtop is K17's oracle's; the
    answer is not the input where the plane has a gradient"""
    n = _n_for(plane, ktot, n)
    c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
    want, cmax, mtop, ftop = Run(eng, c).check("n %d plane %s ktot %d" % (n, plane, ktot))
    assert_bits("mtop is K17's", mtop, lvr.oracle(c)[2])
    assert (cmax >= 0).all() and not numpy.signbit(cmax).any() and not numpy.isnan(cmax).any()
    if min(plane) > 2:
        assert (cmax > 0).all() and all((want[k] != c["fields"][k]).any() for k in NAMES)
        if ktot > 1:
            assert all(f.any() for f in ftop.values())


def check_rows(eng, ktot):
    """n = 1, 2, 5 at 3 x 5: hx, hy, g and r differ per LES (and hx from hy), so a wrong l or a swapped profile shows; then the
    same with pitched profiles"""
    for n in NS:
        c = case((n, 3, 5, ktot), np_of(eng), seed=1)
        assert (c["hx"] != c["hy"]).all() and (n == 1 or (c["hx"][0] != c["hx"][1] and (c["g"][0] != c["g"][1]).all() and (c["r"][0] != c["r"][1]).all()))
        Run(eng, c).check("rows n %d ktot %d" % (n, ktot))
        Run(eng, c, pad=3).check("rows n %d ktot %d pitched" % (n, ktot))


def check_tiles(eng):
    """every boundary of the workgroups: n * itot * jtot of C - 1, C, C + 1 and 2 C + 1 columns for every C the dtype gets (a
    tile ends inside a row, inside an LES, and is one column; tests/les_vadvect_ref.split gives LES of up to 3 rows), ktot on
    both sides of every change of spc_les_transport_cols_per_block, and 17 columns at the last supported ktot; the first
    unsupported ktot is refused (SPC_ERR_UNSUPPORTED) and writes nothing.  The thresholds the library reports are the ones that
    follow from the LDS budget and the pitch (derived_cols)"""
    dtype = np_of(eng)
    esize = numpy.dtype(dtype).itemsize
    first, changes, bad = table = cols_table(eng.transport_cols_per_block)
    assert table == cols_table(lambda k: derived_cols(k, esize))
    assert sorted(first) == [16, 32, 64] and len(changes) == 2, table
    for C, k0 in first.items():
        ktot = 7 if C == 64 else k0
        assert eng.transport_cols_per_block(ktot) == C
        for ncols in (C - 1, C, C + 1, 2 * C + 1):
            n, itot, jtot = split(ncols)
            Run(eng, case((n, itot, jtot, ktot), dtype, seed=2, names=("U", "QT"))).check("C %d: %d x %d x %d x %d" % (C, n, itot, jtot, ktot))
    for k in changes:
        for ktot in (k - 1, k):
            Run(eng, case((1, 3, 23, ktot), dtype, seed=3, names=("THL",))).check("change at %d: ktot %d" % (k, ktot))
    Run(eng, case((1, 1, 17, bad - 1), dtype, seed=4, names=("V", "QT"))).check("tall: 17 columns of %d" % (bad - 1))
    rc, got, cmax, mtop, ftop = raw_launch(eng, case((1, 1, 2, bad), dtype, seed=4, names=("QT",)))
    assert rc == _abi.SPC_ERR_UNSUPPORTED and b"levels" in eng.lib.spc_last_error()
    assert (got["QT"] == OUT_FILL).all() and (cmax == -5.0).all() and (mtop == OUT_FILL).all() and (ftop == OUT_FILL).all()
    return table


def check_fields(eng):
    """0 to 6 fields with U and V among them, 1 to 6 without, with and without cmax, mtop and ftop, and the C ABI"""
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
            for ftop in (True, False):
                Run(eng, case((2, 3, 5, 9), dtype, seed=5), cmax=cmax, mtop=mtop, ftop=ftop).check("cmax %s mtop %s ftop %s" % (cmax, mtop, ftop))
    rc, got, cmax, mtop, ftop = raw_launch(eng, case((2, 3, 5, 9), dtype, seed=5))
    want = oracle(case((2, 3, 5, 9), dtype, seed=5))
    assert rc == 0
    for q, k in enumerate(NAMES):
        assert_bits("raw %s" % k, got[k], want[0][k])
        assert_bits("raw ftop %s" % k, ftop[q], want[3][k])
    assert_bits("raw cmax", cmax, want[1])
    assert_bits("raw mtop", mtop, want[2])


def check_probe(eng):
    """n_fields == 0 with cmax and / or mtop: bit-equal to those of a full launch and to the oracle's"""
    dtype = np_of(eng)
    for shape in ((1, 1, 1, 1), (2, 3, 5, 64), (5, 9, 9, 65)):
        c = case(shape, dtype, seed=6)
        _, want, mwant, _ = oracle(c)
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


def check_signs(eng):
    """winds of either sign in all combinations (u, v each +, - per LES, so every horizontal face is an inflow or an outflow
    face everywhere), convergent and divergent columns (M of one sign up a column), exact zeros, and winds uniform per level
    (M = 0, mtop = 0, ftop = 0: the rule is horizontal transport, and the oracle of the horizontal fluxes alone agrees)"""
    dtype = np_of(eng)
    for su in (1, -1):
        for sv in (1, -1):
            c = case((2, 4, 5, 9), dtype, seed=7, names=("THL", "QT"))
            c["u"][...] = dtype(su) * (numpy.abs(c["u"]) + dtype(0.5))
            c["v"][...] = dtype(sv) * (numpy.abs(c["v"]) + dtype(0.5))
            want, cmax, mtop, ftop = Run(eng, c).check("signs %d %d" % (su, sv))
            assert (cmax > 0).all() and (mtop > 0).any() and (mtop < 0).any()
    for sign in (1, -1):
        c = lvr.column_winds(case((2, 4, 3, 9), dtype, seed=8, names=("THL", "QT")), sign)
        want, cmax, mtop, ftop = Run(eng, c).check("column sign %d" % sign)
        assert (mtop[:, 1, :, :] * sign > 0).all() and (mtop[:, 3, :, :] * sign < 0).all() and (mtop[:, 0, :, :] == 0).all()
        assert (ftop["THL"][:, 1] * sign > 0).all() and (ftop["THL"][:, 3] * sign < 0).all() and not ftop["THL"][:, 0].any()
    c = case((2, 3, 5, 9), dtype, seed=8, names=("THL", "QT"))
    c["u"][...] = (numpy.arange(9) - 4.0).astype(dtype)[None, None, None, :]
    c["v"][...] = dtype(3.0)
    want, cmax, mtop, ftop = Run(eng, c).check("uniform per level")
    assert not mtop.any() and not numpy.signbit(mtop).any() and not any(f.any() for f in ftop.values()) and (cmax > 0).all()
    nums = face_numbers(c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])
    for k, x in c["fields"].items():
        Fw, Fe, Fs, Fn, Fb, Ft = fluxes(x, nums)
        assert not Fb.any() and not Ft.any()
        assert_bits("horizontal transport alone: " + k, want[k], x - ((Fe - Fw) + (Fn - Fs)))
        assert (want[k] != x).any()
    c = case((2, 3, 5, 9), dtype, seed=8, names=("THL", "QT"))
    c["u"][...] = 0.0
    c["v"][...] = -0.0
    c["fields"]["QT"][...] = 0.0
    r = Run(eng, c)
    _, cmax, mtop, _ = r.check("zeros")
    assert not cmax.any() and not r.out["QT"].cpu().numpy().any()
    assert_bits("still air keeps THL", r.out["THL"].cpu().numpy(), c["fields"]["THL"])


def near(shape, cell):
    """the mask of ``cell`` (l, i, j, k) and its six neighbours (periodic in i and j, clamped in k)"""
    n, itot, jtot, ktot = shape
    l, i, j, k = cell
    mask = numpy.zeros(shape, dtype=bool)
    mask[l, i, j, max(k - 1, 0):k + 2] = True
    mask[l, (i - 1) % itot, j, k] = mask[l, (i + 1) % itot, j, k] = True
    mask[l, i, (j - 1) % jtot, k] = mask[l, i, (j + 1) % jtot, k] = True
    return mask


def special_case(dtype, ktot=7):
    """(clean case with fields that are not the winds, the same with NaN, +inf, -inf and -0.0 planted in one cell each of THL,
    the mask of the cells within one step of a planted value)"""
    c = case((3, 9, 9, ktot), dtype, seed=9, names=("THL", "QT"))
    s = dict(c, fields={k: x.copy() for k, x in c["fields"].items()})
    planted = {(0, 0, 0, 1): numpy.nan, (0, 4, 8, 2): numpy.inf, (1, 8, 3, 0): -numpy.inf, (1, 2, 6, ktot - 1): -0.0}
    mask = numpy.zeros(c["u"].shape, dtype=bool)
    for cell, val in planted.items():
        s["fields"]["THL"][cell] = val
        mask |= near(c["u"].shape, cell)
    return c, s, mask


def check_special(eng):
    """NaN, +-inf and -0.0 planted in single cells of a field: every output is the oracle's and the cells further than one
    step away hold the bits of a run without them.  A NaN in one wind cell u[l][i][j][k]: every cell outside the columns
    (i - 1 ... i + 1, j) at the levels >= k is bit-equal to the run without it, mtop is NaN there, and cmax stays finite"""
    dtype = np_of(eng)
    c, s, mask = special_case(dtype)
    clean, _, clean_mtop, clean_ftop = Run(eng, c).check("clean")
    r = Run(eng, s)
    want, cmax, _, ftop = r.check("special")
    assert_bits("the cells further away", r.out["THL"].cpu().numpy()[~mask], clean["THL"][~mask])
    assert_bits("QT never sees THL", r.out["QT"].cpu().numpy(), clean["QT"])
    assert_bits("QT's lid flux never sees THL", ftop["QT"], clean_ftop["QT"])
    assert numpy.isnan(want["THL"][0, 0, 0, :3]).all() and numpy.isnan(want["THL"][0, 1, 0, 1]) and numpy.isfinite(cmax).all()
    w = dict(c, u=c["u"].copy())
    w["u"][2, 0, 4, 3] = numpy.nan
    r = Run(eng, w)
    want, cmax, mtop, _ = r.check("NaN wind")
    mask = numpy.zeros(c["u"].shape, dtype=bool)
    for i in (8, 0, 1):
        mask[2, i, 4, 3:] = True
    for k in ("THL", "QT"):
        assert_bits("outside the NaN's columns, " + k, r.out[k].cpu().numpy()[~mask], clean[k][~mask])
    assert_bits("mtop outside the NaN's columns", mtop[~mask], clean_mtop[~mask])
    assert numpy.isnan(mtop[mask]).all() and numpy.isfinite(cmax).all() and not numpy.signbit(cmax).any()


def bad_calls(eng, t, o, u, v, hx, hy, g, r, m, ft):
    """the calls of ``Engine.les_transport`` that are refused, as callables: ``check_refusals`` makes them on a device,
    tests/test_engine_les_args_cpu.py on a stand-in that launches nothing, where it pins their texts"""
    many = {("F%d" % i): t["QT"].clone() for i in range(7)}
    other = torch.float64 if eng.dtype == torch.float32 else torch.float32
    V = eng.les_transport
    return [lambda: V({}, {}, u, v, hx, hy, g, r, cmax=False),
            lambda: V({}, {}, u, v, hx, hy, g, r, cmax=None, mtop=None),
            lambda: V({}, {}, u, v, hx, hy, g, r, ftop=ft[:0]),
            lambda: V(t, dict(o, QT=t["THL"]), u, v, hx, hy, g, r),
            lambda: V(t, dict(o, QT=u), u, v, hx, hy, g, r),
            lambda: V(t, dict(o, QT=o["THL"]), u, v, hx, hy, g, r),
            lambda: V(t, o, u, v, hx, hy, g, r, mtop=o["QT"]),
            lambda: V(t, o, u, v, hx, hy, g, r, mtop=u),
            lambda: V(t, o, u, v, hx, hy, g, r, mtop=m[:, :1]),
            lambda: V(t, o, u, v, hx, hy, g, r, ftop=ft[:3]),
            lambda: V(t, o, u, v, hx, hy, g, r, ftop=ft[:, :1]),
            lambda: V(t, o, u, v, hx, hy, g, r, ftop=ft.to(other)),
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
            lambda: V({"QT": lvr.elsewhere(eng, t["QT"])}, {"QT": o["QT"]}, u, v, hx, hy, g, r)]


def check_refusals(eng):
    """n = 0 is a no-op; nothing to do, a NULL required array, pitch_prof < ktot, an output that is an input or another output,
    a misaligned pointer, a field count outside 0 ... 6 and an extent below 1 are refused by the library and by the engine, and
    no refused call touches anything"""
    dtype = np_of(eng)
    c = case((2, 2, 3, 8), dtype, seed=11)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    for kw, text in ((dict(names=(), cmax=False, mtop=False), b"nothing to do"), (dict(names=(), cmax=False, mtop=False, ftop=True), b"nothing to do"),
                     (dict(null=("u",)), b"u is NULL"), (dict(null=("v",)), b"v is NULL"), (dict(null=("hx",)), b"hx is NULL"),
                     (dict(null=("hy",)), b"hy is NULL"), (dict(null=("g",)), b"g is NULL"), (dict(null=("r",)), b"r is NULL"),
                     (dict(extents={"pitch_prof": 7}), b"pitch_prof"), (dict(alias=((2, "u"),)), b"also an input"),
                     (dict(alias=((2, "QT"),)), b"also an input"), (dict(alias=((3, "THL"),)), b"also an input"),
                     (dict(alias=((2, "hy"),)), b"also an input"), (dict(alias=((2, "g"),)), b"also an input"), (dict(alias=((3, "r"),)), b"also an input"),
                     (dict(alias=((3, "cmax"),)), b"same array"), (dict(alias=((3, "mtop"),)), b"same array"), (dict(alias=((3, "out U"),)), b"same array"),
                     (dict(alias=((1, "ftop"),)), b"same array"),
                     (dict(alias=(("mtop", "v"),)), b"also an input"), (dict(alias=(("mtop", "THL"),)), b"also an input"),
                     (dict(alias=(("mtop", "out QT"),)), b"same array"), (dict(alias=(("cmax", "hx"),)), b"also an input"),
                     (dict(alias=(("cmax", "mtop"),)), b"same array"), (dict(alias=(("ftop", "u"),)), b"also an input"),
                     (dict(alias=(("ftop", "QT"),)), b"also an input"), (dict(alias=(("ftop", "r"),)), b"also an input"),
                     (dict(alias=(("ftop", "out THL"),)), b"same array"), (dict(alias=(("ftop", "mtop"),)), b"same array"),
                     (dict(alias=(("ftop", "cmax"),)), b"same array"),
                     (dict(extents={"n_fields": 7}), b"field count"), (dict(extents={"n_fields": -1}), b"field count"),
                     (dict(extents={"itot": 0}), b">= 1"), (dict(extents={"jtot": 0}), b">= 1"), (dict(extents={"ktot": -1}), b">= 1"),
                     (dict(extents={"n_les": -1}), b"< 0")):
        rc, got, cmax, mtop, ftop = raw_launch(eng, c, **kw)
        assert rc == E and text in eng.lib.spc_last_error(), (kw, rc, eng.lib.spc_last_error())
        assert all((v == OUT_FILL).all() for v in got.values()) and (cmax is None or (cmax == -5.0).all()), kw
        assert (mtop is None or (mtop == OUT_FILL).all()) and (ftop is None or (ftop == OUT_FILL).all()), kw
    rc, got, cmax, mtop, ftop = raw_launch(eng, c, extents={"n_les": 0})
    assert rc == 0 and all((v == OUT_FILL).all() for v in got.values()) and (cmax == -5.0).all() and (mtop == OUT_FILL).all() and (ftop == OUT_FILL).all()
    u, v, hx, hy, g, r = (dev(c[k]) for k in ("u", "v", "hx", "hy", "g", "r"))
    t = {"U": u, "V": v, "THL": dev(c["fields"]["THL"]), "QT": dev(c["fields"]["QT"])}
    o = {k: torch.full_like(x, OUT_FILL) for k, x in t.items()}
    m = torch.full_like(u, OUT_FILL)
    ft = torch.full((4,) + tuple(u.shape[:3]), OUT_FILL, dtype=u.dtype, device=u.device)
    # a view off the element grid: one byte into a buffer
    raw = torch.zeros(u.numel() * u.element_size() + 16, dtype=torch.uint8, device=u.device)
    skew = raw[1:1 + u.numel() * u.element_size()]
    a = _abi.LesTransportArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.pitch_prof = 2, 2, 3, 8, 1, 8
    a.u, a.v, a.hx, a.hy, a.g, a.r = (x.data_ptr() for x in (u, v, hx, hy, g, r))
    a.fields[0], a.out[0] = t["QT"].data_ptr(), skew.data_ptr()
    fn = eng.lib.spc_les_transport_f32 if eng.dtype == torch.float32 else eng.lib.spc_les_transport_f64
    assert fn(ctypes.byref(a), None) == E and b"not aligned" in eng.lib.spc_last_error() and not bool(raw.any())
    got = eng.les_transport({k: x[:0] for k, x in t.items()}, {k: x[:0] for k, x in o.items()}, u[:0], v[:0], hx[:0], hy[:0], g[:0], r[:0],
                            mtop=m[:0], ftop=ft[:, :0])
    assert tuple(got.shape) == (0,)
    for bad in bad_calls(eng, t, o, u, v, hx, hy, g, r, m, ft):
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
    assert bool((m == OUT_FILL).all()) and bool((ft == OUT_FILL).all())
    for k, x in c["fields"].items():
        assert_bits("refused: " + k, t[k].cpu().numpy(), x)


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle, cmax, mtop and ftop included"""
    from sp_coupler_amd.transfer import Sharded
    c = case((n, 3, 5, 40), np_of(one), seed=n)
    want, cmax, mtop, ftop = oracle(c)
    for tag, eng, up in on_both(one, multi, n):
        u, v = up(c["u"]), up(c["v"])
        t = {k: (u if x is c["u"] else v if x is c["v"] else up(x)) for k, x in c["fields"].items()}
        o = {k: up(numpy.full_like(x, OUT_FILL)) for k, x in c["fields"].items()}
        m = up(numpy.full_like(c["u"], OUT_FILL))
        lid = lambda w: torch.full((len(t),) + tuple(w.shape[:3]), OUT_FILL, dtype=w.dtype, device=w.device)          # noqa: E731
        ft = Sharded([lid(w) for w in u.parts], u.bounds) if tag == "multi" else lid(u)
        prof = [up(c[k]) for k in ("hx", "hy", "g", "r")]
        got = eng.les_transport(t, o, u, v, *prof, mtop=m, ftop=ft)
        multi.synchronize()
        for q, k in enumerate(NAMES):
            assert_bits("%s %s" % (tag, k), host_of(o[k]), want[k])
            lidk = numpy.concatenate([p[q].cpu().numpy() for p in ft.parts]) if tag == "multi" else ft[q].cpu().numpy()
            assert_bits("%s ftop %s" % (tag, k), lidk, ftop[k])
        assert_bits("%s cmax" % tag, host_of(got), cmax)
        assert_bits("%s mtop" % tag, host_of(m), mtop)
        probe = eng.les_transport({}, {}, u, v, *prof)
        multi.synchronize()
        assert_bits("%s probe" % tag, host_of(probe), cmax)
    return blocks_of(o["QT"], multi, n)


BODIES = ("parity", "rows", "tiles", "fields", "probe", "alignment", "signs", "special", "refusals")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in (1, 3, 64, 160)]),
            ("rows", lambda: [check_rows(eng, k) for k in (1, 65)]),
            ("tiles", lambda: check_tiles(eng)),
            ("fields", lambda: check_fields(eng)),
            ("probe", lambda: check_probe(eng)),
            ("alignment", lambda: [check_alignment(eng, lead) for lead in (1, 3)]),
            ("signs", lambda: check_signs(eng)),
            ("special", lambda: check_special(eng)),
            ("refusals", lambda: check_refusals(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_transport (CPU suite) ----------------------------------------------------------------------
class TransportOracleEngine(lbr.BuoyancyOracleEngine):
    """tests/les_buoyancy_ref.BuoyancyOracleEngine with ``les_transport`` by the NumPy oracle above: the outputs written whole
    into the caller's tensors, as the HIP engine does"""

    def les_transport(self, fields, out, u, v, hx, hy, g, r, cmax=True, mtop=None, ftop=None, **kw):
        want = cmax is not None and cmax is not False
        if sorted(fields) != sorted(out) or (not fields and not want and mtop is None) or (not fields and ftop is not None):
            raise ValueError("out does not match the fields, or nothing to do")
        if ftop is not None and tuple(ftop.shape) != (len(fields),) + tuple(u.shape[:3]):
            raise ValueError("ftop must be [fields x n x itot x jtot]")
        read = {t.data_ptr() for t in [u, v] + list(fields.values())}
        written = [t.data_ptr() for t in out.values()] + [t.data_ptr() for t in (mtop, ftop) if t is not None]
        if u.shape[0] and (len(set(written)) != len(written) or set(written) & read):
            raise ValueError("an output is an input or another output")
        res, c, m, lid = les_transport({k: t.numpy() for k, t in fields.items()}, u.numpy(), v.numpy(), hx.numpy(), hy.numpy(),
                                       numpy.ascontiguousarray(g.numpy()), numpy.ascontiguousarray(r.numpy()))
        for k, t in out.items():
            t.copy_(torch.from_numpy(res[k]))
        if mtop is not None:
            mtop.copy_(torch.from_numpy(m))
        if ftop is not None:
            for q, k in enumerate(fields):
                ftop[q].copy_(torch.from_numpy(lid[k]))
        if not want:
            return None
        c = torch.from_numpy(c)
        return c if cmax is True else cmax.copy_(c)


# -- the host twins of DeviceLESEnsemble after enable_advection(vertical=True, conservative=True) --------------------------------
class _HostTransport:
    """NumPy fields: the executable definition of what the advection of evolve_model_batched does in the conservative mode:
    with enable_buoyancy() QL, the slab means and K21's profiles of the stepped fields; K22's probe with the coefficients of
    the whole step; the substeps of the probe (or of the gravity wave, whichever are more); per substep K21 where enabled, then
    K22 on the fields that exist; the lid flux summed elementwise in substep order"""

    advect_conservative = False
    _lid = None

    def enable_advection(self, dx=None, dy=None, cfl=None, max_substeps=None, vertical=False, conservative=False):
        if conservative and not vertical:
            raise ValueError("the conservative transport (K22) needs vertical=True")
        super().enable_advection(dx=dx, dy=dy, cfl=cfl, max_substeps=max_substeps, vertical=vertical)
        self.advect_conservative = bool(conservative)

    def _advect(self, dt):
        if not self.advect_conservative:
            return super()._advect(dt)
        f, p, par = self.fields3d, self.p, self.advect_par
        T = f["U"].dtype
        buoyant = self.buoyancy_wave_speed is not None
        if buoyant:
            if self.THERMO:
                self._stale = True
                self._ensure_ql()
            elif "QL" in f or ("QT" in f and "Qsat" in f):
                f["QL"] = numpy.maximum(f["QT"] - f["Qsat"], 0.0)
            self._slab_means()
            ql = f.get("QL")
            t0, lex, s = (a.astype(T) for a in buo.profiles(p["THL"], p["QT"], p["QL"] if ql is not None else None, p["presf"], self.zh_cache,
                                                            zf=self.zf_cache))
        g, r = (a.astype(T) for a in adv.vertical_profiles(self.water_path_weights()))
        hx, hy = (a.astype(T) for a in adv.coefficients(dt, par["dx"], par["dy"], n=self.n))
        c = float(face_numbers(f["U"], f["V"], hx, hy, g, r)["s"].max())
        n_sub = adv.substeps(c, par["cfl"], par["max_substeps"])
        if buoyant:
            n_wave = buo.wave_substeps(dt, par["dx"], par["dy"], par["cfl"], self.buoyancy_wave_speed)
            if n_wave > par["max_substeps"]:
                raise RuntimeError("the pressure force (K21) needs %d substeps" % n_wave)
            n_sub = max(n_sub, n_wave)
        hx, hy = (a.astype(T) for a in adv.coefficients(dt / n_sub, par["dx"], par["dy"], n=self.n))
        worst = worst_b = 0.0
        total = None
        for _ in range(n_sub):
            if buoyant:
                self._phi, _, f["U"], f["V"], amax = lbr.les_buoyancy(f["THL"], f["QT"], ql, f["U"], f["V"], hx, hy, t0, lex, s)
                worst_b = max(worst_b, float(amax.max()))
            new, cmax, self._mtop, lid = les_transport({k: f[k] for k in self.KEYS if k in f}, f["U"], f["V"], hx, hy, g, r)
            f.update(new)
            worst = max(worst, float(cmax.max()))
            total = {k: a.copy() for k, a in lid.items()} if total is None else {k: total[k] + lid[k] for k in lid}
        self.advect_substeps, self.advect_courant, self.advect_courant_z, self._mtop_dt = n_sub, worst, None, dt / n_sub
        self._lid = total
        if buoyant:
            self.buoyancy_wind_change = worst_b

    def get_lid_flux_batched(self):
        return self._lid


class HostTransportLESEnsemble(_HostTransport, lbr.HostBuoyancyLESEnsemble):
    """without enable_thermo()"""


class HostThermoTransportLESEnsemble(_HostTransport, lbr.HostThermoBuoyancyLESEnsemble):
    """after enable_thermo()"""


VARIANTS = {"plain": dict(), "buoyancy": dict(buoyancy=True),
            "all": dict(diffuse=True, radiate=True, thermo=True, micro=True), "all buoyant": dict(diffuse=True, radiate=True, thermo=True, micro=True, buoyancy=True)}
DX = lvr.DX


def ensemble_run(engine, n, device, conservative=True, buoyancy=False, thermo=False, micro=False, diffuse=False, radiate=False, itot=4, jtot=5,
                 nL=20, steps=3):
    """tests/les_buoyancy_ref.ensemble_run with enable_advection(vertical=True, conservative=...): after every step every
    profile, the fields, the substeps, the Courant sum, the lid flux of every transported field, and (with buoyancy) phi and
    the largest wind change.  Returns (ens, list of records)"""
    keys = ("U", "V", "THL", "QT") + (("QR",) if micro else ())

    def record(ens, rec):
        lar.record_substeps(ens, rec, z=True)
        if conservative:
            record_lid(ens, rec, keys)
        if buoyancy:
            lbr.record_pressure(ens, rec)

    def before(ens):
        assert ens.get_vertical_wind_batched() is None and (not conservative or ens.get_lid_flux_batched() is None)
    # (``conservative`` None: the call as it was before K22)
    return ensemble_case(engine, n, models.DeviceLESEnsemble if device else (HostThermoTransportLESEnsemble if thermo else HostTransportLESEnsemble),
                         thermo=thermo, micro=micro, diffuse=diffuse, edit=lvr.raise_u,
                         advection=dict(dx=DX, dy=1.5 * DX, vertical=True, **({} if conservative is None else {"conservative": conservative})),
                         radiation=lrr.radiation_of(n, "f0", "f1") if radiate else None, enable=lambda ens: buoyancy and ens.enable_buoyancy(),
                         record=record, before=before, itot=itot, jtot=jtot, nL=nL, steps=steps)


def record_lid(ens, rec, keys):
    """the lid flux of every transported field (zeros before the first step) into a record of ensemble_case"""
    lid = ens.get_lid_flux_batched()
    assert lid is None or tuple(lid) == keys
    for k in keys:
        rec["lid " + k] = numpy.zeros(rec["field U"].shape[:3]) if lid is None else numpy.array(host_of(lid[k]))


def check_ensemble(one, engines, n, variant):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``: every profile, field and lid flux
    bit-equal after each step, W within a few roundings; the conservative step is not the split one (THL of the twin's first
    step differs from the run with conservative=False), and that run on the device is bit-equal to the run of
    enable_advection(vertical=True) without the argument.  Returns the twin's substeps of the three steps"""
    kw = VARIANTS[variant]
    twin, host = ensemble_run(one, n, False, **kw)
    split_log = ensemble_run(one, n, False, conservative=False, **kw)[1]
    assert (host[1]["field THL"] != split_log[1]["field THL"]).any() and host[1]["courant z"][0] == -1.0 and split_log[1]["courant z"][0] > 0
    assert 0 < host[1]["courant"][0] <= 0.5 and all(numpy.isfinite(r["courant"][0]) for r in host)
    assert all(host[1]["lid " + k].any() for k in ("U", "THL", "QT"))
    for engine in engines:
        ens, log = ensemble_run(engine, n, True, **kw)
        lmr.same_logs(host, log)
        lvr.check_w(ens, twin)
    lmr.same_logs(split_log, ensemble_run(engines[0], n, True, conservative=False, **kw)[1])
    old = ensemble_run(engines[0], n, True, conservative=None, **kw)[1]
    lmr.same_logs(split_log, old)
    return [int(host[q]["substeps"][0]) for q in (1, 2, 4)]         # (record 0: the start; record 3: after the nudge)
