"""NumPy oracle of K16 (include/spc.h: spc_les_advect_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_advect_gpu.py (each takes an engine: tools/mutation_control.py --advect hands them the engines of its mutant
libraries), the host twins of models.DeviceLESEnsemble's advection mode and an oracle-backed engine with ``les_advect`` for the
CPU suite.

The oracle spells the rule out one operation per NumPy call in the element type, the neighbours by numpy.roll, so nothing
fuses.  Every device array of the bodies is the LEADING part of a poisoned buffer (tests/les_harness.Poisoned); the bytes
behind it (and in front of a view off the 16-byte grid) are checked after the launch, the inputs against what was uploaded."""

import numpy
import torch

from sp_coupler_amd import _abi, models
from sp_coupler_amd import advection as adv
from tests import les_diffuse_ref as ldr
from tests import les_micro_ref as lmr
from tests import les_thermo_ref as ltr
from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, ensemble_case, host_of, np_of, on_both, run_bodies)

#: a cell that is its own four neighbours (1 x 1), one extent of 1 either way, both neighbours the same cell (2 x 2, 2 x 3),
#: itot < jtot (3 x 5), exactly one workgroup's rows (8 x 8), one row more than that (9 x 9)
PLANES = [(1, 1), (1, 5), (5, 1), (2, 2), (2, 3), (3, 5), (8, 8), (9, 9)]
KTOTS = [1, 2, 3, 63, 64, 65, 160, 161]
NS = [1, 2, 5]
NAMES = ("U", "V", "THL", "QT")
ALL_NAMES = ("U", "V", "THL", "QT", "QR", "QL")


# -- the rule --------------------------------------------------------------------------------------------------------------
def faces(u, v, hx, hy):
    """(pw, pe, ps, pn, s) of winds [n x itot x jtot x ktot] of dtype T and hx, hy [n] of the same T"""
    T = u.dtype
    assert v.dtype == T and hx.dtype == T and hy.dtype == T
    zero = T.type(0)
    bx, by = hx[:, None, None, None], hy[:, None, None, None]
    with numpy.errstate(all="ignore"):
        aw = numpy.roll(u, 1, axis=1) + u
        ae = u + numpy.roll(u, -1, axis=1)
        as_ = numpy.roll(v, 1, axis=2) + v
        an = v + numpy.roll(v, -1, axis=2)
        cw, ce, cs, cn = aw * bx, ae * bx, as_ * by, an * by
        pw = numpy.where(cw > 0, cw, zero)
        pe = numpy.where(ce < 0, -ce, zero)
        ps = numpy.where(cs > 0, cs, zero)
        pn = numpy.where(cn < 0, -cn, zero)
        s = pw + pe
        s = s + ps
        s = s + pn
    assert all(a.dtype == T for a in (pw, pe, ps, pn, s))
    return pw, pe, ps, pn, s


def les_advect(fields, u, v, hx, hy):
    """(dict name -> the new field (a new array), cmax [n]): fields, u, v [n x itot x jtot x ktot] of dtype T, hx, hy [n]"""
    pw, pe, ps, pn, s = faces(u, v, hx, hy)
    n = u.shape[0]
    cmax = s.reshape(n, -1).max(axis=1) if n else numpy.zeros(0, dtype=u.dtype)
    out = {}
    with numpy.errstate(all="ignore"):
        for k, x in fields.items():
            assert x.dtype == u.dtype and x.shape == u.shape
            t = numpy.roll(x, 1, axis=1) - x
            t = pw * t
            r = x + t
            t = numpy.roll(x, -1, axis=1) - x
            t = pe * t
            r = r + t
            t = numpy.roll(x, 1, axis=2) - x
            t = ps * t
            r = r + t
            t = numpy.roll(x, -1, axis=2) - x
            t = pn * t
            r = r + t
            assert r.dtype == x.dtype
            out[k] = r
    return out, cmax


# -- inputs ------------------------------------------------------------------------------------------------------------------
def field_like(name, shape, dtype, rng):
    z = numpy.arange(shape[-1]) / 160.0
    if name in ("QT", "QR", "QL"):
        return (8e-3 * numpy.exp(-z) + 1e-3 * rng.random(shape)).astype(dtype)
    if name == "THL":
        return (290.0 + 10.0 * z + 0.5 * rng.standard_normal(shape)).astype(dtype)
    return (4.0 * rng.standard_normal(shape)).astype(dtype)


def winds(shape, dtype, rng):
    """u and v of both signs (the upwind side flips from face to face), with cells that are exactly zero and faces whose two
    winds cancel exactly (a face Courant number of +0: closed on both sides)"""
    u, v = field_like("U", shape, dtype, rng), field_like("V", shape, dtype, rng)
    n, itot, jtot, ktot = shape
    u[:, :, :, ::7] = numpy.where(rng.random(u[:, :, :, ::7].shape) < 0.3, 0.0, u[:, :, :, ::7])
    if itot > 1:
        u[:, 1, :, ::3] = -u[:, 0, :, ::3]
    if jtot > 1:
        v[:, :, jtot - 1, ::2] = -v[:, :, 0, ::2]                 # the face across the wrap
    return u, v


def case(shape, dtype, seed=0, dt=6.0, names=NAMES):
    """dict of the arguments: u, v, fields (dict name -> array; "U" and "V" are the winds THEMSELVES), hx, hy [n], each LES with
    another dx and another dy (hx != hy everywhere): Courant sums of a few tenths, some above 1"""
    dtype = numpy.dtype(dtype).type
    n, itot, jtot, ktot = shape
    rng = numpy.random.default_rng(7000 + seed + 7 * ktot + 13 * itot + jtot + 31 * n)
    u, v = winds(shape, dtype, rng)
    fields = {k: (u if k == "U" else v if k == "V" else field_like(k, shape, dtype, rng)) for k in names}
    hx, hy = adv.coefficients(dt, 150.0 + 40.0 * numpy.arange(n), 260.0 - 30.0 * numpy.arange(n) % 100)
    return dict(u=u, v=v, fields=fields, hx=hx.astype(dtype), hy=hy.astype(dtype))


def oracle(c):
    return les_advect(c["fields"], c["u"], c["v"], c["hx"], c["hy"])


# -- device plumbing ---------------------------------------------------------------------------------------------------------
OUT_FILL = 777.0                                                   # what an output holds before the launch


class Run:
    """one launch through ``eng.les_advect`` with every array inside a poisoned buffer; ``check`` compares the outputs and cmax
    with the oracle bit for bit, the inputs with what was uploaded, and looks at the bytes around every array"""

    def __init__(self, eng, c, lead=0, cmax=True):
        self.eng, self.c = eng, c
        self.mem = Poisoned(eng)
        put = lambda tag, a, poison: self.mem.put(tag, a, poison, lead)                    # noqa: E731
        self.du, self.dv = put("u", c["u"], float("nan")), put("v", c["v"], float("nan"))
        self.dev = {k: (self.du if x is c["u"] else self.dv if x is c["v"] else put(k, x, float("nan"))) for k, x in c["fields"].items()}
        self.out = {k: put("out " + k, numpy.full_like(x, OUT_FILL), 1e30) for k, x in c["fields"].items()}
        self.dhx, self.dhy = put("hx", c["hx"], 1e30), put("hy", c["hy"], 1e30)
        self.dcmax = put("cmax", numpy.full_like(c["hx"], -5.0), 1e30) if cmax else None
        self.got = eng.les_advect(self.dev, self.out, self.du, self.dv, self.dhx, self.dhy, cmax=self.dcmax if cmax else False)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def check(self, what=""):
        c = self.c
        want, cmax = oracle(c)
        for k in c["fields"]:
            assert_bits("%s out %s" % (what, k), self.out[k].cpu().numpy(), want[k])
        if self.dcmax is None:
            assert self.got is None
        else:
            assert self.got is self.dcmax
            assert_bits("%s cmax" % what, self.dcmax.cpu().numpy(), cmax)
        for tag, t, a in [("u", self.du, c["u"]), ("v", self.dv, c["v"]), ("hx", self.dhx, c["hx"]), ("hy", self.dhy, c["hy"])] + \
                [(k, self.dev[k], x) for k, x in c["fields"].items()]:
            assert Poisoned.read_only(t, a), (what, tag, "read only")
        self.mem.check_around(what)
        return want, cmax


def raw_launch(eng, c, names=None, cmax=True, alias=None, extents=None):
    """spc_les_advect_* itself: (rc, dict name -> host output, host cmax or None).  ``alias``: (slot, key) pairs that replace
    out[slot] by the pointer of tensor ``key`` ("u", "v", "hx", "hy", "cmax", a field name, or "out <name>"); ``extents``:
    overrides of n_les, itot, jtot, ktot"""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    names = list(c["fields"]) if names is None else list(names)
    n, itot, jtot, ktot = c["u"].shape
    t = {"u": dev(c["u"]), "v": dev(c["v"]), "hx": dev(c["hx"]), "hy": dev(c["hy"]), "cmax": dev(numpy.full_like(c["hx"], -5.0))}
    for k in names:
        x = c["fields"][k]
        t[k] = t["u"] if x is c["u"] else t["v"] if x is c["v"] else dev(x)
        t["out " + k] = dev(numpy.full_like(x, OUT_FILL))
    g = _abi.LesAdvectArgs()
    g.n_les, g.itot, g.jtot, g.ktot, g.n_fields = n, itot, jtot, ktot, len(names)
    for key, val in (extents or {}).items():
        setattr(g, key, val)
    g.u, g.v, g.hx, g.hy = (t[k].data_ptr() for k in ("u", "v", "hx", "hy"))
    if cmax:
        g.cmax = t["cmax"].data_ptr()
    for f, k in enumerate(names):
        g.fields[f], g.out[f] = t[k].data_ptr(), t["out " + k].data_ptr()
    for slot, key in (alias or ()):
        g.out[slot] = t[key].data_ptr()
    rc = abi_call(eng, "spc_les_advect", g)
    return rc, {k: t["out " + k].cpu().numpy() for k in names}, t["cmax"].cpu().numpy() if cmax else None


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, n=3):
    """U, V (the winds themselves), THL and QT against the oracle, cmax included; the answer is not the input where a cell has
    another cell as its neighbour"""
    c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
    want, cmax = Run(eng, c).check("n %d plane %s ktot %d" % (n, plane, ktot))
    assert (cmax >= 0).all() and not numpy.signbit(cmax).any()
    if min(plane) > 2 or (max(plane) > 2 and ktot > 1):          # (every face of level 0 of a plane of 2 cancels: winds())
        assert (cmax > 0).all() and all((want[k] != c["fields"][k]).any() for k in NAMES)


def check_rows(eng, ktot):
    """n = 1, 2, 5 at 3 x 5: hx and hy differ per LES and from each other, so a wrong l or a swapped coefficient shows"""
    for n in NS:
        c = case((n, 3, 5, ktot), np_of(eng), seed=1)
        assert (c["hx"] != c["hy"]).all() and (n == 1 or c["hx"][0] != c["hx"][1])
        Run(eng, c).check("rows n %d ktot %d" % (n, ktot))


MANY = 1100                                                       # LES of one column that make a launch of many workgroups


def strip_shapes(strip, rows, many_rows):
    """(n, itot, jtot, ktot) whose run jtot * ktot stands on q * strip - 1, + 0, + 1 (q = 1, 2) at ktot 1 and at a ktot that does
    not divide the strip, and whose itot stands on q * rows - 1, + 0, + 1, for the rows of a launch of few workgroups and
    (n = MANY) of many"""
    out = []
    for q in (1, 2):
        for d in (-1, 0, 1):
            out.append((2, 3, q * strip + d, 1))
            out.append((2, q * rows + d, 5, 3))
            out.append((MANY, q * many_rows + d, 1, 1))
    out += [(2, 2, (strip - 1) // 3, 3), (2, 2, (strip + 2) // 3, 3), (2, 2, (2 * strip + 2) // 3, 3), (2, 2, 3, strip - 1), (2, 2, 3, strip),
            (2, 2, 3, strip + 1), (MANY, 2 * many_rows + 1, 2, 3)]
    return out


def check_strips(eng):
    """every boundary of the workgroups: the flat run of a row at the strip - 1, + 0, + 1 (the j neighbours of a cell lie in
    another workgroup or across the wrap), the rows at spc_les_advect_rows - 1, + 0, + 1 (and twice that) for a launch of few
    workgroups and for one of many, which walks more rows (asserted for every shape)"""
    strip, rows = eng.advect_strip(2, 8, 8, 160)
    many_rows = eng.advect_strip(MANY, 64, 1, 1)[1]
    assert strip >= 64 and 1 <= rows < many_rows
    for n, itot, jtot, ktot in strip_shapes(strip, rows, many_rows):
        assert eng.advect_strip(n, itot, jtot, ktot) == (strip, many_rows if n == MANY else rows)
        Run(eng, case((n, itot, jtot, ktot), np_of(eng), seed=2, names=("U", "QT"))).check("strip %d x %d x %d x %d" % (n, itot, jtot, ktot))
    return strip, rows, many_rows


def check_fields(eng):
    """1 to 6 fields with U and V among them, 1 to 6 without, and without cmax"""
    dtype = np_of(eng)
    for nf in range(1, 7):
        Run(eng, case((2, 3, 5, 65), dtype, seed=3, names=ALL_NAMES[:nf])).check("%d fields with the winds" % nf)
        c = case((2, 3, 5, 65), dtype, seed=4, names=ALL_NAMES[:nf])
        rng = numpy.random.default_rng(nf)
        c["fields"] = {("F%d" % i): field_like(k, c["u"].shape, dtype, rng) for i, k in enumerate(ALL_NAMES[:nf])}      # none is u or v
        Run(eng, c).check("%d fields without the winds" % nf)
    Run(eng, case((2, 3, 5, 9), dtype, seed=5), cmax=False).check("no cmax")
    rc, got, cmax = raw_launch(eng, case((2, 3, 5, 9), dtype, seed=5))
    want = oracle(case((2, 3, 5, 9), dtype, seed=5))
    assert rc == 0
    for k in NAMES:
        assert_bits("raw %s" % k, got[k], want[0][k])
    assert_bits("raw cmax", cmax, want[1])


def check_probe(eng):
    """n_fields == 0 with cmax: the Courant sums of the winds alone, bit-equal to those of a full launch and to the oracle's;
    a wind that blows north only (pn alone carries the sum)"""
    dtype = np_of(eng)
    for shape in ((1, 1, 1, 1), (2, 3, 5, 64), (5, 9, 9, 161)):
        c = case(shape, dtype, seed=6)
        want = oracle(c)[1]
        full = Run(eng, c)
        full.check("full %s" % (shape,))
        probe = Run(eng, dict(c, fields={}))
        probe.check("probe %s" % (shape,))
        assert_bits("probe == full", probe.dcmax.cpu().numpy(), full.dcmax.cpu().numpy())
        assert_bits("probe == oracle", probe.dcmax.cpu().numpy(), want)
    c = case((2, 3, 5, 7), dtype, seed=7)
    c["u"][...] = 0.0
    c["v"][...] = -numpy.abs(c["v"]) - dtype(1.0)
    cmax = Run(eng, dict(c, fields={})).check("north only")[1]
    assert (cmax > 0).all()


def check_alignment(eng, lead, ktot=65):
    """views one (or more) elements off the 16-byte grid"""
    Run(eng, case((3, 3, 5, ktot), np_of(eng), seed=10 + lead), lead=lead).check("lead %d ktot %d" % (lead, ktot))


def check_signs(eng):
    """winds of one sign each way (the upwind side is the same at every face), all four combinations, and no wind at all: the
    fields keep their bits and cmax is +0"""
    dtype = np_of(eng)
    for su in (1, -1):
        for sv in (1, -1):
            c = case((2, 3, 5, 9), dtype, seed=8, names=("THL", "QT"))
            c["u"][...] = su * (numpy.abs(c["u"]) + dtype(0.5))
            c["v"][...] = sv * (numpy.abs(c["v"]) + dtype(0.5))
            want, _ = Run(eng, c).check("signs %d %d" % (su, sv))
            assert (want["THL"] != c["fields"]["THL"]).any()
    c = case((2, 3, 5, 9), dtype, seed=8, names=("THL", "QT"))
    c["u"][...] = 0.0
    c["v"][...] = -0.0
    r = Run(eng, c)
    _, cmax = r.check("no wind")
    assert not cmax.any() and not numpy.signbit(cmax).any()
    for k, x in c["fields"].items():
        assert_bits("no wind keeps " + k, r.out[k].cpu().numpy(), x)


def near(shape, cell):
    """mask [n x itot x jtot x ktot]: the cell (l, i, j, k) and its four periodic neighbours in the plane"""
    m = numpy.zeros(shape, dtype=bool)
    l, i, j, k = cell
    for di, dj in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
        m[l, (i + di) % shape[1], (j + dj) % shape[2], k] = True
    return m


def special_case(dtype, ktot=7):
    """(clean case with fields that are not the winds, the same with NaN, +inf, -inf and -0.0 planted in one cell each of THL
    and a NaN in one cell of u, the mask of the cells within one step of a planted value)"""
    c = case((3, 9, 9, ktot), dtype, seed=9, names=("THL", "QT"))
    s = dict(c, u=c["u"].copy(), fields={k: x.copy() for k, x in c["fields"].items()})
    planted = {(0, 0, 0, 1): numpy.nan, (0, 4, 8, 2): numpy.inf, (1, 8, 3, 0): -numpy.inf, (1, 2, 6, ktot - 1): -0.0}
    mask = numpy.zeros(c["u"].shape, dtype=bool)
    for cell, val in planted.items():
        s["fields"]["THL"][cell] = val
        mask |= near(mask.shape, cell)
    s["u"][2, 0, 4, 3] = numpy.nan
    mask |= near(mask.shape, (2, 0, 4, 3))
    return c, s, mask


def check_special(eng):
    """NaN, +-inf and -0.0 planted in single cells of a field and a NaN in one wind cell: every output is the oracle's, the cells
    further than one step away hold the bits of a run without them (QT feels only the NaN wind); a constant field keeps its
    bits and a -0.0 constant comes out +0.0"""
    dtype = np_of(eng)
    c, s, mask = special_case(dtype)
    clean, clean_cmax = Run(eng, c).check("clean")
    r = Run(eng, s)
    want, cmax = r.check("special")
    for k in ("THL", "QT"):
        got = r.out[k].cpu().numpy()
        assert_bits("the cells further away, " + k, got[~mask], clean[k][~mask])
    assert numpy.isnan(want["THL"][near(mask.shape, (0, 0, 0, 1))]).any() and numpy.isfinite(cmax).all()
    assert not numpy.isnan(want["QT"]).any()                      # a NaN wind closes its faces: no field takes it
    k = case((2, 3, 5, 9), dtype, seed=10, names=("THL", "QT", "QR"))
    k["fields"]["THL"][...] = dtype(287.3)
    k["fields"]["QT"][...] = dtype(-1e-3)
    k["fields"]["QR"][...] = -0.0
    r = Run(eng, k)
    r.check("constants")
    for name in ("THL", "QT"):
        assert_bits("a constant keeps its bits: " + name, r.out[name].cpu().numpy(), k["fields"][name])
    qr = r.out["QR"].cpu().numpy()
    assert not qr.any() and not numpy.signbit(qr).any()


def elsewhere(eng, t):
    """``t`` on another device than the engine's: the host for an engine on a GPU, the meta device for a stand-in on the host"""
    return t.cpu() if eng.device.type == "cuda" else t.to("meta")


def bad_calls(eng, t, o, u, v, hx, hy):
    """the calls of ``Engine.les_advect`` that are refused, as callables: ``check_refusals`` makes them on a device,
    tests/test_engine_les_args_cpu.py on a stand-in that launches nothing, where it pins their texts"""
    many = {("F%d" % i): t["QT"].clone() for i in range(7)}
    other = torch.float64 if eng.dtype == torch.float32 else torch.float32
    return [lambda: eng.les_advect({}, {}, u, v, hx, hy, cmax=False),
            lambda: eng.les_advect({}, {}, u, v, hx, hy, cmax=None),
            lambda: eng.les_advect(t, dict(o, QT=t["THL"]), u, v, hx, hy),
            lambda: eng.les_advect(t, dict(o, QT=u), u, v, hx, hy),
            lambda: eng.les_advect(t, dict(o, QT=o["THL"]), u, v, hx, hy),
            lambda: eng.les_advect({"QT": t["QT"]}, {"QT": hx.view(2, 1, 1, 1).expand(2, 2, 3, 8)}, u, v, hx, hy),
            lambda: eng.les_advect(t, {k: x for k, x in o.items() if k != "QT"}, u, v, hx, hy),
            lambda: eng.les_advect(many, {k: torch.empty_like(x) for k, x in many.items()}, u, v, hx, hy),
            lambda: eng.les_advect(t, o, u, v[:, :1], hx, hy),
            lambda: eng.les_advect(t, o, u, v, hx[:1], hy),
            lambda: eng.les_advect(t, o, u, v, hx, hy, cmax=hx),
            lambda: eng.les_advect(t, o, u, v, hx, hy, cmax=torch.empty(3, dtype=eng.dtype, device=eng.device)),
            lambda: eng.les_advect({"QT": t["QT"][..., ::2]}, {"QT": o["QT"][..., ::2]}, u, v, hx, hy),
            lambda: eng.les_advect({"QT": t["QT"].to(other)}, {"QT": o["QT"]}, u, v, hx, hy),
            lambda: eng.les_advect({"QT": elsewhere(eng, t["QT"])}, {"QT": o["QT"]}, u, v, hx, hy)]


def check_refusals(eng):
    """n = 0 is a no-op; no field without cmax, an output that is an input, cmax or another output and an extent below 1 are
    refused by the library and by the engine, and no refused call touches anything"""
    dtype = np_of(eng)
    c = case((2, 2, 3, 8), dtype, seed=11)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    for kw, text in ((dict(names=(), cmax=False), b"nothing to do"), (dict(alias=((2, "u"),)), b"also an input"),
                     (dict(alias=((2, "QT"),)), b"also an input"), (dict(alias=((3, "THL"),)), b"also an input"),
                     (dict(alias=((2, "hy"),)), b"also an input"), (dict(alias=((3, "cmax"),)), b"also an input"),
                     (dict(alias=((3, "out U"),)), b"same array"), (dict(extents={"itot": 0}), b">= 1"),
                     (dict(extents={"jtot": 0}), b">= 1"), (dict(extents={"ktot": -1}), b">= 1"), (dict(extents={"n_les": -1}), b"< 0")):
        rc, got, cmax = raw_launch(eng, c, **kw)
        assert rc == E and text in eng.lib.spc_last_error(), (kw, rc, eng.lib.spc_last_error())
        assert all((v == OUT_FILL).all() for v in got.values()) and (cmax is None or (cmax == -5.0).all()), kw
    rc, got, cmax = raw_launch(eng, c, extents={"n_les": 0})
    assert rc == 0 and all((v == OUT_FILL).all() for v in got.values()) and (cmax == -5.0).all()
    u, v, hx, hy = dev(c["u"]), dev(c["v"]), dev(c["hx"]), dev(c["hy"])
    t = {"U": u, "V": v, "THL": dev(c["fields"]["THL"]), "QT": dev(c["fields"]["QT"])}
    o = {k: torch.full_like(x, OUT_FILL) for k, x in t.items()}
    got = eng.les_advect({k: x[:0] for k, x in t.items()}, {k: x[:0] for k, x in o.items()}, u[:0], v[:0], hx[:0], hy[:0])
    assert tuple(got.shape) == (0,)
    for bad in bad_calls(eng, t, o, u, v, hx, hy):
        try:
            bad()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad call was not refused")
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    for k, x in o.items():
        assert bool((x == OUT_FILL).all()), k
    for k, x in c["fields"].items():
        assert_bits("refused: " + k, t[k].cpu().numpy(), x)


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle, cmax included"""
    c = case((n, 3, 5, 40), np_of(one), seed=n)
    want, cmax = oracle(c)
    for tag, eng, up in on_both(one, multi, n):
        u, v = up(c["u"]), up(c["v"])
        t = {k: (u if x is c["u"] else v if x is c["v"] else up(x)) for k, x in c["fields"].items()}
        o = {k: up(numpy.full_like(x, OUT_FILL)) for k, x in c["fields"].items()}
        got = eng.les_advect(t, o, u, v, up(c["hx"]), up(c["hy"]))
        multi.synchronize()
        for k in NAMES:
            assert_bits("%s %s" % (tag, k), host_of(o[k]), want[k])
        assert_bits("%s cmax" % tag, host_of(got), cmax)
        probe = eng.les_advect({}, {}, u, v, up(c["hx"]), up(c["hy"]))
        multi.synchronize()
        assert_bits("%s probe" % tag, host_of(probe), cmax)
    return blocks_of(o["QT"], multi, n)


BODIES = ("parity", "rows", "strips", "fields", "probe", "alignment", "signs", "special", "refusals")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in (1, 3, 64, 161)]),
            ("rows", lambda: [check_rows(eng, k) for k in (1, 65)]),
            ("strips", lambda: check_strips(eng)),
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


# -- an oracle-backed engine with les_advect (CPU suite) -------------------------------------------------------------------------
class AdvectOracleEngine(ldr.DiffuseOracleEngine):
    """tests/les_diffuse_ref.DiffuseOracleEngine with ``les_advect`` by the NumPy oracle above: the outputs written whole into
    the caller's tensors, as the HIP engine does"""

    def les_advect(self, fields, out, u, v, hx, hy, cmax=True, **kw):
        want = cmax is not None and cmax is not False
        if sorted(fields) != sorted(out) or (not fields and not want):
            raise ValueError("out does not match the fields, or nothing to do")
        read = {t.data_ptr() for t in [u, v] + list(fields.values())}
        written = [t.data_ptr() for t in out.values()]
        if u.shape[0] and (len(set(written)) != len(written) or set(written) & read):
            raise ValueError("an output is an input or another output")
        r, c = les_advect({k: t.numpy() for k, t in fields.items()}, u.numpy(), v.numpy(), hx.numpy(), hy.numpy())
        for k, t in out.items():
            t.copy_(torch.from_numpy(r[k]))
        if not want:
            return None
        c = torch.from_numpy(c)
        return c if cmax is True else cmax.copy_(c)


# -- the host twins of models.DeviceLESEnsemble after enable_advection() -------------------------------------------------------
class _HostAdvect:
    """NumPy fields: the executable definition of what evolve_model_batched does after enable_advection(): plain, with
    enable_diffusion(), with enable_thermo() (THERMO) and with enable_microphysics() on top of either"""

    advect_par = None
    advect_substeps = advect_courant = None
    KEYS = ("U", "V", "THL", "QT", "QR")

    def enable_advection(self, dx=None, dy=None, cfl=None, max_substeps=None):
        if "U" not in self.fields3d or "V" not in self.fields3d:
            raise ValueError("the advection (K16) needs the fields U and V")
        self.advect_par = {"dx": adv.DX if dx is None else dx, "dy": adv.DY if dy is None else dy, "cfl": adv.CFL if cfl is None else cfl,
                           "max_substeps": adv.MAX_SUBSTEPS if max_substeps is None else max_substeps}

    def _advect(self, dt):
        f, par = self.fields3d, self.advect_par
        T = f["U"].dtype
        hx, hy = (a.astype(T) for a in adv.coefficients(dt, par["dx"], par["dy"], n=self.n))
        c = float(faces(f["U"], f["V"], hx, hy)[4].max())
        n_sub = adv.substeps(c, par["cfl"], par["max_substeps"])
        hx, hy = (a.astype(T) for a in adv.coefficients(dt / n_sub, par["dx"], par["dy"], n=self.n))
        worst = 0.0
        for _ in range(n_sub):
            new, cmax = les_advect({k: f[k] for k in self.KEYS if k in f}, f["U"], f["V"], hx, hy)
            f.update(new)
            worst = max(worst, float(cmax.max()))
        self.advect_substeps, self.advect_courant = n_sub, worst

    def evolve_model_batched(self, t):
        from sp_coupler_amd import thermo
        dt = float(t) - self.model_time
        if dt <= 0:
            return
        if self.advect_par is None:
            return super().evolve_model_batched(t)
        f, p = self.fields3d, self.p
        self._step(dt)
        if "PS" in self.tend:
            p["PS"] = p["PS"] + dt * self.tend["PS"]
        self._advect(dt)
        if self.diffuse_par is not None:
            a, m, cp, s0 = (self._r(x) for x in ldr.df.profiles(self.zh_cache, self.zf_cache, p["Rhobf"], dt, **self.diffuse_par))
            for key, slot in (("U", None), ("V", None), ("THL", "wt"), ("QT", "wq")):
                if key in f:
                    flux = self._r(numpy.asarray(self.tend[slot], dtype=numpy.float64).reshape(self.n)) if slot in self.tend else None
                    f[key] = ldr.les_diffuse(f[key], a, m, cp, s0 if flux is not None else None, flux)
        if self.THERMO:
            self._stale = True
            self._ensure_ql()
        elif "QL" in f or ("QT" in f and "Qsat" in f):
            f["QL"] = numpy.maximum(f["QT"] - f["Qsat"], 0.0)
        self._slab_means()
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


class HostAdvectLESEnsemble(_HostAdvect, ldr.HostDiffuseLESEnsemble):
    """without enable_thermo(): QL = max(QT - Qsat, 0) of the advected (and diffused) QT, and again after the microphysics"""


class HostThermoAdvectLESEnsemble(_HostAdvect, ldr.HostThermoDiffuseLESEnsemble):
    """after enable_thermo(): K12's oracle on the advected (and diffused) THL and QT, and again after the microphysics"""

    THERMO = True


def ensemble_run(engine, n, thermo, device, micro=False, diffuse=False, advect=True, dx=None, spike=False, itot=4, jtot=5, nL=20, steps=3):
    """an ensemble with attached U, V, THL, QT (and Qsat, or thermo; QR with the microphysics) through ``steps`` calls of
    evolve_model_batched with one variability nudge (constantT) before the last; after each of them every profile and the
    fields.  ``dx``: the grid spacing along i (the winds are about 5 m/s and -2 m/s and a step is 900 s: the default 200 m asks
    for tens of substeps); ``spike``: QT raised in one column of every LES.  Returns (ens, list of records)"""
    def spiked(fields):
        if spike:
            fields["QT"][:, 1, 3, :] *= 1.5

    def record(ens, rec):
        rec["TWP"] = numpy.array(host_of(ens.get_water_paths_batched(("TWP",))["TWP"]))
        if advect:
            record_substeps(ens, rec)
    return ensemble_case(engine, n, models.DeviceLESEnsemble if device else (HostThermoAdvectLESEnsemble if thermo else HostAdvectLESEnsemble),
                         thermo=thermo, micro=micro, diffuse=diffuse, edit=spiked,
                         advection=dict(dx=dx, dy=None if dx is None else 1.5 * numpy.asarray(dx)) if advect else None, record=record,
                         itot=itot, jtot=jtot, nL=nL, steps=steps)


def record_substeps(ens, rec, z=False):
    """the substeps and the Courant sum (``z``: and the vertical one) of the last step into a record of ensemble_case"""
    rec["substeps"] = numpy.array([-1 if ens.advect_substeps is None else ens.advect_substeps], dtype=numpy.float64)
    rec["courant"] = numpy.array([-1.0 if ens.advect_courant is None else ens.advect_courant])
    if z:
        rec["courant z"] = numpy.array([-1.0 if ens.advect_courant_z is None else ens.advect_courant_z])


DX_ONE = 60000.0                                                  # c = 0.5 * 900 / 60000 * 2 |u| of at most ~9 m/s: below cfl, one substep
DX_FEW = 13000.0                                                  # ... c about 0.55 ... 0.75 along i alone, dy = 1.5 dx on top: 2 or 3 substeps


def check_ensemble(one, engines, n, thermo, micro=False, diffuse=False, dx=DX_FEW, **kw):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``; the winds carry the fields: a QT
    raised in one column differs from the same run without enable_advection() in the columns next to it.  Returns the twin's
    substeps of the first step"""
    host = ensemble_run(one, n, thermo, False, micro=micro, diffuse=diffuse, dx=dx, spike=True, **kw)[1]
    plain = ensemble_run(one, n, thermo, False, micro=micro, diffuse=diffuse, dx=dx, spike=True, advect=False, **kw)[1]
    assert (host[1]["field QT"][:, 2, 3, :] != plain[1]["field QT"][:, 2, 3, :]).any()
    assert not numpy.array_equal(host[-1]["p QT"], plain[-1]["p QT"]) or not numpy.array_equal(host[-1]["field U"], plain[-1]["field U"])
    n_sub = int(host[1]["substeps"][0])
    assert n_sub == (1 if dx == DX_ONE else n_sub) and (dx != DX_FEW or n_sub in (2, 3)), n_sub
    assert 0 < host[1]["courant"][0] <= 0.5
    for engine in engines:
        lmr.same_logs(host, ensemble_run(engine, n, thermo, True, micro=micro, diffuse=diffuse, dx=dx, spike=True, **kw)[1])
    return n_sub
