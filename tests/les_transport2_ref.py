"""NumPy oracle of K23 (include/spc.h: spc_les_transport2_*), the bodies of the GPU tests of tests/test_les_transport2_gpu.py
(each takes an engine: tools/mutation_control.py --transport2 hands them the engines of its mutant libraries), an
oracle-backed engine with ``les_transport2`` for the CPU suite and the host twins of DeviceLESEnsemble's
enable_advection(vertical=True, conservative=True, order=2).

The oracle spells the rule out in the statement order of include/spc.h, one operation per NumPy call in the element type,
``numpy.where`` for the selects; the face numbers and the donor fluxes are K22's own (tests/les_transport_ref.face_numbers,
fluxes).  Every device array of the bodies is the LEADING part of a buffer whose poison is NaN (tests/les_harness.Poisoned): a
read of it would show up in a finite result, a write in the bytes that are checked after the launch."""
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
from tests import les_transport_ref as ltr
from tests import les_vadvect_ref as lvr
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, cols_table, ensemble_case, fill_args, host_of, np_of, on_both, run_bodies)

LIMITERS = ("mc", "none")
#: the extents at which the distance-2 neighbours fold onto each other (1, 2, 3, 4) or the boundary slopes meet (ktot 1 ... 5)
PLANES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (4, 3), (8, 8), (5, 33)]
KTOTS = [1, 2, 3, 4, 5, 63, 64, 65, 160]
NS = ltr.NS
NAMES = ltr.NAMES
ALL_NAMES = ltr.ALL_NAMES
OUT_FILL = ltr.OUT_FILL
field_like = ltr.field_like
case = ltr.case
split = ltr.split
derived_cols = ltr.derived_cols
face_numbers = ltr.face_numbers
fluxes = ltr.fluxes


# -- the rule --------------------------------------------------------------------------------------------------------------
def slope(xm, x, xp, limiter):
    """the slope of the cells x from their neighbours xm and xp along one axis"""
    T = x.dtype.type
    with numpy.errstate(all="ignore"):
        a = x - xm
        b = xp - x
        t = a + b
        c0 = T(0.5) * t
        if limiter == "none":
            return c0
        assert limiter == "mc"
        a2 = T(2) * a
        b2 = T(2) * b
        lo = numpy.where(a2 < b2, a2, b2)
        slo = numpy.where(c0 < lo, c0, lo)
        hi = numpy.where(a2 > b2, a2, b2)
        shi = numpy.where(c0 > hi, c0, hi)
        return numpy.where((a > 0) & (b > 0), slo, numpy.where((a < 0) & (b < 0), shi, T(0)))


def slopes(x, limiter):
    """(si, sj, sk) of the field x [n x itot x jtot x ktot]: periodic along i and j, +0 at the lowest and the highest level"""
    si = slope(numpy.roll(x, 1, axis=1), x, numpy.roll(x, -1, axis=1), limiter)
    sj = slope(numpy.roll(x, 1, axis=2), x, numpy.roll(x, -1, axis=2), limiter)
    xm = numpy.concatenate([x[..., :1], x[..., :-1]], axis=3)
    xp = numpy.concatenate([x[..., 1:], x[..., -1:]], axis=3)
    sk = numpy.array(slope(xm, x, xp, limiter))
    sk[..., 0] = 0.0
    sk[..., -1] = 0.0
    return si, sj, sk


def hface(p, q, su, sd):
    """the correction of a horizontal face: su, sd the slopes of the cells upwind of p and of q"""
    T = p.dtype.type
    with numpy.errstate(all="ignore"):
        tp = T(1) - p
        gp = p * tp
        uq = T(1) + q
        hq = q * uq
        m1 = gp * su
        m2 = hq * sd
        d = m1 - m2
        return T(0.5) * d


def vface(p, q, rl, ru, sl, su):
    """the correction of a vertical face: rl, ru 1 / g and sl, su the slopes of the cells below and above it"""
    T = p.dtype.type
    with numpy.errstate(all="ignore"):
        cp = p * rl
        dq = q * ru
        tp = T(1) - cp
        gp = p * tp
        uq = T(1) + dq
        hq = q * uq
        m1 = gp * sl
        m2 = hq * su
        d = m1 - m2
        return T(0.5) * d


def corrections(x, n, r, limiter):
    """(Aw, Ae, As, An, Ab, At) of the field x, the face numbers n and the profile r [n x ktot]"""
    si, sj, sk = slopes(x, limiter)
    zero = numpy.zeros_like(sk[..., :1])
    sk_dn = numpy.concatenate([zero, sk[..., :-1]], axis=3)
    sk_up = numpy.concatenate([sk[..., 1:], zero], axis=3)
    rr = numpy.broadcast_to(r[:, None, None, :], x.shape)
    r_km = numpy.concatenate([rr[..., :1], rr[..., :-1]], axis=3)
    r_kp = numpy.concatenate([rr[..., 1:], rr[..., -1:]], axis=3)
    return (hface(n["pw"], n["qw"], numpy.roll(si, 1, axis=1), si), hface(n["pe"], n["qe"], si, numpy.roll(si, -1, axis=1)),
            hface(n["ps"], n["qs"], numpy.roll(sj, 1, axis=2), sj), hface(n["pn"], n["qn"], sj, numpy.roll(sj, -1, axis=2)),
            vface(n["pb"], n["qb"], r_km, rr, sk_dn, sk), vface(n["pt"], n["qt"], rr, r_kp, sk, sk_up))


def fluxes2(x, n, r, limiter):
    """(Fw2, Fe2, Fs2, Fn2, Fb2, Ft2): K22's donor fluxes plus the corrections"""
    with numpy.errstate(all="ignore"):
        return tuple(F + A for F, A in zip(fluxes(x, n), corrections(x, n, r, limiter)))


def les_transport2(fields, u, v, hx, hy, g, r, limiter="mc"):
    """(dict name -> the new field (a new array), cmax [n], mtop, dict name -> ftop [n x itot x jtot]) as
    tests/les_transport_ref.les_transport returns them"""
    nums = face_numbers(u, v, hx, hy, g, r)
    n = u.shape[0]
    cmax = nums["s"].reshape(n, -1).max(axis=1) if n else numpy.zeros(0, dtype=u.dtype)
    rr = r[:, None, None, :]
    out, ftop = {}, {}
    with numpy.errstate(all="ignore"):
        for k, x in fields.items():
            assert x.dtype == u.dtype and x.shape == u.shape
            Fw, Fe, Fs, Fn, Fb, Ft = fluxes2(x, nums, r, limiter)
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


def oracle(c, limiter):
    return les_transport2(c["fields"], c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"], limiter)


def closed_cell_3d(dtype, target=0.5):
    """the 3-D closed cell: tests/les_transport_ref.closed_cell (n = 2, 8 x 8 x 40) with v = 0.7 u transposed in (i, j), the
    winds scaled to a largest outflow Courant sum of ``target``"""
    c = ltr.closed_cell(dtype, n=2)
    T = c["u"].dtype.type
    c["v"] = numpy.ascontiguousarray(T(0.7) * c["u"].transpose(0, 2, 1, 3))
    return ltr.scaled(c, target=target)


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one launch through ``eng.les_transport2`` with EVERY array the leading part of a buffer poisoned with NaN (the profiles'
    pitch included); ``check`` compares the outputs, cmax, mtop and ftop with the oracle bit for bit, the inputs with what was
    uploaded, and looks at the bytes around every array.  ``pad``: elements between the rows of g and r"""

    def __init__(self, eng, c, limiter, lead=0, cmax=True, mtop=True, ftop=True, pad=0):
        self.eng, self.c, self.limiter = eng, c, limiter
        self.mem = Poisoned(eng)
        put = lambda tag, a: self.mem.put(tag, a, float("nan"), lead)                      # noqa: E731
        prof = lambda tag, a: self.mem.rows(tag, a, float("nan"), lead, pad)               # noqa: E731
        self.du, self.dv = put("u", c["u"]), put("v", c["v"])
        self.dev = {k: (self.du if x is c["u"] else self.dv if x is c["v"] else put(k, x)) for k, x in c["fields"].items()}
        self.out = {k: put("out " + k, numpy.full_like(x, OUT_FILL)) for k, x in c["fields"].items()}
        self.dhx, self.dhy = put("hx", c["hx"]), put("hy", c["hy"])
        self.dg, self.dr = prof("g", c["g"]), prof("r", c["r"])
        self.dcmax = put("cmax", numpy.full_like(c["hx"], -5.0)) if cmax else None
        self.dmtop = put("mtop", numpy.full_like(c["u"], OUT_FILL)) if mtop else None
        nf = len(c["fields"])
        self.dftop = put("ftop", numpy.full((nf,) + c["u"].shape[:3], OUT_FILL, dtype=c["u"].dtype)) if ftop and nf else None
        self.got = eng.les_transport2(self.dev, self.out, self.du, self.dv, self.dhx, self.dhy, self.dg, self.dr, limiter=limiter,
                                      cmax=self.dcmax if cmax else False, mtop=self.dmtop, ftop=self.dftop)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def check(self, what=""):
        c = self.c
        what = "%s %s" % (self.limiter, what)
        want, cmax, mtop, ftop = oracle(c, self.limiter)
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


def raw_launch(eng, c, limiter=_abi.SPC_LIMITER_MC, names=None, cmax=True, mtop=True, ftop=True, alias=None, extents=None, null=()):
    """spc_les_transport2_* itself, as tests/les_transport_ref.raw_launch calls K22's: (rc, dict name -> host output, host cmax
    or None, host mtop or None, host ftop or None); ``limiter`` is the integer of the struct"""
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
    a = _abi.LesTransport2Args()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.pitch_prof, a.limiter = n, itot, jtot, ktot, len(names), ktot, limiter
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
    rc = abi_call(eng, "spc_les_transport2", a)
    host = lambda flag, k: t[k].cpu().numpy() if flag else None                             # noqa: E731
    return rc, {k: t["out " + k].cpu().numpy() for k in names}, host(cmax, "cmax"), host(mtop, "mtop"), host(ftop, "ftop")


def differs(c, want, limiter):
    """the answer is neither the input nor K22's where the plane has a gradient"""
    first = ltr.oracle(c)[0]
    return all((want[k] != c["fields"][k]).any() and (want[k] != first[k]).any() for k in c["fields"])


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, n=3):
    """U, V (the winds themselves), THL and QT against the oracle with both limiters, cmax, mtop and ftop included"""
    n = ltr._n_for(plane, ktot, n)
    c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
    for limiter in LIMITERS:
        want, cmax, mtop, ftop = Run(eng, c, limiter).check("n %d plane %s ktot %d" % (n, plane, ktot))
        if min(plane) > 2:
            assert differs(c, want, limiter)


def check_outputs(eng):
    """cmax and mtop of K23 are K22's outputs bit for bit, from a full launch and from the probe, which is K22's probe"""
    dtype = np_of(eng)
    for shape in ((1, 1, 1, 1), (2, 3, 5, 64), (5, 9, 9, 65)):
        c = case(shape, dtype, seed=6)
        _, want, mwant, _ = ltr.oracle(c)
        first = ltr.Run(eng, c)
        first.check("K22 %s" % (shape,))
        for limiter in LIMITERS:
            full = Run(eng, c, limiter)
            full.check("full %s" % (shape,))
            assert_bits("cmax == K22's", full.dcmax.cpu().numpy(), first.dcmax.cpu().numpy())
            assert_bits("mtop == K22's", full.dmtop.cpu().numpy(), first.dmtop.cpu().numpy())
            for cmax, mtop in ((True, True), (True, False), (False, True)):
                probe = Run(eng, dict(c, fields={}), limiter, cmax=cmax, mtop=mtop)
                probe.check("probe %s" % (shape,))
                if cmax:
                    assert_bits("probe == oracle", probe.dcmax.cpu().numpy(), want)
                if mtop:
                    assert_bits("probe mtop == oracle", probe.dmtop.cpu().numpy(), mwant)


def check_rows(eng, ktot):
    """n = 1, 2, 5 at 3 x 5: hx, hy, g and r differ per LES, with and without a pitch"""
    for n in NS:
        c = case((n, 3, 5, ktot), np_of(eng), seed=1)
        for limiter in LIMITERS:
            Run(eng, c, limiter).check("rows n %d ktot %d" % (n, ktot))
            Run(eng, c, limiter, pad=3).check("rows n %d ktot %d pitched" % (n, ktot))


def check_tiles(eng):
    """every boundary of the workgroups, derived as tests/les_transport_ref.check_tiles derives them: C - 1, C, C + 1 and
    2 C + 1 columns for every C, ktot on both sides of every change of C, 17 columns at the last supported ktot, and the first
    unsupported ktot refused without a write"""
    dtype = np_of(eng)
    esize = numpy.dtype(dtype).itemsize
    first, changes, bad = table = cols_table(eng.transport2_cols_per_block)
    assert table == cols_table(lambda k: derived_cols(k, esize)) == cols_table(eng.transport_cols_per_block)
    assert sorted(first) == [16, 32, 64] and len(changes) == 2, table
    for C, k0 in first.items():
        ktot = 7 if C == 64 else k0
        assert eng.transport2_cols_per_block(ktot) == C
        for ncols in (C - 1, C, C + 1, 2 * C + 1):
            n, itot, jtot = split(ncols)
            for limiter in LIMITERS:
                Run(eng, case((n, itot, jtot, ktot), dtype, seed=2, names=("U", "QT")), limiter).check("C %d: %d x %d x %d x %d" % (C, n, itot, jtot, ktot))
    for k in changes:
        for ktot in (k - 1, k):
            for limiter in LIMITERS:
                Run(eng, case((1, 3, 23, ktot), dtype, seed=3, names=("THL",)), limiter).check("change at %d: ktot %d" % (k, ktot))
    for limiter in LIMITERS:
        Run(eng, case((1, 1, 17, bad - 1), dtype, seed=4, names=("V", "QT")), limiter).check("tall: 17 columns of %d" % (bad - 1))
    rc, got, cmax, mtop, ftop = raw_launch(eng, case((1, 1, 2, bad), dtype, seed=4, names=("QT",)))
    assert rc == _abi.SPC_ERR_UNSUPPORTED and b"levels" in eng.lib.spc_last_error()
    assert (got["QT"] == OUT_FILL).all() and (cmax == -5.0).all() and (mtop == OUT_FILL).all() and (ftop == OUT_FILL).all()
    return table


def check_fields(eng):
    """0 to 6 fields with U and V among them, 1 to 6 without, with and without cmax, mtop and ftop, and the C ABI"""
    dtype = np_of(eng)
    for limiter in LIMITERS:
        for nf in range(0, 7):
            Run(eng, case((2, 3, 5, 65), dtype, seed=3, names=ALL_NAMES[:nf]), limiter).check("%d fields with the winds" % nf)
            if nf:
                c = case((2, 3, 5, 65), dtype, seed=4, names=ALL_NAMES[:nf])
                rng = numpy.random.default_rng(nf)
                c["fields"] = {("F%d" % i): field_like(k, c["u"].shape, dtype, rng) for i, k in enumerate(ALL_NAMES[:nf])}  # none is u or v
                Run(eng, c, limiter).check("%d fields without the winds" % nf)
        for cmax in (True, False):
            for mtop in (True, False):
                for ftop in (True, False):
                    Run(eng, case((2, 3, 5, 9), dtype, seed=5), limiter, cmax=cmax, mtop=mtop, ftop=ftop).check("cmax %s mtop %s ftop %s" % (cmax, mtop, ftop))
        rc, got, cmax, mtop, ftop = raw_launch(eng, case((2, 3, 5, 9), dtype, seed=5), limiter=_abi.LIMITERS[limiter])
        want = oracle(case((2, 3, 5, 9), dtype, seed=5), limiter)
        assert rc == 0
        for q, k in enumerate(NAMES):
            assert_bits("raw %s" % k, got[k], want[0][k])
            assert_bits("raw ftop %s" % k, ftop[q], want[3][k])
        assert_bits("raw cmax", cmax, want[1])
        assert_bits("raw mtop", mtop, want[2])


def check_alignment(eng, lead, ktot=65):
    """views one (or more) elements off the 16-byte grid"""
    for limiter in LIMITERS:
        Run(eng, case((3, 3, 5, ktot), np_of(eng), seed=10 + lead), limiter, lead=lead).check("lead %d ktot %d" % (lead, ktot))


def check_signs(eng):
    """winds of either sign in all combinations (every horizontal face an inflow or an outflow face everywhere: each of the two
    products of a correction is the live one somewhere), convergent and divergent columns, and still air, which keeps every bit"""
    dtype = np_of(eng)
    for limiter in LIMITERS:
        for su in (1, -1):
            for sv in (1, -1):
                c = case((2, 4, 5, 9), dtype, seed=7, names=("THL", "QT"))
                c["u"][...] = dtype(su) * (numpy.abs(c["u"]) + dtype(0.5))
                c["v"][...] = dtype(sv) * (numpy.abs(c["v"]) + dtype(0.5))
                want, cmax, mtop, ftop = Run(eng, c, limiter).check("signs %d %d" % (su, sv))
                assert (cmax > 0).all() and (mtop > 0).any() and (mtop < 0).any() and differs(c, want, limiter)
        for sign in (1, -1):
            c = lvr.column_winds(case((2, 4, 3, 9), dtype, seed=8, names=("THL", "QT")), sign)
            want, cmax, mtop, ftop = Run(eng, c, limiter).check("column sign %d" % sign)
            assert (mtop[:, 1, :, :] * sign > 0).all() and (mtop[:, 3, :, :] * sign < 0).all()
        c = case((2, 3, 5, 9), dtype, seed=8, names=("THL", "QT"))
        c["u"][...] = 0.0
        c["v"][...] = -0.0
        r = Run(eng, c, limiter)
        _, cmax, mtop, _ = r.check("zeros")
        assert not cmax.any()
        assert_bits("still air keeps THL", r.out["THL"].cpu().numpy(), c["fields"]["THL"])


def check_constant(eng):
    """a constant field (and one that is constant along one axis only) equals the oracle; how far the oracle moves a constant
    is the CPU suite's to bound"""
    dtype = np_of(eng)
    for limiter in LIMITERS:
        c = case((2, 4, 5, 9), dtype, seed=12, names=("THL", "QT"))
        c["fields"]["THL"][...] = dtype(287.3)
        c["fields"]["QT"][...] = c["fields"]["QT"][:, :1, :1, :]
        Run(eng, c, limiter).check("constant")


def near2(shape, cell):
    """the mask of ``cell`` (l, i, j, k) and the cells within two steps of it along each axis (periodic in i and j)"""
    n, itot, jtot, ktot = shape
    l, i, j, k = cell
    mask = numpy.zeros(shape, dtype=bool)
    mask[l, i, j, max(k - 2, 0):k + 3] = True
    for d in (-2, -1, 1, 2):
        mask[l, (i + d) % itot, j, k] = mask[l, i, (j + d) % jtot, k] = True
    return mask


def special_case(dtype, ktot=9):
    """(a clean case whose fields are not the winds, the same with NaN, +inf, -inf and -0.0 planted in one cell each of THL, the
    mask of the cells within two steps of a planted value along one axis)"""
    c = case((3, 9, 9, ktot), dtype, seed=9, names=("THL", "QT"))
    s = dict(c, fields={k: x.copy() for k, x in c["fields"].items()})
    planted = {(0, 0, 0, 1): numpy.nan, (0, 4, 8, 4): numpy.inf, (1, 8, 3, 0): -numpy.inf, (1, 2, 6, ktot - 1): -0.0}
    mask = numpy.zeros(c["u"].shape, dtype=bool)
    for cell, val in planted.items():
        s["fields"]["THL"][cell] = val
        mask |= near2(c["u"].shape, cell)
    return c, s, mask


def check_special(eng):
    """NaN, +-inf and -0.0 planted in single cells of a field: every output is the oracle's, and the cells further than two
    steps away along each axis hold the bits of a run without them"""
    dtype = np_of(eng)
    c, s, mask = special_case(dtype)
    for limiter in LIMITERS:
        clean, _, _, clean_ftop = Run(eng, c, limiter).check("clean")
        r = Run(eng, s, limiter)
        want, cmax, _, ftop = r.check("special")
        assert_bits("the cells further away", r.out["THL"].cpu().numpy()[~mask], clean["THL"][~mask])
        assert_bits("QT never sees THL", r.out["QT"].cpu().numpy(), clean["QT"])
        assert_bits("QT's lid flux never sees THL", ftop["QT"], clean_ftop["QT"])
        assert numpy.isnan(want["THL"][0, 0, 0, 1]) and numpy.isfinite(cmax).all()
        assert not numpy.isfinite(want["THL"][mask]).all() and numpy.isfinite(want["THL"][~mask]).all()


def bad_calls(eng, t, o, u, v, hx, hy, g, r, m, ft):
    """the calls of ``Engine.les_transport2`` that are refused, as callables: ``check_refusals`` makes them on a device,
    tests/test_engine_les_args_cpu.py on a stand-in that launches nothing, where it pins their texts"""
    many = {("F%d" % i): t["QT"].clone() for i in range(7)}
    other = torch.float64 if eng.dtype == torch.float32 else torch.float32
    V = eng.les_transport2
    return [lambda: V(t, o, u, v, hx, hy, g, r, limiter="minmod"),
            lambda: V(t, o, u, v, hx, hy, g, r, limiter=1),
            lambda: V(t, o, u, v, hx, hy, g, r, limiter=None),
            lambda: V({}, {}, u, v, hx, hy, g, r, limiter="superbee"),
            lambda: V({}, {}, u, v, hx, hy, g, r, cmax=False),
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
    """K22's refusals through spc_les_transport2_* and ``Engine.les_transport2``, and the limiter that is neither: no refused
    call touches anything"""
    dtype = np_of(eng)
    c = case((2, 2, 3, 8), dtype, seed=11)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    for kw, text in ((dict(limiter=2), b"limiter"), (dict(limiter=-1), b"limiter"), (dict(limiter=2, names=()), b"limiter"),
                     (dict(names=(), cmax=False, mtop=False), b"nothing to do"), (dict(names=(), cmax=False, mtop=False, ftop=True), b"nothing to do"),
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
    a = _abi.LesTransport2Args()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.pitch_prof, a.limiter = 2, 2, 3, 8, 1, 8, _abi.SPC_LIMITER_MC
    a.u, a.v, a.hx, a.hy, a.g, a.r = (x.data_ptr() for x in (u, v, hx, hy, g, r))
    a.fields[0], a.out[0] = t["QT"].data_ptr(), skew.data_ptr()
    fn = eng.lib.spc_les_transport2_f32 if eng.dtype == torch.float32 else eng.lib.spc_les_transport2_f64
    assert fn(ctypes.byref(a), None) == E and b"not aligned" in eng.lib.spc_last_error() and not bool(raw.any())
    got = eng.les_transport2({k: x[:0] for k, x in t.items()}, {k: x[:0] for k, x in o.items()}, u[:0], v[:0], hx[:0], hy[:0], g[:0], r[:0],
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
    for limiter in LIMITERS:
        want, cmax, mtop, ftop = oracle(c, limiter)
        for tag, eng, up in on_both(one, multi, n):
            u, v = up(c["u"]), up(c["v"])
            t = {k: (u if x is c["u"] else v if x is c["v"] else up(x)) for k, x in c["fields"].items()}
            o = {k: up(numpy.full_like(x, OUT_FILL)) for k, x in c["fields"].items()}
            m = up(numpy.full_like(c["u"], OUT_FILL))
            lid = lambda w: torch.full((len(t),) + tuple(w.shape[:3]), OUT_FILL, dtype=w.dtype, device=w.device)          # noqa: E731
            ft = Sharded([lid(w) for w in u.parts], u.bounds) if tag == "multi" else lid(u)
            prof = [up(c[k]) for k in ("hx", "hy", "g", "r")]
            got = eng.les_transport2(t, o, u, v, *prof, limiter=limiter, mtop=m, ftop=ft)
            multi.synchronize()
            for q, k in enumerate(NAMES):
                assert_bits("%s %s %s" % (limiter, tag, k), host_of(o[k]), want[k])
                lidk = numpy.concatenate([p[q].cpu().numpy() for p in ft.parts]) if tag == "multi" else ft[q].cpu().numpy()
                assert_bits("%s %s ftop %s" % (limiter, tag, k), lidk, ftop[k])
            assert_bits("%s cmax" % tag, host_of(got), cmax)
            assert_bits("%s mtop" % tag, host_of(m), mtop)
            probe = eng.les_transport2({}, {}, u, v, *prof, limiter=limiter)
            multi.synchronize()
            assert_bits("%s probe" % tag, host_of(probe), cmax)
    return blocks_of(o["QT"], multi, n)


BODIES = ("parity", "outputs", "rows", "tiles", "fields", "alignment", "signs", "constant", "special", "refusals")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in (1, 3, 4, 5, 64, 160)]),
            ("outputs", lambda: check_outputs(eng)),
            ("rows", lambda: [check_rows(eng, k) for k in (1, 65)]),
            ("tiles", lambda: check_tiles(eng)),
            ("fields", lambda: check_fields(eng)),
            ("alignment", lambda: [check_alignment(eng, lead) for lead in (1, 3)]),
            ("signs", lambda: check_signs(eng)),
            ("constant", lambda: check_constant(eng)),
            ("special", lambda: check_special(eng)),
            ("refusals", lambda: check_refusals(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_transport2 (CPU suite) ---------------------------------------------------------------------
class Transport2OracleEngine(ltr.TransportOracleEngine):
    """tests/les_transport_ref.TransportOracleEngine with ``les_transport2`` by the NumPy oracle above: the outputs written whole
    into the caller's tensors, as the HIP engine does"""

    def les_transport2(self, fields, out, u, v, hx, hy, g, r, limiter="mc", cmax=True, mtop=None, ftop=None, **kw):
        want = cmax is not None and cmax is not False
        if limiter not in LIMITERS:
            raise ValueError("limiter %r" % (limiter,))
        if sorted(fields) != sorted(out) or (not fields and not want and mtop is None) or (not fields and ftop is not None):
            raise ValueError("out does not match the fields, or nothing to do")
        if ftop is not None and tuple(ftop.shape) != (len(fields),) + tuple(u.shape[:3]):
            raise ValueError("ftop must be [fields x n x itot x jtot]")
        read = {t.data_ptr() for t in [u, v] + list(fields.values())}
        written = [t.data_ptr() for t in out.values()] + [t.data_ptr() for t in (mtop, ftop) if t is not None]
        if u.shape[0] and (len(set(written)) != len(written) or set(written) & read):
            raise ValueError("an output is an input or another output")
        res, c, m, lid = les_transport2({k: t.numpy() for k, t in fields.items()}, u.numpy(), v.numpy(), hx.numpy(), hy.numpy(),
                                        numpy.ascontiguousarray(g.numpy()), numpy.ascontiguousarray(r.numpy()), limiter)
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


# -- the host twins of DeviceLESEnsemble after enable_advection(vertical=True, conservative=True, order=2) -----------------------
class _HostTransport2(ltr._HostTransport):
    """tests/les_transport_ref._HostTransport with ``order`` and ``limiter``: with order=2 every substep is K23 (the oracle
    above) where the twin of K22 has K22; the probe, the substeps, K21 and the sum of the lid flux are unchanged"""

    advect_order = 1
    advect_limiter = "mc"

    def enable_advection(self, dx=None, dy=None, cfl=None, max_substeps=None, vertical=False, conservative=False, order=1, limiter="mc"):
        if order not in (1, 2) or limiter not in LIMITERS or (order == 2 and not conservative):
            raise ValueError("order 2 needs conservative=True and a limiter of %s" % (LIMITERS,))
        super().enable_advection(dx=dx, dy=dy, cfl=cfl, max_substeps=max_substeps, vertical=vertical, conservative=conservative)
        self.advect_order, self.advect_limiter = order, limiter

    def _advect(self, dt):
        if self.advect_order != 2:
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
            new, cmax, self._mtop, lid = les_transport2({k: f[k] for k in self.KEYS if k in f}, f["U"], f["V"], hx, hy, g, r, self.advect_limiter)
            f.update(new)
            worst = max(worst, float(cmax.max()))
            total = {k: a.copy() for k, a in lid.items()} if total is None else {k: total[k] + lid[k] for k in lid}
        self.advect_substeps, self.advect_courant, self.advect_courant_z, self._mtop_dt = n_sub, worst, None, dt / n_sub
        self._lid = total
        if buoyant:
            self.buoyancy_wind_change = worst_b


class HostTransport2LESEnsemble(_HostTransport2, lbr.HostBuoyancyLESEnsemble):
    """without enable_thermo()"""


class HostThermoTransport2LESEnsemble(_HostTransport2, lbr.HostThermoBuoyancyLESEnsemble):
    """after enable_thermo()"""


VARIANTS = ltr.VARIANTS
DX = ltr.DX


def ensemble_run(engine, n, device, order=2, limiter="mc", buoyancy=False, thermo=False, micro=False, diffuse=False, radiate=False, itot=4, jtot=5,
                 nL=20, steps=3):
    """tests/les_transport_ref.ensemble_run with enable_advection(vertical=True, conservative=True, order=..., limiter=...);
    ``order=None``: the call as it was before K23.  Returns (ens, list of records)"""
    keys = ("U", "V", "THL", "QT") + (("QR",) if micro else ())

    def record(ens, rec):
        lar.record_substeps(ens, rec)
        ltr.record_lid(ens, rec, keys)
        if buoyancy:
            lbr.record_pressure(ens, rec)

    def before(ens):
        assert ens.get_vertical_wind_batched() is None and ens.get_lid_flux_batched() is None
    return ensemble_case(engine, n, models.DeviceLESEnsemble if device else (HostThermoTransport2LESEnsemble if thermo else HostTransport2LESEnsemble),
                         thermo=thermo, micro=micro, diffuse=diffuse, edit=lvr.raise_u,
                         advection=dict(dx=DX, dy=1.5 * DX, vertical=True, conservative=True, **({} if order is None else {"order": order, "limiter": limiter})),
                         radiation=lrr.radiation_of(n, "f0", "f1") if radiate else None, enable=lambda ens: buoyancy and ens.enable_buoyancy(),
                         record=record, before=before, itot=itot, jtot=jtot, nL=nL, steps=steps)


def check_ensemble(one, engines, n, variant, limiter="mc"):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``: every profile, field and lid flux
    bit-equal after each step, W within a few roundings; the second-order step is not the first-order one (THL of the twin's
    first step differs from the run with order=1), and that run on the device is bit-equal to the twin's and to the run of
    enable_advection(vertical=True, conservative=True) without the new arguments.  Returns the twin's substeps of the three
    steps"""
    kw = VARIANTS[variant]
    twin, host = ensemble_run(one, n, False, limiter=limiter, **kw)
    first_log = ensemble_run(one, n, False, order=1, **kw)[1]
    assert (host[1]["field THL"] != first_log[1]["field THL"]).any()
    assert 0 < host[1]["courant"][0] <= 0.5 and all(numpy.isfinite(r["courant"][0]) for r in host)
    assert all(host[1]["lid " + k].any() for k in ("U", "THL", "QT"))
    for engine in engines:
        ens, log = ensemble_run(engine, n, True, limiter=limiter, **kw)
        lmr.same_logs(host, log)
        lvr.check_w(ens, twin)
    lmr.same_logs(first_log, ensemble_run(engines[0], n, True, order=1, **kw)[1])
    lmr.same_logs(first_log, ensemble_run(engines[0], n, True, order=None, **kw)[1])
    return [int(host[q]["substeps"][0]) for q in (1, 2, 4)]         # (record 0: the start; record 3: after the nudge)
