"""NumPy oracle of K24 (include/spc.h: spc_les_mix_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_mix_gpu.py (each takes an engine: tools/mutation_control.py --mix hands them the engines of its mutant libraries),
the host twins of models.DeviceLESEnsemble's mixing mode and an oracle-backed engine with ``les_mix`` for the CPU suite.

The oracle spells the rule out with ``numpy.roll`` for the periodic neighbours and clamped index vectors along k, one statement
per rounding in the element type, so nothing fuses.  Every device array of the bodies is the LEADING part of a poisoned buffer
(tests/les_harness.Poisoned); the bytes behind it (and in front of a view off the 16-byte grid) are checked after the launch."""
import numpy
import torch

from sp_coupler_amd import _abi, models
from sp_coupler_amd import advection as adv
from sp_coupler_amd import diffusion as dif
from sp_coupler_amd import mixing as mix
from tests import les_advect_ref as lar
from tests import les_full_ref as lfr
from tests import les_micro_ref as lmr
from tests import les_radiate_ref as lrr
from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, ensemble_case, host_of, np_of, on_both, run_bodies)

#: no neighbour at all, planes of two along one axis and along both, an odd plane, the flagship's, and one wider than a wave
#: along j
PLANES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (8, 8), (5, 33)]
#: no vertical neighbour (1), both clamped onto the two levels (2), around one wave (63, 64, 65), the flagship's 160
KTOTS = [1, 2, 63, 64, 65, 160]
NS = [1, 2, 5]
ROWS = [1, 2, 3, 8, 9, 33]                                         # itot of the strip seams
#: the fields of a case in the order of a launch: U, V and THL are u, v and theta themselves, as in the ensemble
NAMES = ("U", "V", "THL", "QT", "QR", "X")
WINDS = ("U", "V")
OUT_FILL = -7.0
DT = 60.0


# -- the rule --------------------------------------------------------------------------------------------------------------
def _L(a):
    return a[:, None, None, None]


def _P(a):
    return a[:, None, None, :]


def eddy(u, v, theta, gx, gy, gz, bz, l2, kcap):
    """(km [n x itot x jtot x ktot], kmax [n], the uncapped kk) of winds of dtype T, ``theta`` or None, gx, gy, kcap [n] and
    gz, bz, l2 [n x ktot]"""
    T = u.dtype.type
    assert all(a.dtype == u.dtype for a in (v, gx, gy, gz, l2, kcap)) and (theta is None or (theta.dtype == u.dtype and bz.dtype == u.dtype))
    n, _, _, ktot = u.shape
    k = numpy.arange(ktot)
    kp, kq = numpy.minimum(k + 1, ktot - 1), numpy.maximum(k - 1, 0)
    with numpy.errstate(all="ignore"):
        dux = numpy.roll(u, -1, axis=1) - numpy.roll(u, 1, axis=1)
        dvx = numpy.roll(v, -1, axis=1) - numpy.roll(v, 1, axis=1)
        duy = numpy.roll(u, -1, axis=2) - numpy.roll(u, 1, axis=2)
        dvy = numpy.roll(v, -1, axis=2) - numpy.roll(v, 1, axis=2)
        duz = u[..., kp] - u[..., kq]
        dvz = v[..., kp] - v[..., kq]
        ux = dux * _L(gx)
        vx = dvx * _L(gx)
        uy = duy * _L(gy)
        vy = dvy * _L(gy)
        uz = duz * _P(gz)
        vz = dvz * _P(gz)
        uxx = ux * ux
        vyy = vy * vy
        a = uxx + vyy
        sh = uy + vx
        a2 = a + a
        sh2 = sh * sh
        d = a2 + sh2
        uzz = uz * uz
        vzz = vz * vz
        z = uzz + vzz
        d = d + z
        if theta is not None:
            dth = theta[..., kp] - theta[..., kq]
            n2 = dth * _P(bz)
            d = d - n2
        e = numpy.where(d > 0, d, T(0))                            # a NaN gives +0
        r = numpy.sqrt(e)
        kk = _P(l2) * r
        kmax = kk.reshape(n, -1).max(axis=1) if n else numpy.zeros(0, dtype=u.dtype)
        km = numpy.where(kk < _L(kcap), kk, _L(kcap))
    assert km.dtype == kk.dtype == kmax.dtype == u.dtype
    return km, kmax, kk


def face_fluxes(x, km, ax, ay):
    """(fw, fe, fs, fn) of the field ``x``: the fluxes through the four faces of every cell"""
    assert x.dtype == km.dtype == ax.dtype == ay.dtype
    with numpy.errstate(all="ignore"):
        kw = numpy.roll(km, 1, axis=1) + km
        ke = km + numpy.roll(km, -1, axis=1)
        ks = numpy.roll(km, 1, axis=2) + km
        kn = km + numpy.roll(km, -1, axis=2)
        cw = kw * _L(ax)
        ce = ke * _L(ax)
        cs = ks * _L(ay)
        cn = kn * _L(ay)
        dw = x - numpy.roll(x, 1, axis=1)
        de = numpy.roll(x, -1, axis=1) - x
        ds = x - numpy.roll(x, 1, axis=2)
        dn = numpy.roll(x, -1, axis=2) - x
        fw = cw * dw
        fe = ce * de
        fs = cs * ds
        fn = cn * dn
    return fw, fe, fs, fn


def hmix(x, km, ax, ay):
    fw, fe, fs, fn = face_fluxes(x, km, ax, ay)
    with numpy.errstate(all="ignore"):
        hx = fe - fw
        hy = fn - fs
        h = hx + hy
        out = x + h
    assert out.dtype == x.dtype
    return out


def les_mix(fields, u, v, theta, gx, gy, gz, bz, l2, kcap, ax, ay):
    """(km, kmax, dict name -> the mixed field), new arrays; ``ax`` and ``ay`` dicts with the names of ``fields``"""
    km, kmax, _ = eddy(u, v, theta, gx, gy, gz, bz, l2, kcap)
    return km, kmax, {k: hmix(x, km, ax[k], ay[k]) for k, x in fields.items()}


# -- inputs ------------------------------------------------------------------------------------------------------------------
def case(shape, dtype, seed=0, dt=DT, cap=mix.CAP):
    """dict of the arguments in ``dtype``: u, v, theta, the fields QT, QR and X, gx, gy, kcap, gz, bz, l2 and ``coef``: name ->
    (ax, ay).  Another grid, dx, dy and so another coefficient and profile per LES; U and V share the winds' pair of vectors, THL
    and QT the scalars', QR and X have a pair of their own each (another Prandtl number); theta is stable in places and unstable
    in others, so km is +0 in some cells and positive in others"""
    dtype = numpy.dtype(dtype).type
    n, itot, jtot, ktot = shape
    rng = numpy.random.default_rng(24000 + seed + 7 * ktot + itot * jtot + 31 * n)
    _, zh, zf, _, _ = lrr.grid(n, ktot, rng)
    dx, dy = 200.0 * (1.0 + 0.1 * numpy.arange(n)), 300.0 * (1.0 + 0.05 * numpy.arange(n))
    k = numpy.arange(ktot)
    c = dict(u=5.0 + rng.standard_normal(shape), v=-2.0 + rng.standard_normal(shape),
             theta=290.0 + 10.0 * k / 160.0 + 0.5 * numpy.arange(n)[:, None, None, None] + 0.5 * rng.standard_normal(shape),
             QT=8e-3 * numpy.exp(-k / 160.0) * (1.0 + 0.05 * rng.standard_normal(shape)), QR=1e-5 * rng.random(shape),
             X=rng.standard_normal(shape))
    c["gx"], c["gy"], wind, scalar = mix.coefficients(dt, dx, dy, n=n)
    own = [mix.coefficients(dt, dx, dy, prandtl=pr, n=n)[3] for pr in (0.5, 0.8)]
    c["kcap"] = mix.cap(wind, scalar, cap)
    c["gz"], c["bz"], c["l2"] = mix.profiles(zf, zh, dx, dy, n=n)
    c = {key: numpy.ascontiguousarray(a.astype(dtype)) for key, a in c.items()}
    pairs = [tuple(numpy.ascontiguousarray(a.astype(dtype)) for a in p) for p in (wind, scalar) + tuple(own)]
    c["coef"] = {"U": pairs[0], "V": pairs[0], "THL": pairs[1], "QT": pairs[1], "QR": pairs[2], "X": pairs[3]}
    return c


def field_of(c, name):
    return c[{"U": "u", "V": "v", "THL": "theta"}.get(name, name)]


def oracle(c, names=NAMES, theta=True):
    """(km, kmax, dict name -> out) of the case"""
    return les_mix({k: field_of(c, k) for k in names}, c["u"], c["v"], c["theta"] if theta else None, c["gx"], c["gy"], c["gz"],
                   c["bz"] if theta else None, c["l2"], c["kcap"], {k: c["coef"][k][0] for k in names}, {k: c["coef"][k][1] for k in names})


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one call of ``eng.les_mix`` with every array inside a poisoned buffer; ``check`` compares km, kmax and every output with
    the oracle bit for bit, the read-only inputs with what was uploaded, and looks at the bytes around every array.
    ``leads``: elements in front of the 4-D arrays, taken in turn (u, v, theta, the other fields, km, the outputs); ``pad``:
    elements between the rows of gz, bz and l2 (pitched profiles).  Arrays that are one object in the case (u as the field U, the
    vectors two fields share) are one device tensor."""

    def __init__(self, eng, c, names=NAMES, theta=True, kmax=True, leads=(0,), pad=0):
        self.eng, self.c, self.names, self.theta = eng, c, tuple(names), theta
        self.mem = Poisoned(eng)
        self.inputs, seen, turn = [], {}, [0]

        def lead():
            turn[0] += 1
            return leads[(turn[0] - 1) % len(leads)]

        def put(tag, a, poison, ld=0):
            if id(a) not in seen:
                seen[id(a)] = self.mem.put(tag, a, poison, ld)
                self.inputs.append((tag, seen[id(a)], a))
            return seen[id(a)]
        nan = float("nan")
        self.du, self.dv = put("u", c["u"], nan, lead()), put("v", c["v"], nan, lead())
        self.dtheta = put("theta", c["theta"], nan, lead()) if theta else None
        self.dfields = {k: put(k, field_of(c, k), nan, lead()) for k in self.names}
        self.dgx, self.dgy, self.dkcap = (put(k, c[k], 1e30) for k in ("gx", "gy", "kcap"))
        prof = lambda tag: self.mem.rows(tag, c[tag], 1e30, pad=pad)                            # noqa: E731
        self.dgz, self.dl2 = prof("gz"), prof("l2")
        self.dbz = prof("bz") if theta else None
        self.inputs += [(k, t, c[k]) for k, t in (("gz", self.dgz), ("l2", self.dl2), ("bz", self.dbz)) if t is not None]
        self.dax = {k: put("ax " + k, c["coef"][k][0], 1e30) for k in self.names}
        self.day = {k: put("ay " + k, c["coef"][k][1], 1e30) for k in self.names}
        fill = numpy.full_like(c["u"], OUT_FILL)
        self.dkm = self.mem.put("km", fill, 1e30, lead())
        self.dout = {k: self.mem.put("out " + k, fill, 1e30, lead()) for k in self.names}
        self.dkmax = self.mem.put("kmax", numpy.full_like(c["gx"], -5.0), 1e30) if kmax else None
        self.got = eng.les_mix(self.dfields, self.dout, self.du, self.dv, self.dtheta, self.dgx, self.dgy, self.dgz, self.dbz, self.dl2,
                               self.dkcap, self.dkm, self.dax, self.day, kmax=self.dkmax if kmax else False)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def results(self):
        """(km, kmax or None, dict name -> out) on the host"""
        return (self.dkm.cpu().numpy(), None if self.dkmax is None else self.dkmax.cpu().numpy(), {k: t.cpu().numpy() for k, t in self.dout.items()})

    def check(self, what=""):
        km, kmax, outs = want = oracle(self.c, self.names, self.theta)
        got_km, got_kmax, got = self.results()
        assert_bits("%s km" % what, got_km, km)
        if self.dkmax is None:
            assert self.got is None
        else:
            assert self.got is self.dkmax
            assert_bits("%s kmax" % what, got_kmax, kmax)
        for k in self.names:
            assert_bits("%s out %s" % (what, k), got[k], outs[k])
        for tag, t, a in self.inputs:
            assert Poisoned.read_only(t, a), (what, tag, "read only")
        self.mem.check_around(what)
        return want


SCALARS = ("u", "v", "theta", "gx", "gy", "kcap", "gz", "bz", "l2", "km", "kmax")
ARRAYS = ("fields", "out", "ax", "ay")


def raw_launch(eng, c, names=("U", "QT"), alias=(), extents=None, null=()):
    """spc_les_mix_* itself: (rc, km, kmax, dict name -> out on the host, dict name -> the inputs on the host).  Every field is a
    tensor of its own.  ``alias``: (member, key) pairs that replace a pointer member by that of tensor ``key``, a member or key
    of an array spelled ("out", 0); ``extents``: overrides of the scalar members; ``null``: members set to NULL"""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    n, itot, jtot, ktot = c["u"].shape
    t = {k: dev(c[k]) for k in ("u", "v", "theta", "gx", "gy", "kcap", "gz", "bz", "l2")}
    t["km"], t["kmax"] = dev(numpy.full_like(c["u"], OUT_FILL)), dev(numpy.full_like(c["gx"], -5.0))
    for f, k in enumerate(names):
        t[("fields", f)], t[("out", f)] = dev(field_of(c, k)), dev(numpy.full_like(c["u"], OUT_FILL))
        t[("ax", f)], t[("ay", f)] = dev(c["coef"][k][0]), dev(c["coef"][k][1])
    a = _abi.LesMixArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.pitch_prof = n, itot, jtot, ktot, len(names), ktot

    def point(member, ptr):
        if isinstance(member, tuple):
            getattr(a, member[0])[member[1]] = ptr
        else:
            setattr(a, member, ptr)
    for member, tensor in t.items():
        point(member, tensor.data_ptr())
    for member, key in alias:
        point(member, t[key].data_ptr())
    for key, val in (extents or {}).items():
        setattr(a, key, val)
    for member in null:
        point(member, None)
    rc = abi_call(eng, "spc_les_mix", a)
    host = {k: x.cpu().numpy() for k, x in t.items()}
    return rc, host


# -- bodies ------------------------------------------------------------------------------------------------------------------
FIELD_SETS = [(), ("X",), ("U", "QR"), ("U", "V", "THL", "QT", "QR"), NAMES]      # 0, 1, 2, 5, 6 fields


def check_parity(eng, plane, ktot, n=3):
    """km, kmax and the outputs against the oracle with 0, 1, 2, 5 and 6 fields (U and V share one pair of vectors, QR and X have
    their own), with and without theta and kmax; the closure does something where a cell has different neighbours"""
    c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
    what = "n %d plane %s ktot %d" % (n, plane, ktot)
    for names in FIELD_SETS:
        km, kmax, outs = Run(eng, c, names).check("%s %d fields" % (what, len(names)))
    Run(eng, c, ("U", "QR"), theta=False, kmax=False).check(what + " bare")
    assert (km >= 0).all() and not numpy.signbit(km).any() and (km <= c["kcap"][:, None, None, None]).all()
    if max(plane) > 2:
        assert (km > 0).any() and (kmax > 0).all() and (outs["X"] != c["X"]).any()
    if max(plane) == 1:
        for k in NAMES:
            assert_bits("a plane of one cell keeps " + k, outs[k], field_of(c, k) + 0)


def check_rows(eng, ktot):
    """n = 1, 2, 5 at 3 x 5: gx, gy, kcap, ax, ay and the profiles differ per LES, so a wrong l or a swapped coefficient shows;
    then the same with pitched profiles"""
    for n in NS:
        for pad in (0, 3):
            c = case((n, 3, 5, ktot), np_of(eng), seed=1)
            assert (c["gx"] != c["gy"]).all() and (c["coef"]["U"][0] != c["coef"]["U"][1]).all()
            if n > 1:
                assert c["gx"][0] != c["gx"][1] and c["kcap"][0] != c["kcap"][1] and not numpy.array_equal(c["l2"][0], c["l2"][1])
            Run(eng, c, ("U", "THL", "QR"), pad=pad).check("rows n %d ktot %d pad %d" % (n, ktot, pad))


def strip_shapes(strip):
    """(n, itot, jtot, ktot) whose run jtot * ktot stands one below, at and one above a strip, for every itot of ROWS; the run as
    one level of many j once; and the smallest launch of many workgroups, which walks more rows"""
    out = []
    for run in (strip - 1, strip, strip + 1):
        jtot = next(q for q in (5, 4, 3, 2, 1) if run % q == 0)
        out += [(2, itot, jtot, run // jtot) for itot in ROWS]
        out.append((2, 3, run, 1))
    out.append((lar.MANY, 33, 1, 1))
    return out


def check_strips(eng):
    """the seams of both kernels: the flat run of a row at the strip - 1, + 0, + 1 (the j neighbours of a cell lie in another
    workgroup or across the wrap, the k neighbours of the first and last lane in the next workgroup), rows below, at and above
    what a workgroup walks, and both values of spc_les_advect_rows"""
    strip, rows = eng.advect_strip(2, 8, 8, 160)
    many_rows = eng.advect_strip(lar.MANY, 33, 1, 1)[1]
    assert strip >= 64 and 1 <= rows < many_rows <= 33
    for shape in strip_shapes(strip):
        Run(eng, case(shape, np_of(eng), seed=2), ("V", "QT")).check("strip %d x %d x %d x %d" % shape)
    return strip, rows, many_rows


def clamp_case(dtype, at, shape=(2, 3, 4, 9)):
    """winds and theta uniform on every level, so that the only deformation is the vertical shear, and the same on all levels
    but ``at`` (0 or ktot - 1), which alone differs from its neighbour: (case, the levels that may have km != 0)"""
    c = case(shape, dtype, seed=5)
    ktot = shape[3]
    for key, step in (("u", 3.0), ("v", -2.0), ("theta", 1.5 if at == 0 else -1.5)):          # (theta: unstable there)
        c[key][...] = c[key][:1, :1, :1, :1]
        c[key][..., at] += dtype(step)
    return c, ([0, 1] if at == 0 else [ktot - 2, ktot - 1])


def check_clamp(eng):
    """shear and unstable stratification only between the two lowest, then only between the two highest levels: km > 0 on those
    two levels (the clamped difference of the outer one is the one-sided one) and +0 on every other"""
    dtype = np_of(eng)
    for at in (0, -1):
        for theta in (True, False):
            c, live = clamp_case(dtype, at)
            km, kmax, _ = Run(eng, c, ("QT",), theta=theta).check("clamp at %d theta %s" % (at, theta))
            dead = [k for k in range(km.shape[3]) if k not in live]
            assert (km[..., live] > 0).all() and (kmax > 0).all()
            assert_bits("km away from the shear", km[..., dead], numpy.zeros_like(km[..., dead]))


def check_alignment(eng, leads, ktot=65, pad=0):
    """views 1 to 3 elements off the 16-byte grid, differently per array"""
    c = case((3, 2, 3, ktot), np_of(eng), seed=sum(leads) + 10 * pad)
    Run(eng, c, ("U", "THL", "X"), leads=leads, pad=pad).check("leads %s pad %d ktot %d" % (leads, pad, ktot))


def stable_case(dtype, shape=(2, 3, 4, 9)):
    """winds uniform on every level under a theta that rises with height: nothing to mix with; some field values are -0.0"""
    c = case(shape, dtype, seed=7)
    for key in ("u", "v", "theta"):
        c[key][...] = c[key][:, :1, :1, :1]
    c["theta"] += (0.3 * numpy.arange(shape[3])).astype(dtype)
    c["QR"][0, 0, 0, :] = -0.0
    return c


NAN_CELL = (0, 2, 3, 4)                                            # (l, i, j, k) of the cell that holds the NaN


def nan_reach(shape, key):
    """the cells whose stencil reads NAN_CELL of ``key``: for u the i, j and k neighbours (not the cell itself), for theta the k
    neighbours, for a field the cell and its four horizontal neighbours"""
    l, i, j, k = NAN_CELL
    m = numpy.zeros(shape, dtype=bool)
    if key in ("u", "X"):
        for d in (-1, 1):
            m[l, (i + d) % shape[1], j, k] = m[l, i, (j + d) % shape[2], k] = True
    if key in ("u", "theta"):
        m[l, i, j, k - 1] = m[l, i, j, k + 1] = True
    if key == "X":
        m[NAN_CELL] = True
    return m


def check_special(eng):
    """the uniform stable state keeps every bit and km is +0 with no sign bit set; an unstable theta at rest gives km > 0; one NaN
    in u, in theta and in a field reaches exactly the cells nan_reach names; kk = inf is capped"""
    dtype = np_of(eng)
    c = stable_case(dtype)
    km, kmax, outs = Run(eng, c).check("stable")
    assert_bits("stable: km", km, numpy.zeros_like(km))
    assert_bits("stable: kmax", kmax, numpy.zeros_like(kmax))
    for k in NAMES:
        assert_bits("stable: " + k, outs[k], field_of(c, k) + 0)     # (+ 0: a -0.0 comes out +0.0, as in K16)
    assert numpy.signbit(c["QR"]).any() and not numpy.signbit(outs["QR"]).any()
    c["theta"] -= (0.6 * numpy.arange(c["theta"].shape[3])).astype(dtype)
    km, kmax, _ = Run(eng, c).check("unstable at rest")
    assert (km > 0).all() and (kmax > 0).all()
    shape = (2, 5, 6, 7)
    c = case(shape, dtype, seed=8)
    clean = Run(eng, c, ("X", "QT")).check("clean")
    for key in ("u", "theta", "X"):
        s = dict(c, **{key: c[key].copy()})
        s[key][NAN_CELL] = numpy.nan
        r = Run(eng, s, ("X", "QT"))
        r.check("nan in " + key)
        km, kmax, outs = r.results()
        reach = nan_reach(shape, key)
        assert not numpy.isnan(km).any() and not numpy.isnan(kmax).any()
        if key == "X":
            assert_bits("a NaN field leaves km", km, clean[0])
            assert numpy.isnan(outs["X"][reach]).all() and not numpy.isnan(outs["X"][~reach]).any()
            assert_bits("the other cells of X", outs["X"][~reach], clean[2]["X"][~reach])
            assert_bits("the other field", outs["QT"], clean[2]["QT"])
        else:
            assert_bits("km where the NaN is read", km[reach], numpy.zeros_like(km[reach]))
            assert_bits("km elsewhere", km[~reach], clean[0][~reach])
            assert not numpy.isnan(outs["X"]).any() and not numpy.isnan(outs["QT"]).any()
    s = dict(c, u=c["u"].copy())
    s["u"][NAN_CELL] = numpy.inf
    km, kmax, _ = Run(eng, s, ("X",)).check("inf")
    assert numpy.isinf(kmax[0]) and (km <= c["kcap"][:, None, None, None]).all() and (km[0] == c["kcap"][0]).any()


def check_cap(eng):
    """a step so long that the cap binds in a known share of the cells: between a tenth and nine tenths; kmax is the uncapped
    maximum and lies above the cap"""
    c = case((2, 5, 6, 20), np_of(eng), seed=9, dt=3600.0)
    km, kmax, _ = Run(eng, c, ("U", "QT")).check("cap")
    kk = eddy(c["u"], c["v"], c["theta"], c["gx"], c["gy"], c["gz"], c["bz"], c["l2"], c["kcap"])[2]
    capped = kk >= c["kcap"][:, None, None, None]
    assert 0.1 < capped.mean() < 0.9 and (km[capped] == numpy.broadcast_to(c["kcap"][:, None, None, None], km.shape)[capped]).all()
    assert_bits("kmax is the uncapped maximum", kmax, kk.reshape(2, -1).max(axis=1))
    assert (kmax > c["kcap"]).all()
    return float(capped.mean())


INPUTS = ("u", "v", "theta", "gx", "gy", "kcap", "gz", "bz", "l2", ("fields", 0), ("fields", 1), ("ax", 0), ("ay", 1))
WRITTEN = ("km", "kmax", ("out", 0), ("out", 1))


def check_refusals(eng):
    """n = 0 is a no-op; pitch_prof < ktot, a NULL required pointer, theta without bz, km, kmax or an out[f] equal to an input or
    to each other and n_fields outside 0 ... 6 are refused by the library; the engine refuses the same; no refused call writes"""
    dtype = np_of(eng)
    c = case((2, 2, 3, 8), dtype, seed=13)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731

    def untouched(host, but=()):
        for k, fill in (("km", OUT_FILL), ("kmax", -5.0), (("out", 0), OUT_FILL), (("out", 1), OUT_FILL)):
            assert k in but or (host[k] == fill).all(), k
        for k in ("u", "v", "theta"):
            assert_bits("refused: " + k, host[k], c[k])
    rc, host = raw_launch(eng, c, extents=dict(n_les=0))
    assert rc == 0
    untouched(host)
    rc, host = raw_launch(eng, c, null=("theta", "bz", "kmax"))
    want = oracle(c, ("U", "QT"), theta=False)
    assert rc == 0 and (host["kmax"] == -5.0).all()
    assert_bits("without theta: km", host["km"], want[0])
    assert_bits("without theta: out", host[("out", 1)], want[2]["QT"])
    rc, host = raw_launch(eng, c)
    want = oracle(c, ("U", "QT"))
    assert rc == 0
    for got, w in ((host["km"], want[0]), (host["kmax"], want[1]), (host[("out", 0)], want[2]["U"]), (host[("out", 1)], want[2]["QT"])):
        assert_bits("raw", got, w)
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    bad = [(dict(extents=dict(pitch_prof=7)), b"pitch_prof"), (dict(extents=dict(n_fields=-1)), b"field count"),
           (dict(extents=dict(n_fields=7)), b"field count"), (dict(null=("bz",)), b"theta without bz")]
    bad += [(dict(alias=((out_, key),)), b"also an input") for out_ in WRITTEN for key in INPUTS]
    bad += [(dict(alias=((WRITTEN[y], WRITTEN[x]),)), b"same array") for x in range(4) for y in range(x + 1, 4)]
    bad += [(dict(null=(k,)), b"required pointer " + k.encode()) for k in ("u", "v", "gx", "gy", "kcap", "gz", "l2", "km")]
    bad += [(dict(null=((k, 1),)), b"required pointer " + k.encode() + b"[f]") for k in ARRAYS]
    for kw, text in bad:
        rc, host = raw_launch(eng, c, **kw)
        assert rc == E and text in eng.lib.spc_last_error(), (kw, rc, eng.lib.spc_last_error())
        untouched(host, but=[m for m, _ in kw.get("alias", ())] + list(kw.get("null", ())))
    t = {k: dev(c[k]) for k in ("u", "v", "theta", "gx", "gy", "kcap", "gz", "bz", "l2", "QT")}
    ax, ay = {k: dev(c["coef"][k][0]) for k in ("U", "QT")}, {k: dev(c["coef"][k][1]) for k in ("U", "QT")}
    fields = {"U": t["u"], "QT": t["QT"]}
    fresh = lambda: torch.full_like(t["u"], OUT_FILL)                                          # noqa: E731
    km, out = fresh(), {"U": fresh(), "QT": fresh()}

    def call(fields=fields, out=out, km=km, ax=ax, ay=ay, kmax=True, **kw):
        a = dict(t, **kw)
        return eng.les_mix(fields, out, a["u"], a["v"], a["theta"], a["gx"], a["gy"], a["gz"], a["bz"], a["l2"], a["kcap"], km, ax, ay, kmax=kmax)
    empty = lambda x: x[:0]                                                                    # noqa: E731
    assert eng.les_mix({}, {}, empty(t["u"]), empty(t["v"]), None, empty(t["gx"]), empty(t["gy"]), empty(t["gz"]), None, empty(t["l2"]),
                       empty(t["kcap"]), empty(km), {}, {}) is not None
    other = torch.float64 if eng.dtype == torch.float32 else torch.float32
    seven = {str(i): t["QT"] for i in range(7)}
    for bad_call in (lambda: call(km=t["u"]), lambda: call(km=t["QT"]), lambda: call(out={"U": km, "QT": out["QT"]}),
                     lambda: call(out={"U": out["QT"], "QT": out["QT"]}), lambda: call(out={"U": t["theta"], "QT": out["QT"]}),
                     lambda: call(kmax=t["gx"]), lambda: call(kmax=ax["U"]), lambda: call(bz=None), lambda: call(out={"U": out["U"]}),
                     lambda: call(ax={"U": ax["U"]}), lambda: call(ay={"U": ay["U"], "X": ay["QT"]}),
                     lambda: call(fields=seven, out=seven, ax=seven, ay=seven), lambda: call(gx=t["gx"][:1]),
                     lambda: call(l2=t["l2"][:, :4]), lambda: call(km=km[..., ::2]), lambda: call(km=km.to(other)),
                     lambda: call(u=t["u"].cpu())):
        try:
            bad_call()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad call was not refused")
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    for k in ("u", "v", "theta", "QT"):
        assert_bits("refused: " + k, t[k].cpu().numpy(), c[k])
    assert (km == OUT_FILL).all() and (out["U"] == OUT_FILL).all() and (out["QT"] == OUT_FILL).all()


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    c = case((n, 3, 4, 40), np_of(one), seed=n)
    names = ("U", "THL", "QR")
    km, kmax, outs = oracle(c, names)
    for tag, eng, up in on_both(one, multi, n):
        t = {k: up(c[k]) for k in ("u", "v", "theta", "gx", "gy", "kcap", "gz", "bz", "l2", "QR")}
        fields = {"U": t["u"], "THL": t["theta"], "QR": t["QR"]}
        out = {k: up(numpy.full_like(c["u"], OUT_FILL)) for k in names}
        dkm = up(numpy.full_like(c["u"], OUT_FILL))
        ax, ay = {k: up(c["coef"][k][0]) for k in names}, {k: up(c["coef"][k][1]) for k in names}
        got = eng.les_mix(fields, out, t["u"], t["v"], t["theta"], t["gx"], t["gy"], t["gz"], t["bz"], t["l2"], t["kcap"], dkm, ax, ay)
        multi.synchronize()
        assert_bits("%s km" % tag, host_of(dkm), km)
        assert_bits("%s kmax" % tag, host_of(got), kmax)
        for k in names:
            assert_bits("%s out %s" % (tag, k), host_of(out[k]), outs[k])
    return blocks_of(t["u"], multi, n)


BODIES = ("parity", "rows", "strips", "clamp", "alignment", "special", "cap", "refusals")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in (1, 2, 65)]),
            ("rows", lambda: [check_rows(eng, k) for k in (2, 65)]),
            ("strips", lambda: check_strips(eng)),
            ("clamp", lambda: check_clamp(eng)),
            ("alignment", lambda: [check_alignment(eng, *a) for a in (((1, 2, 3), 65, 0), ((3, 0, 1, 2), 64, 0), ((2, 3, 1, 1, 0), 7, 5))]),
            ("special", lambda: check_special(eng)),
            ("cap", lambda: check_cap(eng)),
            ("refusals", lambda: check_refusals(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_mix (CPU suite) -------------------------------------------------------------------------
class MixOracleEngine(lfr.FullOracleEngine):
    """tests/les_full_ref.FullOracleEngine with ``les_mix`` by the NumPy oracle above: km and the outputs written whole into the
    caller's tensors, as the HIP engine does"""

    def les_mix(self, fields, out, u, v, theta, gx, gy, gz, bz, l2, kcap, km, ax, ay, kmax=True, **kw):
        want = kmax is not None and kmax is not False
        names = list(fields)
        if sorted(out) != sorted(names) or sorted(ax) != sorted(names) or sorted(ay) != sorted(names):
            raise ValueError("out, ax or ay do not hold the names of the fields")
        written = [t.data_ptr() for t in [km, kmax if want and kmax is not True else None] + [out[k] for k in names] if t is not None]
        read = {t.data_ptr() for t in [u, v, theta, gx, gy, kcap, gz, bz, l2] + [fields[k] for k in names] if t is not None}
        if u.shape[0] and (len(set(written)) != len(written) or set(written) & read):
            raise ValueError("km, kmax or an output is an input or another of them")
        c = lambda t: None if t is None else numpy.ascontiguousarray(t.numpy())                 # noqa: E731
        m, top, new = les_mix({k: c(fields[k]) for k in names}, c(u), c(v), c(theta), c(gx), c(gy), c(gz), c(bz), c(l2), c(kcap),
                              {k: c(ax[k]) for k in names}, {k: c(ay[k]) for k in names})
        km.copy_(torch.from_numpy(m))
        for k in names:
            out[k].copy_(torch.from_numpy(new[k]))
        if not want:
            return None
        top = torch.from_numpy(top)
        return top if kmax is True else kmax.copy_(top)


# -- the host twins of models.DeviceLESEnsemble after enable_mixing() -------------------------------------------------------------
class _HostMix:
    """NumPy fields: the executable definition of what evolve_model_batched does after enable_mixing(): behind the advection
    and in front of K15, ONE les_mix on the fields among U, V (the winds' coefficients) and THL, QT, QR (the scalars') that
    exist, theta = THL (``stability=False``: none); with ``vertical=True`` K15's face diffusivity is k_bg + the mean of the slab
    means of km of the two levels of a face.

    The twins below have no step with a place to hang the mixing on where no advection is enabled (each spells its sequence out
    in its own evolve_model_batched, as tests/les_radiate_ref.py's does for K18), so with enable_mixing() this class spells the
    sequence out once more: the tendencies, the transport (the twin's own ``_advect``: K16 / K17 / K22 / K23 with K21), K24,
    K15, K18, K14 and the tail, each by the oracle of its module.  A change of that order has to be made here as well.  K19 is
    NOT part of this sequence and is not left out either: in the classes below ``_HostQtLocal`` stands ABOVE this mixin, does
    the step and K19 itself and then calls this method with the tendencies taken away, as it does with every twin under it
    (the variant "forced" of VARIANTS runs K19 and K21 with the mixing).  Without enable_mixing() the step is the twin's below."""

    MIX_KEYS = ("U", "V", "THL", "QT", "QR")
    mix_par = None
    mixing_k_max = mixing_capped = None
    _km = _mix_kd = None

    def enable_mixing(self, cs=None, prandtl=None, cap=None, theta_ref=None, stability=True, dx=None, dy=None, vertical=False):
        if vertical and self.diffuse_par is None:
            raise ValueError("vertical=True needs enable_diffusion()")
        adv_par = getattr(self, "advect_par", None)
        self.mix_par = dict(cs=mix.CS if cs is None else cs, prandtl=mix.PRANDTL if prandtl is None else prandtl,
                            cap=mix.CAP if cap is None else cap, theta_ref=mix.THETA_REF if theta_ref is None else theta_ref,
                            stability=stability, vertical=vertical,
                            dx=dx if dx is not None else adv_par["dx"] if adv_par else adv.DX,
                            dy=dy if dy is not None else adv_par["dy"] if adv_par else adv.DY)
        self._km = self._mix_kd = None
        self.mixing_k_max = self.mixing_capped = None             # (a second call forgets the last step of the earlier one)

    def _mix(self, dt):
        f, par = self.fields3d, self.mix_par
        T = f["U"].dtype
        gx, gy, wind, scalar = mix.coefficients(dt, par["dx"], par["dy"], par["prandtl"], n=self.n)
        kcap = mix.cap(wind, scalar, par["cap"])
        gz, bz, l2 = mix.profiles(self.zf_cache, self.zh_cache, par["dx"], par["dy"], par["cs"], par["prandtl"], par["theta_ref"], n=self.n)
        r = lambda a: numpy.ascontiguousarray(a.astype(T))                                   # noqa: E731
        keys = [k for k in self.MIX_KEYS if k in f]
        coef = {k: (r(wind[0]), r(wind[1])) if k in WINDS else (r(scalar[0]), r(scalar[1])) for k in keys}
        theta = f["THL"] if par["stability"] and "THL" in f else None
        self._km, kmax, new = les_mix({k: f[k] for k in keys}, f["U"], f["V"], theta, r(gx), r(gy), r(gz), r(bz), r(l2), r(kcap),
                                      {k: coef[k][0] for k in keys}, {k: coef[k][1] for k in keys})
        f.update(new)
        self.mixing_k_max = float(kmax.max())
        self.mixing_capped = self.mixing_k_max > float(r(kcap).min())
        if par["vertical"]:
            m = numpy.asarray(slab_ref.slab_means(self._km), dtype=numpy.float64)
            faces = numpy.concatenate([m[:, :1], 0.5 * (m[:, :-1] + m[:, 1:])], axis=1)          # (the ground's entry is not used)
            self._mix_kd = self.diffuse_par["k_bg"] + faces

    def get_eddy_viscosity_batched(self):
        return self._km

    def evolve_model_batched(self, t):
        from sp_coupler_amd import radiation as rad
        from sp_coupler_amd import thermo
        from tests import les_diffuse_ref as ldr
        from tests import les_thermo_ref as ltr
        dt = float(t) - self.model_time
        if dt <= 0:
            return
        if self.mix_par is None:
            return super().evolve_model_batched(t)
        f, p = self.fields3d, self.p
        self._step(dt)
        if "PS" in self.tend:
            p["PS"] = p["PS"] + dt * self.tend["PS"]
        if self.advect_par is not None:
            self._advect(dt)
        self._mix(dt)
        if self.diffuse_par is not None:
            kd = self._mix_kd if self.mix_par["vertical"] else None
            a, m, cp, s0 = (self._r(x) for x in dif.profiles(self.zh_cache, self.zf_cache, p["Rhobf"], dt, kd=kd, **self.diffuse_par))
            for key, slot in (("U", None), ("V", None), ("THL", "wt"), ("QT", "wq")):
                if key in f:
                    flux = self._r(numpy.asarray(self.tend[slot], dtype=numpy.float64).reshape(self.n)) if slot in self.tend else None
                    f[key] = ldr.les_diffuse(f[key], a, m, cp, s0 if flux is not None else None, flux)
        self._follow()
        if self.radiate_par is not None:
            par = self.radiate_par
            w, c = (self._r(x) for x in rad.profiles(p["Rhobf"], self.zh_cache, p["presf"], dt, par["kappa"]))
            f["THL"], self._flux, _ = lrr.les_radiate(f["QL"], f["THL"], w, c, self._r(par["f0"]), self._r(par["f1"]), rad.exp_table(self.dtype))
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


class HostMixLESEnsemble(lfr._HostFull, lfr.qlr._HostQtLocal, _HostMix, lfr.lt2._HostTransport2, lfr.lbr.HostBuoyancyLESEnsemble):
    """the bases of tests/les_full_ref.HostFullLESEnsemble with the mixing below its K19 (which runs first, on the stepped
    fields) and above its transport (whose ``_advect`` the mixing's step calls, then K24, then K15): QL = max(QT - Qsat, 0)"""


class HostThermoMixLESEnsemble(lfr._HostFull, lfr.qlr._HostQtLocal, _HostMix, lfr.lt2._HostTransport2, lfr.lbr.HostThermoBuoyancyLESEnsemble):
    """after enable_thermo(): K12's oracle wherever QL is read"""


VARIANTS = {"plain": dict(), "all": dict(diffuse=True, radiate=True, thermo=True, micro=True, transport=True),
            "forced": dict(diffuse=True, thermo=True, transport=True, qt="strong", buoyancy=True)}
DX = 250.0


def ensemble_run(engine, n, device, mixing=True, vertical=False, thermo=False, micro=False, diffuse=False, radiate=False, transport=False,
                 qt=None, buoyancy=False, itot=4, jtot=5, nL=20, steps=3):
    """an ensemble with attached U, V, THL, QT (and Qsat, or thermo; QR with the microphysics) and enable_mixing() (``mixing``
    None: never called, and the host twin is tests/les_full_ref's) through ``steps`` calls of evolve_model_batched and one
    variability nudge (constantT) before the last; ``transport``: the conservative second-order transport (K23) in front of it;
    ``qt``: the kind of K19's forcing, which then runs first in every step; ``buoyancy``: K21 in front of every substep.
    After each of them every profile, the fields, km and the largest viscosity.  Returns (ens, list of records)"""
    if device:
        cls = models.DeviceLESEnsemble
    elif mixing:
        cls = HostThermoMixLESEnsemble if thermo else HostMixLESEnsemble
    else:
        cls = lfr.HostThermoFullLESEnsemble if thermo else lfr.HostFullLESEnsemble

    def enable(ens):
        if qt:
            ens.enable_qt_forcing(qt)
        if buoyancy:
            ens.enable_buoyancy()
        if mixing:
            ens.enable_mixing(vertical=vertical, **({} if transport else {"dx": DX, "dy": 1.5 * DX}))

    def record(ens, rec):
        if mixing:
            km = ens.get_eddy_viscosity_batched()
            rec["km"] = numpy.zeros(rec["field U"].shape) if km is None else numpy.array(host_of(km))
            rec["k max"] = numpy.array([-1.0 if ens.mixing_k_max is None else ens.mixing_k_max, float(bool(ens.mixing_capped))])
        if qt:
            counts = ens.get_qt_forcing_counts_batched()
            rec["counts"] = numpy.zeros((n, nL)) if counts is None else numpy.array(host_of(counts), dtype=numpy.float64)

    def before(ens):
        assert not mixing or (ens.get_eddy_viscosity_batched() is None and ens.mixing_k_max is None)
    advection = dict(dx=DX, dy=1.5 * DX, vertical=True, conservative=True, order=2) if transport else None
    forcings = (lambda rng, stack: dict(QL=rng.normal(0, 2e-8, (n, nL)), QLp=stack("ql_ref") * (0.5 + rng.random((n, nL))))) if qt else None
    return ensemble_case(engine, n, cls, thermo=thermo, micro=micro, diffuse=diffuse, advection=advection, forcings=forcings,
                         radiation=lrr.radiation_of(n, "f0", "f1") if radiate else None, enable=enable, record=record, before=before,
                         itot=itot, jtot=jtot, nL=nL, steps=steps)


def check_ensemble(one, engines, n, variant, vertical=False):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``: every profile, field and km bit-equal
    after each step; the mixing changes U: the twin's last step differs from the same run without enable_mixing(), whose device
    run is bit-equal to tests/les_full_ref's twin"""
    kw = dict(VARIANTS[variant], vertical=vertical)
    host = ensemble_run(one, n, False, **kw)[1]
    plain = ensemble_run(one, n, False, mixing=None, **kw)[1]
    assert (host[-1]["field U"] != plain[-1]["field U"]).any() and (host[-1]["km"] > 0).any()      # (a stable first step may mix nothing)
    assert all(numpy.isfinite(r["k max"][0]) for r in host) and host[-1]["k max"][0] > 0
    for engine in engines:
        lmr.same_logs(host, ensemble_run(engine, n, True, **kw)[1])
    lmr.same_logs(plain, ensemble_run(engines[0], n, True, mixing=None, **kw)[1])
    return host
