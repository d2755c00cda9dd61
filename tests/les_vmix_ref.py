"""NumPy oracle of K25 (include/spc.h: spc_les_vmix_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_vmix_gpu.py (each takes an engine: tools/mutation_control.py --vmix hands them the engines of its mutant libraries),
the host twins of models.DeviceLESEnsemble's vertical-mixing mode and an oracle-backed engine with ``les_vmix`` for the CPU suite.

The oracle spells the rule out with a loop over k, vectorised over the columns, one statement per rounding in the element type,
so nothing fuses.  Every device array of the bodies is the LEADING part of a poisoned buffer (tests/les_harness.Poisoned); the
bytes behind it (and in front of a view off the 16-byte grid) are checked after the launch."""
import numpy
import torch

from sp_coupler_amd import _abi, models
from sp_coupler_amd import mixing as mix
from sp_coupler_amd import vertical_mixing as vm
from tests import les_full_ref as lfr
from tests import les_mix_ref as lxr
from tests import les_radiate_ref as lrr
from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, cols_table, ensemble_case, host_of, np_of, on_both, run_bodies)

#: (n, plane): 1 to 3 LES of 3 x 5 (a tile of 16, 32 or 64 columns spans several LES) and of 8 x 8 columns (an LES is a tile or more)
PLANES = [(1, (3, 5)), (2, (8, 8)), (3, (3, 5)), (3, (8, 8))]
#: one level (no face), two (no interior level), three (one), below a chunk of the sweeps (7), a whole number of chunks behind
#: level 0 (64: 1 + 7 * 8 + 7), the flagship's 160 and an odd 161
KTOTS = [1, 2, 3, 7, 64, 160, 161]
#: the fields of a case in the order of a launch
NAMES = ("U", "V", "THL", "QT", "QR", "X")
WINDS = ("U", "V")
FLUXED = ("THL", "QT")
DT = 60.0
KV_CAP = 20.0
SPEED_FILL = -7.0


# -- the rule --------------------------------------------------------------------------------------------------------------
def speed(u, v):
    """sp [n x itot x jtot] of the winds' lowest level"""
    with numpy.errstate(all="ignore"):
        u0, v0 = u[..., 0], v[..., 0]
        uu = u0 * u0
        vv = v0 * v0
        e = uu + vv
        sp = numpy.sqrt(e)
    assert sp.dtype == u.dtype
    return sp


def faces(km, kb, kv2):
    """s [n x itot x jtot x ktot]: twice the diffusivity of face k = 1 ... ktot - 1 (entry 0 is +0 and stands for no face)"""
    T = km.dtype.type
    assert kb.dtype == km.dtype == kv2.dtype
    s = numpy.zeros_like(km)
    cap = kv2[:, None, None, None]
    with numpy.errstate(all="ignore"):
        h = km[..., :-1] + km[..., 1:]
        t = h + kb[:, None, None, 1:]
        t = numpy.where(t > 0, t, T(0))                            # a NaN or a negative sum gives +0
        s[..., 1:] = numpy.where(t < cap, t, cap)
    return s


def vmix(x, s, el, eu, s0=None, flux=None, dr=None, sp=None):
    """x' of the field ``x`` [n x itot x jtot x ktot] with the faces ``s``, el and eu [n x ktot], the flux [n] (with s0 [n]) or None
    and the drag [n] (with the plane sp) or None; a new array"""
    T = x.dtype.type
    assert x.dtype == s.dtype == el.dtype == eu.dtype and (flux is None or flux.dtype == s0.dtype == x.dtype)
    assert dr is None or dr.dtype == sp.dtype == x.dtype
    ktot = x.shape[3]
    P = lambda a, k: a[:, None, None, k]                                                   # noqa: E731
    one, zero = T(1), numpy.zeros(x.shape[:3], dtype=x.dtype)
    q, y = numpy.empty_like(x), numpy.empty_like(x)
    with numpy.errstate(all="ignore"):
        for k in range(ktot):
            lo = P(el, k) * s[..., k] if k > 0 else zero
            up = P(eu, k) * s[..., k + 1] if k + 1 < ktot else zero
            b = one + lo
            b = b + up
            d = x[..., k]
            if k == 0:
                if dr is not None:
                    g = dr[:, None, None] * sp
                    b = b + g
                if flux is not None:
                    t = s0 * flux
                    d = d + t[:, None, None]
                m = one / b
                y[..., 0] = d * m
            else:
                lq = lo * q[..., k - 1]
                den = b - lq
                m = one / den
                ly = lo * y[..., k - 1]
                r = d + ly
                y[..., k] = r * m
            q[..., k] = up * m
        out = numpy.empty_like(x)
        out[..., ktot - 1] = y[..., ktot - 1]
        for k in range(ktot - 2, -1, -1):
            t = q[..., k] * out[..., k + 1]
            out[..., k] = y[..., k] + t
    assert out.dtype == x.dtype
    return out


def les_vmix(fields, km, el, eu, kb, kv2, s0=None, flux=None, drag=None, u=None, v=None):
    """(dict name -> the mixed field, sp or None), new arrays; ``el`` and ``eu`` dicts with the names of ``fields``, ``flux`` and
    ``drag`` dicts with some of them"""
    flux, drag = flux or {}, drag or {}
    sp = speed(u, v) if drag else None
    s = faces(km, kb, kv2)
    return {k: vmix(x, s, el[k], eu[k], s0, flux.get(k), drag.get(k), sp) for k, x in fields.items()}, sp


# -- inputs ------------------------------------------------------------------------------------------------------------------
def case(shape, dtype, seed=0, dt=DT, kv_cap=KV_CAP, k_bg=vm.K_BG):
    """dict of the arguments in ``dtype``: the fields U, V, THL, QT, QR and X, km, kb, kv2, s0, dr, ``flux``: name -> [n] (THL, QT)
    ``coef``: name -> (el, eu) and ``w``, the float64 weights Rhobf dz.  Another grid, density and roughness per LES; U and V share the winds' pair of profiles, THL
    and QT the scalars', QR and X have a pair of their own each (another Prandtl number); km is +0 in a fifth of the cells and
    reaches above the cap in others"""
    dtype = numpy.dtype(dtype).type
    n, itot, jtot, ktot = shape
    rng = numpy.random.default_rng(25000 + seed + 7 * ktot + itot * jtot + 31 * n)
    rhobf, zh, zf, _, _ = lrr.grid(n, ktot, rng)
    k = numpy.arange(ktot)
    c = dict(U=5.0 + rng.standard_normal(shape), V=-2.0 + rng.standard_normal(shape),
             THL=290.0 + 10.0 * k / 160.0 + 0.5 * rng.standard_normal(shape),
             QT=8e-3 * numpy.exp(-k / 160.0) * (1.0 + 0.05 * rng.standard_normal(shape)), QR=1e-5 * rng.random(shape),
             X=rng.standard_normal(shape), km=30.0 * rng.random(shape) ** 2 * (rng.random(shape) > 0.2))
    wind, scalar, c["s0"] = vm.coefficients(zh, zf, rhobf, dt)
    own = [vm.coefficients(zh, zf, rhobf, dt, prandtl=pr)[1] for pr in (0.5, 0.8)]
    c["kb"], c["kv2"] = vm.background(n, ktot, k_bg * (1.0 + 0.1 * rng.random((n, ktot))), kv_cap * (1.0 + 0.1 * numpy.arange(n)))
    c["dr"] = vm.drag(0.01 * (1.0 + numpy.arange(n)), zf, 2.0 * (zf - zh), dt)
    flux = {"THL": 0.12 * (0.5 + rng.random(n)), "QT": 6e-5 * (0.5 + rng.random(n))}
    c = {key: numpy.ascontiguousarray(a.astype(dtype)) for key, a in c.items()}
    pairs = [tuple(numpy.ascontiguousarray(a.astype(dtype)) for a in p) for p in (wind, scalar) + tuple(own)]
    c["coef"] = {"U": pairs[0], "V": pairs[0], "THL": pairs[1], "QT": pairs[1], "QR": pairs[2], "X": pairs[3]}
    c["flux"] = {key: numpy.ascontiguousarray(a.astype(dtype)) for key, a in flux.items()}
    c["w"] = rhobf * (2.0 * (zf - zh))                              # float64 [n x ktot]: the weights of the conserved column sum
    return c


def oracle(c, names=NAMES, flux=True, drag=True):
    """(dict name -> x', sp or None) of the case: the fluxes of THL and QT and the drag of U and V where asked and launched"""
    fl = {k: c["flux"][k] for k in names if flux and k in c["flux"]}
    dg = {k: c["dr"] for k in names if drag and k in WINDS}
    return les_vmix({k: c[k] for k in names}, c["km"], {k: c["coef"][k][0] for k in names}, {k: c["coef"][k][1] for k in names},
                    c["kb"], c["kv2"], c["s0"], fl, dg, c["U"], c["V"])


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one call of ``eng.les_vmix`` with every array inside a poisoned buffer; ``check`` compares every field and the speed plane
    with the oracle bit for bit, the read-only inputs with what was uploaded, and looks at the bytes around every array.
    ``leads``: elements in front of the 4-D arrays, taken in turn (the fields, u and v where they are no fields, km); ``pad``:
    elements between the rows of the profiles.  Arrays that are one object in the case (the profiles two fields share) are one
    device tensor; u and v are the fields U and V where those are launched."""

    def __init__(self, eng, c, names=NAMES, flux=True, drag=True, leads=(0,), pad=0):
        self.eng, self.c, self.names, self.flux, self.drag = eng, c, tuple(names), flux, drag
        self.mem = Poisoned(eng)
        self.inputs, seen, turn = [], {}, [0]

        def lead():
            turn[0] += 1
            return leads[(turn[0] - 1) % len(leads)]

        def put(tag, a, poison, ld=0, rows=False):
            if id(a) not in seen:
                seen[id(a)] = self.mem.rows(tag, a, poison, pad=pad) if rows else self.mem.put(tag, a, poison, ld)
                self.inputs.append((tag, seen[id(a)], a))
            return seen[id(a)]
        nan = float("nan")
        self.dfields = {k: self.mem.put(k, c[k], nan, lead()) for k in self.names}
        wind = drag and any(k in WINDS for k in self.names)
        self.du = self.dv = self.dspeed = None
        if wind:
            self.du = self.dfields["U"] if "U" in self.names else put("u", c["U"], nan, lead())
            self.dv = self.dfields["V"] if "V" in self.names else put("v", c["V"], nan, lead())
            self.dspeed = self.mem.put("speed", numpy.full(c["U"].shape[:3], SPEED_FILL, dtype=c["U"].dtype), 1e30)
        self.dkm = put("km", c["km"], nan, lead())
        self.dkb = put("kb", c["kb"], 1e30, rows=True)
        self.dkv2, self.ds0 = put("kv2", c["kv2"], 1e30), put("s0", c["s0"], 1e30)
        self.del_ = {k: put("el " + k, c["coef"][k][0], 1e30, rows=True) for k in self.names}
        self.deu = {k: put("eu " + k, c["coef"][k][1], 1e30, rows=True) for k in self.names}
        self.dflux = {k: put("flux " + k, c["flux"][k], 1e30) for k in self.names if flux and k in c["flux"]}
        self.ddrag = {k: put("dr", c["dr"], 1e30) for k in self.names if drag and k in WINDS}
        eng.les_vmix(self.dfields, self.dkm, self.del_, self.deu, self.dkb, self.dkv2, s0=self.ds0, flux=self.dflux, drag=self.ddrag,
                     u=self.du, v=self.dv, speed=self.dspeed)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def results(self):
        """(dict name -> x', speed or None) on the host"""
        return {k: t.cpu().numpy() for k, t in self.dfields.items()}, None if self.dspeed is None else self.dspeed.cpu().numpy()

    def check(self, what=""):
        outs, sp = want = oracle(self.c, self.names, self.flux, self.drag)
        got, got_sp = self.results()
        for k in self.names:
            assert_bits("%s field %s" % (what, k), got[k], outs[k])
        if sp is not None:
            assert_bits("%s speed" % what, got_sp, sp)
        for tag, t, a in self.inputs:
            assert Poisoned.read_only(t, a), (what, tag, "read only")
        self.mem.check_around(what)
        return want


FIELD_ARRAYS = ("fields", "flux", "dr", "el", "eu")


def raw_launch(eng, c, names=("U", "QT", "X"), alias=(), extents=None, null=(), offset=()):
    """spc_les_vmix_* itself: (rc, dict member -> the array on the host afterwards).  Every member is a tensor of its own: U has a
    drag, QT a flux, X neither; u and v are tensors of their own.  ``alias``: (member, key) pairs that replace a pointer member by
    that of tensor ``key``, a member or key of an array spelled ("el", 0); ``extents``: overrides of the scalar members;
    ``null``: members set to NULL; ``offset``: members whose pointer is moved one byte"""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    n, itot, jtot, ktot = c["U"].shape
    t = {k: dev(c[k]) for k in ("km", "kb", "kv2", "s0")}
    t["u"], t["v"] = dev(c["U"]), dev(c["V"])
    t["speed"] = dev(numpy.full(c["U"].shape[:3], SPEED_FILL, dtype=c["U"].dtype))
    for f, k in enumerate(names):
        t[("fields", f)] = dev(c[k])
        t[("el", f)], t[("eu", f)] = dev(c["coef"][k][0]), dev(c["coef"][k][1])
        if k in c["flux"]:
            t[("flux", f)] = dev(c["flux"][k])
        if k in WINDS:
            t[("dr", f)] = dev(c["dr"])
    a = _abi.LesVmixArgs()
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
    for member in offset:
        point(member, t[member].data_ptr() + 1)
    rc = abi_call(eng, "spc_les_vmix", a)
    return rc, {k: x.cpu().numpy() for k, x in t.items()}


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, ktot):
    """six fields with the fluxes and the drag against the oracle, 1 to 3 LES of 3 x 5 and 8 x 8 columns; the mixing does
    something, and the cap binds at some faces and not at others"""
    for n, plane in PLANES:
        c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
        outs, sp = Run(eng, c).check("n %d plane %s ktot %d" % (n, plane, ktot))
        assert (sp > 0).all()
        for k in NAMES:
            assert (outs[k] != c[k]).any() or (ktot == 1 and k not in WINDS + FLUXED)
        if ktot >= 7:
            s = faces(c["km"], c["kb"], c["kv2"])[..., 1:]
            top = numpy.broadcast_to(c["kv2"][:, None, None, None], s.shape)
            assert (s == top).any() and (s < top).any() and (s > 0).all()


def check_tiles(eng):
    """LES of 2 x 3 columns: 7 of them are 42 columns, no multiple of any C, and a tile of 16 spans three LES; ktot on both sides
    of every change of C = 64, 32, 16, at the largest supported ktot, and the first unsupported ktot refused"""
    dtype = np_of(eng)
    first, changes, bad = cols_table(eng.vmix_cols_per_block)
    assert sorted(first) == [16, 32, 64] and len(changes) == 2
    for ktot in changes:
        for k in (ktot - 1, ktot):
            assert eng.vmix_cols_per_block(k) == (eng.vmix_cols_per_block(ktot) * (2 if k < ktot else 1))
            Run(eng, case((7, 2, 3, k), dtype, seed=3), ("U", "THL", "X")).check("7 LES of 2 x 3 around the change at ktot %d: %d" % (ktot, k))
    for cols in (1, 3):
        Run(eng, case((cols, 2, 3, bad - 1), dtype, seed=4), ("V", "QT")).check("%d LES at the last ktot %d" % (cols, bad - 1))
    try:
        Run(eng, case((1, 2, 3, bad), dtype, seed=5), ("V", "QT"))
    except _abi.SpcError as e:
        assert e.code == _abi.SPC_ERR_UNSUPPORTED and str(bad - 1) in str(e), str(e)
    else:
        raise AssertionError("ktot %d was not refused" % bad)
    return first, changes, bad


def check_alignment(eng, leads, ktot=65, pad=0):
    """views 1 to 3 elements off the 16-byte grid, differently per array; pitched profiles"""
    c = case((3, 2, 3, ktot), np_of(eng), seed=sum(leads) + 10 * pad)
    Run(eng, c, ("U", "THL", "X"), leads=leads, pad=pad).check("leads %s pad %d ktot %d" % (leads, pad, ktot))


COLTILE_KTOTS = (1, 2, 7, 8, 9, 17)


def check_coltile(eng):
    """the cases of the column tile (spc_coltile.hpp) together: 3 LES of 3 x 5 (one partial tile that spans three LES, more than
    DIF_STAGE) and 6 of them (a whole 64-column tile that spans five LES, then a partial one); ktot 1, 2, 7, 8, 9 and 17, and at
    n = 3 the last ktot of every C and the first of the next; the six fields and km led by 0 ... V - 1 elements, equally and each another way;
    the bytes around every array are looked at by Run.check"""
    dtype = np_of(eng)
    V = 16 // numpy.dtype(dtype).itemsize
    for n in (3, 6):
        for ktot in COLTILE_KTOTS:
            for leads in [(lead,) for lead in range(V)] + [tuple(range(1, V)) + (0,)]:
                Run(eng, case((n, 3, 5, ktot), dtype, seed=11 + sum(leads)), leads=leads).check("coltile n %d ktot %d leads %s" % (n, ktot, leads))
    first, changes, bad = cols_table(eng.vmix_cols_per_block)
    for ktot in [k for c in changes for k in (c - 1, c)] + [bad - 1]:
        for leads in ((0,), (1,)):
            Run(eng, case((3, 3, 5, ktot), dtype, seed=12), ("U", "THL", "X"), leads=leads).check("coltile C %d ktot %d leads %s" % (eng.vmix_cols_per_block(ktot), ktot, leads))


COLUMN = (1, 2, 1)                                                 # (l, i, j) of the column that is special


def check_viscosity(eng):
    """km NaN, negative, infinite and at the cap give the faces the rule names; km = 0 with kb = 0 keeps every value of a finite
    column; calm columns (km = 0, kb = 0) beside one column of large km keep every value while that column mixes: what a slab
    mean of km cannot do"""
    dtype = np_of(eng)
    shape = (2, 3, 4, 9)
    c = case(shape, dtype, seed=6)
    c["km"][0, 0, 0, 2], c["km"][0, 0, 1, 3], c["km"][0, 1, 0, 4] = numpy.nan, -50.0, numpy.inf
    c["km"][1, 0, 0, 5] = c["km"][1, 0, 0, 6] = c["kv2"][1] / 2 - c["kb"][1, 6] / 2
    s = faces(c["km"], c["kb"], c["kv2"])
    assert_bits("a NaN gives +0", s[0, 0, 0, 2:4], numpy.zeros(2, dtype=dtype))
    assert s[0, 0, 1, 3] == 0 and s[0, 1, 0, 4] == c["kv2"][0] and s[0, 1, 0, 5] == c["kv2"][0] and not numpy.signbit(s).any()
    outs, _ = Run(eng, c).check("special km")
    assert all(numpy.isfinite(outs[k]).all() for k in NAMES)
    c = case(shape, dtype, seed=7)
    c["km"][...] = 0
    c["kb"][...] = 0
    outs, _ = Run(eng, c, flux=False, drag=False).check("no viscosity")
    for k in NAMES:
        assert_bits("nothing to mix with keeps " + k, outs[k], c[k])
    c["km"][COLUMN] = 25.0
    outs, _ = Run(eng, c, flux=False, drag=False).check("one plume")
    calm = numpy.ones(shape[:3], dtype=bool)
    calm[COLUMN] = False
    for k in NAMES:
        assert_bits("the calm columns keep " + k, outs[k][calm], c[k][calm])
        assert (outs[k][COLUMN] != c[k][COLUMN]).all()


def check_boundary(eng):
    """with and without the fluxes and the drag; a flux changes exactly its field, a drag exactly the winds; zero wind in one
    column gives sp = +0 and no drag there; a NaN wind stays in its column of U and V"""
    dtype = np_of(eng)
    shape = (2, 3, 4, 9)
    c = case(shape, dtype, seed=8)
    runs = {(fl, dg): Run(eng, c, flux=fl, drag=dg).check("flux %s drag %s" % (fl, dg)) for fl in (True, False) for dg in (True, False)}
    bare = runs[False, False][0]
    assert runs[False, False][1] is None and runs[True, False][1] is None
    for k in NAMES:
        assert ((runs[True, False][0][k] != bare[k]).any()) == (k in FLUXED), k
        assert ((runs[False, True][0][k] != bare[k]).any()) == (k in WINDS), k
    for k in WINDS:
        assert (numpy.abs(runs[False, True][0][k][..., 0]) < numpy.abs(bare[k][..., 0])).all()      # the drag slows the lowest level
    Run(eng, c, ("V", "QT")).check("u is no field")
    Run(eng, c, ("THL", "X")).check("no wind among the fields: no speed plane")
    z = dict(c, U=c["U"].copy(), V=c["V"].copy())
    z["U"][COLUMN + (0,)] = z["V"][COLUMN + (0,)] = 0
    outs, sp = Run(eng, z).check("zero wind")
    assert_bits("sp = +0", sp[COLUMN], numpy.zeros((), dtype=dtype))
    nodrag = oracle(z, drag=False)[0]
    assert_bits("no drag at rest", outs["U"][COLUMN], nodrag["U"][COLUMN])
    assert (outs["U"] != nodrag["U"]).any()
    z = dict(c, U=c["U"].copy())
    z["U"][COLUMN + (0,)] = numpy.nan
    outs, sp = Run(eng, z).check("NaN wind")
    clean = runs[True, True][0]
    other = numpy.ones(shape[:3], dtype=bool)
    other[COLUMN] = False
    assert numpy.isnan(sp[COLUMN]) and not numpy.isnan(sp[other]).any()
    for k in WINDS:
        assert numpy.isnan(outs[k][COLUMN]).all()
        assert_bits("the other columns of " + k, outs[k][other], clean[k][other])
    for k in ("THL", "QT", "QR", "X"):
        assert_bits("a NaN wind leaves " + k, outs[k], clean[k])


def check_special(eng):
    """a NaN and an infinity in a field spread through their own column and reach no other column and no other field"""
    dtype = np_of(eng)
    shape = (2, 3, 4, 9)
    c = case(shape, dtype, seed=9)
    clean = Run(eng, c).check("clean")[0]
    other = numpy.ones(shape[:3], dtype=bool)
    other[COLUMN] = False
    for value in (numpy.nan, numpy.inf):
        s = dict(c, X=c["X"].copy())
        s["X"][COLUMN + (4,)] = value
        outs, _ = Run(eng, s).check("%s in X" % value)
        assert not numpy.isfinite(outs["X"][COLUMN]).any()
        assert_bits("the other columns of X", outs["X"][other], clean["X"][other])
        for k in ("U", "V", "THL", "QT", "QR"):
            assert_bits("the other field " + k, outs[k], clean[k])


FIELD_SETS = [("X",), ("U", "QR"), ("QT", "V", "THL"), ("U", "V", "THL", "QT"), ("QR", "U", "V", "THL", "QT"), NAMES]


def check_fields(eng, ktot=20):
    """1 to 6 fields of mixed classes in changing order: each field takes its own pair, its own flux and the drag of a wind"""
    c = case((2, 3, 5, ktot), np_of(eng), seed=10)
    for names in FIELD_SETS:
        Run(eng, c, names).check("%d fields %s" % (len(names), names))
    assert not numpy.array_equal(c["coef"]["QR"][0], c["coef"]["X"][0]) and not numpy.array_equal(c["coef"]["U"][0], c["coef"]["THL"][0])


def check_refusals(eng):
    """n = 0 is a no-op; two equal fields, a field equal to km, speed, a profile, s0, its flux or its drag, a flux without s0, a
    dr without u, v or speed, pitch_prof < ktot, a misaligned pointer, a NULL required pointer and n_fields outside 1 ... 6 are
    refused by the library; the engine refuses the same; no refused call writes"""
    dtype = np_of(eng)
    c = case((2, 2, 3, 8), dtype, seed=13)
    names = ("U", "QT", "X")

    def untouched(host):
        for f, k in enumerate(names):
            assert_bits("refused: " + k, host[("fields", f)], c[k])
        assert (host["speed"] == SPEED_FILL).all()
    rc, host = raw_launch(eng, c, extents=dict(n_les=0))
    assert rc == 0
    untouched(host)
    rc, host = raw_launch(eng, c)
    want, sp = les_vmix({k: c[k] for k in names}, c["km"], {k: c["coef"][k][0] for k in names}, {k: c["coef"][k][1] for k in names},
                        c["kb"], c["kv2"], c["s0"], {"QT": c["flux"]["QT"]}, {"U": c["dr"]}, c["U"], c["V"])
    assert rc == 0
    for f, k in enumerate(names):
        assert_bits("raw " + k, host[("fields", f)], want[k])
    assert_bits("raw speed", host["speed"], sp)
    rc, host = raw_launch(eng, c, null=(("dr", 0), "u", "v", "speed", ("flux", 1), "s0"))
    assert rc == 0 and (host["speed"] == SPEED_FILL).all()
    assert_bits("bare", host[("fields", 0)], vmix(c["U"], faces(c["km"], c["kb"], c["kv2"]), *c["coef"]["U"]))
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    bad = [(dict(extents=dict(pitch_prof=7)), b"pitch_prof"), (dict(extents=dict(n_fields=0)), b"field count"),
           (dict(extents=dict(n_fields=7)), b"field count"), (dict(null=("s0",)), b"without s0"),
           (dict(alias=((("fields", 2), ("fields", 0)),)), b"same field")]
    bad += [(dict(null=(k,)), b"without u, v and speed") for k in ("u", "v", "speed")]
    bad += [(dict(alias=((("fields", f), key),)), b"is also") for f, key in
            ((0, "km"), (0, "speed"), (1, "kb"), (1, "kv2"), (1, "s0"), (2, ("el", 2)), (2, ("eu", 0)), (1, ("flux", 1)), (0, ("dr", 0)))]
    bad += [(dict(alias=(("speed", key),)), b"speed is also an input") for key in ("u", "v", "km", ("el", 1))]
    bad += [(dict(offset=(k,)), b"not aligned") for k in ("km", ("fields", 1), ("el", 0), ("flux", 1), ("dr", 0), "speed")]
    bad += [(dict(null=(k,)), b"required pointer " + k.encode()) for k in ("km", "kb", "kv2")]
    bad += [(dict(null=((k, 1),)), b"required pointer " + k.encode() + b"[f]") for k in ("fields", "el", "eu")]
    for kw, text in bad:
        rc, host = raw_launch(eng, c, **kw)
        assert rc == E and text in eng.lib.spc_last_error(), (kw, rc, eng.lib.spc_last_error())
        untouched(host)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    t = {k: dev(c[k]) for k in ("U", "V", "QT", "X", "km", "kb", "kv2", "s0", "dr")}
    t["speed"] = dev(numpy.full(c["U"].shape[:3], SPEED_FILL, dtype=dtype))
    el, eu = {k: dev(c["coef"][k][0]) for k in names}, {k: dev(c["coef"][k][1]) for k in names}
    fields, flux, drag = {k: t[k] for k in names}, {"QT": dev(c["flux"]["QT"])}, {"U": t["dr"]}

    def call(fields=fields, el=el, eu=eu, flux=flux, drag=drag, **kw):
        a = dict(t, **kw)
        return eng.les_vmix(fields, a["km"], el, eu, a["kb"], a["kv2"], s0=a["s0"], flux=flux, drag=drag, u=a["U"], v=a["V"], speed=a["speed"])
    other = torch.float64 if eng.dtype == torch.float32 else torch.float32
    seven = {str(i): t["QT"] for i in range(7)}
    for bad_call in (lambda: call(km=t["U"]), lambda: call(speed=t["V"]), lambda: call(fields={"U": t["U"], "QT": t["U"], "X": t["X"]}),
                     lambda: call(kb=t["QT"].view(-1)[:16].view(2, 8)), lambda: call(flux={"QT": t["QT"].view(-1)[:2]}),
                     lambda: call(drag={"U": t["U"].view(-1)[:2]}), lambda: call(s0=None), lambda: call(speed=None), lambda: call(U=None),
                     lambda: call(el={"U": el["U"]}), lambda: call(eu=dict(eu, Y=eu["X"])), lambda: call(flux={"Y": flux["QT"]}),
                     lambda: call(drag={"Y": t["dr"]}), lambda: call(fields=seven, el=seven, eu=seven), lambda: call(fields={}, el={}, eu={}),
                     lambda: call(kv2=t["kv2"][:1]), lambda: call(kb=t["kb"][:, :4]), lambda: call(km=t["km"][..., ::2]),
                     lambda: call(km=t["km"].to(other)), lambda: call(km=t["km"].cpu()), lambda: call(speed=t["speed"][..., None])):
        try:
            bad_call()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad call was not refused")
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    for k in ("U", "V", "QT", "X"):
        assert_bits("refused: " + k, t[k].cpu().numpy(), c[k])
    assert (t["speed"] == SPEED_FILL).all()


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    c = case((n, 3, 4, 40), np_of(one), seed=n)
    names = ("U", "V", "THL", "QR")
    outs, sp = oracle(c, names)
    for tag, eng, up in on_both(one, multi, n):
        t = {k: up(c[k].copy()) for k in names + ("km", "kb", "kv2", "s0", "dr")}      # (a copy: on a CPU engine a tensor shares the array's memory)
        fields = {k: t[k] for k in names}
        el, eu = {k: up(c["coef"][k][0]) for k in names}, {k: up(c["coef"][k][1]) for k in names}
        dsp = up(numpy.full(c["U"].shape[:3], SPEED_FILL, dtype=c["U"].dtype))
        eng.les_vmix(fields, t["km"], el, eu, t["kb"], t["kv2"], s0=t["s0"], flux={"THL": up(c["flux"]["THL"])},
                     drag={"U": t["dr"], "V": t["dr"]}, u=t["U"], v=t["V"], speed=dsp)
        multi.synchronize()
        assert_bits("%s speed" % tag, host_of(dsp), sp)
        for k in names:
            assert_bits("%s field %s" % (tag, k), host_of(fields[k]), outs[k])
    return blocks_of(t["U"], multi, n)


BODIES = ("parity", "tiles", "coltile", "alignment", "viscosity", "boundary", "special", "fields", "refusals")
ALIGNMENTS = [((1, 2, 3), 65, 0), ((3, 3, 3), 64, 0), ((1, 0, 2, 3), 161, 2), ((2, 1), 7, 5)]


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, k) for k in (1, 2, 3, 7, 64)]),
            ("tiles", lambda: check_tiles(eng)),
            ("coltile", lambda: check_coltile(eng)),
            ("alignment", lambda: [check_alignment(eng, *a) for a in ALIGNMENTS]),
            ("viscosity", lambda: check_viscosity(eng)),
            ("boundary", lambda: check_boundary(eng)),
            ("special", lambda: check_special(eng)),
            ("fields", lambda: check_fields(eng)),
            ("refusals", lambda: check_refusals(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_vmix (CPU suite) ------------------------------------------------------------------------
class VmixOracleEngine(lxr.MixOracleEngine):
    """tests/les_mix_ref.MixOracleEngine with ``les_vmix`` by the NumPy oracle above: the fields updated in place and the speed
    plane written whole, as the HIP engine does; ``vmix_cols_per_block`` is that of the library's rule for f64 and f32"""

    def les_vmix(self, fields, km, el, eu, kb, kv2, s0=None, flux=None, drag=None, u=None, v=None, speed=None, **kw):
        names = list(fields)
        flux = {k: t for k, t in (flux or {}).items() if t is not None}
        drag = {k: t for k, t in (drag or {}).items() if t is not None}
        if not 1 <= len(names) <= _abi.SPC_VMIX_MAX_FIELDS or sorted(el) != sorted(names) or sorted(eu) != sorted(names):
            raise ValueError("1 ... 6 fields, and el and eu hold their names")
        if [k for k in list(flux) + list(drag) if k not in fields] or (flux and s0 is None) or (drag and (u is None or v is None or speed is None)):
            raise ValueError("a flux or a drag without its field, s0, u, v or speed")
        written = [fields[k].data_ptr() for k in names] + ([speed.data_ptr()] if drag else [])
        read = {t.data_ptr() for t in [km, kb, kv2, s0] + [el[k] for k in names] + [eu[k] for k in names] + list(flux.values()) + list(drag.values())
                if t is not None}
        if drag:
            read |= {x.data_ptr() for x in (u, v) if x.data_ptr() == speed.data_ptr()}
        if km.shape[0] and (len(set(written)) != len(written) or set(written) & read):
            raise ValueError("a field or speed is another field, km, a profile, s0, a flux or a drag")
        ktot = int(km.shape[3])
        if not self.vmix_cols_per_block(ktot):
            top = next(k for k in range(ktot, 0, -1) if self.vmix_cols_per_block(k))
            raise _abi.SpcError(_abi.SPC_ERR_UNSUPPORTED, "les_vmix: ktot %d above the %d levels of which 16 columns fit the LDS twice" % (ktot, top))
        c = lambda t: None if t is None else numpy.ascontiguousarray(t.numpy())                 # noqa: E731
        new, sp = les_vmix({k: c(fields[k]) for k in names}, c(km), {k: c(el[k]) for k in names}, {k: c(eu[k]) for k in names}, c(kb), c(kv2),
                           c(s0), {k: c(t) for k, t in flux.items()}, {k: c(t) for k, t in drag.items()}, c(u), c(v))
        if sp is not None:
            speed.copy_(torch.from_numpy(sp))
        for k in names:
            fields[k].copy_(torch.from_numpy(new[k]))

    def vmix_cols_per_block(self, ktot):
        esize = 4 if self.dtype == torch.float32 else 8
        col = 2 * (ktot | 1) * esize
        return 0 if ktot < 1 else 64 if 64 * col <= 65536 else 32 if 32 * col <= 65536 else 16 if 16 * col <= 163840 else 0


# -- the host twins of models.DeviceLESEnsemble after enable_vertical_mixing() ------------------------------------------------
class _HostVmix:
    """NumPy fields: the executable definition of what evolve_model_batched does after enable_vertical_mixing(): behind K24 and
    where K15 stands, ONE les_vmix on the fields among U, V (the winds' pair, the drag where a z0m was set) and THL, QT, QR (the
    scalars' pair; THL and QT with the fluxes wt and wq) that exist, by the UNCAPPED viscosity: K24's km where its cap did not
    bind in this step, else K24's eddy viscosity of the same (unmixed) winds and theta under a cap of the type's largest value.

    The step of tests/les_mix_ref._HostMix is one method, so with enable_vertical_mixing() this class spells the sequence out once
    more with K25 where K15 stood; K19 stands above it, as it does above _HostMix.  Without the call the step is _HostMix's."""

    vmix_par = None
    _kv = None

    def enable_vertical_mixing(self, kv_cap=None, k_bg=None, drag=True):
        if self.mix_par is None or self.diffuse_par is not None or self.mix_par["vertical"]:
            raise ValueError("needs enable_mixing(), and neither enable_diffusion() nor vertical=True")
        self.vmix_par = dict(kv_cap=vm.KV_CAP if kv_cap is None else kv_cap, k_bg=vm.K_BG if k_bg is None else k_bg, drag=drag)
        self._kv = None

    def enable_mixing(self, *a, **kw):
        super().enable_mixing(*a, **kw)
        self._kv = None                                            # (a second call forgets the viscosity of the earlier one's last step)

    def enable_diffusion(self, *a, **kw):
        if self.vmix_par is not None:
            raise ValueError("a step has one vertical diffusion")
        return super().enable_diffusion(*a, **kw)

    def _mix(self, dt):
        f, par = self.fields3d, self.mix_par
        u, v, theta = f["U"], f["V"], f["THL"] if par["stability"] and "THL" in f else None
        super()._mix(dt)
        self._kv = self._km
        if self.vmix_par is not None and self.mixing_capped:
            T = u.dtype
            r = lambda a: numpy.ascontiguousarray(a.astype(T))                               # noqa: E731
            gx, gy, _, _ = mix.coefficients(dt, par["dx"], par["dy"], par["prandtl"], n=self.n)
            gz, bz, l2 = mix.profiles(self.zf_cache, self.zh_cache, par["dx"], par["dy"], par["cs"], par["prandtl"], par["theta_ref"], n=self.n)
            huge = numpy.full(self.n, numpy.finfo(T).max, dtype=T)
            self._kv = lxr.eddy(u, v, theta, r(gx), r(gy), r(gz), r(bz), r(l2), huge)[0]

    def _vmix(self, dt):
        from sp_coupler_amd import microphysics as mp
        f, p, par = self.fields3d, self.p, self.vmix_par
        T = f["U"].dtype
        r = lambda a: numpy.ascontiguousarray(numpy.asarray(a).astype(T))                   # noqa: E731
        wind, scalar, s0 = vm.coefficients(self.zh_cache, self.zf_cache, p["Rhobf"], dt, self.mix_par["prandtl"])
        kb, kv2 = vm.background(self.n, wind[0].shape[-1], par["k_bg"], par["kv_cap"])
        keys = [k for k in self.MIX_KEYS if k in f]
        coef = {k: (r(wind[0]), r(wind[1])) if k in WINDS else (r(scalar[0]), r(scalar[1])) for k in keys}
        flux = {k: r(numpy.asarray(self.tend[slot], dtype=numpy.float64).reshape(self.n)) for k, slot in (("THL", "wt"), ("QT", "wq"))
                if k in keys and slot in self.tend}
        drag = {}
        if par["drag"] and "z0m" in self.tend:
            dr = r(vm.drag(numpy.asarray(self.tend["z0m"], dtype=numpy.float64).reshape(self.n), self.zf_cache,
                           mp.layer_thickness(self.zh_cache, self.zf_cache), dt))
            drag = {k: dr for k in WINDS if k in keys}
        new, _ = les_vmix({k: f[k] for k in keys}, self._kv, {k: coef[k][0] for k in keys}, {k: coef[k][1] for k in keys}, r(kb), r(kv2),
                          r(s0), flux, drag, f["U"], f["V"])
        f.update(new)

    def get_vertical_viscosity_batched(self):
        return self._kv if self.vmix_par is not None else None

    def evolve_model_batched(self, t):
        from sp_coupler_amd import radiation as rad
        from sp_coupler_amd import thermo
        from tests import les_thermo_ref as ltr
        dt = float(t) - self.model_time
        if dt <= 0:
            return
        if self.vmix_par is None:
            return super().evolve_model_batched(t)
        f, p = self.fields3d, self.p
        self._step(dt)
        if "PS" in self.tend:
            p["PS"] = p["PS"] + dt * self.tend["PS"]
        if self.advect_par is not None:
            self._advect(dt)
        self._mix(dt)
        self._vmix(dt)
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


class HostVmixLESEnsemble(lfr._HostFull, lfr.qlr._HostQtLocal, _HostVmix, lxr._HostMix, lfr.lt2._HostTransport2, lfr.lbr.HostBuoyancyLESEnsemble):
    """the bases of tests/les_mix_ref.HostMixLESEnsemble with the vertical mixing above K24's twin: QL = max(QT - Qsat, 0)"""


class HostThermoVmixLESEnsemble(lfr._HostFull, lfr.qlr._HostQtLocal, _HostVmix, lxr._HostMix, lfr.lt2._HostTransport2,
                                lfr.lbr.HostThermoBuoyancyLESEnsemble):
    """after enable_thermo(): K12's oracle wherever QL is read"""


VARIANTS = {"plain": dict(), "all": dict(radiate=True, thermo=True, micro=True, transport=True),
            "forced": dict(thermo=True, transport=True, qt="strong", buoyancy=True)}
DX = 250.0
Z0M = 0.05


def ensemble_run(engine, n, device, vmix=True, drag=True, z0m=True, cap=None, thermo=False, micro=False, radiate=False, transport=False,
                 qt=None, buoyancy=False, itot=4, jtot=5, nL=20, steps=3, change=None, vmix_kw=None):
    """an ensemble with attached U, V, THL, QT (and Qsat, or thermo; QR with the microphysics), enable_mixing() and
    enable_vertical_mixing() (``vmix`` False: only the former) through ``steps`` calls of evolve_model_batched and one
    variability nudge (constantT) before the last; ``z0m``: a roughness length is handed over; ``cap``: that of enable_mixing (a
    small one binds: the second viscosity buffer); ``change(ens, step)`` runs before every step.  After each of them every
    profile, the fields and both viscosities.  Returns (ens, list of records)"""
    if device:
        cls = models.DeviceLESEnsemble
    else:
        cls = HostThermoVmixLESEnsemble if thermo else HostVmixLESEnsemble

    def enable(ens):
        if qt:
            ens.enable_qt_forcing(qt)
        if buoyancy:
            ens.enable_buoyancy()
        ens.enable_mixing(cap=cap, **({} if transport else {"dx": DX, "dy": 1.5 * DX}))
        if vmix:
            ens.enable_vertical_mixing(drag=drag, **(vmix_kw or {}))
        if change:
            inner = ens.evolve_model_batched
            count = [0]

            def evolve(t):
                change(ens, count[0])
                count[0] += 1
                return inner(t)
            ens.evolve_model_batched = evolve

    def record(ens, rec):
        for tag, km in (("km", ens.get_eddy_viscosity_batched()), ("kv", ens.get_vertical_viscosity_batched() if vmix else None)):
            rec[tag] = numpy.zeros(rec["field U"].shape) if km is None else numpy.array(host_of(km))
        rec["k max"] = numpy.array([-1.0 if ens.mixing_k_max is None else ens.mixing_k_max, float(bool(ens.mixing_capped))])
        if qt:
            counts = ens.get_qt_forcing_counts_batched()
            rec["counts"] = numpy.zeros((n, nL)) if counts is None else numpy.array(host_of(counts), dtype=numpy.float64)

    def before(ens):
        assert ens.get_eddy_viscosity_batched() is None and (not vmix or ens.get_vertical_viscosity_batched() is None)

    def forcings(rng, stack):
        more = dict(QL=rng.normal(0, 2e-8, (n, nL)), QLp=stack("ql_ref") * (0.5 + rng.random((n, nL)))) if qt else {}
        if z0m:
            more["Z0M_surf"] = Z0M * (0.5 + rng.random(n))
        return more
    advection = dict(dx=DX, dy=1.5 * DX, vertical=True, conservative=True, order=2) if transport else None
    return ensemble_case(engine, n, cls, thermo=thermo, micro=micro, advection=advection, forcings=forcings,
                         radiation=lrr.radiation_of(n, "f0", "f1") if radiate else None, enable=enable, record=record, before=before,
                         itot=itot, jtot=jtot, nL=nL, steps=steps)


def check_ensemble(one, engines, n, variant, cap=None, **kw):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``: every profile, field and both
    viscosities bit-equal after each step; the vertical mixing changes U: the twin's last step differs from the same run without
    enable_vertical_mixing(); with a ``cap`` that binds the vertical viscosity differs from K24's km, else it is km"""
    from tests import les_micro_ref as lmr
    kw = dict(VARIANTS[variant], cap=cap, **kw)
    host = ensemble_run(one, n, False, **kw)[1]
    plain = ensemble_run(one, n, False, vmix=False, **kw)[1]
    assert (host[-1]["field U"] != plain[-1]["field U"]).any() and (host[-1]["kv"] > 0).any()
    capped = [bool(r["k max"][1]) for r in host[1:]]
    for r, c in zip(host[1:], capped):
        assert numpy.array_equal(r["kv"], r["km"]) == (not c)
    for engine in engines:
        lmr.same_logs(host, ensemble_run(engine, n, True, **kw)[1])
    return host, capped
