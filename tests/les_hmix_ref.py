"""NumPy oracle of K26 (include/spc.h: spc_les_hmix_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_hmix_gpu.py (each takes an engine: tools/mutation_control.py --hmix hands them the engines of its mutant libraries),
the host twin of models.DeviceLESEnsemble's enable_mixing(implicit=True) and an oracle-backed engine with ``les_hmix`` for the CPU
suite.

The oracle spells the rule out with a loop over the cells of a line, vectorised over the lines, one statement per rounding in the
element type, so nothing fuses.  Every device array of the bodies is the LEADING part of a poisoned buffer
(tests/les_harness.Poisoned); the bytes behind it (and in front of a view off the 16-byte grid) are checked after the launch."""
import numpy
import torch

from sp_coupler_amd import _abi, models
from sp_coupler_amd import horizontal_mixing as hm
from sp_coupler_amd import mixing as mix
from tests import les_mix_ref as lxr
from tests import les_vmix_ref as lvr
from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, host_of, np_of, on_both, run_bodies)

#: one level, a few, a whole number of 16-byte vectors, an odd count beside a wave
KTOTS = [1, 5, 20, 37]
#: (n, plane): 1 to 3 LES; a workgroup of 256 lines spans several LES of the small planes
PLANES = [(1, (3, 5)), (2, (8, 8)), (3, (4, 7))]
#: the extents of a line: none to eliminate (1), the closing unknown beside one (2) and two (3) others, up to a chunk of a walk
#: (8) and four chunks and a cell (33)
EXTENTS = [1, 2, 3, 4, 5, 8, 33]
NAMES = ("U", "V", "THL", "QT", "QR", "X")
WINDS = ("U", "V")
DT = 900.0
DX = 200.0
KH_CAP = 20.0


# -- the rule --------------------------------------------------------------------------------------------------------------
def weights(km, a, kh2, axis):
    """w, the shape of km: the weight of the face between cell i and cell ip = (i + 1) mod n along ``axis`` (1: i, 2: j)"""
    T = km.dtype.type
    assert km.dtype == a.dtype == kh2.dtype
    cap = kh2[:, None, None, None]
    with numpy.errstate(all="ignore"):
        t = km + numpy.roll(km, -1, axis=axis)
        s = numpy.where(t > 0, t, T(0))                            # a NaN or a negative sum gives +0
        s = numpy.where(s < cap, s, cap)
        w = a[:, None, None, None] * s
    assert w.dtype == km.dtype
    return w


def sweep(x, w, axis):
    """x' of one backward-Euler step of every periodic line of ``x`` along ``axis`` with the face weights ``w``; a new array"""
    n = x.shape[axis]
    if n == 1:
        return x.copy()
    T = x.dtype.type
    assert x.dtype == w.dtype
    X, W = numpy.moveaxis(x, axis, 0), numpy.moveaxis(w, axis, 0)
    m = n - 1
    one, zero = T(1), numpy.zeros(X.shape[1:], dtype=x.dtype)
    q, y, z = (numpy.empty((m,) + X.shape[1:], dtype=x.dtype) for _ in range(3))
    out = numpy.empty(X.shape, dtype=x.dtype)
    with numpy.errstate(all="ignore"):
        for i in range(m):
            up, lo = W[i], W[i - 1]                                # (i = 0: W[-1] is the face between n-1 and 0)
            b = one + lo
            b = b + up
            c = (lo if i == 0 else zero) + (up if i == m - 1 else zero)
            if i == 0:
                p = one / b
                y[0] = X[0] * p
                z[0] = c * p
            else:
                lq = lo * q[i - 1]
                den = b - lq
                p = one / den
                ly = lo * y[i - 1]
                r = X[i] + ly
                y[i] = r * p
                lz = lo * z[i - 1]
                r = c + lz
                z[i] = r * p
            q[i] = up * p
        for i in range(m - 2, -1, -1):
            t = q[i] * y[i + 1]
            y[i] = y[i] + t
            t = q[i] * z[i + 1]
            z[i] = z[i] + t
        up, lo = W[m], W[m - 1]
        b = one + lo
        b = b + up
        n1 = up * y[0]
        n2 = X[m] + n1
        n3 = lo * y[m - 1]
        num = n2 + n3
        d1 = up * z[0]
        d2 = b - d1
        d3 = lo * z[m - 1]
        den = d2 - d3
        out[m] = num / den
        for i in range(m):
            t = z[i] * out[m]
            out[i] = y[i] + t
    assert out.dtype == x.dtype
    return numpy.ascontiguousarray(numpy.moveaxis(out, 0, axis))


def les_hmix(fields, km, ax, ay, kh2, axes=3):
    """dict name -> the mixed field, new arrays; ``ax`` and ``ay`` dicts with the names of ``fields``"""
    out = {}
    for k, x in fields.items():
        if axes & 1:
            x = sweep(x, weights(km, ax[k], kh2, 1), 1)
        if axes & 2:
            x = sweep(x, weights(km, ay[k], kh2, 2), 2)
        out[k] = x if axes & 3 else x.copy()
    return out


# -- inputs ------------------------------------------------------------------------------------------------------------------
def case(shape, dtype, seed=0, dt=DT, kh_cap=KH_CAP):
    """dict of the arguments in ``dtype``: the fields U, V, THL, QT, QR and X, km, kh2 and ``coef``: name -> (ax, ay).  Another
    grid spacing per LES and dx != dy; U and V share the winds' pair, THL and QT the scalars', QR and X have a pair of their own each
    (another Prandtl number); km is +0 in a fifth of the cells and reaches above the bound in others"""
    dtype = numpy.dtype(dtype).type
    n, itot, jtot, ktot = shape
    rng = numpy.random.default_rng(26000 + seed + 7 * ktot + 3 * itot + 5 * jtot + 31 * n)
    k = numpy.arange(ktot)
    c = dict(U=5.0 + rng.standard_normal(shape), V=-2.0 + rng.standard_normal(shape),
             THL=290.0 + 10.0 * k / 160.0 + 0.5 * rng.standard_normal(shape),
             QT=8e-3 * numpy.exp(-k / 160.0) * (1.0 + 0.05 * rng.standard_normal(shape)), QR=1e-5 * rng.random(shape),
             X=rng.standard_normal(shape), km=30.0 * rng.random(shape) ** 2 * (rng.random(shape) > 0.2))
    dx, dy = DX * (1.0 + 0.1 * numpy.arange(n)), 1.5 * DX * (1.0 + 0.05 * numpy.arange(n))
    _, _, wind, scalar = mix.coefficients(dt, dx, dy)
    own = [mix.coefficients(dt, dx, dy, prandtl=pr)[3] for pr in (0.5, 0.8)]
    c["kh2"] = hm.bound(n, kh_cap * (1.0 + 0.1 * numpy.arange(n)))
    c = {key: numpy.ascontiguousarray(a.astype(dtype)) for key, a in c.items()}
    pairs = [tuple(numpy.ascontiguousarray(a.astype(dtype)) for a in p) for p in (wind, scalar) + tuple(own)]
    c["coef"] = {"U": pairs[0], "V": pairs[0], "THL": pairs[1], "QT": pairs[1], "QR": pairs[2], "X": pairs[3]}
    return c


def oracle(c, names=NAMES, axes=3):
    return les_hmix({k: c[k] for k in names}, c["km"], {k: c["coef"][k][0] for k in names}, {k: c["coef"][k][1] for k in names}, c["kh2"], axes)


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """``eng.les_hmix`` with every array inside a poisoned buffer, once per entry of ``axes`` on the same buffers; ``check``
    compares every field with the oracle (the sweeps of ``axes`` in turn) bit for bit, the read-only inputs with what was
    uploaded, and looks at the bytes around every array.  ``leads``: elements in front of the 4-D arrays, taken in turn (the
    fields, then km).  Arrays that are one object in the case (the coefficients two fields share) are one device tensor."""

    def __init__(self, eng, c, names=NAMES, axes=(3,), leads=(0,)):
        self.eng, self.c, self.names, self.axes = eng, c, tuple(names), tuple(axes)
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
        self.dfields = {k: self.mem.put(k, c[k], nan, lead()) for k in self.names}
        self.dkm = put("km", c["km"], nan, lead())
        self.dkh2 = put("kh2", c["kh2"], 1e30)
        self.dax = {k: put("ax " + k, c["coef"][k][0], 1e30) for k in self.names}
        self.day = {k: put("ay " + k, c["coef"][k][1], 1e30) for k in self.names}
        for a in self.axes:
            eng.les_hmix(self.dfields, self.dkm, self.dax, self.day, self.dkh2, axes=a)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def results(self):
        return {k: t.cpu().numpy() for k, t in self.dfields.items()}

    def check(self, what=""):
        want = {k: self.c[k] for k in self.names}
        for a in self.axes:
            want = oracle(dict(self.c, **want), self.names, a)
        got = self.results()
        for k in self.names:
            assert_bits("%s field %s" % (what, k), got[k], want[k])
        for tag, t, a in self.inputs:
            assert Poisoned.read_only(t, a), (what, tag, "read only")
        self.mem.check_around(what)
        return want


def raw_launch(eng, c, names=("U", "QT", "X"), axes=3, alias=(), extents=None, null=(), offset=()):
    """spc_les_hmix_* itself: (rc, dict member -> the array on the host afterwards).  Every member is a tensor of its own.
    ``alias``: (member, key) pairs that replace a pointer member by that of tensor ``key``, a member or key of an array spelled
    ("ax", 0); ``extents``: overrides of the scalar members; ``null``: members set to NULL; ``offset``: members whose pointer is
    moved one byte"""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    n, itot, jtot, ktot = c["U"].shape
    t = {k: dev(c[k]) for k in ("km", "kh2")}
    for f, k in enumerate(names):
        t[("fields", f)] = dev(c[k])
        t[("ax", f)], t[("ay", f)] = dev(c["coef"][k][0]), dev(c["coef"][k][1])
    a = _abi.LesHmixArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields, a.axes = n, itot, jtot, ktot, len(names), axes

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
    rc = abi_call(eng, "spc_les_hmix", a)
    return rc, {k: x.cpu().numpy() for k, x in t.items()}


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, ktot):
    """six fields of both classes against the oracle, 1 to 3 LES; the mixing does something, and the bound binds at some faces
    and not at others"""
    for n, plane in PLANES:
        c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
        outs = Run(eng, c).check("n %d plane %s ktot %d" % (n, plane, ktot))
        for k in NAMES:
            assert (outs[k] != c[k]).any()
        s = weights(c["km"], numpy.ones_like(c["kh2"]), c["kh2"], 1)
        top = numpy.broadcast_to(c["kh2"][:, None, None, None], s.shape)
        assert (s == top).any() and (s < top).any() and (s == 0).any() or ktot * n * plane[0] < 100


def check_lines(eng):
    """lines of 1, 2, 3, 4, 5, 8 and 33 cells along i and along j, both sweeps and each alone; 3 LES whose lines (3 x 259 = 777
    along either axis) are no multiple of any count of lines per workgroup, so the last workgroup is partial and workgroups span
    two LES"""
    dtype = np_of(eng)
    for e in EXTENTS:
        L = eng.hmix_lines_per_block(e)
        assert L in (256, 128, 64, 32, 16) and 777 % L and 259 % L, (e, L)
        for shape in ((3, e, 7, 37), (3, 7, e, 37)):
            c = case(shape, dtype, seed=e)
            for axes in (1, 2, 3):
                outs = Run(eng, c, ("U", "QT", "X"), axes=(axes,)).check("shape %s axes %d" % (shape, axes))
                swept = [shape[1 + b] for b in (0, 1) if axes >> b & 1]
                assert (outs["X"] != c["X"]).any() == (max(swept) > 1), (shape, axes)


def check_alignment(eng, leads, ktot=7):
    """views 1 to 3 elements off the 16-byte grid, differently per array; an odd ktot"""
    c = case((3, 4, 5, ktot), np_of(eng), seed=sum(leads))
    Run(eng, c, ("U", "THL", "X"), leads=leads).check("leads %s ktot %d" % (leads, ktot))


LINE = (1, slice(None), 2, 1)                                      # (l, :, j, k): the line along i that is special


def check_viscosity(eng):
    """km NaN, negative, infinite and at the bound give the faces the rule names; km = 0 keeps every value of a finite field and a
    -0.0 among positive values comes out +0.0; calm lines (km = 0) beside one line of large km keep every value while that line
    mixes"""
    dtype = np_of(eng)
    shape = (2, 5, 6, 5)
    c = case(shape, dtype, seed=6)
    c["km"][0, 0, 0, 2], c["km"][0, 1, 1, 3], c["km"][0, 2, 0, 4] = numpy.nan, -50.0, numpy.inf
    c["km"][1, 0, 0, 0] = c["km"][1, 1, 0, 0] = c["kh2"][1] / 2
    one = numpy.ones_like(c["kh2"])
    wi, wj = weights(c["km"], one, c["kh2"], 1), weights(c["km"], one, c["kh2"], 2)
    assert_bits("a NaN decouples its two faces along i", wi[0, [4, 0], 0, 2], numpy.zeros(2, dtype=dtype))
    assert_bits("a NaN decouples its two faces along j", wj[0, 0, [5, 0], 2], numpy.zeros(2, dtype=dtype))
    assert wi[0, 1, 1, 3] == 0 and wi[0, 0, 1, 3] == 0 and wi[0, 2, 0, 4] == c["kh2"][0] and wi[0, 1, 0, 4] == c["kh2"][0]
    assert wi[1, 0, 0, 0] == c["kh2"][1] and not numpy.signbit(wi).any() and not numpy.isnan(wi).any() and not numpy.isnan(wj).any()
    outs = Run(eng, c).check("special km")
    assert all(numpy.isfinite(outs[k]).all() for k in NAMES)
    c = case(shape, dtype, seed=7)
    c["km"][...] = 0
    c["THL"][1, 2, 3, 1] = -0.0
    outs = Run(eng, c).check("no viscosity")
    for k in NAMES:
        assert numpy.array_equal(outs[k], c[k]), k                  # (every value; the sign of a zero is not kept)
    assert outs["THL"][1, 2, 3, 1] == 0 and not numpy.signbit(outs["THL"][1, 2, 3, 1])
    c = case(shape, dtype, seed=7)
    c["km"][...] = 0
    c["km"][LINE] = 25.0
    outs = Run(eng, c, axes=(1,)).check("one violent line")
    calm = numpy.ones(shape, dtype=bool)
    calm[LINE] = False
    for k in NAMES:
        assert_bits("the calm lines keep " + k, outs[k][calm], c[k][calm])
        assert (outs[k][LINE] != c[k][LINE]).all()


def check_special(eng):
    """a NaN and an infinity in a field fill their own line along i in the first sweep and the j lines of those cells in the second:
    the plane (l, :, :, k), no other level, no other LES and no other field"""
    dtype = np_of(eng)
    shape = (2, 4, 5, 5)
    c = case(shape, dtype, seed=9)
    cell = (1, 2, 3, 1)
    for axes in (1, 3):
        clean = Run(eng, c, axes=(axes,)).check("clean axes %d" % axes)
        hit = numpy.zeros(shape, dtype=bool)
        if axes == 1:
            hit[1, :, 3, 1] = True
        else:
            hit[1, :, :, 1] = True
        for value in (numpy.nan, numpy.inf):
            s = dict(c, X=c["X"].copy())
            s["X"][cell] = value
            outs = Run(eng, s, axes=(axes,)).check("%s in X axes %d" % (value, axes))
            assert not numpy.isfinite(outs["X"][hit]).any()
            assert_bits("the other lines of X", outs["X"][~hit], clean["X"][~hit])
            for k in ("U", "V", "THL", "QT", "QR"):
                assert_bits("the other field " + k, outs[k], clean[k])


FIELD_SETS = [("X",), ("U", "QR"), ("QT", "V", "THL"), ("U", "V", "THL", "QT"), ("QR", "U", "V", "THL", "QT"), NAMES]


def check_fields(eng, ktot=20):
    """1 to 6 fields of mixed classes in changing order: each field takes its own pair of coefficients"""
    c = case((2, 3, 5, ktot), np_of(eng), seed=10)
    for names in FIELD_SETS:
        Run(eng, c, names).check("%d fields %s" % (len(names), names))
    assert not numpy.array_equal(c["coef"]["QR"][0], c["coef"]["X"][0]) and not numpy.array_equal(c["coef"]["U"][0], c["coef"]["THL"][0])
    assert not numpy.array_equal(c["coef"]["U"][0], c["coef"]["U"][1])


def check_sweeps(eng):
    """axes 1 and then axes 2 in two calls give the bits of axes 3 in one; 2 then 1 gives other values (the sweeps do not commute)"""
    c = case((2, 4, 5, 20), np_of(eng), seed=11)
    both = Run(eng, c).check("axes 3")
    split = Run(eng, c, axes=(1, 2))
    split.check("axes 1, then 2")
    got = split.results()
    other = Run(eng, c, axes=(2, 1)).check("axes 2, then 1")
    for k in NAMES:
        assert_bits("two calls " + k, got[k], both[k])
    assert any((other[k] != both[k]).any() for k in NAMES)


def check_refusals(eng):
    """n = 0 is a no-op; a NULL required pointer, two equal fields, a field equal to km, kh2 or a coefficient, a misaligned pointer,
    axes outside 1 ... 3, n_fields outside 1 ... 6 and an unsupported extent are refused by the library; the engine refuses the
    same; no refused call writes"""
    dtype = np_of(eng)
    c = case((2, 3, 4, 8), dtype, seed=13)
    names = ("U", "QT", "X")

    def untouched(host):
        for f, k in enumerate(names):
            assert_bits("refused: " + k, host[("fields", f)], c[k])
    rc, host = raw_launch(eng, c, extents=dict(n_les=0))
    assert rc == 0
    untouched(host)
    for axes in (1, 2, 3):
        rc, host = raw_launch(eng, c, axes=axes)
        want = oracle(c, names, axes)
        assert rc == 0
        for f, k in enumerate(names):
            assert_bits("raw %s axes %d" % (k, axes), host[("fields", f)], want[k])
    E = _abi.SPC_ERR_INVALID_ARGUMENT
    bad = [(dict(extents=dict(n_fields=0)), b"field count"), (dict(extents=dict(n_fields=7)), b"field count"),
           (dict(extents=dict(axes=0)), b"axes 0 outside"), (dict(extents=dict(axes=4)), b"axes 4 outside"),
           (dict(extents=dict(n_les=0, axes=0)), b"axes 0 outside"), (dict(alias=((("fields", 2), ("fields", 0)),)), b"same field")]
    bad += [(dict(alias=((("fields", f), key),)), b"is also") for f, key in ((0, "km"), (1, "kh2"), (2, ("ax", 2)), (2, ("ay", 0)))]
    bad += [(dict(offset=(k,)), b"not aligned") for k in ("km", "kh2", ("fields", 1), ("ax", 0), ("ay", 2))]
    bad += [(dict(null=(k,)), b"required pointer " + k.encode()) for k in ("km", "kh2")]
    bad += [(dict(null=((k, 1),)), b"required pointer " + k.encode() + b"[f]") for k in ("fields", "ax", "ay")]
    for kw, text in bad:
        rc, host = raw_launch(eng, c, **kw)
        assert rc == E and text in eng.lib.spc_last_error(), (kw, rc, eng.lib.spc_last_error())
        untouched(host)
    top = next(e for e in range(1, 5000) if not eng.hmix_lines_per_block(e + 1))
    assert top >= 256
    for member, word in (("itot", b"itot"), ("jtot", b"jtot")):     # (refused before a launch: the small arrays are never read)
        rc, host = raw_launch(eng, c, extents={member: top + 1})
        assert rc == _abi.SPC_ERR_UNSUPPORTED and word in eng.lib.spc_last_error() and str(top).encode() in eng.lib.spc_last_error()
        untouched(host)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    t = {k: dev(c[k]) for k in ("U", "QT", "X", "km", "kh2")}
    ax, ay = {k: dev(c["coef"][k][0]) for k in names}, {k: dev(c["coef"][k][1]) for k in names}
    fields = {k: t[k] for k in names}

    def call(fields=fields, ax=ax, ay=ay, axes=3, **kw):
        a = dict(t, **kw)
        return eng.les_hmix(fields, a["km"], ax, ay, a["kh2"], axes=axes)
    other = torch.float64 if eng.dtype == torch.float32 else torch.float32
    seven = {str(i): t["QT"] for i in range(7)}
    for bad_call in (lambda: call(km=t["U"]), lambda: call(fields={"U": t["U"], "QT": t["U"], "X": t["X"]}),
                     lambda: call(kh2=t["QT"].view(-1)[:2]), lambda: call(ax=dict(ax, U=t["U"].view(-1)[:2])),
                     lambda: call(ax={"U": ax["U"]}), lambda: call(ay=dict(ay, Y=ay["X"])), lambda: call(fields=seven, ax=seven, ay=seven),
                     lambda: call(fields={}, ax={}, ay={}), lambda: call(axes=0), lambda: call(axes=4), lambda: call(kh2=t["kh2"][:1]),
                     lambda: call(km=t["km"][..., ::2]), lambda: call(km=t["km"].to(other)), lambda: call(km=t["km"].cpu())):
        try:
            bad_call()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad call was not refused")
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    for k in names:
        assert_bits("refused: " + k, t[k].cpu().numpy(), c[k])


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    c = case((n, 3, 4, 20), np_of(one), seed=n)
    names = ("U", "V", "THL", "QR")
    outs = oracle(c, names)
    for tag, eng, up in on_both(one, multi, n):
        t = {k: up(c[k].copy()) for k in names + ("km", "kh2")}    # (a copy: on a CPU engine a tensor shares the array's memory)
        fields = {k: t[k] for k in names}
        ax, ay = {k: up(c["coef"][k][0]) for k in names}, {k: up(c["coef"][k][1]) for k in names}
        eng.les_hmix(fields, t["km"], ax, ay, t["kh2"])
        multi.synchronize()
        for k in names:
            assert_bits("%s field %s" % (tag, k), host_of(fields[k]), outs[k])
    return blocks_of(t["U"], multi, n)


BODIES = ("parity", "lines", "alignment", "viscosity", "special", "fields", "sweeps", "refusals")
ALIGNMENTS = [((1, 2, 3), 7), ((3, 3, 3), 5), ((1, 0, 2, 3), 37), ((2, 1), 1)]


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, k) for k in KTOTS]),
            ("lines", lambda: check_lines(eng)),
            ("alignment", lambda: [check_alignment(eng, *a) for a in ALIGNMENTS]),
            ("viscosity", lambda: check_viscosity(eng)),
            ("special", lambda: check_special(eng)),
            ("fields", lambda: check_fields(eng)),
            ("sweeps", lambda: check_sweeps(eng)),
            ("refusals", lambda: check_refusals(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_hmix (CPU suite) ------------------------------------------------------------------------
def lines_per_block(n, esize):
    """the library's rule (spc_hmix.hpp: hline_lines)"""
    if n < 1:
        return 0
    line = 2 * max(n - 1, 1) * esize
    for L in (256, 128, 64):
        if L * line <= 65536:
            return L
    return 32 if 32 * line <= 163840 else 16 if 16 * line <= 163840 else 0


class HmixOracleEngine(lvr.VmixOracleEngine):
    """tests/les_vmix_ref.VmixOracleEngine with ``les_hmix`` by the NumPy oracle above: the fields updated in place, as the HIP
    engine does; ``hmix_lines_per_block`` is that of the library's rule for f64 and f32"""

    def les_hmix(self, fields, km, ax, ay, kh2, axes=3, **kw):
        names = list(fields)
        if not 1 <= len(names) <= _abi.SPC_HMIX_MAX_FIELDS or sorted(ax) != sorted(names) or sorted(ay) != sorted(names):
            raise ValueError("1 ... 6 fields, and ax and ay hold their names")
        if axes not in (1, 2, 3):
            raise ValueError("axes is none of 1, 2 and 3")
        for t in [km] + [fields[k] for k in names]:
            if not isinstance(t, torch.Tensor) or t.dtype != self.dtype or t.dim() != 4 or not t.is_contiguous() or t.shape != km.shape:
                raise ValueError("fields and km are contiguous 4-D tensors of one shape in the engine's dtype")
        if any(tuple(t.shape) != (km.shape[0],) for t in [kh2] + [ax[k] for k in names] + [ay[k] for k in names]):
            raise ValueError("kh2 and the coefficients are [n]")
        written = [fields[k].data_ptr() for k in names]
        read = {t.data_ptr() for t in [km, kh2] + [ax[k] for k in names] + [ay[k] for k in names]}
        if km.shape[0] and (len(set(written)) != len(written) or set(written) & read):
            raise ValueError("a field is another field, km, kh2 or a coefficient")
        for b, word in ((0, "itot"), (1, "jtot")):
            e = int(km.shape[1 + b])
            if axes >> b & 1 and e > 1 and not self.hmix_lines_per_block(e):
                top = next(k for k in range(e, 0, -1) if self.hmix_lines_per_block(k))
                raise _abi.SpcError(_abi.SPC_ERR_UNSUPPORTED, "les_hmix: %s %d above the %d cells of a line of which 16 fit the LDS" % (word, e, top))
        c = lambda t: numpy.ascontiguousarray(t.numpy())                                     # noqa: E731
        new = les_hmix({k: c(fields[k]) for k in names}, c(km), {k: c(ax[k]) for k in names}, {k: c(ay[k]) for k in names}, c(kh2), axes)
        for k in names:
            fields[k].copy_(torch.from_numpy(new[k]))

    def hmix_lines_per_block(self, n):
        return lines_per_block(n, 4 if self.dtype == torch.float32 else 8)


# -- the host twin of models.DeviceLESEnsemble after enable_mixing(implicit=True) ---------------------------------------------
class _HostHmix:
    """NumPy fields: the executable definition of what ``_mix`` does after enable_mixing(implicit=True): K24's eddy viscosity of
    the winds and theta under a cap of the type's largest value (so km is the closure's own and ``mixing_capped`` False), then ONE
    les_hmix on the fields among U, V (the winds' coefficients) and THL, QT, QR (the scalars') that exist, in place; K25, where
    enabled, mixes by that km; with ``vertical=True`` K15's face diffusivity comes from its slab means.  The mixin stands over the
    top of the twin chain of tests/les_vmix_ref.py, whose steps call ``_mix``; with implicit=False the step is theirs."""

    def enable_mixing(self, *a, implicit=False, kh_cap=None, **kw):
        super().enable_mixing(*a, **kw)
        self.mix_par["implicit"] = implicit
        self.mix_par["kh_cap"] = hm.KH_CAP if kh_cap is None else kh_cap

    def _mix(self, dt):
        f, par = self.fields3d, self.mix_par
        if not par["implicit"]:
            return super()._mix(dt)
        T = f["U"].dtype
        r = lambda a: numpy.ascontiguousarray(numpy.asarray(a).astype(T))                   # noqa: E731
        gx, gy, wind, scalar = mix.coefficients(dt, par["dx"], par["dy"], par["prandtl"], n=self.n)
        gz, bz, l2 = mix.profiles(self.zf_cache, self.zh_cache, par["dx"], par["dy"], par["cs"], par["prandtl"], par["theta_ref"], n=self.n)
        theta = f["THL"] if par["stability"] and "THL" in f else None
        huge = numpy.full(self.n, numpy.finfo(T).max, dtype=T)
        self._km, kmax = lxr.eddy(f["U"], f["V"], theta, r(gx), r(gy), r(gz), r(bz), r(l2), huge)[:2]
        self._kv = self._km
        keys = [k for k in self.MIX_KEYS if k in f]
        coef = {k: (r(wind[0]), r(wind[1])) if k in WINDS else (r(scalar[0]), r(scalar[1])) for k in keys}
        f.update(les_hmix({k: f[k] for k in keys}, self._km, {k: coef[k][0] for k in keys}, {k: coef[k][1] for k in keys},
                          r(hm.bound(self.n, par["kh_cap"]))))
        self.mixing_k_max = float(kmax.max())
        self.mixing_capped = False
        if par["vertical"]:
            m = numpy.asarray(slab_ref.slab_means(self._km), dtype=numpy.float64)
            faces = numpy.concatenate([m[:, :1], 0.5 * (m[:, :-1] + m[:, 1:])], axis=1)
            self._mix_kd = self.diffuse_par["k_bg"] + faces


class HostHmixLESEnsemble(_HostHmix, lvr.HostVmixLESEnsemble):
    """QL = max(QT - Qsat, 0)"""


class HostThermoHmixLESEnsemble(_HostHmix, lvr.HostThermoVmixLESEnsemble):
    """after enable_thermo(): K12's oracle wherever QL is read"""


#: "forced": K19, K21, K23 and K25 with the mixing; "k15": K15 by the slab mean of the uncapped km (vertical=True)
VARIANTS = {"plain": dict(), "all": dict(radiate=True, thermo=True, micro=True, transport=True, vmix=True),
            "forced": dict(thermo=True, transport=True, qt="strong", buoyancy=True, vmix=True),
            "k15": dict(diffuse=True, vertical=True)}
Z0M = 0.05


def ensemble_run(engine, n, device, implicit=True, vmix=False, vertical=False, thermo=False, micro=False, diffuse=False, radiate=False,
                 transport=False, qt=None, buoyancy=False, itot=4, jtot=5, nL=20, steps=3, change=None, mix_kw=None):
    """an ensemble with attached U, V, THL, QT (and Qsat, or thermo; QR with the microphysics) and enable_mixing(implicit=...)
    through ``steps`` calls of evolve_model_batched and one variability nudge (constantT) before the last; ``vmix``: K25 behind
    it; ``vertical`` (with ``diffuse``): K15 by the slab mean of km; ``change(ens, step)`` runs before every step.  After each of
    them every profile, the fields, km and the largest viscosity.  Returns (ens, list of records)"""
    from tests.les_harness import ensemble_case
    from tests import les_radiate_ref as lrr
    if device:
        cls = models.DeviceLESEnsemble
    else:
        cls = HostThermoHmixLESEnsemble if thermo else HostHmixLESEnsemble

    def enable(ens):
        if qt:
            ens.enable_qt_forcing(qt)
        if buoyancy:
            ens.enable_buoyancy()
        ens.enable_mixing(vertical=vertical, implicit=implicit, **dict({} if transport else {"dx": lxr.DX, "dy": 1.5 * lxr.DX}, **(mix_kw or {})))
        if vmix:
            ens.enable_vertical_mixing()
        if change:
            inner = ens.evolve_model_batched
            count = [0]

            def evolve(t):
                change(ens, count[0])
                count[0] += 1
                return inner(t)
            ens.evolve_model_batched = evolve

    def record(ens, rec):
        km = ens.get_eddy_viscosity_batched()
        rec["km"] = numpy.zeros(rec["field U"].shape) if km is None else numpy.array(host_of(km))
        if vmix:
            kv = ens.get_vertical_viscosity_batched()
            rec["kv"] = numpy.zeros(rec["field U"].shape) if kv is None else numpy.array(host_of(kv))
        rec["k max"] = numpy.array([-1.0 if ens.mixing_k_max is None else ens.mixing_k_max, float(bool(ens.mixing_capped))])
        if qt:
            counts = ens.get_qt_forcing_counts_batched()
            rec["counts"] = numpy.zeros((n, nL)) if counts is None else numpy.array(host_of(counts), dtype=numpy.float64)

    def forcings(rng, stack):
        more = dict(QL=rng.normal(0, 2e-8, (n, nL)), QLp=stack("ql_ref") * (0.5 + rng.random((n, nL)))) if qt else {}
        if vmix:
            more["Z0M_surf"] = Z0M * (0.5 + rng.random(n))
        return more
    advection = dict(dx=lxr.DX, dy=1.5 * lxr.DX, vertical=True, conservative=True, order=2) if transport else None
    return ensemble_case(engine, n, cls, thermo=thermo, micro=micro, diffuse=diffuse, advection=advection, forcings=forcings,
                         radiation=lrr.radiation_of(n, "f0", "f1") if radiate else None, enable=enable, record=record,
                         itot=itot, jtot=jtot, nL=nL, steps=steps)


def check_ensemble(one, engines, n, variant, **kw):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``: every profile, field and km bit-equal
    after each step; the implicit mixing is not the explicit one: the twin's last step differs from the same run with
    implicit=False, whose cap binds; the implicit run's never does, and K25 (where enabled) mixes by K24's own km"""
    from tests import les_micro_ref as lmr
    kw = dict(VARIANTS[variant], **kw)
    host = ensemble_run(one, n, False, **kw)[1]
    explicit = ensemble_run(one, n, False, implicit=False, **kw)[1]
    assert (host[-1]["field U"] != explicit[-1]["field U"]).any() and (host[-1]["km"] > 0).any()
    assert not any(r["k max"][1] for r in host) and any(r["k max"][1] for r in explicit)
    assert max(r["km"].max() for r in host) > max(r["km"].max() for r in explicit)
    for r in host[1:]:
        assert "kv" not in r or numpy.array_equal(r["kv"], r["km"])
    for engine in engines:
        lmr.same_logs(host, ensemble_run(engine, n, True, **kw)[1])
    return host
