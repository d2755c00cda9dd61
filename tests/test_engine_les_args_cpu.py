"""What ``Engine`` hands the library for the K10 - K23 methods, without a GPU: an ``Engine`` on host tensors whose ``_call``
records the symbol and a byte copy of the argument block and launches nothing.  Every member of the block is compared with the
tensors' addresses, the extents, the pitches and the codes; every refusal is compared with its exception type and full text;
and ``MultiDeviceEngine`` over three such engines, one of them without rows, forwards the five calls that return a "largest
value" as it always has."""
import ctypes

import pytest
import torch

import __graft_entry__ as ge
from sp_coupler_amd import _abi, buoyancy, microphysics, radiation, thermo
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from sp_coupler_amd.transfer import Sharded
from tests import les_advect_ref, les_transport2_ref, les_transport_ref, les_vadvect_ref

DTYPES = [torch.float64, torch.float32]
SHAPE = (2, 2, 3, 8)
PITCH = 11


class Recorder(Engine):
    """an Engine on the host: the real library for its symbols, no device, no launch"""

    def __init__(self, dtype):
        ge.build_hip()
        self.device, self.dtype, self.stream = torch.device("cpu"), dtype, None
        self.lib = _abi.load_library()
        self._exp_tab = self._es_tab = None
        self.calls = []

    def _call(self, fn, *args, stream=None):
        ref = args[0]
        self.calls.append((fn.__name__, ctypes.string_at(ctypes.addressof(ref._obj), ctypes.sizeof(ref._obj))))

    def last(self, cls):
        """(symbol, members of the block of the only call made since the last look)"""
        assert len(self.calls) == 1, [c[0] for c in self.calls]
        name, blob = self.calls.pop()
        assert len(blob) == ctypes.sizeof(cls)
        a = cls.from_buffer_copy(blob)
        got = {}
        for k, _ in cls._fields_:
            v = getattr(a, k)
            got[k] = list(v) if isinstance(v, ctypes.Array) else v
        return name, got


def members(cls, **set_):
    """every member of ``cls`` as the block of a call holds it: what ``set_`` names, None or 0 elsewhere; arrays padded"""
    want = {}
    for k, t in cls._fields_:
        if issubclass(t, ctypes.Array):
            fill = None if t._type_ is ctypes.c_void_p else 0
            v = list(set_.get(k, []))
            want[k] = v + [fill] * (t._length_ - len(v))
        else:
            want[k] = set_.get(k, None if t is ctypes.c_void_p else 0)
    assert not set(set_) - set(want), set(set_) - set(want)
    return want


def sfx(dtype):
    return "f32" if dtype == torch.float32 else "f64"


def texts(dtype, lines):
    """the literal texts below are those of a float64 engine; a float32 engine's differ in the two names only"""
    if dtype == torch.float64:
        return list(lines)
    swap = {"torch.float64": "torch.float32", "torch.float32": "torch.float64"}
    out = []
    for s in lines:
        parts = s.split("torch.float")
        out.append(parts[0] + "".join(swap["torch.float" + p[:2]] + p[2:] for p in parts[1:]))
    return out


def refused(eng, calls, want, kinds=None):
    """every call raises the exception of its row (ValueError unless ``kinds`` says otherwise) with exactly its text, and none
    of them reaches the library"""
    assert len(calls) == len(want), (len(calls), len(want))
    for i, (bad, text) in enumerate(zip(calls, want)):
        kind = (kinds or {}).get(i, ValueError)
        with pytest.raises(kind) as e:
            bad()
        assert type(e.value) is kind and str(e.value) == text, (i, str(e.value))
    assert eng.calls == []


class Case:
    """fields U (= u), V (= v), THL, QT of SHAPE with outputs, hx / hy, g / r with rows PITCH apart, and every optional output"""

    def __init__(self, dtype, shape=SHAPE, pitch=PITCH):
        n, itot, jtot, ktot = shape
        new = lambda *s: torch.rand(*s, dtype=dtype)                                            # noqa: E731
        self.shape, self.n = shape, n
        self.u, self.v = new(*shape), new(*shape)
        self.t = {"U": self.u, "V": self.v, "THL": new(*shape), "QT": new(*shape)}
        self.o = {k: torch.full_like(x, -77.0) for k, x in self.t.items()}
        self.hx, self.hy = new(n), new(n)
        self.g, self.r = new(n, pitch)[:, :ktot], new(n, pitch)[:, :ktot]
        self.m = torch.full_like(self.u, -77.0)
        self.ft = torch.full((4, n, itot, jtot), -77.0, dtype=dtype)
        self.cm = torch.full((n,), -5.0, dtype=dtype)

    def wind_args(self):
        return self.u, self.v, self.hx, self.hy

    def ptrs(self, names=("U", "V", "THL", "QT")):
        return dict(fields=[self.t[k].data_ptr() for k in names], out=[self.o[k].data_ptr() for k in names], n_fields=len(names))


FAMILY = {
    # method: (args class, takes g and r, the optional written tensors beyond cmax, limiters)
    "les_advect": (_abi.LesAdvectArgs, False, (), (None,)),
    "les_vadvect": (_abi.LesVadvectArgs, True, ("mtop",), (None,)),
    "les_transport": (_abi.LesTransportArgs, True, ("mtop", "ftop"), (None,)),
    "les_transport2": (_abi.LesTransport2Args, True, ("mtop", "ftop"), ("mc", "none")),
}


def family_call(eng, method, c, fields=None, out=None, limiter=None, **kw):
    cls, prof, extras, _ = FAMILY[method]
    a = [c.t if fields is None else fields, c.o if out is None else out, *c.wind_args()] + ([c.g, c.r] if prof else [])
    if limiter is not None:
        kw["limiter"] = limiter
    return getattr(eng, method)(*a, **kw)


def family_members(method, c, limiter=None, pitch=PITCH, **more):
    cls, prof, extras, _ = FAMILY[method]
    n, itot, jtot, ktot = c.shape
    want = dict(n_les=n, itot=itot, jtot=jtot, ktot=ktot, u=c.u.data_ptr(), v=c.v.data_ptr(), hx=c.hx.data_ptr(), hy=c.hy.data_ptr())
    if prof:
        want.update(g=c.g.data_ptr(), r=c.r.data_ptr(), pitch_prof=pitch)
    if limiter is not None:
        want["limiter"] = {"none": 0, "mc": 1}[limiter]
    want.update(more)
    return members(cls, **want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", list(FAMILY))
def test_the_four_methods_fill_every_member(method, dtype):
    cls, prof, extras, limiters = FAMILY[method]
    eng = Recorder(dtype)
    c = Case(dtype)
    opt = {k: {"mtop": c.m, "ftop": c.ft}[k] for k in extras}
    for limiter in limiters:
        got = family_call(eng, method, c, limiter=limiter, cmax=c.cm, **opt)
        assert got is c.cm
        assert eng.last(cls) == ("spc_%s_%s" % (method, sfx(dtype)),
                                 family_members(method, c, limiter, cmax=c.cm.data_ptr(), **{k: t.data_ptr() for k, t in opt.items()}, **c.ptrs()))
        got = family_call(eng, method, c, limiter=limiter, cmax=True, **opt)
        assert got is not c.cm and tuple(got.shape) == (2,) and got.dtype == dtype and got.device == eng.device
        assert eng.last(cls)[1]["cmax"] == got.data_ptr()
        assert family_call(eng, method, c, limiter=limiter, cmax=False, **opt) is None
        assert eng.last(cls)[1] == family_members(method, c, limiter, **{k: t.data_ptr() for k, t in opt.items()}, **c.ptrs())
        assert family_call(eng, method, c, limiter=limiter, cmax=None) is None
        assert eng.last(cls)[1] == family_members(method, c, limiter, **c.ptrs())
    if method == "les_transport2":                                                               # the default limiter is "mc"
        family_call(eng, method, c)
        assert eng.last(cls)[1]["limiter"] == _abi.SPC_LIMITER_MC
    # the order of the fields is the order of the dict, and out follows it whatever its own order
    names = ("QT", "U", "THL")
    family_call(eng, method, c, fields={k: c.t[k] for k in names}, out={k: c.o[k] for k in reversed(names)}, cmax=False, **({"mtop": c.m} if extras else {}))
    assert eng.last(cls)[1] == family_members(method, c, "mc" if method == "les_transport2" else None, **({"mtop": c.m.data_ptr()} if extras else {}), **c.ptrs(names))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", list(FAMILY))
def test_the_four_methods_at_their_edges(method, dtype):
    cls, prof, extras, limiters = FAMILY[method]
    eng = Recorder(dtype)
    lim = limiters[0]
    # one LES with a pitched profile row: the pitch of one row is its stride (_Checker.mat's n == 1 rule)
    c = Case(dtype, shape=(1, 2, 3, 8))
    c.g, c.r = torch.rand(3, PITCH, dtype=dtype)[1:2, :8], torch.rand(3, PITCH, dtype=dtype)[:1, :8]
    got = family_call(eng, method, c, limiter=lim)
    assert tuple(got.shape) == (1,)
    assert eng.last(cls)[1] == family_members(method, c, lim, cmax=got.data_ptr(), **c.ptrs())
    c.g = torch.rand(1, 8, dtype=dtype)
    family_call(eng, method, c, limiter=lim, cmax=False, **({"mtop": c.m} if extras else {}))
    assert eng.last(cls)[1] == family_members(method, c, lim, pitch=8, **({"mtop": c.m.data_ptr()} if extras else {}), **c.ptrs())
    # no LES: tensors that start at one address are not refused, and the call is made
    c = Case(dtype, shape=(0, 2, 3, 8))
    same = {k: c.u for k in c.t}
    got = family_call(eng, method, c, fields=same, out=same, limiter=lim, **({"mtop": c.u} if extras else {}))
    assert tuple(got.shape) == (0,)
    name, a = eng.last(cls)
    assert name == "spc_%s_%s" % (method, sfx(dtype)) and (a["n_les"], a["itot"], a["jtot"], a["ktot"], a["n_fields"]) == (0, 2, 3, 8, 4)
    # no field: the probe, with cmax alone and with mtop alone
    c = Case(dtype)
    got = family_call(eng, method, c, fields={}, out={}, limiter=lim)
    assert eng.last(cls)[1] == family_members(method, c, lim, cmax=got.data_ptr())
    if extras:
        assert family_call(eng, method, c, fields={}, out={}, limiter=lim, cmax=False, mtop=c.m) is None
        assert eng.last(cls)[1] == family_members(method, c, lim, mtop=c.m.data_ptr())
        assert family_call(eng, method, c, fields={}, out={}, limiter=lim, cmax=None, mtop=c.m) is None
        assert eng.last(cls)[1] == family_members(method, c, lim, mtop=c.m.data_ptr())


FIELD4 = ("%s must be a contiguous torch.float64 [n x itot x jtot x ktot] tensor of shape %s on cpu, got %s %s on %s")
F4 = lambda name, got, shape=SHAPE, dt="torch.float64", dev="cpu": FIELD4 % (name, shape, dt, got, dev)    # noqa: E731
ALIAS = "%s: an output is an input, %s or another output"
COMMON = {
    "alias": None,
    "mtop_shape": F4("mtop", (2, 1, 3, 8)),
    "out_missing": "%s: out holds ['THL', 'U', 'V'], the fields are ['QT', 'THL', 'U', 'V']",
    "many": "%s takes at most 6 fields per launch, got 7",
    "v_shape": F4("v", (2, 1, 3, 8)),
    "hx": "hx must be a contiguous vector of 2, got (1,)",
    "g": "g must have shape [2 x 8], got (1, 8)",
    "r": "r must have shape [2 x 8], got (2, 7)",
    "r_none": "r must be a torch.Tensor, got NoneType",
    "cmax3": "cmax must be a contiguous vector of 2, got (3,)",
    "strided": "QT must be a contiguous torch.float64 [n x itot x jtot x ktot] tensor of shape (2, 2, 3, 8) on cpu, got torch.float64 (2, 2, 3, 4) on cpu",
    "dtype": F4("QT", SHAPE, dt="torch.float32"),
    "device": F4("QT", SHAPE, dev="meta"),
}


def family_texts(method):
    """the texts of ``bad_calls`` of the method's module, in its order"""
    _, prof, extras, _ = FAMILY[method]
    alias = ALIAS % (method, ", ".join(("cmax",) + extras))
    head = {"les_advect": ["les_advect: no field and no cmax: nothing to do"] * 2}.get(
        method, ["%s: no field, no cmax and no mtop: nothing to do" % method] * 2)
    if method == "les_advect":
        return head + [alias] * 3 + [F4("out[QT]", SHAPE), COMMON["out_missing"] % method, COMMON["many"] % method, COMMON["v_shape"],
                                      COMMON["hx"], alias, COMMON["cmax3"], COMMON["strided"], COMMON["dtype"], COMMON["device"]]
    ftop = []
    if "ftop" in extras:
        head.append("%s: ftop without a field" % method)
        ftop = [FIELD4 % ("ftop", (4, 2, 2, 3), "torch.float64", (3, 2, 2, 3), "cpu"), FIELD4 % ("ftop", (4, 2, 2, 3), "torch.float64", (4, 1, 2, 3), "cpu"),
                FIELD4 % ("ftop", (4, 2, 2, 3), "torch.float32", (4, 2, 2, 3), "cpu")]
    if method == "les_transport2":
        head = ["les_transport2: limiter %s is none of ['mc', 'none']" % x for x in ("'minmod'", "1", "None", "'superbee'")] + head
    return head + [alias] * 5 + [COMMON["mtop_shape"]] + ftop + [COMMON["out_missing"] % method, COMMON["many"] % method, COMMON["v_shape"], COMMON["hx"],
                                                                 COMMON["g"], COMMON["r"], COMMON["r_none"], alias, COMMON["cmax3"], COMMON["strided"],
                                                                 COMMON["dtype"], COMMON["device"]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", list(FAMILY))
def test_the_four_methods_refuse_with_their_texts(method, dtype):
    eng = Recorder(dtype)
    c = Case(dtype, pitch=8)
    mod = {"les_advect": les_advect_ref, "les_vadvect": les_vadvect_ref, "les_transport": les_transport_ref, "les_transport2": les_transport2_ref}[method]
    more = {"les_advect": (), "les_vadvect": (c.g, c.r, c.m), "les_transport": (c.g, c.r, c.m, c.ft), "les_transport2": (c.g, c.r, c.m, c.ft)}[method]
    calls = mod.bad_calls(eng, c.t, c.o, c.u, c.v, c.hx, c.hy, *more)
    want = texts(dtype, family_texts(method))
    r_none = want.index(texts(dtype, [COMMON["r_none"]])[0]) if method != "les_advect" else -1
    refused(eng, calls, want, kinds={r_none: TypeError})
    for x in list(c.o.values()) + [c.m, c.ft]:
        assert bool((x == -77.0).all())
    # the empty extent, which the library's own check would refuse as well
    z = Case(dtype, shape=(2, 2, 3, 0), pitch=1)
    refused(eng, [lambda: family_call(eng, method, z)], ["%s: empty field shape (2, 2, 3, 0)" % method])


# -- the other K10 - K23 methods: one good call each, and the refusals whose code the methods share ----------------------------------
def prof(dtype, n=2, ktot=8, pitch=PITCH):
    return torch.rand(n, pitch, dtype=dtype)[:, :ktot]


def f4(dtype, shape=SHAPE):
    return torch.rand(*shape, dtype=dtype)


EMPTY = (2, 2, 3, 0)
PLANE = "%s must be a contiguous %s tensor of shape %s on cpu"


@pytest.mark.parametrize("dtype", DTYPES)
def test_slab_means_and_cloud_fraction(dtype):
    eng = Recorder(dtype)
    x, y = f4(dtype), f4(dtype)
    res = eng.slab_means({"A": x, "B": y})
    assert eng.last(_abi.SlabMeansArgs) == ("spc_slab_means_" + sfx(dtype), members(
        _abi.SlabMeansArgs, n_les=2, itot=2, jtot=3, ktot=8, n_fields=2, fields=[x.data_ptr(), y.data_ptr()],
        out=[res["A"].data_ptr(), res["B"].data_ptr()], pitch_out=8))
    o = {"A": prof(dtype), "B": prof(dtype)}
    assert eng.slab_means({"A": x, "B": y}, out=o)["B"] is o["B"]
    assert eng.last(_abi.SlabMeansArgs)[1]["pitch_out"] == PITCH
    idx = torch.zeros(2, 5, dtype=torch.int32)
    got = eng.slab_cloud_fraction(x, idx)
    assert eng.last(_abi.SlabCloudArgs) == ("spc_slab_cloud_fraction_" + sfx(dtype), members(
        _abi.SlabCloudArgs, n_les=2, itot=2, jtot=3, ktot=8, nG=5, ql=x.data_ptr(), idx=idx.data_ptr(), out=got.data_ptr(), pitch_idx=5, pitch_out=5))
    e = f4(dtype, EMPTY)
    refused(eng, [lambda: eng.slab_means({"A": e}), lambda: eng.slab_cloud_fraction(e, idx),
                  lambda: eng.slab_means({"A": x, "B": y}, out={"A": prof(dtype), "B": prof(dtype, pitch=12)})],
            ["slab_means: empty field shape (2, 2, 3, 0)", "slab_cloud_fraction: empty field shape (2, 2, 3, 0)",
             "slab_means: out[B] has row pitch 12, the others 11"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_les_advance(dtype):
    eng = Recorder(dtype)
    x, y, qs, ql = f4(dtype), f4(dtype), f4(dtype), f4(dtype)
    ty = prof(dtype)
    res = eng.les_advance({"THL": x, "QT": y}, {"QT": ty}, 2.5, qsat=qs, sat="QT", ql=ql)
    assert list(res) == ["THL", "QT", "QL"]
    assert eng.last(_abi.LesAdvanceArgs) == ("spc_les_advance_" + sfx(dtype), members(
        _abi.LesAdvanceArgs, n_les=2, itot=2, jtot=3, ktot=8, n_fields=2, fields=[x.data_ptr(), y.data_ptr()], tend=[None, ty.data_ptr()],
        mean=[res["THL"].data_ptr(), res["QT"].data_ptr()], pitch_tend=PITCH, pitch_mean=8, dt=2.5, sat_field=1, qsat=qs.data_ptr(),
        ql=ql.data_ptr(), ql_mean=res["QL"].data_ptr()))
    e = f4(dtype, EMPTY)
    refused(eng, [lambda: eng.les_advance({"THL": e}, {}, 1.0),
                  lambda: eng.les_advance({"THL": x, "QT": y}, {}, 1.0, means={"THL": prof(dtype), "QT": prof(dtype, pitch=9)}),
                  lambda: eng.les_advance({"THL": x, "QT": y}, {}, 1.0, qsat=qs, sat="QT", means={"QL": prof(dtype)})],
            ["les_advance: empty field shape (2, 2, 3, 0)", "les_advance: means[QT] has row pitch 9, the others 11",
             "les_advance: means[QL] has row pitch 11, the others 8"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_les_thermo(dtype):
    eng = Recorder(dtype)
    thl, qt, qs, ql, tt = (f4(dtype) for _ in range(5))
    p, ex = prof(dtype), prof(dtype)
    res = eng.les_thermo(thl, qt, p, ex, n_iter=3, qsat=qs, ql=ql, temp=tt)
    assert eng.last(_abi.LesThermoArgs) == ("spc_les_thermo_" + sfx(dtype), members(
        _abi.LesThermoArgs, n_les=2, itot=2, jtot=3, ktot=8, n_iter=3, thl=thl.data_ptr(), qt=qt.data_ptr(), presf=p.data_ptr(), ex=ex.data_ptr(),
        pitch_prof=PITCH, es_tab=eng._es_tab.data_ptr(), n_tab=eng._es_tab.numel(), t_lo=thermo.T_LO, inv_step=thermo.INV_STEP,
        qsat=qs.data_ptr(), ql=ql.data_ptr(), temp=tt.data_ptr(), ql_mean=res["QL"].data_ptr(), t_mean=res["T"].data_ptr(), pitch_mean=8))
    assert eng.les_thermo(thl, qt, p, ex, qsat=qs, ql=ql, means=False) == {}
    assert eng.last(_abi.LesThermoArgs)[1]["n_iter"] == thermo.DEFAULT_N_ITER
    e = f4(dtype, EMPTY)
    refused(eng, [lambda: eng.les_thermo(e, e, prof(dtype, ktot=0, pitch=1), prof(dtype, ktot=0, pitch=1)),
                  lambda: eng.les_thermo(thl, qt, p, ex, means={"QL": prof(dtype), "T": prof(dtype, pitch=9)})],
            ["les_thermo: empty field shape (2, 2, 3, 0)", "les_thermo: means[T] has row pitch 9, means[QL] 11"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_les_water_paths(dtype):
    eng = Recorder(dtype)
    x, y = f4(dtype), f4(dtype)
    w = prof(dtype)
    top, cover, oy = torch.zeros(2, 2, 3, dtype=torch.int32), torch.zeros(2, dtype=dtype), torch.zeros(2, 2, 3, dtype=dtype)
    res = eng.les_water_paths({"QL": x, "QT": y}, w, cloud="QL", out={"QT": oy}, top=top, cover=cover)
    assert res["QT"] is oy and res["top"] is top and res["cover"] is cover
    assert eng.last(_abi.WaterPathArgs) == ("spc_les_water_paths_" + sfx(dtype), members(
        _abi.WaterPathArgs, n_les=2, itot=2, jtot=3, ktot=8, n_fields=2, fields=[x.data_ptr(), y.data_ptr()], out=[res["QL"].data_ptr(), oy.data_ptr()],
        w=w.data_ptr(), pitch_w=PITCH, top=top.data_ptr(), cover=cover.data_ptr()))
    res = eng.les_water_paths({"QL": x}, w, cloud="QL", top=True)
    assert res["top"].dtype == torch.int32 and tuple(res["top"].shape) == (2, 2, 3)
    assert eng.last(_abi.WaterPathArgs)[1]["cloud_field"] == 0
    eng.les_water_paths({"QL": x}, w)
    assert eng.last(_abi.WaterPathArgs)[1]["cloud_field"] == -1
    n0 = f4(dtype, (0, 2, 3, 8))                                   # empty outputs all start at one address: skipped, not refused
    eng.les_water_paths({"A": n0, "B": n0[:]}, prof(dtype, n=0), out={"A": torch.zeros(0, 2, 3, dtype=dtype), "B": torch.zeros(0, 2, 3, dtype=dtype)})
    assert eng.last(_abi.WaterPathArgs)[1]["n_les"] == 0
    e = f4(dtype, EMPTY)
    alias = "les_water_paths: an output is an input or another output"
    refused(eng, [lambda: eng.les_water_paths({"QL": e}, prof(dtype, ktot=0, pitch=1)),
                  lambda: eng.les_water_paths({"QL": x}, w, out={"QL": oy[:, :1]}),
                  lambda: eng.les_water_paths({"QL": x}, w, cloud="QL", top=oy),
                  lambda: eng.les_water_paths({"QL": x}, w, cloud="QL", cover=torch.zeros(3, dtype=dtype)),
                  lambda: eng.les_water_paths({"QL": x, "QT": y}, w, out={"QL": oy, "QT": oy}),
                  lambda: eng.les_water_paths({"QL": x}, w, out={"QL": x[..., 0]}),
                  lambda: eng.les_water_paths({"QL": x}, w, cloud="QL", cover=w[:, 0])],
            texts(dtype, ["les_water_paths: empty field shape (2, 2, 3, 0)", "les_water_paths: " + PLANE % ("out[QL]", "torch.float64", (2, 2, 3)),
                          "les_water_paths: " + PLANE % ("top", "torch.int32", (2, 2, 3)), "les_water_paths: " + PLANE % ("cover", "torch.float64", (2,)),
                          alias, "les_water_paths: " + PLANE % ("out[QL]", "torch.float64", (2, 2, 3)),
                          "les_water_paths: " + PLANE % ("cover", "torch.float64", (2,))]))
    one, w1 = f4(dtype, (2, 1, 1, 1)), torch.rand(2, 1, dtype=dtype)
    refused(eng, [lambda: eng.les_water_paths({"QL": one}, w1, out={"QL": w1.view(2, 1, 1)})], [alias])


@pytest.mark.parametrize("dtype", DTYPES)
def test_les_microphysics(dtype):
    eng = Recorder(dtype)
    qt, ql, qr, qn, thl, tt = (f4(dtype) for _ in range(6))
    so, si, lc, w = (prof(dtype) for _ in range(4))
    rain = torch.zeros(2, 2, 3, dtype=dtype)
    res = eng.les_microphysics(qt, ql, qr, qn, so, si, lc, w, 3.0, thl=thl, temp=tt, rain=rain, k_acc=7.0)
    assert list(res) == ["QT", "QR", "THL", "QI"]
    assert eng.last(_abi.LesMicroArgs) == ("spc_les_microphysics_" + sfx(dtype), members(
        _abi.LesMicroArgs, n_les=2, itot=2, jtot=3, ktot=8, qt=qt.data_ptr(), ql=ql.data_ptr(), qr=qr.data_ptr(), qr_new=qn.data_ptr(),
        thl=thl.data_ptr(), temp=tt.data_ptr(), rain=rain.data_ptr(), sed_out=so.data_ptr(), sed_in=si.data_ptr(), lcpex=lc.data_ptr(), w=w.data_ptr(),
        pitch_prof=PITCH, dt=3.0, qc0=microphysics.QC0, k_auto=microphysics.K_AUTO, k_acc=7.0, t_up=microphysics.T_UP, t_dn=microphysics.T_DN,
        qt_mean=res["QT"].data_ptr(), thl_mean=res["THL"].data_ptr(), qr_mean=res["QR"].data_ptr(), qi_mean=res["QI"].data_ptr(), pitch_mean=8))
    n0 = f4(dtype, (0, 2, 3, 8))
    p0 = prof(dtype, n=0)
    assert eng.les_microphysics(n0, n0, n0, n0, p0, p0, p0, p0, 1.0, means=False) == {}       # no LES: nothing is refused as an alias
    assert eng.last(_abi.LesMicroArgs)[1]["n_les"] == 0
    e = f4(dtype, EMPTY)
    alias = "les_microphysics: a written array is an input or another written array (qr_new must not be qr)"
    refused(eng, [lambda: eng.les_microphysics(e, e, e, e, so, si, lc, w, 1.0),
                  lambda: eng.les_microphysics(qt, ql, qr, qn, so, si, lc, w, 1.0, rain=rain[:, :1]),
                  lambda: eng.les_microphysics(qt, ql, qr, qn, so, si, lc, w, 1.0, means={"QT": prof(dtype), "QR": prof(dtype, pitch=13)}),
                  lambda: eng.les_microphysics(qt, ql, qr, qr, so, si, lc, w, 1.0),
                  lambda: eng.les_microphysics(qt, ql, qr, qn, so, si, lc, w, 1.0, thl=qt),
                  lambda: eng.les_microphysics(qt, ql, qr, qn, so, si, lc, w, 1.0, means={"QT": so, "QR": prof(dtype)})],
            texts(dtype, ["les_microphysics: empty field shape (2, 2, 3, 0)", "les_microphysics: " + PLANE % ("rain", "torch.float64", (2, 2, 3)),
                          "les_microphysics: means[QR] has row pitch 13, the others 11", alias, alias, alias]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_les_diffuse(dtype):
    eng = Recorder(dtype)
    x, y = f4(dtype), f4(dtype)
    a, m, cp = prof(dtype), prof(dtype), prof(dtype)
    s0, fy = torch.rand(2, dtype=dtype), torch.rand(2, dtype=dtype)
    assert eng.les_diffuse({"THL": x, "QT": y}, a, m, cp, s0=s0, flux={"QT": fy}) is None
    assert eng.last(_abi.LesDiffuseArgs) == ("spc_les_diffuse_" + sfx(dtype), members(
        _abi.LesDiffuseArgs, n_les=2, itot=2, jtot=3, ktot=8, n_fields=2, fields=[x.data_ptr(), y.data_ptr()], flux=[None, fy.data_ptr()],
        a=a.data_ptr(), m=m.data_ptr(), cp=cp.data_ptr(), s0=s0.data_ptr(), pitch_prof=PITCH))
    n0, p0 = f4(dtype, (0, 2, 3, 8)), prof(dtype, n=0)
    eng.les_diffuse({"A": n0, "B": n0}, p0, p0, p0)
    assert eng.last(_abi.LesDiffuseArgs)[1]["n_les"] == 0
    e = f4(dtype, EMPTY)
    alias = "les_diffuse: a field is another field, a profile, s0 or a flux"
    refused(eng, [lambda: eng.les_diffuse({"THL": e}, a, m, cp), lambda: eng.les_diffuse({"THL": x, "QT": x}, a, m, cp),
                  lambda: eng.les_diffuse({"THL": x}, a, m, cp, s0=s0, flux={"THL": x.view(-1)[:2]})],
            ["les_diffuse: empty field shape (2, 2, 3, 0)", alias, alias])
    assert eng.diffuse_cols_per_block(160) == eng.lib.spc_les_diffuse_cols_per_block(160, 4 if dtype == torch.float32 else 8) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_les_radiate(dtype):
    eng = Recorder(dtype)
    ql, thl, flux = f4(dtype), f4(dtype), f4(dtype)
    w, c = prof(dtype), prof(dtype)
    f0, f1 = torch.rand(2, dtype=dtype), torch.rand(2, dtype=dtype)
    fsfc = torch.zeros(2, 2, 3, dtype=dtype)
    assert eng.les_radiate(ql, thl, w, c, f0, f1, flux=flux, fsfc=fsfc) is None
    assert eng.last(_abi.LesRadiateArgs) == ("spc_les_radiate_" + sfx(dtype), members(
        _abi.LesRadiateArgs, n_les=2, itot=2, jtot=3, ktot=8, n_tab=eng._exp_tab.numel(), ql=ql.data_ptr(), thl=thl.data_ptr(), w=w.data_ptr(),
        c=c.data_ptr(), pitch_prof=PITCH, f0=f0.data_ptr(), f1=f1.data_ptr(), etab=eng._exp_tab.data_ptr(), inv_step=radiation.INV_STEP,
        flux=flux.data_ptr(), fsfc=fsfc.data_ptr()))
    n0, p0, v0 = f4(dtype, (0, 2, 3, 8)), prof(dtype, n=0), torch.rand(0, dtype=dtype)
    eng.les_radiate(n0, n0, p0, p0, v0, v0)
    assert eng.last(_abi.LesRadiateArgs)[1]["n_les"] == 0
    e = f4(dtype, EMPTY)
    alias = "les_radiate: thl, flux or fsfc is an input or another of them"
    refused(eng, [lambda: eng.les_radiate(e, e, w, c, f0, f1), lambda: eng.les_radiate(ql, thl, w, c, f0, f1, fsfc=fsfc[:1]),
                  lambda: eng.les_radiate(ql, ql, w, c, f0, f1), lambda: eng.les_radiate(ql, thl, w, c, f0, f1, flux=thl)],
            texts(dtype, ["les_radiate: empty field shape (2, 2, 3, 0)", "les_radiate: " + PLANE % ("fsfc", "torch.float64", (2, 2, 3)), alias, alias]))
    assert eng.radiate_cols_per_block(160) == eng.lib.spc_les_radiate_cols_per_block(160, 4 if dtype == torch.float32 else 8) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_les_qt_local(dtype):
    eng = Recorder(dtype)
    qt, ql = f4(dtype), f4(dtype)
    a, qtm = prof(dtype), prof(dtype)
    got = eng.les_qt_local(qt, ql, a, qtm, split=3)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, 8)
    assert eng.last(_abi.LesQtLocalArgs) == ("spc_les_qt_local_" + sfx(dtype), members(
        _abi.LesQtLocalArgs, n_les=2, itot=2, jtot=3, ktot=8, split=3, qt=qt.data_ptr(), ql=ql.data_ptr(), a=a.data_ptr(), qtm=qtm.data_ptr(),
        pitch_prof=PITCH, count=got.data_ptr(), pitch_count=8))
    n0, p0 = f4(dtype, (0, 2, 3, 8)), prof(dtype, n=0)
    eng.les_qt_local(n0, n0, p0, p0)
    assert eng.last(_abi.LesQtLocalArgs)[1]["n_les"] == 0
    e = f4(dtype, EMPTY)
    refused(eng, [lambda: eng.les_qt_local(e, e, a, qtm), lambda: eng.les_qt_local(qt, qt, a, qtm)],
            ["les_qt_local: empty field shape (2, 2, 3, 0)", "les_qt_local: qt and ql are the same tensor"])
    assert eng.qt_local_split(2, 64, 64, 8) == eng.lib.spc_les_qt_local_split(2, 64, 64, 8, 4 if dtype == torch.float32 else 8) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_les_moments(dtype):
    eng = Recorder(dtype)
    w, x = f4(dtype), f4(dtype)
    res = eng.les_moments({"W": w, "QT": x}, pairs=[("W", "QT")], std=True, face="W")
    assert eng.last(_abi.LesMomentsArgs) == ("spc_les_moments_" + sfx(dtype), members(
        _abi.LesMomentsArgs, n_les=2, itot=2, jtot=3, ktot=8, n_fields=2, n_pairs=1, face_field=0, fields=[w.data_ptr(), x.data_ptr()], pair_a=[0], pair_b=[1],
        mean=[res["mean"][k].data_ptr() for k in ("W", "QT")], var=[res["var"][k].data_ptr() for k in ("W", "QT")],
        std=[res["std"][k].data_ptr() for k in ("W", "QT")], cov=[res["cov"][("W", "QT")].data_ptr()], pitch_out=8))
    e = f4(dtype, EMPTY)
    refused(eng, [lambda: eng.les_moments({"W": e}),
                  lambda: eng.les_moments({"W": w}, out={"mean": {"W": prof(dtype)}, "var": {"W": prof(dtype, pitch=10)}})],
            ["les_moments: empty field shape (2, 2, 3, 0)", "les_moments: out[var][W] has row pitch 10, the others 11"])


def buoyancy_case(dtype, shape=SHAPE):
    n, itot, jtot, ktot = shape
    c = dict(thl=f4(dtype, shape), qt=f4(dtype, shape), ql=f4(dtype, shape), u=f4(dtype, shape), v=f4(dtype, shape), hx=torch.rand(n, dtype=dtype),
             hy=torch.rand(n, dtype=dtype), t0=prof(dtype, n, ktot), lex=prof(dtype, n, ktot), s=prof(dtype, n, ktot), phi=f4(dtype, shape))
    return c


@pytest.mark.parametrize("dtype", DTYPES)
def test_les_buoyancy(dtype):
    eng = Recorder(dtype)
    c = buoyancy_case(dtype)
    psfc, am = torch.zeros(2, 2, 3, dtype=dtype), torch.zeros(2, dtype=dtype)
    assert eng.les_buoyancy(*c.values(), psfc=psfc, amax=am) is am
    want = dict(n_les=2, itot=2, jtot=3, ktot=8, pitch_prof=PITCH, c1=buoyancy.C1, c2=buoyancy.C2, **{k: t.data_ptr() for k, t in c.items()})
    assert eng.last(_abi.LesBuoyancyArgs) == ("spc_les_buoyancy_" + sfx(dtype), members(_abi.LesBuoyancyArgs, psfc=psfc.data_ptr(), amax=am.data_ptr(), **want))
    got = eng.les_buoyancy(*c.values())
    assert tuple(got.shape) == (2,) and got.dtype == dtype
    assert eng.last(_abi.LesBuoyancyArgs)[1] == members(_abi.LesBuoyancyArgs, amax=got.data_ptr(), **want)
    assert eng.les_buoyancy(*c.values(), amax=False) is None and eng.les_buoyancy(*dict(c, ql=None).values(), amax=None) is None
    assert eng.calls.pop()[0] == "spc_les_buoyancy_" + sfx(dtype) and eng.last(_abi.LesBuoyancyArgs)[1] == members(_abi.LesBuoyancyArgs, **want)
    z = buoyancy_case(dtype, (0, 2, 3, 8))
    got = eng.les_buoyancy(*dict(z, u=z["thl"], v=z["thl"], phi=z["thl"]).values())
    assert tuple(got.shape) == (0,) and eng.last(_abi.LesBuoyancyArgs)[1]["n_les"] == 0
    e = buoyancy_case(dtype, EMPTY)
    alias = "les_buoyancy: phi, u, v, psfc or amax is an input or another of them"
    refused(eng, [lambda: eng.les_buoyancy(*e.values()), lambda: eng.les_buoyancy(*c.values(), psfc=psfc[..., :2]),
                  lambda: eng.les_buoyancy(*c.values(), amax=torch.zeros(3, dtype=dtype)), lambda: eng.les_buoyancy(*dict(c, phi=c["u"]).values()),
                  lambda: eng.les_buoyancy(*dict(c, u=c["qt"]).values()), lambda: eng.les_buoyancy(*c.values(), amax=c["hx"]),
                  lambda: eng.les_buoyancy(*c.values(), psfc=psfc, amax=psfc.view(-1)[:2])],
            texts(dtype, ["les_buoyancy: empty field shape (2, 2, 3, 0)", "les_buoyancy: " + PLANE % ("psfc", "torch.float64", (2, 2, 3)),
                          "amax must be a contiguous vector of 2, got (3,)", alias, alias, alias, alias]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_columns_per_block_come_from_the_library(dtype):
    eng = Recorder(dtype)
    esize = 4 if dtype == torch.float32 else 8
    for ktot in (1, 160, 1279, 1280, 2559, 2560, 5000):
        for name in ("diffuse", "vadvect", "transport", "transport2", "radiate", "buoyancy"):
            got = getattr(eng, name + "_cols_per_block")(ktot)
            assert type(got) is int and got == getattr(eng.lib, "spc_les_%s_cols_per_block" % name)(ktot, esize), (name, ktot)
    assert eng.vadvect_cols_per_block(160) in (16, 32, 64) and eng.vadvect_cols_per_block(2560) == 0
    assert eng.advect_strip(2, 8, 8, 40) == (eng.lib.spc_les_advect_strip(8, 40, esize), eng.lib.spc_les_advect_rows(2, 8, 8, 40))


# -- MultiDeviceEngine: the five forwarders ------------------------------------------------------------------------------------------
FIVE = ("les_advect", "les_vadvect", "les_transport", "les_transport2", "les_buoyancy")


class Spy(Recorder):
    """a Recorder that also notes how the five methods were called"""

    def __init__(self, dtype):
        super().__init__(dtype)
        self.seen = []


def _spied(name):
    def method(self, *a, **kw):
        self.seen.append((name, a, kw))
        return getattr(Recorder, name)(self, *a, **kw)
    return method


for _name in FIVE:
    setattr(Spy, _name, _spied(_name))

BOUNDS = [0, 2, 2, 3]


def shard(t, rows_axis=0):
    return Sharded([t.narrow(rows_axis, BOUNDS[d], BOUNDS[d + 1] - BOUNDS[d]).contiguous() for d in range(3)], BOUNDS)


def multi_args(method, dtype):
    """(positional arguments, optional written tensors, the keyword of the largest value), plain tensors of three LES"""
    if method == "les_buoyancy":
        c = buoyancy_case(dtype, (3, 2, 3, 8))
        return list(c.values()), {"psfc": torch.zeros(3, 2, 3, dtype=dtype)}, "amax"
    cls, prof_, extras, _ = FAMILY[method]
    c = Case(dtype, shape=(3, 2, 3, 8))
    opt = {k: {"mtop": c.m, "ftop": c.ft}[k] for k in extras}
    return [c.t, c.o, *c.wind_args()] + ([c.g, c.r] if prof_ else []), opt, "cmax"


def sharded(x, key=None):
    if isinstance(x, dict):
        return {k: sharded(v) for k, v in x.items()}
    return shard(x, 1 if key == "ftop" else 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", FIVE)
def test_multi_device_engine_forwards_the_five(method, dtype):
    engines = [Spy(dtype) for _ in range(3)]
    multi = MultiDeviceEngine(engines, min_cols_per_device=1)
    pos, opt, key = multi_args(method, dtype)
    more = {"limiter": "none"} if method == "les_transport2" else {}
    # plain tensors: the primary engine alone, with what the caller gave
    top = torch.zeros(3, dtype=dtype)
    for given in (True, top, False, None):
        got = getattr(multi, method)(*pos, **opt, **more, **{key: given})
        assert (got is top) if given is top else (got is None) if not given else (isinstance(got, torch.Tensor) and tuple(got.shape) == (3,))
        (name, a, kw), = engines[0].seen
        assert name == method and len(a) == len(pos) and all(x is y for x, y in zip(a, pos))
        assert set(kw) == set(opt) | set(more) | {key} and kw[key] is given and all(kw[k] is t for k, t in opt.items()) and all(kw[k] == v for k, v in more.items())
        assert [len(e.seen) for e in engines] == [1, 0, 0] and [len(e.calls) for e in engines] == [1, 0, 0]
        engines[0].seen.clear()
        engines[0].calls.clear()
    # Sharded row blocks: one call on every engine that holds rows, none on the empty one
    spos = [sharded(x) for x in pos]
    sopt = {k: sharded(t, k) for k, t in opt.items()}
    stop = shard(top)
    for given in (True, stop, False, None):
        got = getattr(multi, method)(*spos, **sopt, **more, **{key: given})
        if given is stop:
            assert got is stop
        elif not given:
            assert got is None
        else:
            assert isinstance(got, Sharded) and got.bounds == BOUNDS and [tuple(p.shape) for p in got.parts] == [(2,), (0,), (1,)]
        assert [len(e.seen) for e in engines] == [1, 0, 1] and [len(e.calls) for e in engines] == [1, 0, 1]
        for d in (0, 2):
            (name, a, kw), = engines[d].seen
            assert name == method and len(a) == len(pos)
            for x, s in zip(a, spos):
                assert all(x[k] is s[k].parts[d] for k in s) if isinstance(s, dict) else x is s.parts[d]
            assert set(kw) == set(opt) | set(more) | {key} and all(kw[k] is sopt[k].parts[d] for k in opt) and all(kw[k] == v for k, v in more.items())
            assert kw[key] is (stop.parts[d] if given is stop else given)
            if given is True:
                assert got.parts[d].data_ptr() == Recorder.last(engines[d], FAMILY[method][0] if method in FAMILY else _abi.LesBuoyancyArgs)[1][key]
            engines[d].seen.clear()
            engines[d].calls.clear()
