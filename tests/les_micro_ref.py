"""NumPy oracle of K14 (include/spc.h: spc_les_microphysics_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_micro_gpu.py (each takes an engine: tools/mutation_control.py --micro hands them the engines of its mutant
libraries), the host twin of models.DeviceLESEnsemble's microphysics mode and an oracle-backed engine with
``les_microphysics`` for the CPU suite.

The oracle spells the rule out one operation per NumPy call in the element type, so nothing fuses.  Every device array of the
bodies is the LEADING part of a poisoned buffer (tests/les_harness.Poisoned); the bytes behind it (and in front of a view
off the 16-byte grid) are checked after the launch."""
import numpy
import torch

from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import microphysics as mp
from tests import les_advance_ref as lar
from tests import les_thermo_ref as ltr
from tests import les_water_paths_ref as wpr
from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, chain_cases, counted_cus, host_of, np_of, on_both, run_bodies, twin_kw)
from tests.test_vnudge import make_les_fields

PLANES = [(1, 1), (3, 5), (8, 8)]
#: the k + 1 neighbour inside a lane's vector, in the next lane and in the next wave (64 lanes of 2 doubles / 4 floats, or of
#: one element), odd sizes (one element per lane) and multiples of 4 (16-byte accesses in both types)
KTOTS = [2, 3, 7, 8, 9, 63, 64, 65, 66, 127, 128, 129, 160]
NS = [1, 2, 5]
#: itot * jtot = 1 ... 17: every remainder of the look-ahead (batches of 4 rows), one, two and more whole batches
ROW_PLANES = lar.PLANES
FIELD_OUTS = ("qt", "thl", "qr_new", "rain")
MEAN_OUTS = ("qt_mean", "thl_mean", "qr_mean", "qi_mean")
MEAN_KEYS = {"QT": "qt_mean", "THL": "thl_mean", "QR": "qr_mean", "QI": "qi_mean"}
CONSTANTS = dict(qc0=mp.QC0, k_auto=mp.K_AUTO, k_acc=mp.K_ACC, t_up=mp.T_UP, t_dn=mp.T_DN)


# -- the rule --------------------------------------------------------------------------------------------------------------
def les_micro(qt, ql, qr, sed_out, sed_in, lcpex, w, dt, thl=None, temp=None, rain=None, qc0=mp.QC0, k_auto=mp.K_AUTO, k_acc=mp.K_ACC,
              t_up=mp.T_UP, t_dn=mp.T_DN):
    """dict qt, qr_new (thl, rain where given) -- new arrays, the arguments are not modified --, s and qs of every cell, qi
    where temp is given, and qt_mean, qr_mean (thl_mean, qi_mean) [n x ktot] by k_slab_means' rule.  Fields
    [n x itot x jtot x ktot] of ONE dtype T, profiles [n x ktot], rain [n x itot x jtot]"""
    T = qt.dtype.type
    assert qt.shape[-1] >= 2 and all(a.dtype == qt.dtype for a in (ql, qr, sed_out, sed_in, lcpex, w))
    c0, tu, td = T(qc0), T(t_up), T(t_dn)
    ka = T(T(k_auto) * T(dt))
    kc = T(T(k_acc) * T(dt))
    den = T(tu - td)
    b = lambda a: a[:, None, None, :]                                                    # noqa: E731
    with numpy.errstate(all="ignore"):
        up = numpy.zeros_like(qr)
        up[..., :-1] = qr[..., 1:]                               # the OLD qr of the level above; +0.0 at the top
        out = b(sed_out) * qr
        rest = qr - out
        inn = b(sed_in) * up
        qs = rest + inn
        d = ql - c0
        x = numpy.where(d > 0, d, numpy.where(d != d, d, T(0)))
        au = ka * x
        kq = kc * ql
        ac = kq * qs
        s = au + ac
        s = numpy.where(s > ql, ql, s).astype(qt.dtype)
        res = {"qt": (qt - s).astype(qt.dtype), "qr_new": (qs + s).astype(qt.dtype), "s": s, "qs": qs.astype(qt.dtype)}
        if thl is not None:
            heat = b(lcpex) * s
            res["thl"] = (thl + heat).astype(qt.dtype)
        if rain is not None:
            out0 = sed_out[:, 0][:, None, None] * qr[..., 0]
            res["rain"] = (rain + out0 * w[:, 0][:, None, None]).astype(qt.dtype)
        if temp is not None:
            num = tu - temp
            fi = numpy.where(temp >= tu, T(0), numpy.where(temp <= td, T(1), num / den))
            rem = ql - s
            res["qi"] = (rem * fi).astype(qt.dtype)
    for k, name in (("qt", "qt_mean"), ("thl", "thl_mean"), ("qr_new", "qr_mean"), ("qi", "qi_mean")):
        if k in res:
            res[name] = lar.mean_rows(res[k])
    return res


def column_water(qt, qr, w, rain):
    """float64 [n x itot x jtot]: sum_k((qt + qr) * w) + rain -- what the rule conserves but for its roundings"""
    f = lambda a: numpy.asarray(a, dtype=numpy.float64)                                   # noqa: E731
    return ((f(qt) + f(qr)) * f(w)[:, None, None, :]).sum(axis=3) + f(rain)


# -- inputs ------------------------------------------------------------------------------------------------------------------
def grid_profiles(n, ktot, dtype, rng, dt, v_fall=mp.V_FALL):
    """(sed_out, sed_in, lcpex, w) in ``dtype`` of LES with layers of 40 ... 100 m, by microphysics.profiles"""
    dz = 40.0 + 60.0 * rng.random((n, ktot))
    zh = numpy.concatenate([numpy.zeros((n, 1)), numpy.cumsum(dz, axis=1)[:, :-1]], axis=1)
    dz[:, -1] = dz[:, -2]                                         # (the top layer takes the thickness of the layer below it)
    zf = zh + 0.5 * dz
    rhobf = 1.2 * numpy.exp(-zf / 9000.0)
    presf = 1e5 * numpy.exp(-zf / 8000.0)
    return tuple(numpy.ascontiguousarray(a.astype(dtype)) for a in mp.profiles(zh, zf, rhobf, presf, dt, v_fall))


def case(shape, dtype, seed=0, dt=60.0, neighbour=False, special=False):
    """dict of the arguments of ``les_micro``: ql up to 2e-3 in 30 % of the cells, qr up to 1e-3 in 30 %, temp 240 ... 280 K
    (below t_dn, between, above t_up), a rain plane that already holds something.  ``neighbour``: level 0 of every column
    holds LARGE qr (0.3 ... 0.7), so the element that follows the top level of a column in memory -- level 0 of the next
    column, of the next LES behind the last column -- is never what the top level may read, and sed_in of the top level is
    0.5, so that whatever is read there shows.  ``special``: NaN, +-inf and -0.0
    in ql, qr and temp, temp exactly t_up and t_dn, ql = qt = -0.0, in plane points of their own (itot * jtot >= 12)"""
    dtype = numpy.dtype(dtype).type
    n, itot, jtot, ktot = shape
    rng = numpy.random.default_rng(3000 + seed + 7 * ktot + itot * jtot + 31 * n)
    prof = grid_profiles(n, ktot, dtype, rng, dt)
    ql = numpy.where(rng.random(shape) < 0.3, 2e-3 * rng.random(shape), 0.0).astype(dtype)
    qr = numpy.where(rng.random(shape) < 0.3, 1e-3 * rng.random(shape), 0.0).astype(dtype)
    qt = (8e-3 + 4e-3 * rng.random(shape)).astype(dtype)
    thl = (290.0 + 5.0 * rng.standard_normal(shape)).astype(dtype)
    temp = (240.0 + 40.0 * rng.random(shape)).astype(dtype)
    rain = (1e-2 * rng.random(shape[:3])).astype(dtype)
    if neighbour:
        qr[..., 0] = (0.3 + 0.4 * rng.random(shape[:3])).astype(dtype)
        prof[1][:, -1] = 0.5                                     # (profiles() has sed_in == 0 at the top, which would hide what is read there)
    if special:
        assert itot * jtot >= 12
        pt = lambda r: (slice(None), r // jtot, r % jtot)                                  # noqa: E731
        ql[pt(0)] = numpy.nan
        qr[pt(1)] = numpy.nan
        temp[pt(2)] = numpy.nan
        ql[pt(3)] = numpy.inf
        qr[pt(4)] = numpy.inf
        temp[pt(5)][..., ::2] = numpy.inf
        temp[pt(5)][..., 1::2] = -numpy.inf
        ql[pt(6)] = -numpy.inf
        qr[pt(7)] = -0.0
        temp[pt(8)] = -0.0
        ql[pt(9)], qt[pt(9)], qr[pt(9)] = -0.0, -0.0, 0.0        # s == +0.0 where ql == -0.0: qt keeps its -0.0 (the cap is s > ql)
        temp[pt(10)], ql[pt(10)] = mp.T_UP, 1e-3                 # exactly t_up: no ice
        temp[pt(11)], ql[pt(11)] = mp.T_DN, 1e-3                 # exactly t_dn: all ice
        qr[:, 0, 0, ktot - 1] = -numpy.inf                       # (a single cell: its column and the level below it)
    return dict(qt=qt, ql=ql, qr=qr, thl=thl, temp=temp, rain=rain, prof=prof, dt=dt)


def cap_case(shape, dtype, seed=0):
    """dt = 3600: the autoconversion of an hour exceeds the cloud water, s is capped at ql in the cloudy cells"""
    return case(shape, dtype, seed=seed + 500, dt=3600.0)


def oracle(c, thl=True, temp=True, rain=True, **kw):
    return les_micro(c["qt"], c["ql"], c["qr"], *c["prof"], c["dt"], thl=c["thl"] if thl else None, temp=c["temp"] if temp else None,
                     rain=c["rain"] if rain else None, **kw)


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one launch through ``eng.les_microphysics`` with every array inside a poisoned buffer; ``check`` compares qt, thl,
    qr_new, rain and the means with the oracle bit for bit, ql, qr, temp and the profiles with what was uploaded, and looks at
    the bytes around every array"""

    def __init__(self, eng, c, want_thl=True, want_temp=True, want_rain=True, means=True, lead=0, pad=0, lead_rows=0, **kw):
        self.eng, self.c, self.pad, self.kw = eng, c, pad, kw
        self.opt = dict(thl=want_thl, temp=want_temp, rain=want_rain)
        dtype, shape = c["qt"].dtype, c["qt"].shape
        n, ktot = shape[0], shape[-1]
        self.mem = Poisoned(eng)
        put = self.mem.put
        rows = lambda tag, a, poison, lead: self.mem.rows(tag, a, poison, lead, pad)        # noqa: E731
        self.dev = {k: put(k, c[k], float("nan"), lead) for k in ("qt", "ql", "qr") + (("thl",) if want_thl else ()) + (("temp",) if want_temp else ())}
        self.dev["qr_new"] = put("qr_new", numpy.full(shape, -3.0, dtype), -5.0, lead)
        self.drain = put("rain", c["rain"], float("nan"), lead) if want_rain else None
        self.dprof = [rows("prof %d" % i, a, 1e30, lead_rows) for i, a in enumerate(c["prof"])]
        names = ["QT", "QR"] + (["THL"] if want_thl else []) + (["QI"] if want_temp else [])
        self.dmeans = {k: rows("mean " + k, numpy.full((n, ktot), -1.0, dtype), -7.0, lead_rows) for k in names} if means else False
        self.got = eng.les_microphysics(self.dev["qt"], self.dev["ql"], self.dev["qr"], self.dev["qr_new"], *self.dprof, c["dt"],
                                        thl=self.dev.get("thl"), temp=self.dev.get("temp"), rain=self.drain, means=self.dmeans, **kw)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def check(self, what=""):
        c = self.c
        want = oracle(c, **self.opt, **self.kw)
        for k in ("qt", "qr_new") + (("thl",) if self.opt["thl"] else ()):
            assert_bits("%s %s" % (what, k), self.dev[k].cpu().numpy(), want[k])
        if self.drain is not None:
            assert_bits("%s rain" % what, self.drain.cpu().numpy(), want["rain"])
        if self.dmeans:
            assert sorted(self.got) == sorted(self.dmeans), (what, sorted(self.got))
            for k, t in self.dmeans.items():
                assert self.got[k].data_ptr() == t.data_ptr(), (what, k)
                assert_bits("%s %s" % (what, MEAN_KEYS[k]), t.cpu().numpy(), want[MEAN_KEYS[k]])
        else:
            assert self.got == {}, (what, self.got)
        same = Poisoned.read_only
        for k in ("ql", "qr") + (("temp",) if self.opt["temp"] else ()):
            assert same(self.dev[k], c[k]), (what, k, "read only")
        for t, a in zip(self.dprof, c["prof"]):
            assert same(t, a), (what, "a profile", "read only")
        self.mem.check_around(what)
        return want


def raw_launch(eng, c, null=(), **consts):
    """spc_les_microphysics_* itself, with the arguments named in ``null`` NULL (``Engine.les_microphysics`` always asks for
    every mean it can): (rc, dict of host arrays named like the oracle's, None for what was not passed)"""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    n, itot, jtot, ktot = c["qt"].shape
    t = {k: dev(c[k]) for k in ("qt", "ql", "qr", "thl", "temp", "rain")}
    t["qr_new"] = torch.full(c["qt"].shape, -3.0, dtype=eng.dtype, device=eng.device)
    t.update({k: dev(a) for k, a in zip(("sed_out", "sed_in", "lcpex", "w"), c["prof"])})
    t.update({k: torch.full((n, ktot), -3.0, dtype=eng.dtype, device=eng.device) for k in MEAN_OUTS})
    a = _abi.LesMicroArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.dt = n, itot, jtot, ktot, c["dt"]
    a.pitch_prof = a.pitch_mean = ktot
    for k, v in dict(CONSTANTS, **consts).items():
        setattr(a, k, v)
    for k, v in t.items():
        if k not in null:
            setattr(a, k, v.data_ptr())
    rc = abi_call(eng, "spc_les_microphysics", a)
    return rc, {k: (None if k in null else v.cpu().numpy()) for k, v in t.items()}


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, n=3):
    """qt, thl, qr_new, rain and the four means against the oracle; rain forms, falls and reaches the ground"""
    c = case((n,) + tuple(plane) + (ktot,), np_of(eng))
    want = Run(eng, c).check("n %d plane %s ktot %d" % (n, plane, ktot))
    if c["qt"].size >= 1000:
        assert (want["s"] > 0).any() and (want["s"] == 0).any() and (want["rain"] != c["rain"]).any()
        assert (want["qi"] > 0).any() and (want["qi"] < c["ql"] - want["s"]).any()


def check_neighbour(eng, ktot, n):
    """the top level of every column is followed in memory by a level 0 that holds large qr (for the last column of LES l:
    level 0 of LES l + 1; behind the last LES: the NaN tail of the buffer)"""
    c = case((n, 3, 5, ktot), np_of(eng), seed=1, neighbour=True)
    want = Run(eng, c).check("neighbour n %d ktot %d" % (n, ktot))
    assert numpy.isfinite(want["qr_new"]).all() and (want["qr_new"][..., ktot - 1] < 4e-3).all() and (c["qr"][..., 0] >= 0.3).all()


def check_rows(eng, ktot):
    """itot * jtot = 1 ... 17: whole batches of the look-ahead, single rows behind them, fewer rows than one batch.
    ktot picks the instantiation (160: 16-byte accesses; 33: one element per lane)"""
    for plane in ROW_PLANES:
        Run(eng, case((2,) + plane + (ktot,), np_of(eng), seed=3)).check("plane %s ktot %d" % (plane, ktot))


def check_alignment(eng, lead, lead_rows, pad):
    """views one (or more) elements off the 16-byte grid and pitched profiles / means: one element per lane"""
    c = case((3, 3, 5, 64), np_of(eng), seed=lead + 10 * lead_rows + 100 * pad, neighbour=True)
    Run(eng, c, lead=lead, lead_rows=lead_rows, pad=pad).check("lead %d %d pad %d" % (lead, lead_rows, pad))


def check_optional(eng):
    """thl, temp and rain NULL through the engine, no means; each optional pointer NULL on its own through the C ABI"""
    dtype = np_of(eng)
    c = case((2, 3, 5, 64), dtype, seed=5)
    Run(eng, c, want_thl=False).check("thl NULL")
    Run(eng, c, want_temp=False).check("temp NULL")
    Run(eng, c, want_rain=False).check("rain NULL")
    Run(eng, c, means=False).check("no means")
    Run(eng, c, qc0=1e-4, k_auto=5e-3, k_acc=1.0, t_up=270.0, t_dn=250.0).check("constants of the caller")
    for shape in ((2, 3, 5, 64), (2, 3, 3, 7)):
        c = case(shape, dtype, seed=6)
        for null in (("thl", "thl_mean"), ("temp", "qi_mean"), ("rain",), ("qt_mean",), ("thl_mean",), ("qr_mean",), ("qi_mean",),
                     ("rain", "w"), ("thl", "thl_mean", "lcpex"), MEAN_OUTS):
            rc, got = raw_launch(eng, c, null)
            assert rc == 0, (null, rc)
            want = oracle(c, thl="thl" not in null, temp="temp" not in null, rain="rain" not in null)
            for k in FIELD_OUTS + MEAN_OUTS:
                if got[k] is not None:
                    assert_bits("NULL %s: %s" % (null, k), got[k], want[k])
            for k in ("ql", "qr", "temp", "thl"):
                if got[k] is not None and k not in want:
                    assert_bits("NULL %s: %s untouched" % (null, k), got[k], c[k])


def check_special(eng):
    """NaN, +-inf and -0.0 in ql, qr and temp; temp exactly t_up and t_dn; ql = qt = -0.0; a NaN threshold"""
    for ktot in (7, 64):
        c = case((3, 3, 5, ktot), np_of(eng), seed=2, special=True)
        want = Run(eng, c).check("special ktot %d" % ktot)
        assert numpy.isnan(want["qt"][:, 0, 0]).all() and numpy.isnan(want["qr_new"][:, 0, 1]).all() and numpy.isnan(want["qi_mean"]).all()
        assert numpy.signbit(want["qt"][:, 1, 4]).all() and (want["qt"][:, 1, 4] == 0).all()         # pt(9) of a 3 x 5 plane
        c = case((3, 3, 5, ktot), np_of(eng), seed=4)
        want = Run(eng, c, qc0=float("nan")).check("qc0 NaN, ktot %d" % ktot)
        assert numpy.isnan(want["s"]).all()


def check_cap(eng):
    """dt = 3600: s reaches ql"""
    for ktot in (7, 160):
        c = cap_case((2, 3, 5, ktot), np_of(eng))
        want = Run(eng, c).check("cap ktot %d" % ktot)
        assert ((want["s"] == c["ql"]) & (c["ql"] > 0)).any()


def check_refusals(eng):
    """n = 0 is a no-op, ktot = 1 is refused, so is every aliased pair that is written"""
    dtype = np_of(eng)
    c = case((2, 2, 3, 8), dtype, seed=9)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    t = {k: dev(c[k]) for k in ("qt", "ql", "qr", "thl", "temp", "rain")}
    p = [dev(a) for a in c["prof"]]
    new = torch.zeros_like(t["qt"])
    call = lambda qt, ql, qr, qn, **kw: eng.les_microphysics(qt, ql, qr, qn, *p, 60.0, **kw)  # noqa: E731
    res = eng.les_microphysics(t["qt"][:0], t["ql"][:0], t["qr"][:0], new[:0], *[a[:0] for a in p], 60.0, thl=t["thl"][:0], rain=t["rain"][:0])
    assert sorted(res) == ["QR", "QT", "THL"] and all(v.shape == (0, 8) for v in res.values())
    for bad in (lambda: call(t["qt"], t["ql"], t["qr"], t["qr"]),                            # qr_new is qr
                lambda: call(t["qt"], t["ql"], t["qr"], t["qt"]),
                lambda: call(t["qt"], t["ql"], t["qr"], t["ql"]),
                lambda: call(t["qt"], t["qt"], t["qr"], new),                                # qt is written, ql is read
                lambda: call(t["qt"], t["ql"], t["qr"], new, thl=t["qt"]),
                lambda: call(t["qt"], t["ql"], t["qr"], new, thl=new),
                lambda: call(t["qt"], t["ql"], t["qr"], new, temp=new),
                lambda: call(t["qt"], t["ql"], t["qr"], new, means={"QT": p[0]}),
                lambda: call(t["qt"], t["ql"], t["qr"], new, means={"QT": p[0].clone(), "QR": None, "U": p[1].clone()}),
                lambda: call(t["qt"], t["ql"], t["qr"][..., ::2], new),                      # another shape / not contiguous
                lambda: call(t["qt"], t["ql"].to(torch.float64 if eng.dtype == torch.float32 else torch.float32), t["qr"], new),
                lambda: call(t["qt"], t["ql"].cpu(), t["qr"], new),
                lambda: call(t["qt"], t["ql"], t["qr"], new, rain=t["rain"][:, :1]),
                lambda: eng.les_microphysics(t["qt"], t["ql"], t["qr"], new, p[0], p[1][:, :4], p[2], p[3], 60.0)):
        try:
            bad()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad call was not refused")
    a1 = {k: v[..., :1].contiguous() for k, v in t.items()}
    try:
        eng.les_microphysics(a1["qt"], a1["ql"], a1["qr"], torch.zeros_like(a1["qt"]), *[a[:, :1].contiguous() for a in p], 60.0)
    except _abi.SpcError as e:
        assert e.code == _abi.SPC_ERR_UNSUPPORTED and "ktot == 1" in str(e)
    else:
        raise AssertionError("ktot == 1 was not refused")
    rc, _ = raw_launch(eng, c, ("temp",))                                                     # qi_mean without temp
    assert rc == _abi.SPC_ERR_INVALID_ARGUMENT and b"qi_mean without temp" in eng.lib.spc_last_error()
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    for k in ("qt", "ql", "qr", "thl", "temp", "rain"):                                       # no refused call touched anything
        assert_bits("refused: " + k, t[k].cpu().numpy(), c[k])


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    c = case((n, 3, 5, 40), np_of(one), seed=n, neighbour=True)
    want = oracle(c)
    res = {}
    for tag, eng, up in on_both(one, multi, n):
        t = {k: up(c[k]) for k in ("qt", "ql", "qr", "thl", "temp", "rain")}
        t["qr_new"] = up(numpy.full(c["qt"].shape, -3.0, dtype=c["qt"].dtype))
        m = eng.les_microphysics(t["qt"], t["ql"], t["qr"], t["qr_new"], *[up(a) for a in c["prof"]], c["dt"], thl=t["thl"], temp=t["temp"],
                                 rain=t["rain"])
        res[tag] = (t, m)
    multi.synchronize()
    blocks = blocks_of(res["multi"][0]["qt"], multi, n)
    for tag, (t, m) in res.items():
        assert sorted(m) == ["QI", "QR", "QT", "THL"]
        for k in FIELD_OUTS:
            assert_bits("%s %s" % (tag, k), host_of(t[k]), want[k])
        for k, name in MEAN_KEYS.items():
            assert_bits("%s %s" % (tag, name), host_of(m[k]), want[name])
    return blocks


def check_many_waves(eng):
    """the instantiations a launch of more than one wave per SIMD takes (2 rows per batch), which the sizes of the other bodies
    never reach on a whole card: parity, the top level, every remainder of the look-ahead and views off the 16-byte grid again,
    on 5 ... 40 waves with one compute unit counted; a launch of 1 ... 4 waves (ktot 7: 21 lanes) still takes the others"""
    with counted_cus(1):
        for plane in ((3, 5), (8, 8)):
            for ktot in (7, 64, 129, 160):
                check_parity(eng, plane, ktot, n=5)
        for ktot in (66, 128, 129):
            check_neighbour(eng, ktot, 5)
        for ktot in (160, 65):
            for plane in ROW_PLANES:
                Run(eng, case((5,) + plane + (ktot,), np_of(eng), seed=8, neighbour=True)).check("many waves: plane %s ktot %d" % (plane, ktot))
        c = case((5, 3, 5, 128), np_of(eng), seed=12, neighbour=True)
        Run(eng, c, lead=1, lead_rows=1, pad=3).check("many waves: off the grid")
        check_special(eng)


def check_chain(eng):
    """the cases of the lane's walk (les_harness.chain_cases) for the batches of 4 rows of a launch of few waves; then, with one
    compute unit counted as in many_waves, nij = 1 ... 5 for the batches of 2 rows at five LES of 256 and 255 levels (5 to 20
    waves: above one wave per SIMD), on and off the 16-byte grid"""
    dtype = np_of(eng)
    for shape, lead in chain_cases(4, dtype):
        Run(eng, case(shape, dtype, seed=9, neighbour=True), lead=lead, lead_rows=lead).check("chain %s lead %d" % (shape, lead))
    with counted_cus(1):
        for nij in range(1, 6):
            for ktot, lead in ((256, 0), (255, 0), (256, 1)):
                Run(eng, case((5, 1, nij, ktot), dtype, seed=10, neighbour=True), lead=lead, lead_rows=lead).check("chain, many waves: nij %d ktot %d lead %d" % (nij, ktot, lead))


BODIES = ("parity", "neighbour", "rows", "alignment", "optional", "special", "cap", "refusals", "many_waves", "chain")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in (2, 7, 64, 65, 160)]),
            ("neighbour", lambda: [check_neighbour(eng, k, n) for k in (3, 64, 66, 128) for n in (1, 5)]),
            ("rows", lambda: [check_rows(eng, k) for k in (160, 33)]),
            ("alignment", lambda: [check_alignment(eng, *a) for a in ((1, 0, 0), (0, 1, 0), (0, 0, 4), (0, 0, 3))]),
            ("optional", lambda: check_optional(eng)),
            ("special", lambda: check_special(eng)),
            ("cap", lambda: check_cap(eng)),
            ("refusals", lambda: check_refusals(eng)),
            ("many_waves", lambda: check_many_waves(eng)),
            ("chain", lambda: check_chain(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_microphysics (CPU suite) ---------------------------------------------------------------
class MicroOracleEngine(wpr.WaterPathOracleEngine):
    """tests/les_water_paths_ref.WaterPathOracleEngine with ``les_microphysics`` by the NumPy oracle above: qt, thl, qr_new
    and rain written in place, as the HIP engine does"""

    def les_microphysics(self, qt, ql, qr, qr_new, sed_out, sed_in, lcpex, w, dt, thl=None, temp=None, rain=None, means=True, **kw):
        if qr_new.data_ptr() in (qr.data_ptr(), qt.data_ptr(), ql.data_ptr()):
            raise ValueError("qr_new is another argument")
        opt = lambda t: None if t is None else t.numpy()                                    # noqa: E731
        kw = {k: v for k, v in kw.items() if v is not None and k != "stream"}
        r = les_micro(qt.numpy(), ql.numpy(), qr.numpy(), sed_out.numpy(), sed_in.numpy(), lcpex.numpy(), w.numpy(), dt, thl=opt(thl),
                      temp=opt(temp), rain=opt(rain), **kw)
        for t, k in ((qt, "qt"), (thl, "thl"), (qr_new, "qr_new"), (rain, "rain")):
            if t is not None:
                t.copy_(torch.from_numpy(r[k]))
        if means is False or means is None:
            return {}
        return lar._t({k: r[name] for k, name in MEAN_KEYS.items() if name in r}, means if isinstance(means, dict) else None)


# -- the host twin of models.DeviceLESEnsemble after enable_microphysics() -----------------------------------------------------
class _HostMicro:
    """NumPy fields: the executable definition of what evolve_model_batched does after enable_microphysics()"""

    micro_par = None
    rain2d = None

    def enable_microphysics(self, v_fall=None, qc0=None, k_auto=None, k_acc=None):
        if self.nL == 1:
            raise ValueError("the microphysics (K14) does not take LES of one level")
        f = self.fields3d
        if "QT" not in f:
            raise ValueError("the microphysics (K14) needs a QT field")
        if "QR" not in f:
            f["QR"] = numpy.zeros_like(f["QT"])
        self.rain2d = numpy.zeros(f["QT"].shape[:3], dtype=f["QT"].dtype)
        self._stale = True              # thermo: K12 runs again before the next use of QL (K14 needs the cells' temperature), at presf as it is then
        self.micro_par = {"v_fall": mp.V_FALL if v_fall is None else v_fall, "qc0": mp.QC0 if qc0 is None else qc0,
                          "k_auto": mp.K_AUTO if k_auto is None else k_auto, "k_acc": mp.K_ACC if k_acc is None else k_acc}

    def _micro_step(self, dt, temp):
        """the oracle on the stepped fields and the current QL; returns its result"""
        f, p, par = self.fields3d, self.p, self.micro_par
        prof = mp.profiles(self.zh_cache, self.zf_cache, p["Rhobf"], p["presf"], dt, par["v_fall"])
        r = les_micro(f["QT"], f["QL"], f["QR"], *[self._r(a) for a in prof], dt, thl=f.get("THL"), temp=temp, rain=self.rain2d,
                      qc0=par["qc0"], k_auto=par["k_auto"], k_acc=par["k_acc"])
        f["QT"], f["QR"], self.rain2d = r["qt"], r["qr_new"], r["rain"]
        p["QT"], p["QR"] = self._w(r["qt_mean"]), self._w(r["qr_mean"])
        if "thl" in r:
            f["THL"], p["THL"] = r["thl"], self._w(r["thl_mean"])
        if "qi_mean" in r:
            p["QL_ice"] = self._w(r["qi_mean"])
        p["Rain"] = self._w(numpy.array([x.mean() for x in self.rain2d], dtype=self.dtype))
        return r


class HostMicroLESEnsemble(_HostMicro, wpr.HostWaterPathLESEnsemble):
    """without enable_thermo(): QL = max(QT - Qsat, 0) before and after the microphysics"""

    def evolve_model_batched(self, t):
        dt = float(t) - self.model_time
        if dt <= 0:
            return
        if self.micro_par is None:
            return super().evolve_model_batched(t)
        f, p = self.fields3d, self.p
        self._step(dt)
        f["QL"] = numpy.maximum(f["QT"] - f["Qsat"], 0.0)
        self._slab_means()
        if "PS" in self.tend:
            p["PS"] = p["PS"] + dt * self.tend["PS"]
        self._micro_step(dt, None)
        f["QL"] = numpy.maximum(f["QT"] - f["Qsat"], 0.0)
        p["QL"] = self._w(slab_ref.slab_means(f["QL"]))
        p["QL_ice"] = numpy.minimum(p["QL_ice"], p["QL"])
        p["T"] = p["THL"] * (p["presf"] / 1e5) ** (287.04 / 1004.) + 2.53e6 * p["QL"] / 1004.
        self.model_time = float(t)


class HostThermoMicroLESEnsemble(_HostMicro, wpr.HostThermoWaterPathLESEnsemble):
    """after enable_thermo(): K12's oracle before the microphysics (QL and the cells' temperature) and after it"""

    def evolve_model_batched(self, t):
        from sp_coupler_amd import thermo
        dt = float(t) - self.model_time
        if dt <= 0:
            return
        if self.micro_par is None:
            return super().evolve_model_batched(t)
        f, p = self.fields3d, self.p
        self._step(dt)
        self._stale = True
        self._slab_means()
        if "PS" in self.tend:
            p["PS"] = p["PS"] + dt * self.tend["PS"]
        presf = numpy.asarray(p["presf"], dtype=numpy.float64)
        temp = ltr.les_thermo(f["THL"], f["QT"], self._r(presf), self._r(thermo.exner(presf)), self.n_iter)["temp"]
        self._micro_step(dt, temp)
        self._stale = True
        self._ensure_ql()
        p["QL_ice"] = numpy.minimum(p["QL_ice"], p["QL"])
        self.model_time = float(t)


def ensemble_run(engine, n, thermo, device, itot=4, jtot=5, nL=20, steps=3, micro=True):
    """an ensemble with attached fields (QR included: rain that reaches the ground from the first step on) through ``steps`` calls of
    evolve_model_batched with one variability nudge (constantT) before the last; after each of them every profile, the fields,
    rain2d and RWP (a row's get_field on the device ensemble).  Returns (ens, list of records)"""
    spcpl.set_engine(engine)
    cls = models.DeviceLESEnsemble if device else (HostThermoMicroLESEnsemble if thermo else HostMicroLESEnsemble)
    fs = [make_les_fields(itot, jtot, nL, seed=60 + (i % 7)) for i in range(n)]
    stack = lambda k: numpy.stack([f[k] for f in fs])                                      # noqa: E731
    gcm = models.BatchedSyntheticGCM(n + 4, 19, 21)
    ens = cls.for_gcm(gcm, numpy.arange(1, n + 1), nL=nL, seed=21, itot=itot, jtot=jtot, **twin_kw(cls, engine))
    fields = {"Qsat": stack("qsat"), "QT": stack("qt"), "THL": stack("thl")}
    if thermo:
        del fields["Qsat"]
        fields["THL"] = fields["THL"] - 25.0                      # cells between t_dn and t_up: ice and water
        fields["QT"] = fields["QT"] * 0.35
        fields["QT"][:, 2, 1, :] *= 2.0                           # one column K12 finds cloudy whatever the profile
    fields["QR"] = numpy.random.default_rng(n).random((n, itot, jtot, nL)) * 1e-5
    ens.attach_fields({k: v.copy() for k, v in fields.items()})
    ens.p["presf"] = stack("presf")
    ens.ql_ref = stack("ql_ref")
    ens.model_time = 900.0
    if thermo:
        ens.enable_thermo()
    if micro:
        ens.enable_microphysics(qc0=1e-4, v_fall=0.05)           # (layers of the synthetic grid in 900 s: part of the rain stays)
    rng = numpy.random.default_rng(5)
    ens.set_forcings_batched(THL=rng.normal(0, 2e-4, (n, nL)), QT=rng.normal(0, 2e-7, (n, nL)))
    log = []

    def record():
        prof = {k: numpy.empty((n, nL)) for k in ("U", "V", "THL", "QT", "QL")}
        ens.get_profiles_batched(tuple(prof), prof)
        rec = {"p " + k: numpy.array(v) for k, v in ens.p.items()}
        rec.update({"got " + k: v for k, v in prof.items()})
        rec.update({"field " + k: numpy.array(host_of(ens.get_fields_batched(k))) for k in ("QT", "THL", "QL") + (("QR",) if micro else ())})
        if micro:
            rec["rain2d"] = numpy.array(host_of(ens.rain2d))
            rec["RWP"] = numpy.array(host_of(ens.get_water_paths_batched(("RWP",))["RWP"]))
            rec["row RWP"] = numpy.array(ens[n - 1].get_field("RWP") if device else ens.row_field(n - 1, "RWP"))
        log.append(rec)
    record()
    for step in range(steps):
        if step == steps - 1:
            numpy.random.seed(11)
            spcpl.variability_nudge_ensemble(ens, 900.0, True, write=False)
            record()
        ens.evolve_model_batched(1800.0 + 900.0 * step)
        record()
    return ens, log


def same_logs(host, dev):
    assert len(host) == len(dev) >= 5
    for step, (a, b) in enumerate(zip(host, dev)):
        assert set(a) == set(b), (step, sorted(a), sorted(b))
        for k in a:
            assert a[k].shape == b[k].shape, (step, k)
            assert_bits("step %d %s" % (step, k), b[k], a[k], dtypes=True)


def check_ensemble(one, engines, n, thermo, **kw):
    """the host twin (on engine ``one``) against the device ensemble on each of ``engines``; the rain evolves"""
    host = ensemble_run(one, n, thermo, False, **kw)[1]
    first, last = host[0], host[-1]
    for k in ("p Rain", "p QR", "RWP", "field QR"):
        assert not numpy.array_equal(first[k], last[k]) and not numpy.array_equal(host[1][k], host[2][k]), k
    assert (last["p Rain"] > 0).all() and (last["p QR"] > 0).any() and (last["RWP"] > 0).any()
    if thermo:
        assert (last["p QL_ice"] > 0).any() and (last["p QL_ice"] < last["p QL"]).any()
    for engine in engines:
        same_logs(host, ensemble_run(engine, n, thermo, True, **kw)[1])
    return host
