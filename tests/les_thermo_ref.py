"""NumPy oracle of K12 (include/spc.h: spc_les_thermo_*), the inputs of its tests, the bodies of the GPU tests of
tests/test_les_thermo_gpu.py (each takes an engine: tools/mutation_control.py --thermo hands them the engines of its mutant
libraries), the host twin of models.DeviceLESEnsemble's thermo mode and an oracle-backed engine with ``les_thermo`` for the
CPU suite.

The oracle spells the rule out one operation per NumPy call in the element type, so nothing fuses.  Every device array of the
bodies is the LEADING part of a poisoned buffer (tests/les_harness.Poisoned); the bytes behind it (and in front of a view
off the 16-byte grid) are checked after the launch."""

import numpy
import torch

from sp_coupler_amd import _abi, driver, models, spcpl, sputils, thermo
from tests import les_advance_ref as lar
from tests import slab_ref
from tests.gpu_util import assert_bits
from tests.les_harness import (  # noqa: F401  (DTYPES, NP: for the tests)
    DTYPES, NP, Poisoned, abi_call, blocks_of, chain_cases, fill_args, np_of, on_both, run_bodies, twin_kw)

#: n = 3; planes 1 x 1, 3 x 5 (15 rows: three batches of 4 and single rows behind them) and 8 x 8; ktot 2 and 7 (one element per
#: lane), 64 and 160 (16-byte accesses), 65 (odd again, beyond one wave)
PLANES = [(1, 1), (3, 5), (8, 8)]
KTOTS = [2, 7, 64, 65, 160]
OUTS = ("qsat", "ql", "temp", "ql_mean", "t_mean")


# -- the rule --------------------------------------------------------------------------------------------------------------
def constants(dtype):
    """(T, eps, om, c) in the element type"""
    T = numpy.dtype(dtype).type
    eps = T(sputils.rd) / T(sputils.rv)
    return T, eps, T(1) - eps, T(sputils.rlv) / T(sputils.cp)


def table_top(dtype, n_tab, t_lo, inv_step):
    """t_hi as the library forms it: in double, rounded once"""
    return numpy.dtype(dtype).type(float(t_lo) + float(n_tab - 1) / float(inv_step))


def sat(Tk, p, tab, t_lo=thermo.T_LO, inv_step=thermo.INV_STEP, want_dqs=True):
    """(qs, dqs) at temperature Tk and pressure p from the table ``tab``"""
    T, eps, om, _ = constants(tab.dtype)
    n_tab = len(tab)
    lo, hi, s = T(t_lo), table_top(tab.dtype, n_tab, t_lo, inv_step), T(inv_step)
    with numpy.errstate(all="ignore"):
        Tc = numpy.where(Tk < lo, lo, numpy.where(Tk > hi, hi, Tk))
        x = (Tc - lo) * s
        m = numpy.minimum(numpy.where(x >= 0, x, T(0)).astype(numpy.int64), n_tab - 2)      # truncation; NaN gives 0
        w = x - m.astype(tab.dtype)
        d = tab[m + 1] - tab[m]
        wd = w * d
        e = tab[m] + wd
        ome = om * e
        den = p - ome
        epse = eps * e
        qs = epse / den
        dqs = None
        if want_dqs:
            epsp = eps * p
            ds = d * s
            numr = epsp * ds
            den2 = den * den
            dqs = numr / den2
    return qs, dqs


def cells(thl, qt, p, ex, tab, n_iter, t_lo=thermo.T_LO, inv_step=thermo.INV_STEP):
    """(qs, ql, temp) of every cell; all arguments broadcast against each other, in tab's dtype"""
    T, eps, om, c = constants(tab.dtype)
    with numpy.errstate(all="ignore"):
        Tl = thl * ex
        Tk = Tl
        for _ in range(n_iter):
            qs, dqs = sat(Tk, p, tab, t_lo, inv_step)
            a = Tk - Tl
            b = qt - qs
            cb = c * b
            num = a - cb
            cd = c * dqs
            dn = T(1) + cd
            step = num / dn
            Tk = numpy.where(qt > qs, Tk - step, Tl)
        qs, _ = sat(Tk, p, tab, t_lo, inv_step, want_dqs=False)
        dq = qt - qs
        ql = numpy.where(dq > 0, dq, numpy.where(dq != dq, dq, T(0)))
        lq = T(sputils.rlv) * ql
        temp = Tl + lq / T(sputils.cp)
    return qs.astype(tab.dtype), ql.astype(tab.dtype), temp.astype(tab.dtype)


def les_thermo(thl, qt, presf, ex, n_iter=None, tab=None, t_lo=thermo.T_LO, inv_step=thermo.INV_STEP):
    """dict qsat, ql, temp [n x itot x jtot x ktot] and ql_mean, t_mean [n x ktot] (k_slab_means' rule, spelled out) of fields
    of ONE dtype; presf and ex [n x ktot]"""
    tab = thermo.saturation_table(thl.dtype) if tab is None else tab
    n_iter = thermo.DEFAULT_N_ITER if n_iter is None else n_iter
    assert thl.shape[-1] >= 2 and tab.dtype == thl.dtype == qt.dtype == presf.dtype == ex.dtype
    qs, ql, temp = cells(thl, qt, presf[:, None, None, :], ex[:, None, None, :], tab, n_iter, t_lo, inv_step)
    return {"qsat": qs, "ql": ql, "temp": temp, "ql_mean": lar.mean_rows(ql), "t_mean": lar.mean_rows(temp)}


# -- inputs ------------------------------------------------------------------------------------------------------------------
def profiles(n, ktot, dtype, rng):
    """presf [n x ktot] falling from about 1e5 Pa (exactly 1e5 at level 0, where ex == 1 and Tl == thl) and its Exner factor"""
    presf = 1e5 - numpy.linspace(0.0, 4e4, ktot)[None, :] * (1.0 + 0.05 * rng.random((n, 1)))
    presf[:, 0] = 1e5
    presf = presf.astype(dtype)
    return presf, thermo.exner(presf.astype(numpy.float64)).astype(dtype)


def case(shape, dtype, seed=0, special=False):
    """thl, qt, presf, ex: cells from 40 % below to 40 % above saturation (about half of them cloudy).  ``special`` also sets,
    in plane points of their own: qt == qs(Tl) exactly, Tl below the table and above it, Tl exactly on table knots (level 0,
    where ex == 1), NaN in thl and in qt, qt = -0.0 and qt = 0"""
    dtype = numpy.dtype(dtype).type
    n, itot, jtot, ktot = shape
    rng = numpy.random.default_rng(2000 + seed + 7 * ktot + itot * jtot)
    presf, ex = profiles(n, ktot, dtype, rng)
    thl = (290.0 + 6.0 * rng.standard_normal(shape)).astype(dtype)
    tab = thermo.saturation_table(dtype)
    qs0 = sat((thl * ex[:, None, None, :]).astype(dtype), presf[:, None, None, :], tab, want_dqs=False)[0]
    qt = (qs0 * (0.6 + 0.8 * rng.random(shape))).astype(dtype)
    if special:
        assert itot * jtot >= 9
        pt = lambda r: (slice(None), r // jtot, r % jtot)                                  # noqa: E731
        qt[pt(0)] = qs0[pt(0)]                                    # qt == qs(Tl): the Newton branch is not taken, ql == +0.0
        thl[pt(1)] = 100.0                                        # below t_lo: the lookup clamps
        qt[pt(1)] = 1e-3
        thl[pt(2)] = 700.0                                        # above t_hi
        qt[pt(2)] = 1e-3
        knots = numpy.array([150.0, 151.0, 273.0, 280.0, 300.0, 549.0, 549.8, 280.2, 290.4, 300.6])
        thl[pt(3) + (0,)] = knots[numpy.arange(n) % len(knots)]   # level 0: ex == 1, Tl is the knot itself
        thl[pt(4) + (0,)] = knots[(numpy.arange(n) + 5) % len(knots)]
        qt[pt(4) + (0,)] = 2e-2
        thl[pt(5)] = numpy.nan
        qt[pt(6)] = numpy.nan
        qt[pt(7)] = -0.0
        qt[pt(8)] = 0.0
        thl[:, 0, 0, ktot - 1], qt[:, 0, 0, ktot - 1] = 310.0, 3e-2                       # strongly supersaturated
    return thl, qt, presf, ex


# -- device plumbing ---------------------------------------------------------------------------------------------------------
class Run:
    """one launch through ``eng.les_thermo`` with every array inside a poisoned buffer; ``check`` compares qsat, ql, temp and
    the means with the oracle bit for bit, thl and qt with what was uploaded, and looks at the bytes around every array"""

    def __init__(self, eng, thl, qt, presf, ex, n_iter=None, want_temp=True, means=True, lead=0, pad=0, lead_rows=0, **kw):
        self.eng, self.host, self.n_iter, self.pad = eng, (thl, qt, presf, ex), n_iter, pad
        dtype, shape = thl.dtype, thl.shape
        n, ktot = shape[0], shape[-1]
        self.mem = Poisoned(eng)
        put = self.mem.put
        rows = lambda tag, a, poison, lead: self.mem.rows(tag, a, poison, lead, pad)        # noqa: E731
        self.dthl, self.dqt = put("thl", thl, float("nan"), lead), put("qt", qt, float("nan"), lead)
        self.dpresf, self.dex = rows("presf", presf, 1e30, lead_rows), rows("ex", ex, 1e30, lead_rows)
        self.out = {k: put(k, numpy.full(shape, -3.0, dtype), -5.0, lead) for k in ("qsat", "ql") + (("temp",) if want_temp else ())}
        self.dmeans = {k: rows("mean " + k, numpy.full((n, ktot), -1.0, dtype), -7.0, lead_rows) for k in ("QL", "T")} if means else False
        self.got = eng.les_thermo(self.dthl, self.dqt, self.dpresf, self.dex, n_iter=n_iter, qsat=self.out["qsat"], ql=self.out["ql"],
                                  temp=self.out.get("temp"), means=self.dmeans, **kw)
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def check(self, what=""):
        thl, qt, presf, ex = self.host
        want = les_thermo(thl, qt, presf, ex, self.n_iter)
        for k, t in self.out.items():
            assert_bits("%s %s" % (what, k), t.cpu().numpy(), want[k])
        if self.dmeans:
            assert sorted(self.got) == ["QL", "T"], (what, sorted(self.got))
            for k, name in (("QL", "ql_mean"), ("T", "t_mean")):
                assert self.got[k].data_ptr() == self.dmeans[k].data_ptr(), (what, k)
                assert_bits("%s %s" % (what, name), self.dmeans[k].cpu().numpy(), want[name])
        else:
            assert self.got == {}, (what, self.got)
        for name, t, a in (("thl", self.dthl, thl), ("qt", self.dqt, qt), ("presf", self.dpresf, presf), ("ex", self.dex, ex)):
            assert Poisoned.read_only(t, a), (what, name, "read only")
        self.mem.check_around(what)
        return want


def raw_launch(eng, thl, qt, presf, ex, tab, t_lo, inv_step, n_iter):
    """spc_les_thermo_* itself with a table of the caller's (``Engine.les_thermo`` always hands in thermo.saturation_table):
    dict of host arrays like the oracle's"""
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(eng.device)              # noqa: E731
    n, itot, jtot, ktot = thl.shape
    ins = [dev(a) for a in (thl, qt, presf, ex, tab)]
    outs = {k: torch.full(thl.shape if k in OUTS[:3] else (n, ktot), -3.0, dtype=eng.dtype, device=eng.device) for k in OUTS}
    a = _abi.LesThermoArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_iter = n, itot, jtot, ktot, n_iter
    a.thl, a.qt, a.presf, a.ex, a.es_tab = (t.data_ptr() for t in ins)
    a.pitch_prof = a.pitch_mean = ktot
    a.n_tab, a.t_lo, a.inv_step = len(tab), t_lo, inv_step
    fill_args(a, outs)
    _abi.check(eng.lib, abi_call(eng, "spc_les_thermo", a))
    return {k: t.cpu().numpy() for k, t in outs.items()}


# -- a table of the test's own: exact coincidences that thermo.saturation_table does not offer -----------------------------
TAB_T_LO, TAB_INV_STEP = 250.0, 0.125                              # entries 8 K apart


def knot_case(dtype):
    """(thl, qt, presf, ex, tab): the first Newton step of the cells of level 0 starts in a flat stretch of the table (dqs == 0)
    and lands EXACTLY on knot 2, where qs == qt exactly and the slope is not zero: the rule's ``qt > qs`` returns to Tl there
    (a ``>=`` would go on with a Newton step into the stretch below the knot).  Level 1 holds ordinary cells."""
    T, eps, om, c = constants(dtype)
    tab = numpy.array([1000.0, 1000.0, 1600.0, 2600.0, 4000.0, 6000.0], dtype=dtype)
    p = T(1e5)
    knot = T(TAB_T_LO + 2 / TAB_INV_STEP)
    qs_a = sat(T(252.0), p, tab, TAB_T_LO, TAB_INV_STEP, want_dqs=False)[0]
    qt0 = sat(knot, p, tab, TAB_T_LO, TAB_INV_STEP, want_dqs=False)[0]
    cb = c * (qt0 - qs_a)
    Tl = knot - cb
    for _ in range(8):                                             # a Tl whose step lands on the knot itself
        if Tl + cb == knot:
            break
        Tl = numpy.nextafter(Tl, T(0) if Tl + cb > knot else T(1e3))
    assert Tl + cb == knot and T(TAB_T_LO) < Tl < T(TAB_T_LO + 1 / TAB_INV_STEP)
    shape = (2, 2, 3, 2)
    thl = numpy.full(shape, Tl, dtype=dtype)
    qt = numpy.full(shape, qt0, dtype=dtype)
    thl[..., 1] = [[262.0, 270.0, 281.0], [255.0, 266.0, 290.0]]
    qt[..., 1] = 1.2e-2
    presf = numpy.full((2, 2), 1e5, dtype=dtype)
    return thl, qt, presf, numpy.ones((2, 2), dtype=dtype), tab


def zero_case(dtype):
    """a table that starts with zeros: qs == +0.0 there, so qt = -0.0 gives dq == -0.0 (the q rule turns it into +0.0), qt = 0
    gives dq == +0.0 and a positive qt passes unchanged"""
    tab = numpy.array([0.0, 0.0, 0.0, 900.0, 2000.0], dtype=dtype)
    shape = (1, 2, 2, 3)
    thl = numpy.full(shape, 255.0, dtype=dtype)
    thl[..., 2] = 280.0
    qt = numpy.zeros(shape, dtype=dtype)
    qt[0, 0, 0, :] = -0.0
    qt[0, 0, 1, :] = 2e-3
    qt[0, 1, 0, :] = numpy.nan
    presf = numpy.full((1, 3), 1e5, dtype=dtype)
    return thl, qt, presf, numpy.ones((1, 3), dtype=dtype), tab


# -- bodies ------------------------------------------------------------------------------------------------------------------
def check_parity(eng, plane, ktot, n_iter=None):
    """qsat, ql, temp and both means against the oracle on cells on both sides of saturation"""
    thl, qt, presf, ex = case((3,) + tuple(plane) + (ktot,), np_of(eng))
    want = Run(eng, thl, qt, presf, ex, n_iter).check("plane %s ktot %d" % (plane, ktot))
    if want["ql"].size >= 100:
        assert (want["ql"] > 0).any() and (want["ql"] == 0).any()


def check_special(eng, ktot, n_iter=None):
    """the mix of the issue in one field: unsaturated and saturated cells, qt == qs, Tl outside the table on either side and
    on its knots, NaN in thl and in qt, qt = -0.0"""
    thl, qt, presf, ex = case((3, 3, 5, ktot), np_of(eng), seed=1, special=True)
    want = Run(eng, thl, qt, presf, ex, n_iter).check("special ktot %d n_iter %s" % (ktot, n_iter))
    assert numpy.isnan(want["ql"][:, 1, 0]).all() and numpy.isnan(want["ql"][:, 1, 1]).all()
    assert numpy.isnan(want["t_mean"]).all() and (want["qsat"][:, 0, 1] > 0).all()


def check_alignment(eng, lead, lead_rows, pad):
    """views one (or more) elements off the 16-byte grid and pitched profiles / means"""
    thl, qt, presf, ex = case((3, 3, 5, 64), np_of(eng), seed=lead + 10 * lead_rows + 100 * pad)
    Run(eng, thl, qt, presf, ex, lead=lead, lead_rows=lead_rows, pad=pad).check("lead %d %d pad %d" % (lead, lead_rows, pad))


def check_options(eng):
    """n_iter 0, 1 and the default; temp NULL; no means; the table staged in LDS and read from global memory"""
    thl, qt, presf, ex = case((3, 3, 5, 160), np_of(eng), seed=4, special=True)
    wants = {n: Run(eng, thl, qt, presf, ex, n).check("n_iter %s" % n) for n in (0, 1, None)}
    assert not numpy.array_equal(wants[0]["ql"], wants[1]["ql"], equal_nan=True)
    assert not numpy.array_equal(wants[1]["ql"], wants[None]["ql"], equal_nan=True)
    Run(eng, thl, qt, presf, ex, want_temp=False).check("temp NULL")
    Run(eng, thl, qt, presf, ex, means=False).check("no means")
    for mode in (_abi.THERMO_TABLE_LDS, _abi.THERMO_TABLE_GLOBAL):
        Run(eng, thl, qt, presf, ex, table_mode=mode).check("table_mode %d" % mode)
        Run(eng, thl[..., :7].copy(), qt[..., :7].copy(), presf[:, :7].copy(), ex[:, :7].copy(), table_mode=mode).check("table_mode %d, ktot 7" % mode)


def check_table(eng):
    """the C ABI with tables of the test's own: a Newton step that lands on a knot where qs == qt exactly, and dq == -0.0"""
    dtype = np_of(eng)
    for n_iter in (1, 2, 3):
        thl, qt, presf, ex, tab = knot_case(dtype)
        want = les_thermo(thl, qt, presf, ex, n_iter, tab, TAB_T_LO, TAB_INV_STEP)
        got = raw_launch(eng, thl, qt, presf, ex, tab, TAB_T_LO, TAB_INV_STEP, n_iter)
        for k in OUTS:
            assert_bits("knot n_iter %d %s" % (n_iter, k), got[k], want[k])
    thl, qt, presf, ex, tab = zero_case(dtype)
    want = les_thermo(thl, qt, presf, ex, 2, tab, TAB_T_LO, TAB_INV_STEP)
    got = raw_launch(eng, thl, qt, presf, ex, tab, TAB_T_LO, TAB_INV_STEP, 2)
    for k in OUTS:
        assert_bits("zero table " + k, got[k], want[k])


def check_multi(one, multi, n):
    """a MultiDeviceEngine with Sharded row blocks gives the bits of one engine and of the oracle"""
    thl, qt, presf, ex = case((n, 3, 5, 40), np_of(one), seed=n, special=True)
    want = les_thermo(thl, qt, presf, ex)
    (_, _, dev), (_, _, sh) = on_both(one, multi, n)
    o1 = {k: torch.full(thl.shape, -3.0, dtype=one.dtype, device=one.device) for k in OUTS[:3]}
    m1 = one.les_thermo(dev(thl), dev(qt), dev(presf), dev(ex), **o1)
    om = {k: sh(numpy.full(thl.shape, -3.0, dtype=thl.dtype)) for k in OUTS[:3]}
    mm = multi.les_thermo(sh(thl), sh(qt), sh(presf), sh(ex), **om)
    multi.synchronize()
    blocks = blocks_of(om["ql"], multi, n)
    for k in OUTS[:3]:
        assert_bits("multi " + k, om[k].to_host(), want[k])
        assert_bits("one " + k, o1[k].cpu().numpy(), want[k])
    assert sorted(mm) == sorted(m1) == ["QL", "T"]
    for k, name in (("QL", "ql_mean"), ("T", "t_mean")):
        assert_bits("multi mean " + k, mm[k].to_host(), want[name])
        assert_bits("one mean " + k, m1[k].cpu().numpy(), want[name])
    return blocks


def check_chain(eng):
    """the cases of the lane's walk (les_harness.chain_cases) for batches of 4 rows, which PLANES does not hold: the tail alone,
    one whole batch with no successor, a batch with a successor and then one without, a batch with a tail behind it"""
    for shape, lead in chain_cases(4, np_of(eng)):
        thl, qt, presf, ex = case(shape, np_of(eng), seed=9)
        Run(eng, thl, qt, presf, ex, lead=lead, lead_rows=lead).check("chain %s lead %d" % (shape, lead))


BODIES = ("parity", "special", "alignment", "options", "table", "chain")


def jobs(eng):
    return [("parity", lambda: [check_parity(eng, p, k) for p in PLANES for k in KTOTS]),
            ("special", lambda: [check_special(eng, k, n) for k in (7, 64) for n in (0, 1, None)]),
            ("alignment", lambda: [check_alignment(eng, *a) for a in ((1, 0, 0), (0, 1, 0), (0, 0, 4), (0, 0, 3))]),
            ("options", lambda: check_options(eng)),
            ("table", lambda: check_table(eng)),
            ("chain", lambda: check_chain(eng))]


def check_everything(eng):
    """every single-engine body above on one engine: what tools/mutation_control.py runs on a mutant library.  Returns the
    names of the bodies that failed (AssertionError)."""
    return run_bodies(BODIES, jobs(eng))


# -- an oracle-backed engine with les_thermo (CPU suite) ---------------------------------------------------------------------
class ThermoOracleEngine(lar.AdvanceOracleEngine):
    """tests/les_advance_ref.AdvanceOracleEngine with ``les_thermo`` by the NumPy oracle above: qsat, ql and temp written in
    place, as the HIP engine does"""

    def les_thermo(self, thl, qt, presf, ex, n_iter=None, qsat=None, ql=None, temp=None, means=True, **kw):
        r = les_thermo(thl.numpy(), qt.numpy(), presf.numpy(), ex.numpy(), n_iter)
        for t, k in ((qsat, "qsat"), (ql, "ql"), (temp, "temp")):
            if t is not None:
                t.copy_(torch.from_numpy(r[k]))
        if means is False or means is None:
            return {}
        return lar._t({"QL": r["ql_mean"], "T": r["t_mean"]}, means if isinstance(means, dict) else None)


# -- the host twin of models.DeviceLESEnsemble after enable_thermo() ---------------------------------------------------------
class HostThermoLESEnsemble(slab_ref.HostFieldLESEnsemble):
    """slab_ref.HostFieldLESEnsemble whose Qsat and QL fields are the oracle's saturation adjustment of THL and QT, redone
    before their next use whenever a field has been set or stepped, with p["QL"] and p["T"] its slab means: the executable
    definition of what models.DeviceLESEnsemble computes after enable_thermo()"""

    n_iter = None
    _stale = True

    def enable_thermo(self, n_iter=None):
        if self.nL == 1:
            raise ValueError("the saturation adjustment (K12) does not take LES of one level")
        self.n_iter = n_iter

    def set_fields_batched(self, name, values):
        super().set_fields_batched(name, values)
        self._stale = True

    def _ensure_ql(self):
        f = self.fields3d
        if not self._stale or "THL" not in f or "QT" not in f:
            return
        presf = numpy.asarray(self.p["presf"], dtype=numpy.float64)
        r = les_thermo(f["THL"], f["QT"], self._r(presf), self._r(thermo.exner(presf)), self.n_iter)     # (the Exner factor of the float64 presf)
        f["Qsat"], f["QL"] = r["qsat"], r["ql"]
        self.p["QL"], self.p["T"] = self._w(r["ql_mean"]), self._w(r["t_mean"])
        self._stale = False

    def get_fields_batched(self, name):
        if name in ("QL", "Qsat"):
            self._ensure_ql()
        return self.fields3d[name].copy()

    def _slab_means(self):
        self._ensure_ql()              # (the base class asks for QL only where a Qsat field exists: before K12's first run none does)
        return super()._slab_means()

    def _refresh_profile(self, key):
        self._ensure_ql()
        super()._refresh_profile(key)

    def get_profiles_batched(self, keys, out):
        self._ensure_ql()
        super().get_profiles_batched(keys, out)

    def evolve_model_batched(self, t):
        dt = float(t) - self.model_time
        if dt <= 0:
            return
        f, p = self.fields3d, self.p
        self._step(dt)
        self._stale = True
        self._slab_means()                                        # (runs _ensure_ql: the oracle, p["QL"], p["T"])
        if "PS" in self.tend:
            p["PS"] = p["PS"] + dt * self.tend["PS"]
        p["QL_ice"] = numpy.minimum(p["QL_ice"], p["QL"])
        p["Rain"] = p["Rain"] + 1e-6 * dt
        self.model_time = float(t)


# -- closed loop: Coupler(qt_forcing="variance") on the thermo ensemble ------------------------------------------------------
def loop(engine, cls, n, nG=19, nL=24, itot=4, jtot=4, steps=3):
    """tests/device_fields_multi._loop with enable_thermo(): spin-up, ``steps`` coupled steps, then one variability nudge with
    constantT=True; a log of every tendency and profile after each of them, the fields, and numpy's generator state"""
    spcpl.set_engine(engine)
    gcm = models.BatchedSyntheticGCM(max(2 * n + 3, 11), nG, 3)          # (columns 1, 3, ... 2 n - 1 hold the LES)
    ens = cls.for_gcm(gcm, numpy.arange(1, 2 * n + 1, 2), nL=nL, seed=4, itot=itot, jtot=jtot, **twin_kw(cls, engine))
    ens.enable_thermo()
    cpl = driver.Coupler(gcm, ens, cplsurf=True, qt_forcing="variance")
    numpy.random.seed(42)
    cpl.init_les_state()
    log = []

    def record():
        prof = {k: numpy.empty((n, nL)) for k in ("U", "V", "THL", "QT", "QL", "T")}
        ens.get_profiles_batched(tuple(prof), prof)
        log.append({"tend": {k: numpy.array(v[1]) for k, v in gcm.tendencies.items()},
                    "prof": dict({k: numpy.array(v) for k, v in ens.p.items()}, **{"got " + k: v for k, v in prof.items()}),
                    "time": ens.model_time})
    cpl.run_spinup(900.0, 1)
    record()
    for _ in range(steps):
        cpl.step()
        record()
    spcpl.variability_nudge_ensemble(ens, 900.0, True, write=False)
    record()
    fields = {k: numpy.array(_host(ens.get_fields_batched(k))) for k in ("U", "V", "THL", "QT", "Qsat", "QL")}
    return ens, log, fields, numpy.random.get_state()


def _host(t):
    return t if isinstance(t, numpy.ndarray) else models.DeviceLESEnsemble._host(t)


def same_loops(a, b):
    """two results of ``loop``: every tendency, profile and field bit-equal after every step, equal generator states"""
    (_, log_a, f_a, s_a), (_, log_b, f_b, s_b) = a, b
    assert s_a[0] == s_b[0] and numpy.array_equal(s_a[1], s_b[1]) and tuple(s_a[2:]) == tuple(s_b[2:])
    assert len(log_a) == len(log_b)
    for step, (x, y) in enumerate(zip(log_a, log_b)):
        assert x["time"] == y["time"] and set(x["tend"]) == set(y["tend"]) and set(x["prof"]) == set(y["prof"])
        for k in x["tend"]:
            assert numpy.array_equal(x["tend"][k], y["tend"][k], equal_nan=True), (step, "tendency", k)
        for k in x["prof"]:
            assert numpy.array_equal(x["prof"][k], y["prof"][k], equal_nan=True), (step, "profile", k)
    for k in f_a:
        assert numpy.array_equal(f_a[k], f_b[k], equal_nan=True), ("field", k)


def check_closed_loop(one, engines, n, **kw):
    """the loop on the host twin (engine ``one``) against the device ensemble on each of ``engines``; the state evolved, holds
    cloud, and cloud water followed the temperature (Qsat changed between the steps)"""
    host = loop(one, HostThermoLESEnsemble, n, **kw)
    log = host[1]
    assert len(log) >= 4 and log[-2]["time"] > log[0]["time"] > 0
    assert (log[-1]["prof"]["QL"] > 0).any() and not numpy.array_equal(log[1]["prof"]["T"], log[-2]["prof"]["T"])
    assert not numpy.array_equal(log[-1]["prof"]["THL"], log[-2]["prof"]["THL"])          # constantT moved THL
    for engine in engines:
        dev = loop(engine, models.DeviceLESEnsemble, n, **kw)
        assert dev[0].thermo and not dev[0]._thermo_stale
        same_loops(host, dev)
    return host
