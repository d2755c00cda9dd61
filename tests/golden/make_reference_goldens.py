#!/usr/bin/env python3
"""Records tests/golden/ref_*.npz: inputs, and the numbers the REFERENCE'S OWN unmodified functions return for them.

PROVENANCE: unlike config1_L*.npz and vnudge_small.npz (written by this repo's oracle), every output array here was computed
by the reference's ``splib/spcpl.py``, ``splib/sputils.py`` and ``splib/haversine.py``, imported as they are from
``$SPC_REFERENCE_ROOT`` (default /root/reference) under the units shim of ``oracle/refshim`` and called on fake ``les`` /
``gcm`` objects: the setters record their arguments, ``les.cdf.variables`` records what ``spio.write_les_data`` is given.
Only data is stored -- float64 (indices int64, the MT19937 key uint32), ``allow_pickle=False``; nothing of the reference's
text.  Every file names its family and the numpy / scipy that evaluated it.  CPU only; no GPU, no network.

Families (ISSUE: smallest shapes at which the kernels still branch); one file holds ``COLS_PER_FILE`` columns:
  edge     tests.test_parity_gpu.make_edge_batch() columns 0-5, 91 <-> 160
  geo19    synthetic.make_batch(3, 19, 160)         geo137  make_batch(2, 137, 512)
  runtime  make_batch(4, 60, 100, per_column_grid=True)
      per column: set_les_forcings(couple_surface=True, write=True); convert_profiles; set_gcm_tendencies linear and
      conservative; get_les_profiles (the cloud-fraction indices); write_les_profiles (t, ql_water); output_column_conversion
  thick    one column each at nL = 240, 480, 960, 2000 (1 m ... 0.05 m LES cells): set_gcm_tendencies(conservative=True),
           sputils.interp_c, interp_rho, integral
  vnudge   the inputs of vnudge_small.npz (not stored again), numpy.random.seed(42): variability_nudge, constantT False / True
  state    two LES of 5 x 7 x 16 in sequence after numpy.random.seed(42): set_les_state, and the generator state afterwards
  helpers  sputils.exner, iexner, interp, searchsorted, rms; haversine.haversine; get_mask_indices with Point masks
           (the polygon branch needs shapely itself: out of scope)

usage: python tests/golden/make_reference_goldens.py          (rewrites the files; sizes are printed and checked)
"""
import contextlib
import io
import logging
import os
import sys

import numpy
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SHIM = os.path.join(ROOT, "oracle", "refshim")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
MAX_BYTES = 160000
FACTOR, DT = 0.85, 900.0
COLS_PER_FILE = {"edge": 2, "geo19": 3, "geo137": 1, "runtime": 2}
THICK = ((240, 0.01), (480, 0.004), (960, 0.002), (2000, 0.1))      # test_conservative_coarsening_thick_layers_recursive_pairwise_sums
GCM_VARS = ["U", "V", "T", "SH", "QL", "QI", "Pfull", "Phalf", "A", "Zgfull", "Zghalf"]
SURF_VARS = ["Z0M", "Z0H", "QLflux", "QIflux", "SHflux", "TLflux", "TSflux"]
LES_KEYS = ("U", "V", "THL", "QT", "QL", "QL_ice", "T", "Rhobf", "A", "PS", "Rain", "rain_last")
SETTERS = {"tendency_U": "f_u", "tendency_V": "f_v", "tendency_THL": "f_thl", "tendency_QT": "f_qt", "tendency_QL": "f_ql",
           "tendency_surface_pressure": "f_ps", "ref_profile_QL": "ql_ref", "z0m_surf": "z0m", "z0h_surf": "z0h",
           "wt_surf": "wthl", "wq_surf": "wqt"}


def reference_root():
    return os.environ.get("SPC_REFERENCE_ROOT", "/root/reference")


def available():
    return os.path.isfile(os.path.join(reference_root(), "splib", "spcpl.py"))


_MODS = None


def reference():
    """(spcpl, sputils, haversine, Quantity, Point) of the reference, imported under the shim"""
    global _MODS
    if _MODS is None:
        for p in (reference_root(), SHIM, ROOT):
            if p not in sys.path:
                sys.path.insert(0, p)
        import spc_refshim
        from splib import haversine, spcpl, sputils
        assert os.path.dirname(os.path.abspath(spcpl.__file__)) == os.path.join(os.path.abspath(reference_root()), "splib")
        _MODS = (spcpl, sputils, haversine, spc_refshim.Quantity, spc_refshim.Point)
    return _MODS


def _num(x):
    return numpy.array(getattr(x, "number", x), dtype=numpy.float64)


# ---- fake models ---------------------------------------------------------------------------------------------------------
class _Slot:
    """what ``les.cdf.variables.get(name)`` returns: truthy, and ``slot[cdf_step] = value`` records the value"""

    def __init__(self, store, name):
        self.store, self.name = store, name

    def __setitem__(self, step, value):
        self.store[self.name] = _num(value)


class _Cdf:
    def __init__(self):
        self.written = {}
        self.variables = self

    def get(self, name, default=None):
        return _Slot(self.written, name)


class FakeLES:
    """one LES column as the reference's coupling functions see it: GCM profiles as attributes, cached grids, getters that
    return the slab means, setters that record"""

    def __init__(self, Q, gcm_col, zf, zh, prof, grid_index=0):
        self.Q, self.prof, self.grid_index = Q, prof, grid_index
        self.set, self.indices, self.cdf = {}, None, _Cdf()
        for k, v in gcm_col.items():
            setattr(self, k, Q(numpy.array(v)))
        self.zf_cache, self.zh_cache = Q(numpy.array(zf)), Q(numpy.array(zh))

    def _p(self, key):
        return self.Q(numpy.array(self.prof[key]))

    def __getattr__(self, name):
        if name.startswith("set_"):
            def setter(value, return_request=False):
                self.set[name[4:]] = _num(value)
            return setter
        if name.startswith("get_profile_"):
            return lambda return_request=False: self._p(name[12:])
        raise AttributeError(name)

    def get_presf(self, return_request=False):
        return self._p("presf")

    def get_rhof(self, return_request=False):
        return self._p("Rhof")

    def get_rhobf(self, return_request=False):
        return self._p("Rhobf")

    def get_surface_pressure(self, return_request=False):
        return self._p("PS")

    def get_rain(self, return_request=False):
        return self._p("Rain")

    def get_cloudfraction(self, indices, return_request=False):
        self.indices = numpy.array(indices)
        return self._p("A")


class FakeGCM:
    def __init__(self):
        self.tend = {}

    def set_profile_tendency(self, var, grid_index, value):
        self.tend[var] = _num(value)


@contextlib.contextmanager
def quiet():
    """sputils.integral prints 'len(z) should be len(q) + 1' for every layer (the LES has as many cells as half levels: a
    reference quirk), spcpl prints brentq timings; the reference's log.error for cdf variables is not raised by the fakes"""
    with contextlib.redirect_stdout(io.StringIO()) as out, numpy.errstate(all="ignore"):
        yield out


# ---- the column-exchange families ----------------------------------------------------------------------------------------
def exchange_column(gcm, zf, zh, prof, c):
    """every recorded reference output of column ``c`` -> dict name -> array"""
    spcpl, sputils, _, Q, _ = reference()
    gcol = {k: gcm[k][c] for k in GCM_VARS + SURF_VARS}
    pcol = {k: v[c] for k, v in prof.items()}
    zf_c, zh_c = (zf if zf.ndim == 1 else zf[c]), (zh if zh.ndim == 1 else zh[c])
    P = {k: Q(numpy.array(v)) for k, v in pcol.items()}
    out = {}
    with quiet():
        les = FakeLES(Q, gcol, zf_c, zh_c, pcol, c)
        les.rain = Q(pcol["rain_last"])
        spcpl.set_les_forcings(les, None, False, False, P, Q(DT), FACTOR, True, write=True)
        w = les.cdf.written
        for a, k in SETTERS.items():
            out["fwd_" + k] = les.set[a]
        for k in ("f_u", "f_v", "f_thl", "f_qt", "z0m", "z0h", "wthl", "wqt"):       # written to spifs: the same numbers
            assert numpy.array_equal(w[k], out["fwd_" + k], equal_nan=True), k
        out["fwd_Zf"], out["fwd_Zh"] = _num(les.gcm_Zf), _num(les.gcm_Zh)
        assert numpy.array_equal(w["Zf"], out["fwd_Zf"]) and numpy.array_equal(w["Zh"], out["fwd_Zh"][1:])
        assert numpy.array_equal(w["Ph"], gcol["Phalf"][1:]) and numpy.array_equal(w["Pf"], gcol["Pfull"])
        for k in ("Tv", "THL", "QT", "Psurf", "rainrate"):                          # K5's Tv THL QT (Zf Zh above), K1's rain rate x 3600
            out["cdf_" + k] = w[k]
        u, v, thl, qt, ps, ql = spcpl.convert_profiles(les, write=False)
        for k, x in (("u", u), ("v", v), ("thl", thl), ("qt", qt), ("ps", ps)):
            out["fwd_" + k] = _num(x)
        assert numpy.array_equal(_num(ql), out["fwd_ql_ref"], equal_nan=True)
        for tag, cons in (("bwd_", False), ("bwdc_", True)):
            g = FakeGCM()
            spcpl.set_gcm_tendencies(g, les, P, Q(DT), FACTOR, write=False, conservative=cons)
            for k, x in g.tend.items():
                out[tag + "f_" + k] = x
        spcpl.get_les_profiles(les, False)
        out["idx"] = les.indices.astype(numpy.int64)
        les.cdf = _Cdf()
        spcpl.write_les_profiles(les)
        out["wlp_t"], out["wlp_ql_water"] = les.cdf.written["t"], les.cdf.written["ql_water"]
        assert numpy.array_equal(les.indices, out["idx"])
        C = {"T": "T", "SH": "SH", "QL": "QL", "QI": "QI", "Zghalf": "Zghalf", "Zgfull": "Zgfull", "Ph": "Phalf", "Pf": "Pfull"}
        C = {k: Q(numpy.array(gcol[v])) for k, v in C.items()}
        spcpl.output_column_conversion(C)
        for k in ("Tv", "Zh", "Zf", "Psurf", "Ph", "THL", "QT"):
            out["occ_" + k] = _num(C[k])
    return out


def exchange_inputs(name):
    from sp_coupler_amd import synthetic
    if name == "edge":
        from tests.test_parity_gpu import make_edge_batch
        gcm, zf, zh, prof = make_edge_batch()[:4]
        n = 6
    elif name == "geo19":
        gcm, zf, zh, prof = synthetic.make_batch(3, 19, 160, seed=1919)
        n = 3
    elif name == "geo137":
        gcm, zf, zh, prof = synthetic.make_batch(2, 137, 512, seed=137512)
        n = 2
    elif name == "runtime":
        gcm, zf, zh, prof = synthetic.make_batch(4, 60, 100, seed=60100, per_column_grid=True)
        n = 4
    else:
        raise KeyError(name)
    gcm = {k: numpy.ascontiguousarray(v[:n]) for k, v in gcm.items()}
    prof = {k: numpy.ascontiguousarray(v[:n]) for k, v in prof.items()}
    if zf.ndim == 2:
        zf, zh = numpy.ascontiguousarray(zf[:n]), numpy.ascontiguousarray(zh[:n])
    return gcm, zf, zh, prof


def record_exchange(name):
    """{file stem: arrays} of one column-exchange family"""
    gcm, zf, zh, prof = exchange_inputs(name)
    n = gcm["T"].shape[0]
    cols = [exchange_column(gcm, zf, zh, prof, c) for c in range(n)]
    full = {k: numpy.stack([col[k] for col in cols]) for k in cols[0]}
    check_exchange_family(name, gcm, zf, zh, full)
    files = {}
    per = COLS_PER_FILE[name]
    for f, lo in enumerate(range(0, n, per)):
        sl = slice(lo, min(lo + per, n))
        d = {"in_gcm_" + k: v[sl] for k, v in gcm.items()}
        d.update({"in_les_" + k: prof[k][sl] for k in LES_KEYS})
        d.update(in_zf=zf if zf.ndim == 1 else zf[sl], in_zh=zh if zh.ndim == 1 else zh[sl],
                 in_factor=numpy.float64(FACTOR), in_dt=numpy.float64(DT), in_first_column=numpy.int64(lo))
        d.update({k: v[sl] for k, v in full.items()})
        files["ref_%s_%d" % (name, f)] = d
    return files


def check_exchange_family(name, gcm, zf, zh, out):
    """the family exercises what it claims (as tests/test_parity_gpu.py::test_edge_columns asserts of its batch)"""
    nG = gcm["T"].shape[1]
    zf_top = zf[-1] if zf.ndim == 1 else zf[:, -1]
    start = (out["fwd_Zf"] > numpy.reshape(zf_top, (-1, 1) if zf.ndim == 2 else ())).sum(axis=1)     # Zf descends: searchsorted(-Zf, -h[-1])
    if name == "edge":
        from tests.test_parity_gpu import make_edge_batch
        _, _, _, _, Zf1, Zh1, exact_full, exact_half = make_edge_batch()
        assert len(exact_full) >= 17 and len(exact_half) >= 3
        assert all(out["fwd_Zf"][1, k] == Zf1[k] and Zf1[k] in zf for k in exact_full)          # exact hits on LES full levels
        assert all(out["fwd_Zh"][1, k] == Zh1[k] and Zh1[k] in zh for k in exact_half)
        assert start[2] == 0 and start[3] == nG                                                  # start_index 0 and nG
        assert (out["bwd_f_T"][3] == 0).all() and (out["bwd_f_T"][2] != 0).all()
        assert (out["fwd_u"][2] == gcm["U"][2, 0]).all() and (out["fwd_u"][3] == gcm["U"][3, -1]).all()   # clamping both ways
        assert numpy.isnan(out["bwd_f_T"][4, 0]) and numpy.isnan(out["bwdc_f_T"][4, 0])          # NaN survives `*= 0`
        assert numpy.signbit(out["bwd_f_U"][4][out["bwd_f_U"][4] == 0]).any()                    # -0.0
        for k in ("bwd_f_U", "bwd_f_T", "fwd_u", "fwd_f_u"):                                     # infinities through numpy.interp
            assert not numpy.isfinite(out[k][5]).all(), k
        assert (out["fwd_ql_ref"][0] == 0).all()
        assert (out["idx"][1] != numpy.searchsorted(zh, out["fwd_Zh"][1], side="left")[:-1][::-1]).sum() >= 3   # side='right' ties
    else:
        assert ((start > 0) & (start < nG)).all()
        assert (numpy.diff(out["fwd_Zf"], axis=1) < 0).all()
        for c in range(len(start)):
            m = out["bwd_f_U"][c, :start[c]]
            assert (m == 0).all() and numpy.signbit(m).any() and not numpy.signbit(m).all()      # +0.0 and -0.0 above the LES top
        assert (out["bwdc_f_T"] != out["bwd_f_T"]).any() and numpy.array_equal(out["bwdc_f_A"], out["bwd_f_A"])
    if name == "runtime":
        assert zf.ndim == 2 and len({tuple(r) for r in zf}) == zf.shape[0]                        # a grid per column


# ---- thick layers ----------------------------------------------------------------------------------------------------------
def thick_inputs(nL, scale):
    from sp_coupler_amd import synthetic
    gcm, zf, zh, prof = synthetic.make_batch(12, 91, nL, seed=52)
    gcm = {k: numpy.ascontiguousarray(v[:1]) for k, v in gcm.items()}
    prof = {k: numpy.ascontiguousarray(v[:1]) for k, v in prof.items()}
    return gcm, numpy.ascontiguousarray(zf * scale), numpy.ascontiguousarray(zh * scale), prof


def record_thick():
    spcpl, sputils, _, Q, _ = reference()
    files = {}
    for nL, scale in THICK:
        gcm, zf, zh, prof = thick_inputs(nL, scale)
        gcol = {k: gcm[k][0] for k in GCM_VARS + SURF_VARS}
        pcol = {k: v[0] for k, v in prof.items()}
        P = {k: Q(numpy.array(v)) for k, v in pcol.items()}
        out = {}
        with quiet():
            les = FakeLES(Q, gcol, zf, zh, pcol)
            spcpl.convert_profiles(les, write=False)
            g = FakeGCM()
            spcpl.set_gcm_tendencies(g, les, P, Q(DT), FACTOR, write=False, conservative=True)
            for k, x in g.tend.items():
                out["bwdc_f_" + k] = x[None]
            Zh = _num(les.gcm_Zh)
            out["ic_T"] = _num(sputils.interp_c(Q(Zh.copy()), Q(zh.copy()), P["T"], P["Rhobf"]))[None]
            out["irho"] = _num(sputils.interp_rho(Q(Zh.copy()), Q(zh.copy()), P["Rhobf"]))[None]
            cells = numpy.diff(numpy.searchsorted(zh, Zh[::-1]))
            assert cells.max() > 128, (nL, cells.max())                    # a GCM layer spanning more than 128 LES levels
            inside = Zh[::-1][1:] <= zh[-1]
            k = 90 - int(numpy.argmax(numpy.where(inside, cells, 0)))      # the thickest layer k = [Zh[k + 1], Zh[k]] inside the LES
            assert Zh[k] <= zh[-1] and numpy.where(inside, cells, 0).max() > 128
            ab = numpy.array([[Zh[k + 1], Zh[k]], [Zh[k], Zh[k + 1]], [zh[0], zh[-1]], [zh[1], zh[2]], [zh[-1] * 0.25, zh[-1] * 0.75]])
            out["in_integral_ab"] = ab
            out["integral_w"] = numpy.array([sputils.integral(a, b, zh, pcol["T"], pcol["Rhobf"]) for a, b in ab])
            out["integral"] = numpy.array([sputils.integral(a, b, zh, pcol["T"]) for a, b in ab])
        assert (out["bwdc_f_T"] != 0).any() and numpy.isfinite(out["integral_w"]).all() and out["integral"][1] == -out["integral"][0]
        d = {"in_gcm_" + k: gcm[k] for k in GCM_VARS}
        d.update({"in_les_" + k: prof[k] for k in ("U", "V", "QT", "QL", "QL_ice", "T", "Rhobf", "A")})    # (THL, PS: no part in these outputs)
        d.update(in_zf=zf, in_zh=zh, in_factor=numpy.float64(FACTOR), in_dt=numpy.float64(DT), in_max_cells=numpy.int64(cells.max()))
        d.update(out)
        files["ref_thick_%d" % nL] = d
    return files


# ---- variability nudge -----------------------------------------------------------------------------------------------------
class _Capture(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self, level=logging.DEBUG)
        self.text = []

    def emit(self, record):
        self.text.append(record.getMessage())


def record_vnudge():
    spcpl, _, _, Q, _ = reference()
    z = numpy.load(os.path.join(HERE, "vnudge_small.npz"))
    itot, jtot, ktot = z["in_qt"].shape
    d = {}

    class Holder:
        pass

    for cT in (False, True):
        fld = {"Qsat": z["in_qsat"].copy(), "QT": z["in_qt"].copy(), "THL": z["in_thl"].copy(), "QL": z["in_ql"].copy()}
        prof = {"QL": z["in_ql_av"].copy(), "QT": z["in_qt_av"].copy()}
        les = Holder()
        les.cdf, les.fields, les.parameters_DOMAIN = _Cdf(), Holder(), Holder()
        les.parameters_DOMAIN.kmax = ktot
        les.get_itot, les.get_jtot = (lambda: itot), (lambda: jtot)
        les.get_field, les.get_profile = (lambda n: Q(fld[n])), (lambda n: Q(prof[n]))
        les.get_presf = lambda: Q(z["in_presf"].copy())
        les.ql_ref = Q(z["in_ql_ref"].copy())
        cap, logger = _Capture(), logging.getLogger(spcpl.__name__)
        level = logger.level
        logger.addHandler(cap)
        logger.setLevel(logging.INFO)
        try:
            numpy.random.seed(42)                          # splib.initialize seeds numpy's global generator with 42
            with quiet() as out:
                spcpl.variability_nudge(les, Q(DT), cT)
        finally:
            logger.removeHandler(cap)
            logger.setLevel(level)
        tag = "cT%d_" % int(cT)
        w = les.cdf.written
        d[tag + "qt"] = _num(les.fields.QT)
        d[tag + "qt_beta"], d[tag + "qt_alpha"], d[tag + "qt_std"] = w["qt_beta"], w["qt_alpha"], w["qt_std"]
        if cT:
            d[tag + "thl"] = _num(les.fields.THL)
            assert (d[tag + "thl"] != z["in_thl"]).any()
        else:
            assert not hasattr(les.fields, "THL")
        # every branch is reached: brentq, "no bracket", additive noise, additive refused, barely unsaturated, skip
        log = "\n".join(cap.text)
        ql_ref, ql_av = z["in_ql_ref"], z["in_ql_av"]
        assert out.getvalue().count("brent took") >= 2 and "didn't bracket a zero" in log and "additive brent took" in log
        assert ((ql_ref <= 1e-9) & (ql_av > ql_ref)).any() and ((ql_ref <= 1e-9) & ~(ql_av > ql_ref)).any()
        skip = (ql_ref <= 1e-9) & ~(ql_av > ql_ref)
        assert (d[tag + "qt_beta"][skip] == 1).all() and numpy.array_equal(d[tag + "qt"][:, :, skip], z["in_qt"][:, :, skip])
        assert ((d[tag + "qt_beta"] != 1) & (d[tag + "qt_beta"] < 5)).sum() >= 3
    assert numpy.array_equal(d["cT0_qt"], d["cT1_qt"])
    d["in_dt"] = numpy.float64(DT)
    return {"ref_vnudge": d}


# ---- the initial LES state -------------------------------------------------------------------------------------------------
STATE_SHAPE = (5, 7, 16)


class _StateLES:
    def __init__(self):
        self.fields, self.ps = {}, None

    def get_itot(self):
        return STATE_SHAPE[0]

    def get_jtot(self):
        return STATE_SHAPE[1]

    def get_ktot(self):
        return STATE_SHAPE[2]

    def set_field(self, name, value):
        self.fields[name] = _num(value)

    def set_surface_pressure(self, ps):
        self.ps = _num(ps)


def record_state():
    spcpl, _, _, Q, _ = reference()
    rng = numpy.random.default_rng(3)
    prof = numpy.stack([[rng.normal(m, 1.0, STATE_SHAPE[2]) for m in (5.0, -3.0, 300.0, 0.01)] for _ in range(2)])   # [les, field, k]
    ps = [101325.0, None]
    saved = numpy.random.get_state()
    try:
        numpy.random.seed(42)
        s0 = numpy.random.get_state()
        les = [_StateLES(), _StateLES()]
        for l in range(2):
            spcpl.set_les_state(les[l], *[Q(prof[l, f].copy()) for f in range(4)], ps=None if ps[l] is None else Q(ps[l]))
        s1 = numpy.random.get_state()
    finally:
        numpy.random.set_state(saved)
    cells = STATE_SHAPE[0] * STATE_SHAPE[1] * STATE_SHAPE[2]
    words = 8 * cells                                       # 4 fields x 2 words per double
    assert s0[2] == 624 and (s0[2] + words) // 624 >= 7 and (s0[2] + words) % 624 not in (0, 624)    # the second LES starts mid-state
    assert s1[2] == (s0[2] + 2 * words - 1) % 624 + 1 and s1[3] == 0 and not numpy.array_equal(s0[1], s1[1])
    assert les[0].ps == 101325.0 and les[1].ps is None
    d = dict(in_profiles=prof, in_ps0=numpy.float64(ps[0]), in_seed=numpy.int64(42), in_shape=numpy.array(STATE_SHAPE, dtype=numpy.int64),
             key=numpy.array(s1[1], dtype=numpy.uint32), pos=numpy.int64(s1[2]), has_gauss=numpy.int64(s1[3]),
             cached_gaussian=numpy.float64(s1[4]))
    for l in range(2):
        for name in ("U", "V", "THL", "QT"):
            d["les%d_%s" % (l, name)] = les[l].fields[name]
    return {"ref_state": d}


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def helper_inputs():
    rng = numpy.random.default_rng(77)
    xp = numpy.sort(rng.uniform(0.0, 4000.0, 37))
    fp = rng.normal(size=37)
    x = numpy.concatenate([xp[[0, 5, 17, 36]], [-5.0, 4100.0, -numpy.inf, numpy.inf, numpy.nan], rng.uniform(-100.0, 4100.0, 28),
                           numpy.nextafter(xp[9], [-numpy.inf, numpy.inf])])
    a = numpy.sort(numpy.concatenate([rng.uniform(0.0, 100.0, 40), [12.5, 12.5, 12.5, 50.0, 50.0]]))
    v = numpy.concatenate([[12.5, 50.0, a[0], a[-1], -1.0, 101.0, -numpy.inf, numpy.inf, numpy.nan], rng.uniform(-5.0, 105.0, 20)])
    p = numpy.concatenate([numpy.exp(rng.uniform(numpy.log(1.0), numpy.log(1.1e5), 40)),
                           [1e5, 1e5 * (1 + 2.0 ** -52), 0.0, -1.0, numpy.inf, numpy.nan, 5e-324, 1e-300, 1e300]])
    rms = numpy.stack([rng.normal(size=131), numpy.full(131, 3.204), numpy.where(numpy.arange(131) == 7, numpy.nan, 1.0),
                       rng.normal(size=131) * 1e100])
    lon = numpy.concatenate([rng.uniform(0.0, 360.0, 60), [0.0, 359.9, 180.0, 4.9, 5.6]])
    lat = numpy.concatenate([rng.uniform(-89.0, 89.0, 60), [90.0, -90.0, 0.0, 52.0, 51.9]])
    targets = numpy.array([[4.93, 51.97], [-70.0, -33.0], [179.5, 0.2], [0.0, 89.5]])
    return dict(in_interp_x=x, in_interp_xp=xp, in_interp_fp=fp, in_ss_a=a, in_ss_v=v, in_p=p, in_rms=rms,
                in_points=numpy.stack([lon, lat], axis=1), in_targets=targets)


def record_helpers():
    _, sputils, haversine, Q, Point = reference()
    d = helper_inputs()
    with quiet():
        d["exner"], d["iexner"] = _num(sputils.exner(Q(d["in_p"].copy()))), _num(sputils.iexner(Q(d["in_p"].copy())))
        d["interp"] = _num(sputils.interp(Q(d["in_interp_x"].copy()), Q(d["in_interp_xp"].copy()), Q(d["in_interp_fp"].copy())))
        for side in ("left", "right"):
            d["ss_" + side] = numpy.asarray(sputils.searchsorted(Q(d["in_ss_a"].copy()), Q(d["in_ss_v"].copy()), side=side), dtype=numpy.int64)
        d["rms"] = numpy.array([sputils.rms(r) for r in d["in_rms"]])
    pts = [(float(x), float(y)) for x, y in d["in_points"]]
    d["haversine"] = numpy.array([[haversine.haversine(p, (float(t[0]), float(t[1]))) for p in pts] for t in d["in_targets"]])
    t0 = Point(float(d["in_targets"][0, 0]), float(d["in_targets"][0, 1]))
    for nmax in (-1, 1, 5):
        d["mask_single_nmax%d" % nmax] = numpy.asarray(sputils.get_mask_indices(pts, [t0], nmax), dtype=numpy.int64)
    several = sputils.get_mask_indices(pts, [Point(float(x), float(y)) for x, y in d["in_targets"]], 5)
    d["mask_several"] = numpy.asarray(several, dtype=numpy.int64)
    # ties in searchsorted, exact hits / both ends / NaN in interp, the sort has no equal distances to order differently
    assert (d["ss_left"] != d["ss_right"]).sum() >= 3 and d["ss_left"].max() == len(d["in_ss_a"]) and d["ss_left"].min() == 0
    assert numpy.isnan(d["interp"]).sum() == 1 and (d["interp"][:4] == d["in_interp_fp"][[0, 5, 17, 36]]).all()
    assert numpy.isnan(d["exner"]).sum() >= 2 and numpy.isinf(d["iexner"]).any() and numpy.isnan(d["rms"][2])
    assert d["exner"][40] == 1.0
    assert all(len(numpy.unique(row)) == len(row) for row in d["haversine"])
    assert len(d["mask_single_nmax5"]) == 5 and len(d["mask_single_nmax-1"]) == 1 and len(set(several)) == len(several) == 4
    return {"ref_helpers": d}


# ---- all of it -------------------------------------------------------------------------------------------------------------
FAMILIES = ("edge", "geo19", "geo137", "runtime", "thick", "vnudge", "state", "helpers")


def record(family):
    if family in COLS_PER_FILE:
        files = record_exchange(family)
    else:
        files = {"thick": record_thick, "vnudge": record_vnudge, "state": record_state, "helpers": record_helpers}[family]()
    for d in files.values():
        d.update(meta_family=numpy.array(family), meta_numpy=numpy.array(numpy.__version__), meta_scipy=numpy.array(scipy.__version__))
    return files


def main():
    if not available():
        sys.exit("no reference at %s (set SPC_REFERENCE_ROOT)" % reference_root())
    total = 0
    for family in FAMILIES:
        for stem, d in record(family).items():
            for k, v in d.items():
                assert numpy.asarray(v).dtype.kind in "fiuU" and numpy.asarray(v).dtype != object, (stem, k)
            path = os.path.join(HERE, stem + ".npz")
            numpy.savez_compressed(path, **d)
            size = os.path.getsize(path)
            numpy.load(path, allow_pickle=False).close()
            n_out = sum(1 for k in d if not k.startswith(("in_", "meta_")))
            print("%-22s %7d bytes  %3d reference arrays" % (stem + ".npz", size, n_out))
            assert size <= MAX_BYTES, (path, size)
            total += size
    print("total %d bytes" % total)


if __name__ == "__main__":
    main()
