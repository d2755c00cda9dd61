"""CPU: both oracles, and the MT19937 restatement, against numbers the REFERENCE ITSELF produced (tests/golden/ref_*.npz, recorded
by tests/golden/make_reference_goldens.py from the reference's unmodified splib/spcpl.py, sputils.py and haversine.py under the
units shim of oracle/refshim).  From the fixtures alone; only the last test touches the reference, and it is skipped where
the reference root does not exist.

* oracle.spcpl_oracle (forward_batched, backward_batched, the helpers, output_column_conversion) and oracle.vnudge_oracle
  reproduce EVERY recorded array bit for bit, NaN positions and the sign of zero included.
* The C oracle (tests/oracle_c.py, float64) does the same, except what passes through pow() -- thl, f_thl, wthl, THL, t --
  which gets exactly the tolerance tests/test_oracle.py::test_c_oracle_matches_numpy_oracle gives C against NumPy
  (4 x 2.3e-16 of the array's scale; f_thl on the scale of thl x factor / dt).
* start_index is internal to the reference's set_gcm_tendencies (no setter receives it): pinned through the zeroed tendencies.
* rainrate reaches spifs multiplied by 3600 (spcpl.py:358): the oracles' rainrate x 3600 is compared.

Each test prints how many arrays it compared and how many needed a tolerance (pytest -s)."""
import importlib.util
import os

import numpy
import pytest

from oracle import spcpl_oracle as orc
from oracle import vnudge_oracle as vo
from tests import oracle_c
from tests import reference_pins as rp
from tests.reference_pins import Tally
from tests.test_les_state_cpu import PyMT19937

C_TOL = 4 * 2.3e-16              # tests/test_oracle.py:99-104


def _numpy_oracle(family):
    gcm, zf, zh, prof, factor, dt, ref = rp.exchange(family)
    with numpy.errstate(all="ignore"):
        f = orc.forward_batched(gcm, prof, zf, zh, factor, dt, couple_surface=True)
        b = orc.backward_batched(gcm, f["Zf"], prof, zf, factor, dt)
        bc = orc.backward_batched(gcm, f["Zf"], prof, zf, factor, dt, conservative=True, Zh=f["Zh"], zh=zh)
    return f, b, bc


@pytest.mark.parametrize("family", rp.EXCHANGE)
def test_numpy_oracle_reproduces_the_reference(family):
    gcm, zf, zh, prof, factor, dt, ref = rp.exchange(family)
    f, b, bc = _numpy_oracle(family)
    t = Tally(family)
    for k in rp.FWD_BITS + rp.FWD_POW:
        t.bits("fwd " + k, f[k], ref["fwd_" + k])
    t.bits("idx", f["idx"], ref["idx"])
    for k in ("Tv", "THL", "QT"):
        t.bits("spifs " + k, f[k], ref["cdf_" + k])
    t.bits("spifs Psurf", f["ps"], ref["cdf_Psurf"])
    t.bits("spifs rainrate", f["rainrate"] * 3600, ref["cdf_rainrate"])
    for k in rp.TEND:
        t.bits("linear " + k, b[k], ref["bwd_" + k])
        t.bits("conservative " + k, bc[k], ref["bwdc_" + k])
    t.bits("write_les_profiles t", b["t"], ref["wlp_t"])
    t.bits("write_les_profiles ql_water", b["ql_water"], ref["wlp_ql_water"])
    occ = []
    for c in range(gcm["T"].shape[0]):
        C = {"T": gcm["T"][c], "SH": gcm["SH"][c], "QL": gcm["QL"][c], "QI": gcm["QI"][c], "Zghalf": gcm["Zghalf"][c],
             "Zgfull": gcm["Zgfull"][c], "Ph": gcm["Phalf"][c], "Pf": gcm["Pfull"][c]}
        with numpy.errstate(all="ignore"):
            orc.output_column_conversion(C)
        occ.append(C)
    for k in ("Tv", "Zh", "Zf", "Psurf", "Ph", "THL", "QT"):
        t.bits("output_column_conversion " + k, numpy.stack([C[k] for C in occ]), ref["occ_" + k])
    assert t.n_bits == len(ref) and t.n_tol == 0           # every recorded array
    t.report()


@pytest.mark.parametrize("family", rp.EXCHANGE)
def test_c_oracle_reproduces_the_reference(family):
    gcm, zf, zh, prof, factor, dt, ref = rp.exchange(family)
    with numpy.errstate(all="ignore"):
        f = oracle_c.forward(gcm, zf, zh, prof, factor, dt, couple_surface=True)
        b = oracle_c.backward(gcm, ref["fwd_Zf"], zf, prof, factor, dt)
        b0 = oracle_c.backward(gcm, None, zf, prof, factor, dt)
        bc = oracle_c.backward(gcm, ref["fwd_Zf"], zf, prof, factor, dt, conservative=True, zh=zh, Zh=ref["fwd_Zh"])
        d = oracle_c.diagnostics(gcm, zf, prof)
    t = Tally(family + " (C)")
    for k in rp.FWD_BITS:
        t.bits("fwd " + k, f[k], ref["fwd_" + k])
    thl_scale = rp.finite_max(ref["fwd_thl"])
    t.close("fwd thl", f["thl"], ref["fwd_thl"], C_TOL, thl_scale)
    t.close("fwd f_thl", f["f_thl"], ref["fwd_f_thl"], C_TOL, thl_scale * abs(factor) / dt)
    t.close("fwd wthl", f["wthl"], ref["fwd_wthl"], C_TOL)
    t.bits("idx", f["idx"], ref["idx"])
    t.bits("idx (standalone)", oracle_c.cloud_indices(zh, numpy.ascontiguousarray(ref["fwd_Zh"])), ref["idx"])
    for k in ("Tv", "QT"):
        t.bits("spifs " + k, d[k], ref["cdf_" + k])
    t.close("spifs THL", d["THL"], ref["cdf_THL"], C_TOL)
    t.bits("spifs Psurf", f["ps"], ref["cdf_Psurf"])
    t.bits("spifs rainrate", f["rainrate"] * 3600, ref["cdf_rainrate"])
    for k in rp.TEND:
        t.bits("linear " + k, b[k], ref["bwd_" + k])
        t.bits("linear, Zf recomputed " + k, b0[k], ref["bwd_" + k])
        t.bits("conservative " + k, bc[k], ref["bwdc_" + k])
    t.close("write_les_profiles t", d["t"], ref["wlp_t"], C_TOL)
    t.bits("write_les_profiles ql_water", d["ql_water"], ref["wlp_ql_water"])
    for k in ("Tv", "QT", "Zf"):
        t.bits("output_column_conversion " + k, d[k], ref["occ_" + k])
    t.bits("output_column_conversion Zh", d["Zh"][:, 1:], ref["occ_Zh"])
    t.close("output_column_conversion THL", d["THL"], ref["occ_THL"], C_TOL)
    t.report()


@pytest.mark.parametrize("nL", rp.THICK_NL)
def test_oracles_reproduce_the_thick_layer_sums(nL):
    """GCM layers of more than 128 LES cells: ndarray.sum()'s pairwise recursion, as the reference ran it"""
    gcm, zf, zh, prof, factor, dt, ab, ref = rp.thick(nL)
    assert int(rp.load("ref_thick_%d" % nL)["in_max_cells"]) > 128
    p = dict(prof, THL=numpy.zeros_like(prof["T"]))          # THL only enters t, which set_gcm_tendencies does not hand on
    Zf = (gcm["Zgfull"] - gcm["Zghalf"][:, -1:]) / orc.grav
    Zh = (gcm["Zghalf"] - gcm["Zghalf"][:, -1:]) / orc.grav
    t = Tally("thick %d" % nL)
    bc = orc.backward_batched(gcm, Zf, p, zf, factor, dt, conservative=True, Zh=Zh, zh=zh)
    cc = oracle_c.backward(gcm, None, zf, prof, factor, dt, conservative=True, zh=zh)
    for k in rp.TEND:
        t.bits("conservative " + k, bc[k], ref["bwdc_" + k])
        t.bits("conservative (C) " + k, cc[k], ref["bwdc_" + k])
    t.bits("interp_c", orc.interp_c(Zh[0], zh, prof["T"][0], prof["Rhobf"][0])[None], ref["ic_T"])
    t.bits("interp_rho", orc.interp_rho(Zh[0], zh, prof["Rhobf"][0])[None], ref["irho"])
    t.bits("integral weighted", numpy.array([orc.integral(a, b, zh, prof["T"][0], prof["Rhobf"][0]) for a, b in ab]), ref["integral_w"])
    t.bits("integral", numpy.array([orc.integral(a, b, zh, prof["T"][0]) for a, b in ab]), ref["integral"])
    assert t.n_bits == len(ref) + len(rp.TEND)
    t.report()


@pytest.mark.parametrize("constantT", [False, True])
def test_vnudge_oracle_reproduces_the_reference(constantT):
    z, ref = rp.load("vnudge_small"), rp.load("ref_vnudge")
    numpy.random.seed(42)
    R = vo.make_R(*z["in_qt"].shape[:2])
    r = vo.variability_nudge(z["in_qt"], z["in_qsat"], z["in_ql_av"], z["in_qt_av"], z["in_presf"], z["in_ql_ref"], R, float(ref["in_dt"]),
                             constantT, thl=z["in_thl"], ql=z["in_ql"])
    assert r["error"] is None
    tag = "cT%d_" % int(constantT)
    t = Tally("vnudge constantT=%s" % constantT)
    for k, o in (("qt", "qt"), ("qt_beta", "beta"), ("qt_alpha", "alpha"), ("qt_std", "qt_std")):
        t.bits(k, r[o], ref[tag + k])
    if constantT:
        t.bits("thl", r["thl"], ref[tag + "thl"])
    s = r["status"]                                          # the levels reach both root finders, "no bracket", the refusal and the skip
    assert (s == 1).any() and (s & 16).any() and (s & 4).any() and (s & 2).any() and (s == 0).any()
    t.report()


def test_mt19937_restatement_reproduces_the_reference_state():
    """set_les_state on two LES in sequence: NumPy's generator word by word (tests/test_les_state_cpu.py: PyMT19937), the
    generator state afterwards, and the host jump-ahead of the library"""
    from sp_coupler_amd import _abi
    ref = rp.load("ref_state")
    shape = tuple(int(x) for x in ref["in_shape"])
    s0 = numpy.random.RandomState(int(ref["in_seed"])).get_state()
    py = PyMT19937(s0[1], s0[2])
    t = Tally("state")
    cells = shape[0] * shape[1] * shape[2]
    for l in range(2):
        for f, (name, amp) in enumerate(zip(("U", "V", "THL", "QT"), (0.5, 0.5, 0.1, 2.5e-5))):
            got = amp * py.uniform(-1., 1., cells).reshape(shape) + ref["in_profiles"][l, f]
            t.bits("les %d %s" % (l, name), got, ref["les%d_%s" % (l, name)])
    t.bits("key", numpy.array(py.key, dtype=numpy.uint32), ref["key"])
    assert py.pos == int(ref["pos"]) and int(ref["has_gauss"]) == 0
    key, pos = _abi.mt19937_jump(s0[1], s0[2], 2 * 8 * cells)
    t.bits("key (host jump)", key, ref["key"])
    assert pos == int(ref["pos"])
    t.report()


def test_helper_oracles_reproduce_the_reference():
    from tests import geo_ref
    ref = rp.load("ref_helpers")
    t = Tally("helpers")
    with numpy.errstate(all="ignore"):
        t.bits("exner", orc.exner(ref["in_p"]), ref["exner"])
        t.bits("iexner", orc.iexner(ref["in_p"]), ref["iexner"])
        t.bits("interp", orc.interp(ref["in_interp_x"], ref["in_interp_xp"], ref["in_interp_fp"]), ref["interp"])
        t.bits("interp (restated)", orc.interp_restated(ref["in_interp_x"], ref["in_interp_xp"], ref["in_interp_fp"]), ref["interp"])
        for side in ("left", "right"):
            t.bits("searchsorted " + side, orc.searchsorted(ref["in_ss_a"], ref["in_ss_v"], side=side), ref["ss_" + side])
        t.bits("rms", numpy.array([orc.rms(r) for r in ref["in_rms"]]), ref["rms"])
    pts = ref["in_points"]
    hav = numpy.stack([geo_ref.haversine(pts[:, 0], pts[:, 1], x, y) for x, y in ref["in_targets"]])
    keep = ref["haversine"] < numpy.pi * 6371 - 111.0          # tests/geo_edges.py::check_haversine: 1e-12, a degree off the antipode
    t.rel("haversine (NumPy's sin / cos / arcsin against libm's)", hav, ref["haversine"], 1e-12, keep)
    order = numpy.argsort(ref["haversine"][0], kind="stable")
    assert ref["mask_single_nmax-1"].tolist() == [order[0]] and ref["mask_single_nmax1"].tolist() == [order[0]]
    assert ref["mask_single_nmax5"].tolist() == order[:5].tolist()
    assert sorted(ref["mask_several"].tolist()) == sorted(set(numpy.argmin(ref["haversine"], axis=1).tolist()))
    t.report()


def test_every_fixture_is_small_and_names_its_provenance():
    import glob
    paths = sorted(glob.glob(os.path.join(rp.GOLDEN, "ref_*.npz")))
    assert len(paths) == 15
    for p in paths:
        assert os.path.getsize(p) <= 160000, p
        with numpy.load(p, allow_pickle=False) as z:
            assert str(z["meta_family"]) in os.path.basename(p) and str(z["meta_numpy"]) and str(z["meta_scipy"])
            for k in z.files:
                assert z[k].dtype in (numpy.float64, numpy.int64, numpy.uint32) or k.startswith("meta_"), (p, k)


def _recorder():
    spec = importlib.util.spec_from_file_location("make_reference_goldens", os.path.join(rp.GOLDEN, "make_reference_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference_readable():
    path = os.path.join(os.environ.get("SPC_REFERENCE_ROOT", "/root/reference"), "splib", "spcpl.py")
    return os.path.isfile(path) and os.access(path, os.R_OK)


@pytest.mark.skipif(not _reference_readable(), reason="no reference root here; the fixtures alone are checked above")
def test_live_reference_reproduces_the_committed_fixtures():
    """the recorder's functions, re-run in memory on the reference as it is: every committed array, inputs included, comes out
    again (the family assertions of the recorder hold on the way)"""
    import sys
    rec = _recorder()
    saved_path, saved_rng, saved_modules = list(sys.path), numpy.random.get_state(), set(sys.modules)
    try:
        n = 0
        for family in rec.FAMILIES:
            for stem, d in rec.record(family).items():
                want = rp.load(stem)
                assert set(d) == set(want), (stem, set(d) ^ set(want))
                for k, v in d.items():
                    if k in ("meta_numpy", "meta_scipy"):
                        continue
                    v = numpy.asarray(v)
                    if v.dtype.kind == "U":
                        assert str(v) == str(want[k]), (stem, k)
                    else:
                        assert v.dtype == want[k].dtype, (stem, k)
                        rp.assert_bits("%s %s" % (stem, k), v, want[k])
                    n += 1
        print("live reference: %d arrays reproduced" % n)
    finally:
        sys.path[:] = saved_path
        numpy.random.set_state(saved_rng)
        for m in set(sys.modules) - saved_modules:        # the stand-ins (omuse, amuse, netCDF4, shapely) and the reference's splib
            if m.split(".")[0] in ("omuse", "amuse", "netCDF4", "shapely", "splib", "spc_refshim", "make_reference_goldens"):
                del sys.modules[m]
