"""-m gpu: the float64 HIP kernels against numbers the REFERENCE ITSELF produced (tests/golden/ref_*.npz; recorder and provenance:
tests/golden/make_reference_goldens.py).  Reads tests/golden/ only, never the reference.  One Engine("cuda:0") in float64, a
few launches on at most 8 columns per test.

Tolerances are the project's own, now applied against the reference's numbers instead of the oracle's:
* bit for bit (tests.gpu_util.assert_bits: NaN positions and the sign of zero included) wherever no pow() is involved;
* thl, f_thl, wthl as tests/test_parity_gpu.py::check_forward (8 ulp of the scale of thl, f_thl on thl x factor / dt, and the
  1e-10 north-star bar on f_thl's own scale);
* K5's THL and t, and K6's thl with constantT, within 8 ulp of their scale (tests/test_dispatch_gpu.py header, tests/test_vnudge.py);
* K7's exner / iexner within 2 ulp of each value, special values alike (tests/test_sputils_gpu.py);
* K8's distances within 1e-12 relative, a degree off the antipode (tests/geo_edges.py::check_haversine); its ORDERING is exact.

float32 has no reference counterpart (the reference computes in float64 only): the float kernels stay with the float32 oracle
(tests/test_f32_oracle_cpu.py, the *_float32_* tests of tests/test_parity_gpu.py).  start_index is internal to the reference
(pinned through the zeroed tendencies); the polygon branch of get_mask_indices, splib.step sequencing and spio stay unpinned.

Each test prints how many recorded arrays it compared and how many needed a tolerance (pytest -s)."""
import ctypes

import numpy
import pytest
import torch

from tests import reference_pins as rp
from tests.gpu_util import EPS, host, to_dev
from tests.reference_pins import Tally

pytestmark = pytest.mark.gpu
ULP8 = 8 * EPS
REL_TOL = 1e-10              # tests/test_parity_gpu.py: the north-star bar on f_thl


@pytest.fixture(scope="module")
def eng():
    from sp_coupler_amd.engine import Engine
    return Engine("cuda:0")


@pytest.fixture()
def drop_in(eng):
    """the drop-in modules (spcpl, sputils) on the module's engine"""
    from sp_coupler_amd import spcpl, sputils
    spcpl.set_engine(eng)
    yield spcpl, sputils
    spcpl.set_engine(None)


def _to_dev(d, eng):
    return to_dev({k: v.copy() for k, v in d.items()}, eng.device)


def _dev(eng, family):
    gcm, zf, zh, prof, factor, dt, ref = rp.exchange(family)
    assert gcm["T"].shape[0] <= 8
    g, p = _to_dev(gcm, eng), _to_dev(prof, eng)                # (copies: the shared fixture arrays are read-only)
    zf_d, zh_d = torch.from_numpy(zf.copy()).to(eng.device), torch.from_numpy(zh.copy()).to(eng.device)
    return g, p, zf_d, zh_d, factor, dt, ref


def _f_thl(t, name, got, ref, factor, dt):
    scale = rp.finite_max(ref["fwd_thl"])
    t.close(name, got, ref["fwd_f_thl"], ULP8, scale * abs(factor) / dt)
    t.close(name + " (1e-10)", got, ref["fwd_f_thl"], REL_TOL, rp.finite_max(ref["fwd_f_thl"]))
    t.n_tol -= 1                                             # one recorded array, two bars


@pytest.mark.parametrize("family", rp.EXCHANGE)
def test_k1_full_and_k2(eng, family):
    """K1 with every optional output (want_profiles, couple_surface, rain rate, the fused index map) and the standalone K2"""
    g, p, zf_d, zh_d, factor, dt, ref = _dev(eng, family)
    fwd = eng.forward(g, zf_d, p, factor, dt, zh=zh_d, want_profiles=True, couple_surface=True)
    idx = eng.cloud_indices(zh_d, torch.from_numpy(ref["fwd_Zh"].copy()).to(eng.device))
    torch.cuda.synchronize()
    fwd = {k: host(v) for k, v in fwd.items()}
    t = Tally("%s K1/K2" % family)
    for k in rp.FWD_BITS:
        t.bits("K1 " + k, fwd[k], ref["fwd_" + k])
    t.bits("K1 ps (spifs Psurf)", fwd["ps"], ref["cdf_Psurf"])
    t.bits("K1 rainrate x 3600", fwd["rainrate"] * 3600, ref["cdf_rainrate"])
    t.close("K1 thl", fwd["thl"], ref["fwd_thl"], ULP8)
    _f_thl(t, "K1 f_thl", fwd["f_thl"], ref, factor, dt)
    t.close("K1 wthl", fwd["wthl"], ref["fwd_wthl"], ULP8)
    t.bits("K1 idx", fwd["idx"], ref["idx"])
    t.bits("K2 idx", host(idx), ref["idx"])
    t.report()


@pytest.mark.parametrize("family", rp.EXCHANGE)
def test_lean_k1_and_k3_through_plan_exchange(eng, family):
    """what a steady-state step (and bench.py) launches: lean K1, K3 with Zf recomputed and no start_index"""
    g, p, zf_d, zh_d, factor, dt, ref = _dev(eng, family)
    fp, bp = eng.plan_exchange(g, zf_d, zh_d, p, factor, factor, dt)
    for x in list(fp.outputs.values()) + list(bp.outputs.values()):
        x.fill_(float("nan")) if x.is_floating_point() else x.fill_(-7)
    sptr = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    fp.launch_raw(sptr)
    bp.launch_raw(sptr)
    torch.cuda.synchronize()
    t = Tally("%s lean K1 + K3" % family)
    for k in ("f_u", "f_v", "f_qt", "f_ql", "ql_ref", "f_ps"):
        t.bits("K1 " + k, host(fp.outputs[k]), ref["fwd_" + k])
    t.bits("K1 idx", host(fp.outputs["idx"]), ref["idx"])
    _f_thl(t, "K1 f_thl", host(fp.outputs["f_thl"]), ref, factor, dt)
    for k in rp.TEND:
        t.bits("K3 " + k, host(bp.outputs[k]), ref["bwd_" + k])
    t.report()


@pytest.mark.parametrize("family", rp.EXCHANGE)
def test_k3_and_k4(eng, family):
    """K3 with K1's Zf and with Zf=None; K4 (conservative=True) with K1's heights and with the heights recomputed"""
    g, p, zf_d, zh_d, factor, dt, ref = _dev(eng, family)
    fwd = eng.forward(g, zf_d, p, factor, dt, zh=zh_d)
    runs = (("K3 (Zf from K1)", "bwd_", eng.backward(g, zf_d, p, factor, dt, Zf=fwd["Zf"])),
            ("K3 (Zf=None)", "bwd_", eng.backward(g, zf_d, p, factor, dt, Zf=None)),
            ("K4 (Zf, Zh from K1)", "bwdc_", eng.backward(g, zf_d, p, factor, dt, Zf=fwd["Zf"], conservative=True, zh=zh_d, Zh=fwd["Zh"])),
            ("K4 (heights recomputed)", "bwdc_", eng.backward(g, zf_d, p, factor, dt, Zf=None, conservative=True, zh=zh_d)))
    torch.cuda.synchronize()
    t = Tally("%s K3/K4" % family)
    zf, nG = rp.exchange(family)[1], ref["fwd_Zf"].shape[1]
    top = zf[-1] if zf.ndim == 1 else zf[:, -1:]
    start = (ref["fwd_Zf"] > top).sum(axis=1)                # searchsorted(-Zf, -h[-1]) on the reference's own Zf
    for name, tag, got in runs:
        for k in rp.TEND:
            t.bits("%s %s" % (name, k), host(got[k]), ref[tag + k])
        assert numpy.array_equal(host(got["start_index"]), start), name
    assert family != "edge" or (start[2] == 0 and start[3] == nG)
    t.report()


@pytest.mark.parametrize("family", rp.EXCHANGE)
def test_k5_diagnostics(eng, family):
    """what reaches spifs.nc: Tv THL QT Zf Zh of convert_profiles / output_column_conversion, t and ql_water of write_les_profiles"""
    g, p, zf_d, zh_d, factor, dt, ref = _dev(eng, family)
    d = {k: host(v) for k, v in eng.diagnostics(g, zf_d, p).items()}
    torch.cuda.synchronize()
    t = Tally("%s K5" % family)
    for k in ("Tv", "QT"):
        t.bits(k, d[k], ref["cdf_" + k])
        t.bits(k + " (output_column_conversion)", d[k], ref["occ_" + k])
    t.bits("Zf", d["Zf"], ref["fwd_Zf"])
    t.bits("Zh", d["Zh"], ref["fwd_Zh"])
    t.bits("Zf (output_column_conversion)", d["Zf"], ref["occ_Zf"])
    t.bits("Zh (output_column_conversion)", d["Zh"][:, 1:], ref["occ_Zh"])
    t.close("THL", d["THL"], ref["cdf_THL"], ULP8)
    t.close("THL (output_column_conversion)", d["THL"], ref["occ_THL"], ULP8)
    t.close("t", d["t"], ref["wlp_t"], ULP8)
    t.bits("ql_water", d["ql_water"], ref["wlp_ql_water"])
    t.report()


@pytest.mark.parametrize("nL", rp.THICK_NL)
def test_k4_and_k7_thick_layers(eng, drop_in, nL):
    """GCM layers of more than 128 LES cells: the kernels' sums follow ndarray.sum()'s recursion AS THE REFERENCE RAN IT -- K4,
    and K7's interp_c / interp_rho / integral through the drop-in sputils"""
    _, sputils = drop_in
    gcm, zf, zh, prof, factor, dt, ab, ref = rp.thick(nL)
    g, p = _to_dev(gcm, eng), _to_dev(prof, eng)
    zf_d, zh_d = torch.from_numpy(zf.copy()).to(eng.device), torch.from_numpy(zh.copy()).to(eng.device)
    got = eng.backward(g, zf_d, p, factor, dt, Zf=None, conservative=True, zh=zh_d)
    torch.cuda.synchronize()
    t = Tally("thick %d K4/K7" % nL)
    for k in rp.TEND:
        t.bits("K4 " + k, host(got[k]), ref["bwdc_" + k])
    Zh = (gcm["Zghalf"] - gcm["Zghalf"][:, -1:]) / 9.81
    t.bits("K7 interp_c", sputils.interp_c(Zh, zh, prof["T"], prof["Rhobf"]), ref["ic_T"])
    t.bits("K7 interp_rho", sputils.interp_rho(Zh, zh, prof["Rhobf"]), ref["irho"])
    q, w = numpy.repeat(prof["T"], len(ab), axis=0), numpy.repeat(prof["Rhobf"], len(ab), axis=0)
    t.bits("K7 integral weighted", sputils.integral(ab[:, 0].copy(), ab[:, 1].copy(), zh, q, w), ref["integral_w"])
    t.bits("K7 integral", sputils.integral(ab[:, 0].copy(), ab[:, 1].copy(), zh, q), ref["integral"])
    t.report()


@pytest.mark.parametrize("constantT", [False, True])
def test_k6_variability_nudge(drop_in, constantT):
    from tests.test_vnudge import FieldLES
    spcpl, _ = drop_in
    z, ref = rp.load("vnudge_small"), rp.load("ref_vnudge")
    f = {k[3:]: v for k, v in z.items() if k.startswith("in_")}
    les = FieldLES(f, f["ql_ref"].copy())
    saved = numpy.random.get_state()
    try:
        numpy.random.seed(42)
        g = spcpl.variability_nudge(les, float(ref["in_dt"]), constantT, write=False)
    finally:
        numpy.random.set_state(saved)
    tag = "cT%d_" % int(constantT)
    t = Tally("vnudge constantT=%s K6" % constantT)
    t.bits("qt", les.fields.QT, ref[tag + "qt"])
    for k, o in (("qt_beta", "beta"), ("qt_alpha", "alpha"), ("qt_std", "qt_std")):
        t.bits(k, g[o], ref[tag + k])
    if constantT:
        t.close("thl", les.fields.THL, ref[tag + "thl"], ULP8)
    else:
        assert not hasattr(les.fields, "THL")
    t.report()


def test_k7_helpers(drop_in):
    _, sputils = drop_in
    ref = rp.load("ref_helpers")
    t = Tally("helpers K7")
    for name, fn in (("exner", sputils.exner), ("iexner", sputils.iexner)):
        got, want = fn(ref["in_p"].copy()), ref[name]
        fin = numpy.isfinite(want)
        assert numpy.array_equal(numpy.isnan(got), numpy.isnan(want)) and numpy.array_equal(numpy.isfinite(got), fin), name
        assert numpy.array_equal(got[numpy.isinf(want)], want[numpy.isinf(want)]), name
        t.rel(name, got, want, 2 * EPS, fin)
    t.bits("interp", sputils.interp(ref["in_interp_x"].copy(), ref["in_interp_xp"].copy(), ref["in_interp_fp"].copy()), ref["interp"])
    for side in ("left", "right"):
        t.bits("searchsorted " + side, sputils.searchsorted(ref["in_ss_a"].copy(), ref["in_ss_v"].copy(), side=side), ref["ss_" + side])
    t.bits("rms", sputils.rms(ref["in_rms"].copy(), axis=-1), ref["rms"])
    t.report()


def test_k8_haversine_ordering(eng, drop_in):
    from sp_coupler_amd import geometry
    _, sputils = drop_in
    ref = rp.load("ref_helpers")
    pts = [(float(x), float(y)) for x, y in ref["in_points"]]
    t = Tally("helpers K8")
    lon, lat = (torch.from_numpy(ref["in_points"][:, i].copy()).to(eng.device) for i in (0, 1))
    d = numpy.stack([host(eng.haversine(lon, lat, float(x), float(y))) for x, y in ref["in_targets"]])
    t.rel("haversine", d, ref["haversine"], 1e-12, ref["haversine"] < numpy.pi * 6371 - 111.0)
    t0 = geometry.Point(float(ref["in_targets"][0, 0]), float(ref["in_targets"][0, 1]))
    for nmax in (-1, 1, 5):
        t.bits("get_mask_indices nmax=%d" % nmax, numpy.asarray(sputils.get_mask_indices(pts, [t0], nmax), dtype=numpy.int64),
               ref["mask_single_nmax%d" % nmax])
    several = sputils.get_mask_indices(pts, [geometry.Point(float(x), float(y)) for x, y in ref["in_targets"]], 5)
    t.bits("get_mask_indices, several points", numpy.sort(numpy.asarray(several, dtype=numpy.int64)), numpy.sort(ref["mask_several"]))
    t.report()


def test_k9_set_les_state_batched(drop_in):
    """two LES in one launch: the fields the reference's loop gave them, and the generator state it left"""
    from tests.les_state_ref import RecLES
    spcpl, _ = drop_in
    ref = rp.load("ref_state")
    shape = tuple(int(x) for x in ref["in_shape"])
    les = [RecLES(shape), RecLES(shape)]
    prof = ref["in_profiles"]
    saved = numpy.random.get_state()
    try:
        numpy.random.seed(int(ref["in_seed"]))
        spcpl.set_les_state_batched(les, *[numpy.ascontiguousarray(prof[:, f]) for f in range(4)], ps=[float(ref["in_ps0"]), None])
        s = numpy.random.get_state()
    finally:
        numpy.random.set_state(saved)
    t = Tally("state K9")
    for l in range(2):
        calls = dict(les[l].calls)
        assert [c[0] for c in les[l].calls] == ["U", "V", "THL", "QT"] + (["PS"] if l == 0 else [])
        for name in ("U", "V", "THL", "QT"):
            t.bits("les %d %s" % (l, name), calls[name], ref["les%d_%s" % (l, name)])
    assert dict(les[0].calls)["PS"] == float(ref["in_ps0"])
    t.bits("key", numpy.asarray(s[1], dtype=numpy.uint32), ref["key"])
    assert s[2] == int(ref["pos"]) and s[3] == int(ref["has_gauss"]) and s[4] == float(ref["cached_gaussian"])
    t.report()
