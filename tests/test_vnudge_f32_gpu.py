"""K6 on a float32 engine (spc_variability_nudge_f32) against tests/vnudge_f32_ref.py: the reference's lines evaluated by
NumPy on float32 arrays, bit for bit (thl within a few float32 ulp: exner's powf)."""
import numpy
import pytest
import torch

from oracle import vnudge_oracle as vo
from tests import vnudge_f32_ref as v32
from tests.test_vnudge import FieldLES, make_les_fields

EPS32 = float(numpy.finfo(numpy.float32).eps)
THL_ULP = 4          # thl: spc_powf (<= 0.5 + 2^-14 ulp) against the host libm's powf in exner, and one float32 multiply-add on top


def _f32_engine():
    from sp_coupler_amd import spcpl
    from sp_coupler_amd.engine import Engine
    eng = Engine("cuda:0", dtype=torch.float32)
    spcpl.set_engine(eng)
    return spcpl, eng


def _ref(f, R, constantT):
    return v32.variability_nudge(f["qt"], f["qsat"], f["ql_av"], f["qt_av"], f["presf"], f["ql_ref"], R, 900.0, constantT,
                                 thl=f["thl"], ql=f["ql"])


def _check(g, r, m, f, constantT):
    assert r["error"] is None
    assert numpy.array_equal(g["status"], r["status"]), (g["status"], r["status"])
    assert g["beta"].dtype == numpy.float64 and g["a"].dtype == numpy.float64 and g["qt_std"].dtype == numpy.float32
    assert numpy.array_equal(g["beta"], r["beta"]) and numpy.array_equal(g["a"], r["a"])
    assert m.fields.QT.dtype == numpy.float32 and numpy.array_equal(m.fields.QT, r["qt"])
    assert numpy.array_equal(g["qt_std"], r["qt_std"]) and numpy.array_equal(g["alpha"], r["alpha"])
    if constantT:
        assert m.fields.THL.dtype == numpy.float32
        err = numpy.abs(m.fields.THL.astype(numpy.float64) - r["thl"]).max()
        assert err <= THL_ULP * EPS32 * numpy.abs(r["thl"]).max(), ("thl beyond %d float32 ulp (exner's powf)" % THL_ULP, err)
        assert not numpy.array_equal(m.fields.THL, f["thl"].astype(numpy.float32))
    else:
        assert not hasattr(m.fields, "THL")


@pytest.mark.gpu
@pytest.mark.parametrize("lds", ["1", "pair", "strided", "global"])
@pytest.mark.parametrize("constantT", [False, True])
def test_f32_kernel_matches_the_float32_numpy_scipy_restatement(constantT, lds):
    """the matrix of tests/test_vnudge.py::test_kernel_matches_the_numpy_scipy_oracle on a float32 engine: every device path
    (planes in LDS with 512- or paired 256-thread workgroups, loaded strided without the workspace, streamed from the
    workspace), the same ten plane shapes -- in float 128 x 128 is LDS-resident, 200 x 170 is not"""
    spcpl, _ = _f32_engine()
    try:
        def check(g, r, m, f):
            assert m.ktot < 12 or ((r["status"] & 1).any() and (r["status"] & 4).any())   # both root finders reached
            _check(g, r, m, f, constantT)
        from tests import vnudge_edges
        vnudge_edges.old_matrix(spcpl, constantT, lds, True, check)      # the shapes and launches of the float64 test
    finally:
        spcpl.set_engine(None)


@pytest.mark.gpu
def test_f32_nudge_in_chunks_gives_the_bits_of_one_launch(monkeypatch):
    """7 LES of 16 x 16 x 40 in chunks of 3 on a float32 engine"""
    spcpl, _ = _f32_engine()
    try:
        runs = []
        for limit in (32767, 3):
            monkeypatch.setattr(spcpl, "VN_MAX_COLS", limit)
            les = [FieldLES(make_les_fields(16, 16, 40, seed=70 + i), make_les_fields(16, 16, 40, seed=70 + i)["ql_ref"], i + 1)
                   for i in range(7)]
            numpy.random.seed(3)
            out = spcpl.variability_nudge_batched(les, 900.0, constantT=True, write=False)
            runs.append((out, [m.fields.QT for m in les], [m.fields.THL for m in les]))
        (o1, q1, t1), (o2, q2, t2) = runs
        for i in range(7):
            for k in ("beta", "alpha", "qt_std", "a", "status"):
                assert numpy.array_equal(o1[i][k], o2[i][k]), (i, k)
            assert numpy.array_equal(q1[i], q2[i]) and numpy.array_equal(t1[i], t2[i]), i
        assert any((o["status"] != 0).any() for o in o1)
    finally:
        spcpl.set_engine(None)


@pytest.mark.gpu
def test_f32_no_sign_change_for_the_additive_noise_raises_like_scipy():
    spcpl, _ = _f32_engine()
    try:
        f = make_les_fields(8, 8, 10, seed=9)
        f["ql_ref"][:] = 0.0
        f["ql_ref"][4] = 50.0
        les = FieldLES(f, f["ql_ref"].copy())
        numpy.random.seed(1)
        with pytest.raises(ValueError, match="different signs"):
            spcpl.variability_nudge(les, 900.0)
        numpy.random.seed(1)
        assert isinstance(_ref(f, vo.make_R(8, 8), False)["error"], ValueError)
    finally:
        spcpl.set_engine(None)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["per_les", "batched"])
def test_f32_variance_forcing_through_set_les_forcings(route):
    """qt_forcing='variance' on a float32 engine (splib/spcpl.py:377-382), through the per-LES drop-in the reference's step
    calls (set_les_forcings, one LES at a time) and through set_les_forcings_batched: the LES with model time > 0 get the
    float32 nudge of their fields toward les.ql_ref, the one at time 0 is left alone; R in les order"""
    from sp_coupler_amd import models
    spcpl, _ = _f32_engine()

    class FieldSyntheticLES(models.SyntheticLES):
        def attach_fields(self, seed):
            self.f3 = make_les_fields(8, 8, self.nL, seed)
            self.fields = FieldLES._Fields()

        def get_itot(self):
            return 8

        def get_jtot(self):
            return 8

        def get_field(self, name):
            return {"Qsat": self.f3["qsat"], "QT": self.f3["qt"], "THL": self.f3["thl"], "QL": self.f3["ql"]}[name].copy()

        def get_profile(self, name):
            return {"QL": self.f3["ql_av"], "QT": self.f3["qt_av"]}[name].copy()

    try:
        gcm = models.SyntheticGCM(8, 91, seed=4)
        les_models = []
        for i in (1, 2, 3):
            les = FieldSyntheticLES(gcm, i, 160, seed=4)
            les.zf_cache, les.zh_cache = les.get_zf(), les.get_zh()
            les.attach_fields(seed=40 + i)
            les_models.append(les)
        les_models[0].model_time = les_models[1].model_time = 900.0
        spcpl.gather_gcm_data(gcm, les_models, False, write=False)
        numpy.random.seed(7)
        if route == "batched":
            reqs = spcpl.set_les_forcings_batched(les_models, gcm, True, True, {}, dt_gcm=900.0, factor=1.0, couple_surface=False,
                                                  qt_forcing='variance', write=False, variability_nudge_constant_T=True)
        else:
            reqs = [spcpl.set_les_forcings(les, gcm, True, True, {}, 900.0, 1.0, False, qt_forcing='variance', write=False,
                                           variability_nudge_constant_T=True) for les in les_models]
        assert len(reqs) == 3
        assert not hasattr(les_models[2].fields, "QT")
        numpy.random.seed(7)
        for les in les_models[:2]:
            f = dict(les.f3, presf=les.get_presf(), ql_ref=numpy.asarray(les.ql_ref))
            r = _ref(f, vo.make_R(8, 8), True)
            assert r["error"] is None and (r["status"] != 0).any()
            assert les.fields.QT.dtype == numpy.float32 and numpy.array_equal(les.fields.QT, r["qt"])
            assert numpy.abs(les.fields.THL.astype(numpy.float64) - r["thl"]).max() <= THL_ULP * EPS32 * numpy.abs(r["thl"]).max()
    finally:
        spcpl.set_engine(None)


@pytest.mark.gpu
def test_f32_variability_nudge_ensemble():
    """variability_nudge_ensemble on a float32 engine: [n x itot x jtot x k] fields through get/set_fields_batched"""
    spcpl, _ = _f32_engine()

    class Ens:
        def __init__(self, fs):
            self.fs = fs
            self.ql_ref = numpy.stack([f["ql_ref"] for f in fs])
            self.set = {}

        def __len__(self):
            return len(self.fs)

        def get_fields_batched(self, name):
            return numpy.stack([{"Qsat": f["qsat"], "QT": f["qt"], "THL": f["thl"], "QL": f["ql"]}[name] for f in self.fs])

        def get_profiles_batched(self, names, out):
            for n in names:
                out[n][:] = numpy.stack([{"QL": f["ql_av"], "QT": f["qt_av"], "presf": f["presf"]}[n] for f in self.fs])

        def set_fields_batched(self, name, arr):
            self.set[name] = arr

    try:
        fs = [make_les_fields(24, 20, 30, seed=90 + i) for i in range(3)]
        ens = Ens(fs)
        numpy.random.seed(5)
        out = spcpl.variability_nudge_ensemble(ens, 900.0, constantT=True, write=False)
        numpy.random.seed(5)
        for i, f in enumerate(fs):
            r = _ref(f, vo.make_R(24, 20), True)
            assert r["error"] is None
            assert numpy.array_equal(out[i]["beta"], r["beta"]) and numpy.array_equal(out[i]["qt_std"], r["qt_std"])
            assert ens.set["QT"].dtype == numpy.float32 and numpy.array_equal(ens.set["QT"][i], r["qt"])
            assert numpy.abs(ens.set["THL"][i].astype(numpy.float64) - r["thl"]).max() <= THL_ULP * EPS32 * numpy.abs(r["thl"]).max()
    finally:
        spcpl.set_engine(None)


@pytest.mark.gpu
def test_f64_and_f32_engines_one_after_the_other_give_their_own_bits():
    """a float64 and a float32 engine in one process, alternating (library plan / LDS-limit caches, per-engine workspaces):
    each gives its own restatement's bits"""
    from sp_coupler_amd import spcpl
    from sp_coupler_amd.engine import Engine
    engines = {torch.float64: Engine("cuda:0"), torch.float32: Engine("cuda:0", dtype=torch.float32)}
    try:
        for dtype in (torch.float64, torch.float32, torch.float64, torch.float32):
            spcpl.set_engine(engines[dtype])
            f = make_les_fields(64, 64, 40, seed=21)
            m = FieldLES(f, f["ql_ref"].copy())
            numpy.random.seed(8)
            g = spcpl.variability_nudge(m, 900.0, True, write=False)
            numpy.random.seed(8)
            R = vo.make_R(64, 64)
            if dtype == torch.float64:
                r = vo.variability_nudge(f["qt"], f["qsat"], f["ql_av"], f["qt_av"], f["presf"], f["ql_ref"], R, 900.0, True,
                                         thl=f["thl"], ql=f["ql"])
                assert m.fields.QT.dtype == numpy.float64
                assert numpy.array_equal(m.fields.QT, r["qt"]) and numpy.array_equal(g["beta"], r["beta"])
                assert numpy.array_equal(g["qt_std"], r["qt_std"]) and numpy.array_equal(g["status"], r["status"])
            else:
                _check(g, _ref(f, R, True), m, f, True)
    finally:
        spcpl.set_engine(None)


@pytest.mark.gpu
def test_f32_engine_takes_a_strided_float64_R():
    """Engine.variability_nudge on a float32 engine with R given as views the kernel cannot read in place -- a slice whose
    reshape to [n x itot*jtot] is a copy, a view with a larger row pitch -- gives the bits of a contiguous R; a float32 R is
    refused"""
    from sp_coupler_amd.engine import Engine
    eng = Engine("cuda:0", dtype=torch.float32)
    n, it, jt, kt = 3, 16, 12, 40
    fs = [make_les_fields(it, jt, kt, seed=50 + i) for i in range(n)]
    dev = lambda key, dt=torch.float32: torch.from_numpy(numpy.stack([f[key] for f in fs])).to("cuda:0", dt)   # noqa: E731
    R = torch.from_numpy(numpy.random.default_rng(4).normal(size=(n, it, jt))).cuda()
    big = torch.zeros(n, it + 3, jt + 5, dtype=torch.float64, device="cuda:0")
    big[:, :it, :jt] = R
    wide = torch.zeros(n, 2, it, jt, dtype=torch.float64, device="cuda:0")
    wide[:, 1] = R

    def run(Rv):
        qt, thl = dev("qt"), dev("thl")
        res = eng.variability_nudge(qt, dev("qsat"), Rv, dev("ql_av"), dev("qt_av"), dev("ql_ref"), presf=dev("presf"), thl=thl,
                                    ql=dev("ql"), constantT=True)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in dict(res, qt=qt, thl=thl).items()}
    want = run(R)
    assert (want["status"] != 0).any()
    for Rv in (big[:, :it, :jt], wide[:, 1]):
        assert not Rv.is_contiguous()
        got = run(Rv)
        for k, v in want.items():
            assert numpy.array_equal(got[k], v), k
    with pytest.raises(ValueError, match="float64"):
        run(R.float())
