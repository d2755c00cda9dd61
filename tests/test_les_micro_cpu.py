"""K14 without a GPU: the struct layout of spc_les_micro_args, the host-side refusals of spc_les_microphysics_*, the NumPy
oracle of tests/les_micro_ref.py (answers worked out by hand, the identity where nothing can rain, the water budget),
microphysics.profiles, and models.DeviceLESEnsemble's microphysics mode on an oracle-backed engine against its host twin."""
import ctypes
import os
import subprocess

import numpy
import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import microphysics as mp
from tests import les_micro_ref as lmr
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {numpy.float64: 2.0 ** -52, numpy.float32: 2.0 ** -23}


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    return _abi.load_library()


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


def test_struct_layout_of_the_microphysics_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror"""
    cls, cname = _abi.LesMicroArgs, "spc_les_micro_args"
    fields = ["n_les", "itot", "jtot", "ktot", "reserved", "qt", "ql", "qr", "qr_new", "thl", "temp", "rain", "sed_out", "sed_in", "lcpex", "w",
              "pitch_prof", "dt", "qc0", "k_auto", "k_acc", "t_up", "t_dn", "qt_mean", "thl_mean", "qr_mean", "qi_mean", "pitch_mean"]
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%%zu\\n", sizeof(%s));' % cname, 'printf("%d\\n", SPC_ABI_VERSION);']
    want = [ctypes.sizeof(cls), 4]
    for f in fields:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
        want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and _abi.ABI_VERSION == 4


PTRS = ("qt", "ql", "qr", "qr_new", "thl", "temp", "rain", "sed_out", "sed_in", "lcpex", "w", "qt_mean", "thl_mean", "qr_mean", "qi_mean")


def _args(n=4, itot=8, jtot=8, ktot=20, pitch_prof=20, pitch_mean=20, **ptrs):
    a = _abi.LesMicroArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.pitch_prof, a.pitch_mean, a.dt = n, itot, jtot, ktot, pitch_prof, pitch_mean, 60.0
    for i, k in enumerate(PTRS):                                 # distinct, 16-byte aligned, never dereferenced
        setattr(a, k, ptrs.get(k, 4096 * (i + 1)))
    return a


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_microphysics_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch: none of these calls needs a device"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_microphysics_" + sfx)

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
    for k in ("qt", "ql", "qr", "qr_new", "sed_out", "sed_in"):
        assert call(**{k: None}) == (E, b"required pointer %s is NULL" % k.encode())
    assert call(lcpex=None)[0] == E and b"lcpex" in lib.spc_last_error()
    assert call(w=None)[0] == E and b"w (rain is given)" in lib.spc_last_error()
    assert call(n=-1)[0] == E
    for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
        rc, text = call(**bad)
        assert rc == E and b">= 1" in text
    for bad in (dict(pitch_prof=19), dict(pitch_mean=19)):
        rc, text = call(**bad)
        assert rc == E and b"smaller than ktot" in text
    rc, text = call(temp=None)
    assert rc == E and b"qi_mean without temp" in text
    rc, text = call(thl=None)
    assert rc == E and b"thl_mean without thl" in text
    for other in ("qr", "ql", "temp", "sed_out", "sed_in", "lcpex", "w"):    # qr_new (and any written array) must not be an input
        rc, text = call(qr_new=4096 * (PTRS.index(other) + 1))
        assert rc == E and b"also an input" in text, other
    for a, b in (("qt", "ql"), ("thl", "temp"), ("rain", "w"), ("qt_mean", "sed_out"), ("qi_mean", "qr")):
        rc, text = call(**{a: 4096 * (PTRS.index(b) + 1)})
        assert rc == E and b"also an input" in text, (a, b)
    for a, b in (("qr_new", "qt"), ("qr_new", "thl"), ("qt", "thl"), ("qt_mean", "qr_mean"), ("rain", "qt"), ("qi_mean", "qr_new")):
        rc, text = call(**{a: 4096 * (PTRS.index(b) + 1)})
        assert rc == E and b"two written arrays" in text, (a, b)
    rc, text = call(qt=4100 if sfx == "f64" else 4098)
    assert rc == E and b"not aligned" in text
    rc, text = call(n=1 << 40, ktot=3, pitch_prof=3, pitch_mean=3)
    assert rc == U and b"too many workgroups" in text
    rc, text = call(ktot=1, pitch_prof=1, pitch_mean=1)
    assert rc == U and b"ktot == 1" in text
    assert fn(ctypes.byref(_args(n=0, **{k: None for k in PTRS})), None) == 0      # an empty ensemble is a no-op
    assert call(n=0, qr_new=4096 * 3)[0] == 0
    assert call(thl=None, thl_mean=None, lcpex=None, n=1 << 40, ktot=3, pitch_prof=3, pitch_mean=3)[0] == U      # (accepted up to the grid)


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_answers_worked_out_by_hand(dtype):
    """one LES, one column, three levels, numbers whose every operation is exact in float32"""
    T = dtype
    f = lambda *v: numpy.array(v, dtype=T).reshape(1, 1, 1, -1)                            # noqa: E731
    p = lambda *v: numpy.array(v, dtype=T).reshape(1, -1)                                  # noqa: E731
    qt, ql, qr = f(8.0, 8.0, 8.0), f(0.0, 2.0, 1.0), f(4.0, 2.0, 8.0)
    thl, temp, rain = f(300.0, 300.0, 300.0), f(270.0, 268.0 - 7.5, 250.0), numpy.array([[[1.0]]], dtype=T)
    so, si, lc, w = p(0.5, 0.25, 1.0), p(0.5, 2.0, 0.0), p(2.0, 4.0, 8.0), p(16.0, 8.0, 2.0)
    r = lmr.les_micro(qt, ql, qr, so, si, lc, w, 2.0, thl=thl, temp=temp, rain=rain, qc0=1.0, k_auto=0.125, k_acc=0.0078125)
    # qs: level 0: (4 - 2) + 0.5 * 2 = 3; level 1: (2 - 0.5) + 2 * 8 = 17.5; level 2 (top): (8 - 8) + 0 = 0
    assert r["qs"].ravel().tolist() == [3.0, 17.5, 0.0]
    # ka = 0.25, kc = 0.015625: s0 = 0.25 * 0 + 0 * 3 = 0; s1 = 0.25 * 1 + (0.015625 * 2) * 17.5 = 0.796875; s2 = 0.25 * 0 + ... * 0 = 0
    assert r["s"].ravel().tolist() == [0.0, 0.796875, 0.0]
    assert r["qt"].ravel().tolist() == [8.0, 8.0 - 0.796875, 8.0] and r["qr_new"].ravel().tolist() == [3.0, 17.5 + 0.796875, 0.0]
    assert r["thl"].ravel().tolist() == [300.0, 300.0 + 4 * 0.796875, 300.0]
    assert r["rain"].ravel().tolist() == [1.0 + (0.5 * 4.0) * 16.0]
    # fi: 270 >= 268: 0; 260.5: 7.5 / 15 = 0.5; 250 <= 253: 1
    assert r["qi"].ravel().tolist() == [0.0, (2.0 - 0.796875) * 0.5, 1.0]
    for k, name in (("qt", "qt_mean"), ("thl", "thl_mean"), ("qr_new", "qr_mean"), ("qi", "qi_mean")):
        assert_bits(name, r[name], r[k][:, 0, 0, :])
    assert all(v.dtype == T for v in r.values())
    capped = lmr.les_micro(qt, ql, qr, so, si, lc, w, 2.0, qc0=1.0, k_auto=4.0, k_acc=0.0)                # ka = 8: s1 = 8 > ql = 2
    assert capped["s"].ravel().tolist() == [0.0, 2.0, 0.0] and "thl" not in capped and "qi" not in capped and "rain" not in capped


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_on_the_special_inputs_of_the_gpu_test(dtype):
    c = lmr.case((3, 3, 5, 7), dtype, seed=2, special=True)
    r = lmr.oracle(c)
    pt = lambda k: (slice(None), k // 5, k % 5)                                            # noqa: E731
    assert numpy.isnan(r["qt"][pt(0)]).all() and numpy.isnan(r["qr_new"][pt(1)]).all() and numpy.isnan(r["qi"][pt(2)]).all()
    assert numpy.isfinite(r["qt"][pt(2)]).all()                                              # a NaN temperature touches the ice only
    assert (~numpy.isfinite(r["s"][pt(3)])).all() and (~numpy.isfinite(r["qt"][pt(3)])).all()       # inf, or inf * 0 where qs == 0
    assert (~numpy.isfinite(r["s"][pt(6)])).all() and not (r["s"][pt(6)] > 0).any()                # the cap: s > ql gives ql = -inf
    assert (r["qi"][pt(5)][..., ::2] == 0).all()                                                     # temp = +inf: no ice
    assert (r["qi"][pt(5)][..., 1::2] == c["ql"][pt(5)][..., 1::2] - r["s"][pt(5)][..., 1::2]).all()  # temp = -inf: all ice
    assert (r["qi"][pt(8)] == c["ql"][pt(8)] - r["s"][pt(8)]).all()                         # temp = -0.0 <= t_dn: all ice
    assert numpy.signbit(r["qt"][pt(9)]).all() and (r["s"][pt(9)] == 0).all() and not numpy.signbit(r["s"][pt(9)]).any()
    assert (r["qi"][pt(10)] == 0).all() and (r["qi"][pt(11)] == c["ql"][pt(11)] - r["s"][pt(11)]).all() and (r["qi"][pt(11)] > 0).all()
    lo = lmr.oracle(lmr.case((3, 3, 5, 7), dtype, seed=4), qc0=float("nan"))
    assert numpy.isnan(lo["s"]).all()
    nb = lmr.case((2, 3, 5, 8), dtype, seed=1, neighbour=True)
    r = lmr.oracle(nb)
    assert (nb["qr"][..., 0] >= 0.3).all() and (r["qr_new"][..., 7] < 4e-3).all()           # the top level sees +0.0 above it


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_identity_where_nothing_can_rain(dtype):
    """ql <= qc0 everywhere and qr == 0: every field and rain keep their bits (-0.0 and NaN-free values alike)"""
    c = lmr.case((3, 5, 4, 9), dtype, seed=7)
    c["ql"] = numpy.minimum(c["ql"], dtype(mp.QC0)).astype(dtype)
    c["ql"][:, 0, 0, :] = dtype(mp.QC0)
    c["qr"][...] = 0.0
    c["qt"][:, 1, 1, 0] = -0.0
    r = lmr.oracle(c)
    assert (c["ql"] > 0).any() and (r["s"] == 0).all()
    for k, src in (("qt", "qt"), ("thl", "thl"), ("qr_new", "qr"), ("rain", "rain")):
        assert_bits(k, r[k], c[src])


#: the largest residual of the budget measured with this file's cases, in eps of T: 1.60 (f64, ktot 160) and 0.25 (f32, ktot 2)
#: at dt = 60; 1.60 and 0.21 at dt = 3600 (the issue's prototype measured 1.9 and 0.3 on its own cases)
@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("ktot", [2, 7, 64, 160])
@pytest.mark.parametrize("dt", [60.0, 3600.0])
def test_water_budget_of_the_oracle(ktot, dtype, dt):
    """per column sum_k((qt + qr) * w) + rain, evaluated in float64, is the same before and after to within 8 eps of T,
    relative: about four roundings of half an eps along each of the two flux paths (a cell's loss to the layer below -- the
    product sed_out * qr, the difference, the product sed_in * qr_up, the sum -- and the conversion -- s, qt - s, qs + s and the
    rounding of sed_in itself).  Measured maximum over these cases: 1.60 eps (f64) and 0.25 eps (f32) at dt = 60, 1.60 and 0.21
    at dt = 3600 (per ktot 2, 7, 64, 160: f64 1.02, 1.46, 1.50, 1.60 at both dt; f32 0.25, 0.12, 0.04, 0.03 and 0.21, 0.13,
    0.02, 0.02)"""
    c = lmr.case((3, 5, 4, ktot), dtype, seed=11, dt=dt)
    r = lmr.oracle(c)
    w = c["prof"][3]
    before = lmr.column_water(c["qt"], c["qr"], w, c["rain"])
    after = lmr.column_water(r["qt"], r["qr_new"], w, r["rain"])
    res = numpy.abs(after - before) / before
    print("budget ktot %d %s dt %g: max residual %.2f eps" % (ktot, numpy.dtype(dtype).name, dt, res.max() / EPS[dtype]))
    assert res.max() <= 8 * EPS[dtype]
    capped = (r["s"] == c["ql"]) & (c["ql"] > 0)
    if dt == 3600.0:
        assert capped.any()                                       # the cap s = ql is reached
    else:
        assert not capped.any() and (r["rain"] != c["rain"]).sum() >= 10


def test_profiles_of_the_module():
    rng = numpy.random.default_rng(1)
    zh = numpy.concatenate([[0.0], numpy.cumsum(40 + 60 * rng.random(9))])
    zf = zh + 10.0
    rhobf, presf = 1.2 - 0.01 * rng.random((3, 10)), 1e5 - 1e3 * numpy.arange(10) * numpy.ones((3, 1))
    so, si, lc, w = mp.profiles(zh, zf, rhobf, presf, 10.0, 5.0)
    dz = numpy.append(numpy.diff(zh), zh[-1] - zh[-2])
    assert all(a.shape == (3, 10) and a.dtype == numpy.float64 and a.flags.c_contiguous and a.flags.writeable for a in (so, si, lc, w))
    assert numpy.array_equal(w, rhobf * dz) and numpy.array_equal(so[0], numpy.minimum(50.0 / dz, 1.0)) and (so[:, dz < 50].ravel() == 1).all()
    assert numpy.array_equal(si[:, :-1], so[:, 1:] * w[:, 1:] / w[:, :-1]) and (si[:, -1] == 0).all()
    assert numpy.array_equal(lc, (2.53e6 / 1004.) / (presf / 1e5) ** (287.04 / 1004.))
    gcm, ens = models.make_batched_models(3, nL=10)
    dev = models.DeviceLESEnsemble(ens.grid_indices, ens.zf_cache, ens.zh_cache, ens.p)
    got = mp.profiles(dev.zh_cache, dev.zf_cache, dev.p["Rhobf"], dev.p["presf"], 900.0)
    assert numpy.array_equal(got[3], dev.water_path_weights())   # exactly K13's weights
    assert (mp.QC0, mp.K_AUTO, mp.K_ACC, mp.T_UP, mp.T_DN, mp.V_FALL) == (5e-4, 1e-3, 2.2, 268.0, 253.0, 5.0)


def test_engines_have_the_method():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    from tests.fake_engine import OracleEngine
    assert callable(Engine.les_microphysics) and callable(MultiDeviceEngine.les_microphysics) and not hasattr(OracleEngine, "les_microphysics")


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def _counted(engine, calls):
    inner = engine.les_microphysics
    engine.les_microphysics = lambda qt, *a, **kw: (calls.append((int(qt.shape[0]), kw.get("temp") is not None)), inner(qt, *a, **kw))[1]
    return engine


@pytest.mark.parametrize("thermo", [False, True])
def test_ensemble_on_one_engine_equals_the_host_twin(thermo):
    calls = []
    lmr.check_ensemble(lmr.MicroOracleEngine(), [_counted(lmr.MicroOracleEngine(), calls)], 4, thermo)
    assert calls == [(4, thermo)] * 3                            # one launch per step


@pytest.mark.parametrize("thermo", [False, True])
def test_ensemble_as_row_blocks_with_an_empty_device(thermo):
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(lmr.MicroOracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    lmr.check_ensemble(lmr.MicroOracleEngine(), [multi], 2, thermo)
    assert calls == [(1, thermo)] * 6                            # blocks 1 + 1 + 0: the device without rows launches nothing


@pytest.mark.parametrize("thermo", [False, True])
def test_fused_step_then_microphysics(monkeypatch, thermo):
    """K11 steps the fields (FUSED_MIN_LES patched to 0), K14 follows: the same bits as the twin"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    steps = []
    eng = lmr.MicroOracleEngine()
    inner = eng.les_advance
    eng.les_advance = lambda *a, **kw: (steps.append(kw.get("sat")), inner(*a, **kw))[1]
    lmr.check_ensemble(lmr.MicroOracleEngine(), [eng], 3, thermo)
    assert steps == [None if thermo else "QT"] * 3


def test_without_the_call_every_path_keeps_its_bits():
    """enable_microphysics() is opt-in: an ensemble that never calls it evolves as the twin of the parent's path, Rain included"""
    host = lmr.ensemble_run(lmr.MicroOracleEngine(), 3, False, False, micro=False)[1]
    ens, dev = lmr.ensemble_run(lmr.MicroOracleEngine(), 3, False, True, micro=False)
    lmr.same_logs(host, dev)
    assert not ens.micro and ens.rain2d is None and numpy.allclose(dev[-1]["p Rain"], dev[0]["p Rain"] + 3 * (1e-6 * 900.0), rtol=1e-12, atol=0)


def test_enable_microphysics_creates_what_it_needs_and_refuses_what_it_cannot_take():
    eng = lmr.MicroOracleEngine()
    spcpl.set_engine(eng)
    gcm, src = models.make_batched_models(2, nL=6)
    ens = models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, itot=2, jtot=3, engine=eng)
    with pytest.raises(ValueError, match="QT field"):
        ens.enable_microphysics()
    ens.set_fields_batched("QT", numpy.full((2, 2, 3, 6), 1e-2))
    ens.enable_microphysics(k_acc=1.0)
    assert ens.micro and tuple(ens.fields3d["QR"].shape) == (2, 2, 3, 6) and not ens.fields3d["QR"].any()
    assert tuple(ens.rain2d.shape) == (2, 2, 3) and not ens.rain2d.any() and ens._qr_spare is not ens.fields3d["QR"]
    assert ens.micro_par == {"v_fall": 5.0, "qc0": 5e-4, "k_auto": 1e-3, "k_acc": 1.0}
    with pytest.raises(ValueError, match="cloud water"):
        ens.evolve_model_batched(900.0)                          # neither Qsat nor QL nor thermo: no cloud water to convert
    ens.set_fields_batched("Qsat", numpy.full((2, 2, 3, 6), 9e-3))
    ens.evolve_model_batched(900.0)
    first = ens._micro_prof
    ens.evolve_model_batched(1800.0)
    assert ens._micro_prof is first and (ens.p["QR"] > 0).all()  # same dt, grid and profiles: nothing uploaded again
    ens.zh_cache = numpy.asarray(ens.zh_cache) * 2.0             # another grid: other sed_out, sed_in and w
    ens.evolve_model_batched(2700.0)
    assert ens._micro_prof is not first and not numpy.array_equal(ens._micro_prof[0][4], first[0][4])
    one = models.DeviceLESEnsemble(src.grid_indices, src.zf_cache[:1], src.zh_cache[:1], {k: (v[:, :1] if v.ndim == 2 else v) for k, v in src.p.items()},
                                   engine=eng)
    one.set_fields_batched("QT", numpy.zeros((2, 2, 2, 1)))
    with pytest.raises(ValueError, match="one level"):
        one.enable_microphysics()
    from tests.les_thermo_ref import ThermoOracleEngine
    old = models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, engine=ThermoOracleEngine())
    old.set_fields_batched("QT", numpy.zeros((2, 2, 2, 6)))
    with pytest.raises(ValueError, match="les_microphysics"):
        old.enable_microphysics()


def test_the_chain_cases_on_the_oracle_backed_engine():
    """the oracle alone handles every case of the chain body, none skipped; its plumbing runs without a GPU"""
    lmr.check_chain(lmr.MicroOracleEngine())
    assert "chain" in lmr.BODIES


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("thermo", [False, True])
def test_float32_ensemble_on_one_engine_equals_the_host_twin(thermo):
    """test_ensemble_on_one_engine_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    calls = []
    lmr.check_ensemble(f32_of(lmr.MicroOracleEngine)(), [_counted(f32_of(lmr.MicroOracleEngine)(), calls)], 4, thermo)
    assert calls == [(4, thermo)] * 3                            # one launch per step


@pytest.mark.parametrize("thermo", [False, True])
def test_float32_ensemble_as_row_blocks_with_an_empty_device(thermo):
    """test_ensemble_as_row_blocks_with_an_empty_device on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(f32_of(lmr.MicroOracleEngine)(), calls) for _ in range(3)], min_cols_per_device=1)
    lmr.check_ensemble(f32_of(lmr.MicroOracleEngine)(), [multi], 2, thermo)
    assert calls == [(1, thermo)] * 6                            # blocks 1 + 1 + 0: the device without rows launches nothing


@pytest.mark.parametrize("thermo", [False, True])
def test_float32_fused_step_then_microphysics(monkeypatch, thermo):
    """test_fused_step_then_microphysics on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    steps = []
    eng = f32_of(lmr.MicroOracleEngine)()
    inner = eng.les_advance
    eng.les_advance = lambda *a, **kw: (steps.append(kw.get("sat")), inner(*a, **kw))[1]
    lmr.check_ensemble(f32_of(lmr.MicroOracleEngine)(), [eng], 3, thermo)
    assert steps == [None if thermo else "QT"] * 3
