"""K21 without a GPU: the struct layout of spc_les_buoyancy_args, the host-side refusals of spc_les_buoyancy_*, buoyancy.py (the
constants, the profiles and their refusals), properties of the NumPy oracle of tests/les_buoyancy_ref.py (a uniform state moves
no wind, planes of two have no gradient, a NaN reaches its own column below it and the neighbours' winds, a warm column draws
air in and lifts it), and models.DeviceLESEnsemble's enable_buoyancy() on an oracle-backed engine against its host twins."""
import ctypes
import os
import subprocess

import numpy
import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import advection as adv
from sp_coupler_amd import buoyancy as buo
from sp_coupler_amd import sputils
from tests import les_buoyancy_ref as lbr
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [p + (k,) for p in lbr.PLANES for k in (1, 2, 7, 65)]     # itot x jtot x ktot


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


def test_struct_layout_of_the_buoyancy_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror"""
    cls, cname = _abi.LesBuoyancyArgs, "spc_les_buoyancy_args"
    fields = ["n_les", "itot", "jtot", "ktot", "reserved", "thl", "qt", "ql", "u", "v", "hx", "hy", "t0", "lex", "s", "pitch_prof", "c1", "c2",
              "phi", "psfc", "amax"]
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
    assert got == want


def _args(n=4, itot=8, jtot=8, ktot=20, pitch_prof=None, **ptrs):
    a = _abi.LesBuoyancyArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.c1, a.c2 = n, itot, jtot, ktot, buo.C1, buo.C2
    a.pitch_prof = ktot if pitch_prof is None else pitch_prof
    for i, k in enumerate(lbr.PTRS):                              # distinct, 16-byte aligned, never dereferenced
        setattr(a, k, ptrs.get(k, 4096 * (i + 1)))
    return a


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch: none of these calls needs a device"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_buoyancy_" + sfx)

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
    for k in ("thl", "qt", "u", "v", "phi", "hx", "hy", "t0", "lex", "s"):
        assert call(**{k: None}) == (E, b"required pointer %s is NULL" % k.encode())
    assert call(n=-1)[0] == E
    for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
        rc, text = call(**bad)
        assert rc == E and b">= 1" in text
    rc, text = call(pitch_prof=19)
    assert rc == E and b"pitch_prof" in text
    ptr = lambda k: 4096 * (1 + lbr.PTRS.index(k))                                           # noqa: E731
    for key in lbr.INPUTS:
        for out in lbr.WRITTEN:
            rc, text = call(**{out: ptr(key)})
            assert rc == E and b"also an input" in text and out.encode() in text, (out, key)
    for x in range(5):
        for y in range(x + 1, 5):
            rc, text = call(**{lbr.WRITTEN[y]: ptr(lbr.WRITTEN[x])})
            assert rc == E and b"same array" in text and lbr.WRITTEN[y].encode() in text, (x, y)
    rc, text = call(thl=4100 if sfx == "f64" else 4098)
    assert rc == E and b"not aligned" in text
    rc, text = call(n=1 << 40, ktot=3)
    assert rc == U and b"too many workgroups" in text
    last = 1279 if sfx == "f64" else 2559
    rc, text = call(ktot=last + 1, pitch_prof=4000)
    assert rc == U and b"levels" in text and str(last).encode() in text
    assert fn(ctypes.byref(_args(n=0, **{k: None for k in lbr.PTRS})), None) == 0      # an empty ensemble is a no-op
    assert lib.spc_abi_version() == 4


def test_columns_per_block(lib):
    """K15's budget rule on ONE tile of ktot | 1 elements per column: the largest of 64, 32, 16 columns within 64 KiB, 16 may take
    160 KiB"""
    f = lib.spc_les_buoyancy_cols_per_block
    for esize in (4, 8):
        for ktot in (1, 2, 126, 127, 128, 129, 160, 254, 255, 256, 257, 511, 512, 1278, 1279, 1280, 1281, 2558, 2559, 2560, 5000):
            assert f(ktot, esize) == lbr.derived_cols(ktot, esize), (ktot, esize)
    assert f(0, 8) == 0 and f(160, 2) == 0 and (f(160, 8), f(160, 4), f(1279, 8), f(1280, 8), f(2559, 4), f(2560, 4)) == (32, 64, 16, 0, 16, 0)


# -- buoyancy.py -------------------------------------------------------------------------------------------------------------------
def test_constants():
    assert (buo.GRAV, buo.RLV, buo.CP, buo.RD, buo.RV) == (sputils.grav, sputils.rlv, sputils.cp, sputils.rd, sputils.rv)
    assert buo.C1 == 461.5 / 287.04 - 1.0 and buo.C2 == 461.5 / 287.04 and buo.WAVE_SPEED == 30.0
    assert abs(buo.WAVE_SPEED - 0.01 * 1e4 / numpy.pi) < 2.0          # N H / pi of H = 10 km, N = 0.01 / s


def test_profiles_against_a_float64_restatement_and_their_refusals():
    rng = numpy.random.default_rng(1)
    rhobf, zh, zf, presf, _ = lbr.lrr.grid(3, 6, rng)
    thl = 290.0 + rng.random((3, 6))
    qt = 8e-3 * (1.0 + rng.random((3, 6)))
    ql = 3e-4 * rng.random((3, 6))
    t0, lex, s = buo.profiles(thl, qt, ql, presf, zh)
    assert all(a.dtype == numpy.float64 and a.shape == (3, 6) and a.flags.c_contiguous for a in (t0, lex, s))
    dz = numpy.diff(zh, axis=1)
    dz = numpy.concatenate([dz, dz[:, -1:]], axis=1)
    ex = (presf / 1e5) ** (287.04 / 1004.0)
    lex_ = 2.53e6 / (1004.0 * ex)
    t0_ = (thl + lex_ * ql) * (1.0 + (461.5 / 287.04 - 1.0) * qt - (461.5 / 287.04) * ql)
    assert numpy.allclose(lex, lex_, rtol=1e-15) and numpy.allclose(t0, t0_, rtol=1e-14) and numpy.allclose(s, 0.5 * 9.81 * dz / t0_, rtol=1e-14)
    dry = buo.profiles(thl, qt, None, presf, zh)
    assert_bits("no liquid water", dry[0], buo.profiles(thl, qt, numpy.zeros((3, 6)), presf, zh)[0])
    assert numpy.allclose(dry[0], thl * (1.0 + 0.6078 * qt), rtol=1e-4)
    one = buo.profiles(thl[:, :1], qt[:, :1], ql[:, :1], presf[:, :1], zh[:, :1], zf=zf[:, :1])
    assert numpy.allclose(one[2], 0.5 * 9.81 * 2 * (zf[:, :1] - zh[:, :1]) / one[0])
    with pytest.raises(ValueError, match="zf"):
        buo.profiles(thl[:, :1], qt[:, :1], ql[:, :1], presf[:, :1], zh[:, :1])
    for k, bad in ((3, zh[2, 2]), (3, zh[2, 1]), (2, numpy.nan)):       # a dz of zero, a negative one, not finite
        x = zh.copy()
        x[2, k] = bad
        with pytest.raises(ValueError, match="positive and finite"):
            buo.profiles(thl, qt, ql, presf, x)
    for bad in (numpy.nan, -300.0, numpy.inf):
        x = thl.copy()
        x[1, 2] = bad
        with pytest.raises(ValueError, match="virtual potential temperature"):
            buo.profiles(x, qt, ql, presf, zh)
    with pytest.raises(ValueError):
        buo.profiles(thl, qt[:, :4], ql, presf, zh)
    assert buo.wave_substeps(900.0, 30000.0, 45000.0, 0.5) == 2 and buo.wave_substeps(900.0, 30000.0, numpy.array([45000.0, 9000.0]), 0.5) == 6
    assert buo.wave_substeps(1.0, 200.0, 200.0, 0.5) == 1 and buo.wave_substeps(900.0, 30000.0, 45000.0, 0.5, wave_speed=0.0) == 1


# -- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_uniform_state_moves_no_wind(dtype):
    """uniform on every level: the same phi in every column, every gx and gy +0, every wind keeps its bits (-0.0 included),
    amax = +0"""
    for shape in ((2, 3, 4, 9), (1, 1, 1, 1), (3, 8, 8, 65)):
        c = lbr.uniform_case(dtype, shape)
        phi, psfc, un, vn, amax = lbr.oracle(c)
        assert phi.dtype == un.dtype == amax.dtype == dtype
        assert_bits("u", un, c["u"])
        assert_bits("v", vn, c["v"])
        assert_bits("amax", amax, numpy.zeros_like(amax))
        assert_bits("phi", phi, numpy.broadcast_to(phi[:, :1, :1, :], phi.shape))
        assert (phi != 0).any()


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_planes_of_two_have_no_gradient(shape, dtype):
    c = lbr.case((2,) + shape, dtype)
    for ql in (True, False):
        phi, psfc, un, vn, amax = lbr.oracle(c, ql)
        assert (un.tobytes() == c["u"].tobytes()) == (shape[0] <= 2) and (vn.tobytes() == c["v"].tobytes()) == (shape[1] <= 2)
        assert (amax == 0).all() == (max(shape[:2]) <= 2)
        # the chain: q[0] = phi[0] - b[0] and phi[0] = q[1] - b[0], so psfc lies as far below phi[0] as q[1] above it
        if shape[2] == 1:
            assert_bits("one level: psfc = phi - b = 2 phi", psfc, phi[..., 0] + phi[..., 0])


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_reach_of_a_nan(dtype):
    c, s = lbr.nan_case(dtype)
    lbr.check_nan_reach(lbr.oracle(c), lbr.oracle(s), c["thl"].shape)


def warm_column(dtype=numpy.float64):
    """a resting 5 x 5 x 8 LES at its own reference state, with one column 1 K warmer at the levels 2 ... 4"""
    shape, col = (1, 5, 5, 8), (0, 2, 2)
    c = lbr.case(shape, dtype, seed=20)
    thm, qtm = 290.0 + numpy.arange(8.0), numpy.full(8, 5e-3)
    zh = 50.0 * numpy.arange(8.0)
    presf = 1e5 * numpy.exp(-(zh + 25.0) / 8000.0)
    t0, lex, s = buo.profiles(thm[None], qtm[None], None, presf[None], zh)
    c.update(t0=t0.astype(dtype), lex=lex.astype(dtype), s=s.astype(dtype))
    c["qt"][...] = qtm.astype(dtype)
    c["ql"][...] = 0
    c["u"][...] = 0
    c["v"][...] = 0
    # thl such that tv == t0 exactly is not representable in general: take the reference column as the oracle sees it and
    # measure the anomaly against a run without it
    c["thl"][...] = thm.astype(dtype)
    warm = dict(c, thl=c["thl"].copy())
    warm["thl"][col + (slice(2, 5),)] += dtype(1.0)
    return c, warm, col


def test_a_warm_column_draws_air_in_and_lifts_it():
    """phi below the anomaly is lower than in the resting columns and equal to theirs above it; after one substep of twin
    K21 + K16 + K17 the mass flux over the warm column is upward"""
    rest, warm, col = warm_column()
    p0, pw = lbr.oracle(rest)[0], lbr.oracle(warm)[0]
    d = pw - p0
    assert (d[col][:5] < 0).all() and (d[col][5:] == 0).all()
    others = numpy.ones(d.shape[:3], dtype=bool)
    others[col] = False
    assert (d[others] == 0).all()
    assert (numpy.abs(p0 - p0[:, :1, :1, :]) == 0).all()              # the resting state is uniform: no force
    phi, psfc, u, v, amax = lbr.oracle(warm)
    l, i, j = col
    assert (u[l, i - 1, j, :5] > 0).all() and (u[l, i + 1, j, :5] < 0).all() and (v[l, i, j - 1, :5] > 0).all() and (v[l, i, j + 1, :5] < 0).all()
    assert (u[l, i, j] == 0).all() and amax[0] > 0
    f = {"U": u, "V": v, "THL": warm["thl"], "QT": warm["qt"]}
    new, _ = lbr.lar.les_advect(f, u, v, warm["hx"], warm["hy"])
    g, r = adv.vertical_profiles(numpy.full((1, 8), 50.0 * 1.1))
    _, _, mtop = lbr.lvr.les_vadvect(new, new["U"], new["V"], warm["hx"], warm["hy"], g, r)
    assert (mtop[col][:5] > 0).all() and mtop[col][-1] > 0
    assert mtop[others].max() < mtop[col].max()


def test_engines_have_the_method():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    assert callable(Engine.les_buoyancy) and callable(MultiDeviceEngine.les_buoyancy) and callable(Engine.buoyancy_cols_per_block)
    assert not hasattr(lbr.lrr.RadiateOracleEngine, "les_buoyancy")


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def _counted(engine, calls):
    for name in ("les_buoyancy", "les_advect", "les_vadvect", "les_thermo", "slab_means"):
        inner = getattr(engine, name)
        setattr(engine, name, lambda *a, _n=name, _f=inner, **kw: (calls.append(_n), _f(*a, **kw))[1])
    return engine


def substep_calls(calls):
    """the K16 / K17 / K21 calls of a log of engine calls, in order"""
    return [c for c in calls if c in ("les_buoyancy", "les_advect", "les_vadvect")]


@pytest.mark.parametrize("variant", list(lbr.VARIANTS))
def test_ensemble_on_one_engine_equals_the_host_twin(variant):
    """every profile, field and phi bit-equal to the twin after each of three steps and the nudge; per step the two probes, then
    K21, K16 and K17 per substep, in that order"""
    subs = lbr.check_ensemble(lbr.BuoyancyOracleEngine(), [lbr.BuoyancyOracleEngine()], 4, variant)
    calls, without = [], []
    lbr.ensemble_run(_counted(lbr.BuoyancyOracleEngine(), calls), 4, True, **lbr.VARIANTS[variant])
    lbr.ensemble_run(_counted(lbr.BuoyancyOracleEngine(), without), 4, True, buoyancy=None, **lbr.VARIANTS[variant])
    assert len(subs) == 4 and subs[2] == subs[3]                       # (the record after the nudge repeats the second step's)
    want = []
    for n_sub in subs[:2] + subs[3:]:
        want += ["les_advect", "les_vadvect"] + ["les_buoyancy", "les_advect", "les_vadvect"] * n_sub
    assert substep_calls(calls) == want
    assert "les_buoyancy" not in without


def test_ensemble_as_row_blocks_with_an_empty_device():
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(lbr.BuoyancyOracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    subs = lbr.check_ensemble(lbr.BuoyancyOracleEngine(), [multi], 2, "plain")
    assert calls.count("les_buoyancy") == 2 * sum(subs[:2] + subs[3:])          # blocks 1 + 1 + 0: two devices


def _small(eng, n=2, nL=6):
    spcpl.set_engine(eng)
    gcm, src = models.make_batched_models(n, nL=nL)
    return models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, itot=2, jtot=3, engine=eng)


def _fields(rng, names=("THL", "QT", "Qsat", "U", "V")):
    base = {"THL": 290.0, "QT": 9e-3, "Qsat": 8.7e-3, "U": 5.0, "V": -2.0}
    return {k: base[k] * (1.0 + 0.05 * rng.random((2, 2, 3, 6))) for k in names}


def test_enable_buoyancy_refusals():
    eng = lbr.BuoyancyOracleEngine()
    rng = numpy.random.default_rng(1)
    ens = _small(eng)
    ens.attach_fields(_fields(rng))
    with pytest.raises(ValueError, match="vertical=True"):
        ens.enable_buoyancy()
    ens.enable_advection()
    with pytest.raises(ValueError, match="vertical=True"):
        ens.enable_buoyancy()
    ens.enable_advection(vertical=True)
    for bad in (numpy.nan, -1.0, numpy.inf):
        with pytest.raises(ValueError, match="wave_speed"):
            ens.enable_buoyancy(wave_speed=bad)
    assert not ens.buoyancy and ens.get_pressure_batched() is None
    ens.enable_buoyancy()
    assert ens.buoyancy and ens.buoyancy_wave_speed == 30.0 and ens.get_pressure_batched() is None and ens.buoyancy_wind_change is None
    ens.enable_advection(vertical=True)                              # the advection set up anew: the pressure force is off again
    assert not ens.buoyancy
    for missing in ("THL", "QT"):
        ens = _small(eng)
        ens.attach_fields(_fields(rng, tuple(k for k in ("THL", "QT", "Qsat", "U", "V") if k != missing)))
        ens.enable_advection(vertical=True)
        with pytest.raises(ValueError, match=missing):
            ens.enable_buoyancy()
    old = _small(lbr.lrr.RadiateOracleEngine())
    old.attach_fields(_fields(rng))
    old.enable_advection(vertical=True)
    with pytest.raises(ValueError, match="les_buoyancy"):
        old.enable_buoyancy()


def test_substeps_have_a_floor_from_the_wave_speed():
    """n_sub = max(the Courant probes', ceil(wave_speed dt / (cfl min(dx, dy)))); above max_substeps the step is refused"""
    eng = lbr.BuoyancyOracleEngine()
    rng = numpy.random.default_rng(2)
    for speed, want in ((0.0, 1), (None, 2), (100.0, 5)):
        ens = _small(eng)
        ens.attach_fields(_fields(rng))
        ens.enable_advection(dx=30000.0, dy=[45000.0, 36000.0], vertical=True)
        ens.enable_buoyancy(wave_speed=speed)
        ens.evolve_model_batched(float(ens.model_time) + 750.0)
        assert ens.advect_substeps == want == max(1, int(numpy.ceil((30.0 if speed is None else speed) * 750.0 / (0.5 * 30000.0))))
        assert numpy.isfinite(ens.buoyancy_wind_change) and tuple(ens.get_pressure_batched().shape) == (2, 2, 3, 6)
    ens = _small(eng)
    ens.attach_fields(_fields(rng))
    ens.enable_advection(dx=30000.0, dy=45000.0, vertical=True, max_substeps=4)
    ens.enable_buoyancy(wave_speed=100.0)
    with pytest.raises(RuntimeError, match="max_substeps"):
        ens.evolve_model_batched(float(ens.model_time) + 750.0)


def test_a_pressure_that_is_not_finite_ends_the_step():
    eng = lbr.BuoyancyOracleEngine()
    ens = _small(eng)
    f = _fields(numpy.random.default_rng(3))
    f["THL"][0, 1, 1, 3] = numpy.inf
    ens.attach_fields(f)
    ens.enable_advection(dx=30000.0, dy=45000.0, vertical=True)
    ens.enable_buoyancy()
    with pytest.raises((RuntimeError, ValueError)):
        ens.evolve_model_batched(float(ens.model_time) + 750.0)


def test_profiles_are_uploaded_again_only_where_their_inputs_changed():
    eng = lbr.BuoyancyOracleEngine()
    ens = _small(eng)
    ens.attach_fields(_fields(numpy.random.default_rng(4)))
    ens.enable_advection(dx=30000.0, dy=45000.0, vertical=True)
    ens.enable_buoyancy()
    t = float(ens.model_time)
    ens.evolve_model_batched(t + 100.0)
    first = ens._buoyancy_prof
    assert len(first[1]) == 3 and all(tuple(a.shape) == (2, 6) for a in first[1])
    ens.evolve_model_batched(t + 200.0)                              # the advection moved the means: new profiles
    assert ens._buoyancy_prof is not first


@pytest.mark.parametrize("variant", list(lbr.VARIANTS))
def test_without_enable_buoyancy_nothing_changes(variant):
    """enable_buoyancy never called: three steps bit-equal to the ensemble of the K18 tests' engine, which has no les_buoyancy at
    all, on the same inputs, and no K21 launch"""
    calls = []
    new = lbr.ensemble_run(_counted(lbr.BuoyancyOracleEngine(), calls), 4, True, buoyancy=None, **lbr.VARIANTS[variant])[1]
    old = lbr.ensemble_run(lbr.lrr.RadiateOracleEngine(), 4, True, buoyancy=None, **lbr.VARIANTS[variant])[1]
    lbr.lmr.same_logs(old, new)
    assert "les_buoyancy" not in calls


def test_the_column_tile_cases_on_the_oracle_backed_engine(lib):
    """the plumbing of the coltile body runs without a GPU; the columns per workgroup are the library's"""
    eng = lbr.BuoyancyOracleEngine()
    eng.buoyancy_cols_per_block = lambda ktot: lib.spc_les_buoyancy_cols_per_block(ktot, numpy.dtype(lbr.np_of(eng)).itemsize)
    lbr.check_coltile(eng)


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(lbr.VARIANTS))
def test_float32_ensemble_on_one_engine_equals_the_host_twin(variant):
    """test_ensemble_on_one_engine_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    subs = lbr.check_ensemble(f32_of(lbr.BuoyancyOracleEngine)(), [f32_of(lbr.BuoyancyOracleEngine)()], 4, variant)
    calls, without = [], []
    lbr.ensemble_run(_counted(f32_of(lbr.BuoyancyOracleEngine)(), calls), 4, True, **lbr.VARIANTS[variant])
    lbr.ensemble_run(_counted(f32_of(lbr.BuoyancyOracleEngine)(), without), 4, True, buoyancy=None, **lbr.VARIANTS[variant])
    assert len(subs) == 4 and subs[2] == subs[3]                       # (the record after the nudge repeats the second step's)
    want = []
    for n_sub in subs[:2] + subs[3:]:
        want += ["les_advect", "les_vadvect"] + ["les_buoyancy", "les_advect", "les_vadvect"] * n_sub
    assert substep_calls(calls) == want
    assert "les_buoyancy" not in without


def test_float32_ensemble_as_row_blocks_with_an_empty_device():
    """test_ensemble_as_row_blocks_with_an_empty_device on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(f32_of(lbr.BuoyancyOracleEngine)(), calls) for _ in range(3)], min_cols_per_device=1)
    subs = lbr.check_ensemble(f32_of(lbr.BuoyancyOracleEngine)(), [multi], 2, "plain")
    assert calls.count("les_buoyancy") == 2 * sum(subs[:2] + subs[3:])          # blocks 1 + 1 + 0: two devices
