"""K15 without a GPU: the struct layout of spc_les_diffuse_args, the host-side refusals of spc_les_diffuse_* and
spc_les_diffuse_cols_per_block, diffusion.profiles, properties of the float64 NumPy oracle of tests/les_diffuse_ref.py
(conservation, the maximum principle, the identity, isolation of the columns), and models.DeviceLESEnsemble's diffusion mode on
an oracle-backed engine against its host twins."""
import ctypes
import os
import subprocess

import numpy
import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import diffusion as df
from sp_coupler_amd import microphysics as mp
from tests import les_diffuse_ref as ldr
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
DTS = [60.0, 900.0, 3600.0]


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


def test_struct_layout_of_the_diffusion_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror"""
    cls, cname = _abi.LesDiffuseArgs, "spc_les_diffuse_args"
    fields = ["n_les", "itot", "jtot", "ktot", "n_fields", "fields", "flux", "a", "m", "cp", "s0", "pitch_prof"]
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%%zu\\n", sizeof(%s));' % cname, 'printf("%d\\n", SPC_ABI_VERSION);', 'printf("%d\\n", SPC_DIFFUSE_MAX_FIELDS);']
    want = [ctypes.sizeof(cls), 4, _abi.SPC_DIFFUSE_MAX_FIELDS]
    for f in fields:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
        want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and _abi.ABI_VERSION == 4


def _args(n=4, itot=8, jtot=8, ktot=20, n_fields=4, pitch_prof=20, fields=None, flux=None, **ptrs):
    g = _abi.LesDiffuseArgs()
    g.n_les, g.itot, g.jtot, g.ktot, g.n_fields, g.pitch_prof = n, itot, jtot, ktot, n_fields, pitch_prof
    for i, k in enumerate(("a", "m", "cp", "s0")):                # distinct, 16-byte aligned, never dereferenced
        setattr(g, k, ptrs.get(k, 4096 * (i + 1)))
    for f in range(4):
        g.fields[f] = (fields or {}).get(f, 4096 * (f + 10))
        g.flux[f] = (flux or {}).get(f, 4096 * (f + 20) if f >= 2 else None)
    return g


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_diffusion_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch: none of these calls needs a device"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_diffuse_" + sfx)

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
    for k in ("a", "m", "cp"):
        assert call(**{k: None}) == (E, b"required pointer %s is NULL" % k.encode())
    assert call(fields={1: None})[0] == E and b"fields" in lib.spc_last_error()
    assert call(n=-1)[0] == E
    for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
        rc, text = call(**bad)
        assert rc == E and b">= 1" in text
    for nf in (0, 5, -1):
        rc, text = call(n_fields=nf)
        assert rc == E and b"field count" in text
    rc, text = call(pitch_prof=19)
    assert rc == E and b"smaller than ktot" in text
    rc, text = call(fields={3: 4096 * 10})
    assert rc == E and b"same field" in text
    for k, ptr in (("a", 4096), ("m", 2 * 4096), ("cp", 3 * 4096), ("s0", 4 * 4096)):
        rc, text = call(fields={2: ptr})
        assert rc == E and b"also a profile" in text, k
    rc, text = call(fields={2: 4096 * 22})                       # its own flux
    assert rc == E and b"also a profile" in text
    rc, text = call(s0=None)
    assert rc == E and b"without s0" in text
    assert call(s0=None, n_fields=2, n=1 << 40, ktot=3, pitch_prof=3)[0] == U      # (fields 0 and 1 have no flux: accepted up to the grid)
    rc, text = call(fields={0: 4100 if sfx == "f64" else 4098})
    assert rc == E and b"not aligned" in text
    top = 1279 if sfx == "f64" else 2559
    rc, text = call(ktot=top + 1, pitch_prof=top + 1)
    assert rc == U and str(top).encode() in text and b"levels" in text
    rc, text = call(n=1 << 40, ktot=3, pitch_prof=3)
    assert rc == U and b"too many workgroups" in text
    g = _args(n=0, a=None, m=None, cp=None, s0=None, fields={f: None for f in range(4)})
    assert fn(ctypes.byref(g), None) == 0                         # an empty ensemble is a no-op


def test_cols_per_block(lib):
    """64, 32 or 16 columns: the largest whose tile of odd pitch fits 64 KiB, 16 columns up to the 160 KiB of a CU"""
    f = lib.spc_les_diffuse_cols_per_block
    want = lambda ktot, es: next((c for c in (64, 32) if c * (ktot | 1) * es <= 65536), 16 if 16 * (ktot | 1) * es <= 163840 else 0)   # noqa: E731
    for es in (4, 8):
        assert all(f(k, es) == want(k, es) for k in range(1, 3000))
        assert [c for _, c in ldr.boundaries(lambda k: f(k, es))] == [64, 32, 32, 16, 16, 0]
    assert ldr.boundaries(lambda k: f(k, 8)) == [(127, 64), (128, 32), (255, 32), (256, 16), (1279, 16), (1280, 0)]
    assert ldr.boundaries(lambda k: f(k, 4))[-2:] == [(2559, 16), (2560, 0)]
    assert f(160, 8) == 32 and f(160, 4) == 64 and f(1024, 8) == 16
    assert f(0, 8) == 0 and f(-1, 8) == 0 and f(160, 2) == 0 and f(160, 16) == 0 and f(1 << 30, 4) == 0


# -- diffusion.profiles ---------------------------------------------------------------------------------------------------------
def synthetic_grid(n=3, nL=160):
    """the synthetic grid: 160 levels of 25 m"""
    zh = 25.0 * numpy.arange(nL)
    zf = zh + 12.5
    rhobf = 1.2 * numpy.exp(-zf / 9000.0) * (1.0 + 0.05 * numpy.arange(n))[:, None]
    return zh, zf, rhobf


@pytest.mark.parametrize("dt", DTS)
def test_profiles_of_the_module(dt):
    zh, zf, rhobf = synthetic_grid()
    a, b, c, w, dz = df.matrix(zh, zf, rhobf, dt)
    am, m, cp, s0 = df.profiles(zh, zf, rhobf, dt)
    assert all(x.shape == (3, 160) and x.dtype == numpy.float64 and x.flags.c_contiguous for x in (am, m, cp)) and s0.shape == (3,)
    assert numpy.array_equal(am, a) and numpy.array_equal(w, rhobf * mp.layer_thickness(zh, zf)) and (s0 == dt / 25.0).all()
    assert numpy.array_equal(b - 1.0, -(a + c)) or numpy.abs((b - 1.0) + (a + c)).max() <= 4 * EPS * numpy.abs(b).max()
    assert (a[:, 0] == 0).all() and (c[:, -1] == 0).all() and (a[:, 1:] < 0).all() and (c[:, :-1] < 0).all()
    assert (m > 0).all() and (m <= 1).all() and (cp > -1).all() and (cp <= 0).all()
    assert numpy.array_equal(w[:, :-1] * c[:, :-1], w[:, 1:] * a[:, 1:]) or numpy.allclose(w[:, :-1] * c[:, :-1], w[:, 1:] * a[:, 1:], rtol=4 * EPS, atol=0)
    if dt == 3600.0:
        assert 250 < numpy.abs(a).max() < 320                    # an explicit step would not do
    s = numpy.clip(zh[1:] / df.H_MIX, 0, 1)
    assert numpy.array_equal(df.diffusivity(zh[1:]), df.K_BG + df.K_MAX * 6.75 * s * (1 - s) ** 2)
    assert abs(df.diffusivity(numpy.array([500.0]))[0] - (df.K_BG + df.K_MAX)) < 1e-12 and df.diffusivity(numpy.array([1500.0, 4000.0])).tolist() == [df.K_BG] * 2
    assert (df.K_MAX, df.H_MIX, df.K_BG) == (50.0, 1500.0, 0.1)
    one = df.profiles(zh[:1], zf[:1], rhobf[:, :1], dt)          # an LES of one level: nothing to mix with
    assert (one[0] == 0).all() and (one[1] == 1).all() and (one[2] == 0).all() and (one[3] == dt / 25.0).all()


def thl_columns(n, nL, seed):
    rng = numpy.random.default_rng(seed)
    return 290.0 + 0.004 * 25.0 * numpy.arange(nL) + 0.5 * rng.standard_normal((n, 4, 5, nL))


# -- properties of the float64 oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_oracle_conserves_the_column(dt):
    """| sum_k w (x' - x) - dt rhobf[0] flux | <= ktot 2^-52 sum_k w |x| per column (evaluated in float64): every one of the
    ktot levels is rounded a few times to half an eps of values of the size of x, and w (x' - x) telescopes to the flux through
    the ground.  Measured on the synthetic grid with these THL-like columns: at most 0.06 of the bound at all three dt."""
    zh, zf, rhobf = synthetic_grid()
    a, m, cp, s0 = df.profiles(zh, zf, rhobf, dt)
    w = df.matrix(zh, zf, rhobf, dt)[3]
    x = thl_columns(3, 160, 1)
    flux = numpy.array([0.1, -0.05, 0.3])
    new = ldr.les_diffuse(x, a, m, cp, s0, flux)
    res = numpy.abs(((new - x) * w[:, None, None, :]).sum(axis=3) - (dt * rhobf[:, 0] * flux)[:, None, None])
    bound = 160 * EPS * (numpy.abs(x) * w[:, None, None, :]).sum(axis=3)
    print("conservation dt %g: worst residual %.3f of the bound" % (dt, (res / bound).max()))
    assert (res <= bound).all()
    assert (ldr.les_diffuse(x, a, m, cp)[..., 0] < new[..., 0])[[0, 2]].all()           # a positive flux raises level 0


@pytest.mark.parametrize("dt", DTS)
def test_oracle_keeps_the_maximum_principle(dt):
    """without a flux min(x) - e <= x' <= max(x) + e per column, e = ktot 2^-52 max|x|; and the answer is not the input"""
    zh, zf, rhobf = synthetic_grid()
    a, m, cp, _ = df.profiles(zh, zf, rhobf, dt)
    x = thl_columns(3, 160, 2)
    new = ldr.les_diffuse(x, a, m, cp)
    e = 160 * EPS * numpy.abs(x).max(axis=3)
    assert (new.min(axis=3) >= x.min(axis=3) - e).all() and (new.max(axis=3) <= x.max(axis=3) + e).all()
    assert (new != x).mean() > 0.99 and numpy.abs(new - x).max() > 0.1
    assert (numpy.abs(numpy.diff(new[..., :40], axis=3)).mean() < numpy.abs(numpy.diff(x[..., :40], axis=3)).mean())      # the mixed layer is smoother


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_identity_keeps_every_bit(dtype):
    for ktot in (1, 2, 7, 64):
        c = ldr.identity_case(dtype, ktot)
        r = ldr.oracle(c)
        assert numpy.signbit(c["fields"]["QT"][:, 0, 0, 0]).all()
        for k, v in c["fields"].items():
            assert_bits(k, r[k], v)


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_isolates_the_columns_and_rounds_in_the_element_type(dtype):
    """a NaN (an infinity) in one column changes no other column; f32 and f64 agree to 6.5e-7 relative at dt 60 ... 3600"""
    c, s, cols = ldr.special_case(dtype, 7)
    clean, got = ldr.oracle(c), ldr.oracle(s)
    others = numpy.ones(got["THL"].shape[:3], dtype=bool)
    for col in cols:
        others[col] = False
    assert_bits("others", got["THL"][others], clean["THL"][others])
    assert numpy.isnan(got["THL"][1, 1, 2]).all() and not numpy.isfinite(got["THL"][1, 2, 4]).any() and not numpy.isfinite(got["THL"][2, 0, 0]).any()
    assert all(v.dtype == dtype for v in got.values())
    if dtype == numpy.float32:
        zh, zf, rhobf = synthetic_grid()
        x = thl_columns(3, 160, 3)
        for dt in DTS:
            p = df.profiles(zh, zf, rhobf, dt)
            flux = numpy.array([0.1, 0.2, 0.3])
            r64 = ldr.les_diffuse(x, *p[:3], p[3], flux)
            r32 = ldr.les_diffuse(x.astype(dtype), *[q.astype(dtype) for q in p], flux.astype(dtype))
            assert numpy.abs(r32 / r64 - 1).max() <= 6.5e-7


def test_oracle_answer_worked_out_by_hand():
    """one column of three levels, numbers whose every operation is exact"""
    x = numpy.array([4.0, 8.0, 16.0]).reshape(1, 1, 1, 3)
    a, m, cp = numpy.array([[0.0, -2.0, -4.0]]), numpy.array([[0.5, 0.25, 0.125]]), numpy.array([[-0.5, -0.25, 0.0]])
    r = ldr.les_diffuse(x, a, m, cp, numpy.array([2.0]), numpy.array([6.0]))
    # d = 4 + 12 = 16; y0 = 8; y1 = (8 + 16) / 4 = 6; y2 = (16 + 24) / 8 = 5; x2 = 5; x1 = 6 + 1.25 = 7.25; x0 = 8 + 3.625
    assert r.ravel().tolist() == [11.625, 7.25, 5.0]
    assert ldr.les_diffuse(x[..., :1], a[:, :1], m[:, :1], cp[:, :1]).ravel().tolist() == [2.0]


def test_engines_have_the_method():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    assert callable(Engine.les_diffuse) and callable(MultiDeviceEngine.les_diffuse) and callable(Engine.diffuse_cols_per_block)
    assert not hasattr(ldr.lmr.MicroOracleEngine, "les_diffuse")


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def _counted(engine, calls):
    inner = engine.les_diffuse
    engine.les_diffuse = lambda fields, *a, **kw: (calls.append((sorted(fields), int(next(iter(fields.values())).shape[0]), sorted(kw.get("flux") or {}))),
                                                   inner(fields, *a, **kw))[1]
    return engine


@pytest.mark.parametrize("micro", [False, True])
@pytest.mark.parametrize("thermo", [False, True])
def test_ensemble_on_one_engine_equals_the_host_twin(thermo, micro):
    calls = []
    ldr.check_ensemble(ldr.DiffuseOracleEngine(), [_counted(ldr.DiffuseOracleEngine(), calls)], 4, thermo, micro=micro)
    assert calls == [(["QT", "THL", "U", "V"], 4, ["QT", "THL"])] * 3                     # one launch per step


@pytest.mark.parametrize("thermo", [False, True])
def test_ensemble_as_row_blocks_with_an_empty_device(thermo):
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(ldr.DiffuseOracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    ldr.check_ensemble(ldr.DiffuseOracleEngine(), [multi], 2, thermo, micro=thermo)
    assert calls == [(["QT", "THL", "U", "V"], 1, ["QT", "THL"])] * 6                     # blocks 1 + 1 + 0: the device without rows launches nothing


@pytest.mark.parametrize("thermo", [False, True])
def test_fused_step_then_diffusion(monkeypatch, thermo):
    """K11 steps the fields (FUSED_MIN_LES patched to 0), K15 follows: the same bits as the twin"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    steps = []
    eng = ldr.DiffuseOracleEngine()
    inner = eng.les_advance
    eng.les_advance = lambda *a, **kw: (steps.append(kw.get("sat")), inner(*a, **kw))[1]
    ldr.check_ensemble(ldr.DiffuseOracleEngine(), [eng], 3, thermo)
    assert steps == [None if thermo else "QT"] * 3


def test_without_the_call_every_path_keeps_its_bits():
    """enable_diffusion() is opt-in: an ensemble that never calls it evolves as the twin of the parent's path"""
    calls = []
    host = ldr.ensemble_run(ldr.DiffuseOracleEngine(), 3, False, False, diffuse=False)[1]
    ens, dev = ldr.ensemble_run(_counted(ldr.DiffuseOracleEngine(), calls), 3, False, True, diffuse=False)
    ldr.lmr.same_logs(host, dev)
    assert not ens.diffusion and ens._diffuse_prof is None and calls == []


def test_enable_diffusion_refuses_what_it_cannot_take_and_uploads_only_what_changed():
    eng = ldr.DiffuseOracleEngine()
    spcpl.set_engine(eng)
    gcm, src = models.make_batched_models(2, nL=6)
    ens = models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, itot=2, jtot=3, engine=eng)
    ens.set_fields_batched("QR", numpy.zeros((2, 2, 3, 6)))
    with pytest.raises(ValueError, match="needs one of the fields"):
        ens.enable_diffusion()
    ens.set_fields_batched("THL", 290.0 + numpy.arange(6.0) * numpy.ones((2, 2, 3, 6)))
    ens.enable_diffusion(k_bg=0.5)
    assert ens.diffusion and ens.diffuse_par == {"k_max": 50.0, "h_mix": 1500.0, "k_bg": 0.5}
    ens.evolve_model_batched(900.0)                              # no flux was ever set: NULL, and THL mixes
    first = ens._diffuse_prof
    before = ens.p["THL"].copy()
    ens.set_forcings_batched(WT_surf=numpy.array([0.1, 0.2]))
    ens.evolve_model_batched(1800.0)
    assert ens._diffuse_prof is first and (ens.p["THL"][:, 0] > before[:, 0]).all()      # same dt, grid and density: nothing uploaded again
    ens.evolve_model_batched(2000.0)                             # another dt
    second = ens._diffuse_prof
    assert second is not first
    ens.p["Rhobf"] = ens.p["Rhobf"] * 1.5
    ens.evolve_model_batched(2200.0)
    assert ens._diffuse_prof is not second
    third = ens._diffuse_prof
    ens.zh_cache = numpy.asarray(ens.zh_cache) * 2.0
    ens.evolve_model_batched(2400.0)
    assert ens._diffuse_prof is not third
    ens.enable_diffusion()
    assert ens._diffuse_prof is None and ens.diffuse_par["k_bg"] == 0.1
    old = models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, engine=ldr.lmr.MicroOracleEngine())
    old.set_fields_batched("QT", numpy.zeros((2, 2, 2, 6)))
    with pytest.raises(ValueError, match="les_diffuse"):
        old.enable_diffusion()


def test_the_column_tile_cases_on_the_oracle_backed_engine(lib):
    """the plumbing of the coltile body runs without a GPU; the columns per workgroup are the library's"""
    eng = ldr.DiffuseOracleEngine()
    eng.diffuse_cols_per_block = lambda ktot: lib.spc_les_diffuse_cols_per_block(ktot, numpy.dtype(ldr.np_of(eng)).itemsize)
    ldr.check_coltile(eng)


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("micro", [False, True])
@pytest.mark.parametrize("thermo", [False, True])
def test_float32_ensemble_on_one_engine_equals_the_host_twin(thermo, micro):
    """test_ensemble_on_one_engine_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    calls = []
    ldr.check_ensemble(f32_of(ldr.DiffuseOracleEngine)(), [_counted(f32_of(ldr.DiffuseOracleEngine)(), calls)], 4, thermo, micro=micro)
    assert calls == [(["QT", "THL", "U", "V"], 4, ["QT", "THL"])] * 3                     # one launch per step


@pytest.mark.parametrize("thermo", [False, True])
def test_float32_ensemble_as_row_blocks_with_an_empty_device(thermo):
    """test_ensemble_as_row_blocks_with_an_empty_device on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(f32_of(ldr.DiffuseOracleEngine)(), calls) for _ in range(3)], min_cols_per_device=1)
    ldr.check_ensemble(f32_of(ldr.DiffuseOracleEngine)(), [multi], 2, thermo, micro=thermo)
    assert calls == [(["QT", "THL", "U", "V"], 1, ["QT", "THL"])] * 6                     # blocks 1 + 1 + 0: the device without rows launches nothing


@pytest.mark.parametrize("thermo", [False, True])
def test_float32_fused_step_then_diffusion(monkeypatch, thermo):
    """test_fused_step_then_diffusion on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    steps = []
    eng = f32_of(ldr.DiffuseOracleEngine)()
    inner = eng.les_advance
    eng.les_advance = lambda *a, **kw: (steps.append(kw.get("sat")), inner(*a, **kw))[1]
    ldr.check_ensemble(f32_of(ldr.DiffuseOracleEngine)(), [eng], 3, thermo)
    assert steps == [None if thermo else "QT"] * 3
