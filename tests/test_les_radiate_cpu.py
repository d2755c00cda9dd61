"""K18 without a GPU: the struct layout of spc_les_radiate_args, the host-side refusals of spc_les_radiate_*, radiation.py (the
table, its accuracy, the profiles and their refusals), properties of the NumPy oracle of tests/les_radiate_ref.py (a clear
column keeps its bits, the cloud top cools, the cloud base warms, the flux divergence telescopes, a NaN stays in its column),
and models.DeviceLESEnsemble's enable_radiation() on an oracle-backed engine against its host twins."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy
import pytest
import torch

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import radiation as rad
from tests import les_radiate_ref as lrr
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {numpy.float64: 2.0 ** -52, numpy.float32: 2.0 ** -23}
SHAPES = [p + (k,) for p in lrr.PLANES for k in lrr.KTOTS]         # itot x jtot x ktot


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


def test_struct_layout_of_the_radiation_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror"""
    cls, cname = _abi.LesRadiateArgs, "spc_les_radiate_args"
    fields = ["n_les", "itot", "jtot", "ktot", "n_tab", "ql", "thl", "w", "c", "pitch_prof", "f0", "f1", "etab", "inv_step", "flux", "fsfc"]
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


def _args(n=4, itot=8, jtot=8, ktot=20, n_tab=2049, inv_step=64.0, pitch_prof=None, **ptrs):
    a = _abi.LesRadiateArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_tab, a.inv_step = n, itot, jtot, ktot, n_tab, inv_step
    a.pitch_prof = ktot if pitch_prof is None else pitch_prof
    for i, k in enumerate(lrr.PTRS):                              # distinct, 16-byte aligned, never dereferenced
        setattr(a, k, ptrs.get(k, 4096 * (i + 1)))
    return a


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch: none of these calls needs a device"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_radiate_" + sfx)

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
    for k in ("ql", "thl", "w", "c", "f0", "f1", "etab"):
        assert call(**{k: None}) == (E, b"required pointer %s is NULL" % k.encode())
    assert call(n=-1)[0] == E
    for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
        rc, text = call(**bad)
        assert rc == E and b">= 1" in text
    for bad in (1, 0, -5):
        rc, text = call(n_tab=bad)
        assert rc == E and b"n_tab" in text
    for bad in (0.0, -64.0, float("nan")):
        rc, text = call(inv_step=bad)
        assert rc == E and b"inv_step" in text
    rc, text = call(pitch_prof=19)
    assert rc == E and b"pitch_prof" in text
    inputs = [4096 * (1 + lrr.PTRS.index(k)) for k in ("ql", "w", "c", "f0", "f1", "etab")]
    for ptr in inputs:
        for out in ("thl", "flux", "fsfc"):
            rc, text = call(**{out: ptr})
            assert rc == E and b"also an input" in text and out.encode() in text, (out, ptr)
    thl, flux = 4096 * (1 + lrr.PTRS.index("thl")), 4096 * (1 + lrr.PTRS.index("flux"))
    for kw in (dict(flux=thl), dict(fsfc=thl), dict(fsfc=flux)):
        rc, text = call(**kw)
        assert rc == E and b"same array" in text, kw
    rc, text = call(thl=4100 if sfx == "f64" else 4098)
    assert rc == E and b"not aligned" in text
    rc, text = call(n=1 << 40, ktot=3)
    assert rc == U and b"too many workgroups" in text
    last = 638 if sfx == "f64" else 1278
    rc, text = call(ktot=last + 1, pitch_prof=4000)
    assert rc == U and b"levels" in text and str(last).encode() in text
    assert call(ktot=1, n=1 << 40)[0] == U                        # (one level is allowed up to the grid)
    assert fn(ctypes.byref(_args(n=0, **{k: None for k in lrr.PTRS})), None) == 0       # an empty ensemble is a no-op
    assert lib.spc_abi_version() == 4


def test_columns_per_block(lib):
    """K15's budget rule on TWO tiles of (ktot + 1) | 1 elements per column: the largest of 64, 32, 16 columns within 64 KiB,
    16 may take 160 KiB"""
    f = lib.spc_les_radiate_cols_per_block
    for esize in (4, 8):
        for ktot in (1, 2, 61, 62, 63, 125, 126, 127, 160, 253, 254, 255, 637, 638, 639, 640, 1277, 1278, 1279, 5000):
            col = 2 * ((ktot + 1) | 1) * esize
            want = 64 if 64 * col <= 65536 else 32 if 32 * col <= 65536 else 16 if 16 * col <= 163840 else 0
            assert f(ktot, esize) == want, (ktot, esize)
    assert f(0, 8) == 0 and f(160, 2) == 0 and (f(160, 8), f(160, 4), f(638, 8), f(639, 8), f(1278, 4), f(1279, 4)) == (16, 32, 16, 0, 16, 0)


# -- radiation.py ------------------------------------------------------------------------------------------------------------------
def test_constants_and_table():
    assert (rad.F0, rad.F1, rad.KAPPA, rad.STEP, rad.INV_STEP, rad.N_TAB) == (70.0, 22.0, 85.0, 1.0 / 64, 64.0, 2049)
    for dtype in (numpy.float64, numpy.float32, torch.float64, torch.float32):
        t = rad.exp_table(dtype)
        assert t.shape == (2049,) and t.dtype == numpy.dtype(numpy.float32 if dtype in (numpy.float32, torch.float32) else numpy.float64)
        assert t[0] == 1.0 and (numpy.diff(t.astype(numpy.float64)) < 0).all() and t[-1] > 0
    assert_bits("f32 is f64 rounded once", rad.exp_table(numpy.float32), numpy.exp(-numpy.arange(2049) / 64.0).astype(numpy.float32))
    assert rad.x_hi(numpy.float64) == 32.0 and rad.x_hi(numpy.float32) == numpy.float32(32.0)


def test_table_accuracy():
    """|E(x) - exp(-x)| <= STEP ** 2 / 8 + 4 eps on [0, x_hi] in float64: linear interpolation of a function with |f''| <= 1"""
    etab = rad.exp_table(numpy.float64)
    rng = numpy.random.default_rng(0)
    x = numpy.concatenate([numpy.linspace(0.0, 32.0, 400001), rng.random(200000) * 32.0, rng.random(100000) * 0.1,
                           (numpy.arange(2048) + 0.5) / 64.0, numpy.arange(2049) / 64.0])
    err = numpy.abs(lrr.lookup(x, etab) - numpy.exp(-x))
    bound = rad.STEP ** 2 / 8 + 4 * EPS[numpy.float64]
    print("table: largest |E(x) - exp(-x)| = %.6e at x = %.6f, bound %.6e" % (err.max(), x[err.argmax()], bound))
    assert err.max() <= bound and err.max() > 0.9 * rad.STEP ** 2 / 8          # (the bound is sharp at the first segment)
    assert_bits("nodes", lrr.lookup(numpy.arange(2049) / 64.0, etab), etab)
    assert_bits("clamp", lrr.lookup(numpy.array([-1.0, -numpy.inf, 32.5, 1e30, numpy.inf]), etab), etab[[0, 0, 2048, 2048, 2048]])
    assert numpy.isnan(lrr.lookup(numpy.array([numpy.nan]), etab)).all()


def test_profiles_and_their_refusals():
    rng = numpy.random.default_rng(1)
    rhobf, zh, zf, presf, kappa = lrr.grid(3, 6, rng)
    w, c = rad.profiles(rhobf, zh, presf, 60.0, kappa)
    assert w.dtype == c.dtype == numpy.float64 and w.shape == c.shape == (3, 6) and w.flags.c_contiguous and c.flags.c_contiguous
    dz = numpy.diff(zh, axis=1)
    dz = numpy.concatenate([dz, dz[:, -1:]], axis=1)
    assert numpy.allclose(w, kappa[:, None] * rhobf * dz, rtol=1e-15)
    assert numpy.allclose(c, 60.0 / (1004.0 * rhobf * dz * (presf / 1e5) ** (287.04 / 1004.0)), rtol=1e-14)
    assert_bits("a scalar kappa", rad.profiles(rhobf, zh, presf, 60.0)[0], rad.profiles(rhobf, zh, presf, 60.0, numpy.full(3, 85.0))[0])
    assert_bits("a shared grid", rad.profiles(rhobf, zh[0], presf, 60.0)[0][0], rad.profiles(rhobf, zh, presf, 60.0)[0][0])
    one = rad.profiles(rhobf[:, :1], zh[:, :1], presf[:, :1], 60.0, zf=zf[:, :1])[0]
    assert numpy.allclose(one, 85.0 * rhobf[:, :1] * 2 * (zf[:, :1] - zh[:, :1]))
    with pytest.raises(ValueError, match="zf"):
        rad.profiles(rhobf[:, :1], zh[:, :1], presf[:, :1], 60.0)
    for bad in (0.0, -1.0, numpy.nan, numpy.inf):
        x = rhobf.copy()
        x[1, 2] = bad
        with pytest.raises(ValueError, match="positive and finite"):
            rad.profiles(x, zh, presf, 60.0)
    for k, bad in ((3, zh[2, 2]), (3, zh[2, 1]), (2, numpy.nan), (5, numpy.inf)):       # a dz of zero, a negative one, not finite
        x = zh.copy()
        x[2, k] = bad
        with pytest.raises(ValueError, match="positive and finite"):
            rad.profiles(rhobf, x, presf, 60.0)
    for kw in (dict(presf=numpy.where(numpy.arange(6) == 2, numpy.nan, presf)), dict(dt=numpy.inf), dict(kappa=numpy.nan), dict(kappa=numpy.ones(2))):
        a = dict(presf=presf, dt=60.0, kappa=85.0)
        a.update(kw)
        with pytest.raises(ValueError):
            rad.profiles(rhobf, zh, a["presf"], a["dt"], a["kappa"])


# -- the oracle ------------------------------------------------------------------------------------------------------------
def shaped(shape, dtype, n=2, seed=0, kind="mixed"):
    itot, jtot, ktot = shape
    return lrr.case((n, itot, jtot, ktot), dtype, seed=seed, kind=kind)


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_clear_column_keeps_its_bits(shape, dtype):
    """all ql == +0: A = B = 0, E = 1, F = f0 + f1 at every face, F[k + 1] - F[k] = +0: every finite thl keeps its bits, -0.0
    included; in a mixed case the clear columns do"""
    c = shaped(shape, dtype, kind="clear")
    c["thl"][0, 0, 0, :] = -0.0
    c["thl"][1, -1, -1, ::2] = -1e-30
    thl, flux, fsfc = lrr.oracle(c)
    assert thl.dtype == flux.dtype == fsfc.dtype == dtype
    assert_bits("thl", thl, c["thl"])
    total = c["f0"] + c["f1"]
    assert_bits("flux", flux, numpy.broadcast_to(total[:, None, None, None], flux.shape))
    assert_bits("fsfc", fsfc, numpy.broadcast_to(total[:, None, None], fsfc.shape))
    c = shaped(shape, dtype, seed=1)
    clear = ~(c["ql"] > 0).any(axis=3)
    assert_bits("the clear columns", lrr.oracle(c)[0][clear], c["thl"][clear])


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_cloud_top_cools(shape, dtype):
    """with f0 > 0 (and f1 < f0) the topmost cloudy cell of every cloudy column cools"""
    for kind in ("mixed", "deck", "top", "bottom", "middle"):
        c = shaped(shape, dtype, seed=2, kind=kind)
        if kind == "mixed":
            c["ql"][0, 0, 0, shape[2] // 2] = 5e-4
        thl = lrr.oracle(c)[0]
        cloudy = (c["ql"] > 0).any(axis=3)
        top = (shape[2] - 1) - numpy.argmax(c["ql"][..., ::-1] > 0, axis=3)
        pick = lambda a: numpy.take_along_axis(a, top[..., None], axis=3)[..., 0][cloudy]      # noqa: E731
        assert cloudy.any() and (pick(thl) < pick(c["thl"])).all(), kind


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] > 1])
def test_oracle_cloud_base_warms(shape, dtype):
    """f1 > 0, f0 = 0, ql > 0 only in cells k >= k0 >= 1: the cells below k0 keep their bits, cell k0 warms, no cell cools"""
    for k0 in sorted({1, shape[2] // 3 or 1, shape[2] - 1}):
        c = shaped(shape, dtype, seed=3, kind="clear")
        c["ql"][..., k0:] = dtype(3e-4)
        c["f0"][:] = 0
        thl = lrr.oracle(c)[0]
        assert_bits("below the base", thl[..., :k0], c["thl"][..., :k0])
        assert (thl[..., k0] > c["thl"][..., k0]).all() and (thl >= c["thl"]).all(), k0


def telescoping_bound(thl_new, c, F):
    """thl' = (thl - t)(1 + d1), t = c dF (1 + d2), dF = (F[k + 1] - F[k])(1 + d3), |d| <= u = 2 ** -53, so
    |sum_k (thl' - thl) / c + (F[ktot] - F[0])| <= u sum_k (|thl'| / c + (2 + u) |F[k + 1] - F[k]|), as exact rationals"""
    u = Fraction(1, 2 ** 53)
    return u * sum(abs(Fraction(x)) / Fraction(ck) + (2 + u) * abs(Fraction(hi) - Fraction(lo))
                   for x, ck, lo, hi in zip(thl_new, c, F[:-1], F[1:]))


@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_telescoping(shape):
    """sum_k (thl'[k] - thl[k]) / c[k] = -(F[ktot] - F[0]) within the rounding bound of DESIGN.md 7.3, asserted as written on
    the float64 oracle in exact rational arithmetic, in every column of the smaller shapes and in 24 columns of the larger"""
    c = shaped(shape, numpy.float64, seed=4)
    c["ql"][0, 0, 0, shape[2] // 2:] = 5e-4
    thl, flux, fsfc = lrr.oracle(c)
    F = numpy.concatenate([fsfc[..., None], flux], axis=3)
    cols = [(l, i, j) for l in range(2) for i in range(shape[0]) for j in range(shape[1])]
    if len(cols) > 24:
        cols = cols[:1] + [cols[q] for q in numpy.random.default_rng(5).choice(len(cols), 23, replace=False)]
    worst = Fraction(0)
    for l, i, j in cols:
        lhs = sum((Fraction(a) - Fraction(b)) / Fraction(ck) for a, b, ck in zip(thl[l, i, j], c["thl"][l, i, j], c["c"][l]))
        resid = abs(lhs + (Fraction(F[l, i, j, -1]) - Fraction(F[l, i, j, 0])))
        bound = telescoping_bound(thl[l, i, j], c["c"][l], F[l, i, j])
        assert resid <= bound, (l, i, j, float(resid), float(bound))
        worst = max(worst, resid / bound)
    print("telescoping %s: worst residual %.3g of the bound" % (shape, float(worst)))
    assert (thl != c["thl"]).any()


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_special_values(dtype):
    """a NaN in ql makes every F and every thl' of its own column NaN; no other column changes a bit"""
    for ktot in (1, 2, 7, 161):
        c, s, cols = lrr.special_case(dtype, ktot)
        clean, got = lrr.oracle(c), lrr.oracle(s)
        others = numpy.ones(c["ql"].shape[:3], dtype=bool)
        for col in cols:
            others[col] = False
        for a, b in zip(got, clean):
            assert_bits("the other columns", a[others], b[others])
        assert numpy.isnan(got[0][0, 1, 2]).all() and numpy.isnan(got[1][0, 1, 2]).all() and numpy.isnan(got[2][0, 1, 2])
        assert numpy.isnan(got[0]).sum() == ktot + 1 and numpy.isfinite(got[1][others]).all()


def test_lookup_cases_are_what_they_claim():
    for dtype in (numpy.float64, numpy.float32):
        c = lrr.node_case(dtype)
        A, B = lrr.optical_depths(c["ql"], c["w"])
        assert ((A[1] * 64) % 1 == 0).all() and ((B[1] * 64) % 1 == 0).all() and A[0, 0, 1, 0] == dtype(32 - 2.0 ** -10) < rad.x_hi(dtype)
        assert A[0, 1, 0, 0] > 1e4 and A[0, 1, 1, 0] == 32
        F = lrr.fluxes(c["ql"], c["w"], c["f0"], c["f1"], c["etab"])
        assert F[0, 1, 0, 0] == c["f0"][0] * c["etab"][-1] + c["f1"][0]                  # the clamp: E = etab[n_tab - 1]
        c = lrr.coarse_case(dtype)
        e = lrr.lookup(numpy.array([8.0, 50.0, 7.5, 0.75], dtype=dtype), c["etab"], 0.5)
        assert e[0] == e[1] == 0 and e[0] != c["etab"][-1] and e[2] == dtype(0.25) and e[3] == dtype(1.0) + dtype(0.375) * (dtype(0.6) - dtype(1.0))


def test_engines_have_the_method():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    from tests import fake_engine
    assert callable(Engine.les_radiate) and callable(MultiDeviceEngine.les_radiate) and callable(Engine.radiate_cols_per_block)
    assert not hasattr(lrr.lvr.VadvectOracleEngine, "les_radiate") and not hasattr(fake_engine.OracleEngine, "les_radiate")


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def _counted(engine, calls):
    for name in ("les_radiate", "les_thermo", "les_microphysics", "les_diffuse", "les_vadvect"):
        inner = getattr(engine, name)
        setattr(engine, name, lambda *a, _n=name, _f=inner, **kw: (calls.append(_n), _f(*a, **kw))[1])
    return engine


STEP_CALLS = {"plain": ["les_radiate"], "diffuse": ["les_diffuse", "les_radiate"]}


@pytest.mark.parametrize("variant", list(lrr.VARIANTS))
def test_ensemble_on_one_engine_equals_the_host_twin(variant):
    """every profile, field and the flux bit-equal to the twin after each of three steps and the nudge; ONE K18 launch per
    step, after K16 / K17 / K15 and before K14; with thermo one K12 more per step than the run without enable_radiation()"""
    lrr.check_ensemble(lrr.RadiateOracleEngine(), [lrr.RadiateOracleEngine()], 4, variant)
    with_rad, without = [], []
    lrr.ensemble_run(_counted(lrr.RadiateOracleEngine(), with_rad), 4, True, **lrr.VARIANTS[variant])
    lrr.ensemble_run(_counted(lrr.RadiateOracleEngine(), without), 4, True, radiate=None, **lrr.VARIANTS[variant])
    assert with_rad.count("les_radiate") == 3 and "les_radiate" not in without
    if variant in STEP_CALLS:
        assert with_rad == STEP_CALLS[variant] * 3
    else:
        first = with_rad.index("les_diffuse")
        step = with_rad[first:with_rad.index("les_diffuse", first + 1)]
        assert [k for k in step if k != "les_vadvect"] == ["les_diffuse", "les_thermo", "les_radiate", "les_thermo", "les_microphysics", "les_thermo"]
        assert with_rad.count("les_thermo") - without.count("les_thermo") == 3


@pytest.mark.parametrize("variant", ["plain", "all"])
def test_ensemble_as_row_blocks_with_an_empty_device(variant):
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(lrr.RadiateOracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    lrr.check_ensemble(lrr.RadiateOracleEngine(), [multi], 2, variant)
    assert calls.count("les_radiate") == 6                         # blocks 1 + 1 + 0: two devices, three steps


def _small(eng, n=2, nL=6):
    spcpl.set_engine(eng)
    gcm, src = models.make_batched_models(n, nL=nL)
    return models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, itot=2, jtot=3, engine=eng)


def _fields(rng, names=("THL", "QT", "Qsat")):
    base = {"THL": 290.0, "QT": 9e-3, "Qsat": 8.7e-3, "U": 5.0}
    return {k: base[k] * (1.0 + 0.05 * rng.random((2, 2, 3, 6))) for k in names}


def test_enable_radiation_needs_thl_levels_and_cloud_water():
    eng = lrr.RadiateOracleEngine()
    rng = numpy.random.default_rng(1)
    ens = _small(eng)
    ens.attach_fields(_fields(rng, ("QT", "Qsat")))
    with pytest.raises(ValueError, match="THL"):
        ens.enable_radiation()
    ens = _small(eng)
    ens.attach_fields(_fields(rng, ("THL", "QT")))
    with pytest.raises(ValueError, match="Qsat"):
        ens.enable_radiation()
    ens.enable_thermo()
    ens.enable_radiation()
    one = _small(eng, nL=1)
    one.attach_fields({k: v[..., :1] for k, v in _fields(rng).items()})
    with pytest.raises(ValueError, match="one level"):
        one.enable_radiation()
    ens = _small(eng)
    ens.attach_fields(_fields(rng))
    for kw in (dict(f0=numpy.ones(3)), dict(f1=numpy.nan), dict(kappa=numpy.ones((2, 2)))):
        with pytest.raises(ValueError, match="scalar or one value per LES"):
            ens.enable_radiation(**kw)
    assert not ens.radiation and ens.get_radiative_flux_batched() is None
    old = models.DeviceLESEnsemble(ens.grid_indices, ens.zf_cache, ens.zh_cache, ens.p, itot=2, jtot=3, engine=lrr.lvr.VadvectOracleEngine())
    old.attach_fields(_fields(rng))
    with pytest.raises(ValueError, match="les_radiate"):
        old.enable_radiation()


def test_profiles_are_uploaded_again_only_where_their_inputs_changed():
    eng = lrr.RadiateOracleEngine()
    ens = _small(eng)
    ens.attach_fields(_fields(numpy.random.default_rng(2)))
    ens.enable_radiation(f0=[60.0, 80.0], kappa=90.0)
    assert ens.radiation and ens.get_radiative_flux_batched() is None
    t = float(ens.model_time)
    ens.evolve_model_batched(t + 100.0)
    first = ens._radiate_prof
    w, c = rad.profiles(ens.p["Rhobf"], ens.zh_cache, ens.p["presf"], 100.0, 90.0)
    assert_bits("w", first[1][0].numpy(), w)
    assert_bits("c", first[1][1].numpy(), c)
    assert_bits("f0", ens._radiate_scale[0].numpy(), numpy.array([60.0, 80.0]))
    flux = ens.get_radiative_flux_batched()
    assert tuple(flux.shape) == (2, 2, 3, 6) and bool((flux > 0).all()) and bool((flux < 60.0 + 80.0 + 22.0).all())
    ens.evolve_model_batched(t + 200.0)
    assert ens._radiate_prof is first and ens.get_radiative_flux_batched() is flux        # the same inputs: nothing uploaded again
    ens.evolve_model_batched(t + 250.0)
    assert ens._radiate_prof is not first                         # another dt
    second = ens._radiate_prof
    ens.p["presf"] = ens.p["presf"] * 1.001
    ens.evolve_model_batched(t + 300.0)
    assert ens._radiate_prof is not second
    third = ens._radiate_prof
    ens.p["Rhobf"] = ens.p["Rhobf"] * 1.01
    ens.evolve_model_batched(t + 350.0)
    assert ens._radiate_prof is not third


@pytest.mark.parametrize("variant", list(lrr.VARIANTS))
def test_without_enable_radiation_nothing_changes(variant):
    """enable_radiation never called: three steps bit-equal to the ensemble of the K17 tests' engine, which has no les_radiate
    at all, on the same inputs, and no K18 launch"""
    calls = []
    new = lrr.ensemble_run(_counted(lrr.RadiateOracleEngine(), calls), 4, True, radiate=None, **lrr.VARIANTS[variant])[1]
    old = lrr.ensemble_run(lrr.lvr.VadvectOracleEngine(), 4, True, radiate=None, **lrr.VARIANTS[variant])[1]
    lrr.lmr.same_logs(old, new)
    assert "les_radiate" not in calls


def test_the_column_tile_cases_on_the_oracle_backed_engine(lib):
    """the plumbing of the coltile body runs without a GPU; the columns per workgroup are the library's"""
    eng = lrr.RadiateOracleEngine()
    eng.radiate_cols_per_block = lambda ktot: lib.spc_les_radiate_cols_per_block(ktot, numpy.dtype(lrr.np_of(eng)).itemsize)
    lrr.check_coltile(eng)


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(lrr.VARIANTS))
def test_float32_ensemble_on_one_engine_equals_the_host_twin(variant):
    """test_ensemble_on_one_engine_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    lrr.check_ensemble(f32_of(lrr.RadiateOracleEngine)(), [f32_of(lrr.RadiateOracleEngine)()], 4, variant)
    with_rad, without = [], []
    lrr.ensemble_run(_counted(f32_of(lrr.RadiateOracleEngine)(), with_rad), 4, True, **lrr.VARIANTS[variant])
    lrr.ensemble_run(_counted(f32_of(lrr.RadiateOracleEngine)(), without), 4, True, radiate=None, **lrr.VARIANTS[variant])
    assert with_rad.count("les_radiate") == 3 and "les_radiate" not in without
    if variant in STEP_CALLS:
        assert with_rad == STEP_CALLS[variant] * 3
    else:
        first = with_rad.index("les_diffuse")
        step = with_rad[first:with_rad.index("les_diffuse", first + 1)]
        assert [k for k in step if k != "les_vadvect"] == ["les_diffuse", "les_thermo", "les_radiate", "les_thermo", "les_microphysics", "les_thermo"]
        assert with_rad.count("les_thermo") - without.count("les_thermo") == 3


@pytest.mark.parametrize("variant", ["plain", "all"])
def test_float32_ensemble_as_row_blocks_with_an_empty_device(variant):
    """test_ensemble_as_row_blocks_with_an_empty_device on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(f32_of(lrr.RadiateOracleEngine)(), calls) for _ in range(3)], min_cols_per_device=1)
    lrr.check_ensemble(f32_of(lrr.RadiateOracleEngine)(), [multi], 2, variant)
    assert calls.count("les_radiate") == 6                         # blocks 1 + 1 + 0: two devices, three steps
