"""K17 without a GPU: the struct layout of spc_les_vadvect_args, the host-side refusals of spc_les_vadvect_*,
advection.vertical_profiles and vertical_wind, properties of the NumPy oracle of tests/les_vadvect_ref.py (a constant keeps its
bits, winds uniform per level are the identity, the local maximum principle, the plane sum of the mass flux through the lid,
the closed ground and the zero-gradient lid), and models.DeviceLESEnsemble's enable_advection(vertical=True) on an
oracle-backed engine against its host twins."""
import ctypes
import os
import subprocess

import numpy
import pytest
import torch

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import advection as adv
from tests import les_vadvect_ref as lvr
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {numpy.float64: 2.0 ** -52, numpy.float32: 2.0 ** -23}
SHAPES = [(1, 1, 1), (2, 3, 5), (8, 8, 160), (9, 9, 161)]          # itot x jtot x ktot
#: planes with a divergence: on 1 x 1 and 2 x 2 both faces of a cell along an axis are one face (ce == cw, cn == cs bit for bit),
#: so d = +0 whatever the winds are -- those planes are cases of the identity test below
DIVERGENT = [(1, 5, 3), (2, 3, 5), (3, 5, 64), (8, 8, 160), (9, 9, 161)]


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


def test_struct_layout_of_the_vertical_advection_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror"""
    cls, cname = _abi.LesVadvectArgs, "spc_les_vadvect_args"
    fields = ["n_les", "itot", "jtot", "ktot", "n_fields", "u", "v", "fields", "out", "hx", "hy", "cmax", "g", "r", "pitch_prof", "mtop"]
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%%zu\\n", sizeof(%s));' % cname, 'printf("%d\\n", SPC_VADVECT_MAX_FIELDS);']
    want = [ctypes.sizeof(cls), _abi.SPC_VADVECT_MAX_FIELDS]
    for f in fields:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
        want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and _abi.SPC_VADVECT_MAX_FIELDS == 6
    # K16's members come first, in K16's order
    assert fields[:12] == [f[0] for f in _abi.LesAdvectArgs._fields_]


PTRS = ("u", "v", "hx", "hy", "cmax", "g", "r", "mtop")


def _args(n=4, itot=8, jtot=8, ktot=20, n_fields=4, pitch_prof=None, fields=None, out=None, **ptrs):
    a = _abi.LesVadvectArgs()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields = n, itot, jtot, ktot, n_fields
    a.pitch_prof = ktot if pitch_prof is None else pitch_prof
    for i, k in enumerate(PTRS):                                  # distinct, 16-byte aligned, never dereferenced
        setattr(a, k, ptrs.get(k, 4096 * (i + 1)))
    for f in range(6):
        a.fields[f] = (fields or {}).get(f, 4096 * (f + 10))
        a.out[f] = (out or {}).get(f, 4096 * (f + 20))
    return a


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch: none of these calls needs a device"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_vadvect_" + sfx)

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
    for k in ("u", "v", "hx", "hy", "g", "r"):
        assert call(**{k: None}) == (E, b"required pointer %s is NULL" % k.encode())
    assert call(fields={1: None})[0] == E and b"fields" in lib.spc_last_error()
    assert call(out={3: None})[0] == E and b"out" in lib.spc_last_error()
    assert call(n=-1)[0] == E
    for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
        rc, text = call(**bad)
        assert rc == E and b">= 1" in text
    for nf in (7, -1):
        rc, text = call(n_fields=nf)
        assert rc == E and b"field count" in text
    rc, text = call(n_fields=0, cmax=None, mtop=None)
    assert rc == E and b"nothing to do" in text
    rc, text = call(pitch_prof=19)
    assert rc == E and b"pitch_prof" in text
    rc, text = call(out={3: 4096 * 20})
    assert rc == E and b"same array" in text
    inputs = [4096 * (1 + PTRS.index(k)) for k in ("u", "v", "hx", "hy", "g", "r")] + [4096 * 10, 4096 * 13]
    for ptr in inputs:
        for kw in (dict(out={2: ptr}), dict(mtop=ptr), dict(cmax=ptr)):
            rc, text = call(**kw)
            assert rc == E and b"also an input" in text, kw
    for kw in (dict(mtop=4096 * 21), dict(cmax=4096 * 22), dict(cmax=4096 * 8), dict(out={0: 4096 * 5}), dict(out={5: 4096 * 8}, n_fields=6)):
        rc, text = call(**kw)
        assert rc == E and b"same array" in text, kw
    rc, text = call(fields={0: 4100 if sfx == "f64" else 4098})
    assert rc == E and b"not aligned" in text
    rc, text = call(n=1 << 40, ktot=3)
    assert rc == U and b"too many workgroups" in text
    assert call(fields={0: 4096, 1: 2 * 4096}, n=1 << 40, ktot=3)[0] == U      # (a field may be u or v: accepted up to the grid)
    rc, text = call(ktot=2560 if sfx == "f32" else 1280, pitch_prof=4000)
    assert rc == U and b"levels" in text
    a = _args(n=0, fields={f: None for f in range(6)}, out={f: None for f in range(6)}, **{k: None for k in PTRS})
    assert fn(ctypes.byref(a), None) == 0                         # an empty ensemble is a no-op


def test_columns_per_block(lib):
    """K15's budget rule: the largest of 64, 32, 16 columns of ktot | 1 elements within 64 KiB, 16 may take 160 KiB"""
    f = lib.spc_les_vadvect_cols_per_block
    for esize in (4, 8):
        for ktot in (1, 2, 63, 64, 65, 127, 128, 129, 160, 255, 256, 257, 511, 512, 513, 1279, 1280, 2559, 2560, 5000):
            col = (ktot | 1) * esize
            want = 0 if ktot > 163840 // 16 // esize else 64 if 64 * col <= 65536 else 32 if 32 * col <= 65536 else 16 if 16 * col <= 163840 else 0
            assert f(ktot, esize) == want == lib.spc_les_diffuse_cols_per_block(ktot, esize), (ktot, esize)
    assert f(0, 8) == 0 and f(160, 2) == 0 and (f(160, 8), f(160, 4), f(1279, 8), f(1280, 8), f(2559, 4), f(2560, 4)) == (32, 64, 16, 0, 16, 0)


# -- advection.py -----------------------------------------------------------------------------------------------------------------
def test_vertical_profiles_and_their_refusals():
    w = numpy.array([[24.0, 20.0, 0.5], [3.0, 7.0, 1e-3]])
    g, r = adv.vertical_profiles(w)
    assert g.dtype == r.dtype == numpy.float64 and g.shape == r.shape == (2, 3) and g is not w
    assert_bits("g", g, w)
    assert_bits("r", r, 1.0 / w)
    for bad in (0.0, -1.0, numpy.nan, numpy.inf, -numpy.inf):
        x = w.copy()
        x[1, 2] = bad
        with pytest.raises(ValueError, match="positive and finite"):
            adv.vertical_profiles(x)


def test_vertical_wind():
    rho = torch.tensor([[1.2, 1.0, 0.8], [1.0, 1.0, 0.5]], dtype=torch.float64)
    m = torch.ones(2, 1, 2, 3, dtype=torch.float64) * torch.tensor([1.1, -0.9, 0.8], dtype=torch.float64)
    w = adv.vertical_wind(m, rho, 10.0)
    assert tuple(w.shape) == (2, 1, 2, 3)
    want = numpy.array([[1.1 / 11.0, -0.9 / 9.0, 0.8 / 8.0], [1.1 / 10.0, -0.9 / 7.5, 0.8 / 5.0]])
    assert numpy.allclose(w[:, 0, 0, :].numpy(), want, rtol=1e-15, atol=0) and numpy.array_equal(w[:, 0, 0], w[:, 0, 1])


# -- the oracle ------------------------------------------------------------------------------------------------------------
def shaped(shape, dtype, n=2, seed=0, names=("THL", "QT")):
    itot, jtot, ktot = shape
    return lvr.case((n, itot, jtot, ktot), dtype, seed=seed, names=names)


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_keeps_a_constant(shape, dtype):
    """x[km] - x and x[kp] - x are +0 of a constant finite field, whatever the winds: every bit is kept"""
    c = shaped(shape, dtype)
    const = {"a": numpy.full_like(c["u"], 287.3), "b": numpy.full_like(c["u"], -1e-3)}
    kept, cmax, mtop = lvr.les_vadvect(const, c["u"], c["v"], c["hx"], c["hy"], c["g"], c["r"])
    assert_bits("a", kept["a"], const["a"])
    assert_bits("b", kept["b"], const["b"])
    assert cmax.dtype == dtype and mtop.dtype == dtype and not numpy.isnan(cmax).any() and (cmax >= 0).all()


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", SHAPES + [(2, 2, 7)])
def test_oracle_winds_uniform_per_level_are_the_identity(shape, dtype):
    """what set_les_state makes: d = +0, M = 0, cmax = +0, every finite field bit-identical; on 1 x 1 and 2 x 2 that holds for
    ANY winds (both faces of a cell along an axis are one face)"""
    c = shaped(shape, dtype, seed=1)
    if shape[:2] not in ((1, 1), (2, 2)):
        c["u"][...] = (3.0 + numpy.arange(shape[2]) % 5).astype(dtype)[None, None, None, :]
        c["v"][...] = (-2.0 + 0.37 * numpy.arange(shape[2])).astype(dtype)[None, None, None, :]
    new, cmax, mtop = lvr.oracle(c)
    assert not cmax.any() and not numpy.signbit(cmax).any() and not mtop.any() and not numpy.signbit(mtop).any()
    for k, x in c["fields"].items():
        assert_bits(k, new[k], x)


def bounded_case(shape, dtype, seed=0):
    """winds of unit amplitude rescaled to a vertical Courant sum of 0.5 (cmax is linear in the winds); the oracle's cmax of
    the rescaled winds is asserted within [0.25, 1]"""
    c = shaped(shape, dtype, seed=seed)
    unit = lvr.oracle(dict(c, fields={}))[1].max()
    assert unit > 0
    scale = dtype(0.5 / float(unit))
    c["u"], c["v"] = c["u"] * scale, c["v"] * scale
    cmax = lvr.oracle(dict(c, fields={}))[1]
    assert 0.25 <= cmax.max() <= 1.0, cmax
    return c


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", DIVERGENT)
def test_oracle_local_maximum_principle(shape, dtype):
    """s <= 1: x' is a convex combination of the cell and its two vertical neighbours, so it lies in their range within
    8 eps max|x| (two differences, two products and two additions, each rounded once)"""
    c = bounded_case(shape, dtype)
    new, cmax, _ = lvr.oracle(c)
    assert 0.25 <= cmax.max() <= 1.0
    for k, x in c["fields"].items():
        xm = numpy.concatenate([x[..., :1], x[..., :-1]], axis=3)
        xp = numpy.concatenate([x[..., 1:], x[..., -1:]], axis=3)
        nb = numpy.stack([x, xm, xp])
        e = 8 * EPS[dtype] * numpy.abs(x).max()
        assert (new[k] >= nb.min(axis=0) - e).all() and (new[k] <= nb.max(axis=0) + e).all() and new[k].dtype == dtype
        assert (new[k] != x).any()


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_plane_sum_of_the_mass_through_the_lid(shape, dtype):
    """ce of a cell is cw of its neighbour bit for bit, so the plane sum of M[ktot] is rounding alone: within
    (ktot + 4) eps sum g (|cw| + |ce| + |cs| + |cn|), the sums over the LES and in float64"""
    c = shaped(shape, dtype, seed=2)
    cw, ce, cs, cn = lvr.courant_faces(c["u"], c["v"], c["hx"], c["hy"])
    assert_bits("ce is cw of the eastern neighbour", ce, numpy.roll(cw, -1, axis=1))
    assert_bits("cn is cs of the northern neighbour", cn, numpy.roll(cs, -1, axis=2))
    M = lvr.mass_flux(c["u"], c["v"], c["hx"], c["hy"], c["g"])
    lid = M[..., -1].astype(numpy.float64).sum(axis=(1, 2))
    mag = (c["g"].astype(numpy.float64)[:, None, None, :] * sum(numpy.abs(a.astype(numpy.float64)) for a in (cw, ce, cs, cn))).sum(axis=(1, 2, 3))
    bound = (shape[2] + 4) * EPS[dtype] * mag
    print("lid %s %s: worst residual %.3g of the bound" % (shape, numpy.dtype(dtype).name, (numpy.abs(lid) / numpy.maximum(bound, 1e-300)).max()))
    assert (numpy.abs(lid) <= bound).all()


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_closed_ground_and_zero_gradient_lid(dtype):
    """level 0 never takes anything from below (M[0] = +0: pb = +0 there); the top cell takes nothing from above except itself
    (x[kp] is x: the pt term is +0), so both are indifferent to what a wrong neighbour would hold"""
    c = shaped((3, 5, 9), dtype, seed=3)
    M = lvr.mass_flux(c["u"], c["v"], c["hx"], c["hy"], c["g"])
    pb, pt, s = lvr.face_numbers(M, c["r"])
    assert not pb[..., 0].any() and not M[..., 0].any() and (pt[..., -1] > 0).any() and (pb[..., -1] > 0).any()
    new = lvr.oracle(c)[0]
    for k, x in c["fields"].items():
        top, below = x[..., -1], x[..., -2]
        with numpy.errstate(all="ignore"):
            want = top + pb[..., -1] * (below - top)
        assert_bits("top " + k, new[k][..., -1], want + dtype(0))
        x0, x1 = x[..., 0], x[..., 1]
        assert_bits("ground " + k, new[k][..., 0], (x0 + dtype(0)) + pt[..., 0] * (x1 - x0))
    one = lvr.case((1, 3, 5, 1), dtype, seed=3, names=("THL",))         # ktot == 1: the cell is both of its neighbours
    assert_bits("one level", lvr.oracle(one)[0]["THL"], one["fields"]["THL"])


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_special_values(dtype):
    c, s, mask = lvr.special_case(dtype)
    clean, got = lvr.oracle(c)[0], lvr.oracle(s)[0]
    assert_bits("THL", got["THL"][~mask], clean["THL"][~mask])
    assert_bits("QT", got["QT"], clean["QT"])
    assert numpy.isnan(got["THL"][0, 0, 0, 1]) and numpy.isfinite(lvr.oracle(s)[1]).all()


def test_engines_have_the_method():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    assert callable(Engine.les_vadvect) and callable(MultiDeviceEngine.les_vadvect) and callable(Engine.vadvect_cols_per_block)
    assert not hasattr(lvr.lar.AdvectOracleEngine, "les_vadvect")


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def _counted(engine, calls):
    for name in ("les_advect", "les_vadvect"):
        inner = getattr(engine, name)
        setattr(engine, name, lambda fields, *a, _n=name, _f=inner, **kw: (calls.append((_n, sorted(fields), int(a[1].shape[0]))), _f(fields, *a, **kw))[1])
    return engine


def _step_calls(keys, rows, n_sub):
    return [("les_advect", [], rows), ("les_vadvect", [], rows)] + [("les_advect", keys, rows), ("les_vadvect", keys, rows)] * n_sub


@pytest.mark.parametrize("thermo,micro,diffuse", [(False, False, False), (False, False, True), (True, True, True)])
def test_ensemble_on_one_engine_equals_the_host_twin(thermo, micro, diffuse):
    calls = []
    n_sub = lvr.check_ensemble(lvr.VadvectOracleEngine(), [_counted(lvr.VadvectOracleEngine(), calls)], 4, thermo, micro=micro, diffuse=diffuse)
    keys = sorted(["QT", "THL", "U", "V"] + (["QR"] if micro else []))
    assert n_sub in (2, 3) and calls[:2 + 2 * n_sub] == _step_calls(keys, 4, n_sub)      # the probes, then K16 and K17 per substep
    vertical = calls[:[i for i, c in enumerate(calls) if c[0] == "les_vadvect"][-1] + 1]   # (the runs with vertical=False follow)
    assert len([c for c in vertical if c[0] == "les_vadvect" and not c[1]]) == 3 and all(c[0] == "les_advect" for c in calls[len(vertical):])
    assert len([c for c in vertical if c[0] == "les_advect"]) == len([c for c in vertical if c[0] == "les_vadvect"])


@pytest.mark.parametrize("thermo", [False, True])
def test_ensemble_as_row_blocks_with_an_empty_device(thermo):
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(lvr.VadvectOracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    n_sub = lvr.check_ensemble(lvr.VadvectOracleEngine(), [multi], 2, thermo, micro=thermo, diffuse=True)
    assert all(c[2] == 1 for c in calls) and len([c for c in calls if c[0] == "les_vadvect" and not c[1]]) == 6   # blocks 1 + 1 + 0
    assert n_sub in (2, 3)


def _small(eng, n=2, nL=6):
    spcpl.set_engine(eng)
    gcm, src = models.make_batched_models(n, nL=nL)
    return models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, itot=2, jtot=3, engine=eng)


def test_vertical_is_opt_in_and_the_profiles_are_uploaded_once():
    eng = lvr.VadvectOracleEngine()
    ens = _small(eng)
    rng = numpy.random.default_rng(1)
    ens.attach_fields({k: rng.standard_normal((2, 2, 3, 6)) + m for k, m in (("U", 5.0), ("V", -2.0), ("THL", 290.0), ("QT", 5.0))})
    ens.enable_advection(dx=50000.0, dy=50000.0)
    assert ens.advection and not ens.advect_vertical and ens.get_vertical_wind_batched() is None
    ens.evolve_model_batched(100.0)
    assert ens.advect_courant_z is None and ens._vadvect_prof is None and ens.get_vertical_wind_batched() is None
    ens.enable_advection(dx=50000.0, dy=50000.0, vertical=True)
    assert ens.advect_vertical and ens.get_vertical_wind_batched() is None
    ens.evolve_model_batched(200.0)
    first = ens._vadvect_prof
    g, r = first[1]
    assert_bits("g", g.numpy(), ens.water_path_weights())
    assert_bits("r", r.numpy(), 1.0 / ens.water_path_weights())
    w = ens.get_vertical_wind_batched()
    assert tuple(w.shape) == (2, 2, 3, 6) and bool(torch.isfinite(w).all()) and bool((w != 0).any())
    assert ens.advect_substeps == 1 and 0 < ens.advect_courant_z < 0.5
    ens.evolve_model_batched(300.0)
    assert ens._vadvect_prof is first                             # the same weights: nothing uploaded again
    old = models.DeviceLESEnsemble(ens.grid_indices, ens.zf_cache, ens.zh_cache, ens.p, itot=2, jtot=3, engine=lvr.lar.AdvectOracleEngine())
    old.attach_fields({"U": numpy.zeros((2, 2, 3, 6)), "V": numpy.zeros((2, 2, 3, 6))})
    old.enable_advection()
    with pytest.raises(ValueError, match="les_vadvect"):
        old.enable_advection(vertical=True)


def test_a_mass_flux_that_is_not_finite_raises():
    """the vertical Courant sum of the substeps is recorded, and refused only where it is not finite"""
    eng = lvr.VadvectOracleEngine()
    ens = _small(eng)
    rng = numpy.random.default_rng(1)
    ens.attach_fields({k: rng.standard_normal((2, 2, 3, 6)) + m for k, m in (("U", 5.0), ("V", -2.0), ("THL", 290.0))})
    ens.enable_advection(dx=50000.0, dy=50000.0, vertical=True)
    inner = eng.les_vadvect

    def grown(fields, *a, **kw):
        res = inner(fields, *a, **kw)
        return res.fill_(float("inf")) if fields else res            # the probe passes; the substep's sum is not finite
    eng.les_vadvect = grown
    with pytest.raises(RuntimeError, match="K17"):
        ens.evolve_model_batched(100.0)
    assert ens.advect_courant_z == float("inf")


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("thermo,micro,diffuse", [(False, False, False), (False, False, True), (True, True, True)])
def test_float32_ensemble_on_one_engine_equals_the_host_twin(thermo, micro, diffuse):
    """test_ensemble_on_one_engine_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    calls = []
    n_sub = lvr.check_ensemble(f32_of(lvr.VadvectOracleEngine)(), [_counted(f32_of(lvr.VadvectOracleEngine)(), calls)], 4, thermo, micro=micro, diffuse=diffuse)
    keys = sorted(["QT", "THL", "U", "V"] + (["QR"] if micro else []))
    assert n_sub in (2, 3) and calls[:2 + 2 * n_sub] == _step_calls(keys, 4, n_sub)      # the probes, then K16 and K17 per substep
    vertical = calls[:[i for i, c in enumerate(calls) if c[0] == "les_vadvect"][-1] + 1]   # (the runs with vertical=False follow)
    assert len([c for c in vertical if c[0] == "les_vadvect" and not c[1]]) == 3 and all(c[0] == "les_advect" for c in calls[len(vertical):])
    assert len([c for c in vertical if c[0] == "les_advect"]) == len([c for c in vertical if c[0] == "les_vadvect"])


@pytest.mark.parametrize("thermo", [False, True])
def test_float32_ensemble_as_row_blocks_with_an_empty_device(thermo):
    """test_ensemble_as_row_blocks_with_an_empty_device on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(f32_of(lvr.VadvectOracleEngine)(), calls) for _ in range(3)], min_cols_per_device=1)
    n_sub = lvr.check_ensemble(f32_of(lvr.VadvectOracleEngine)(), [multi], 2, thermo, micro=thermo, diffuse=True)
    assert all(c[2] == 1 for c in calls) and len([c for c in calls if c[0] == "les_vadvect" and not c[1]]) == 6   # blocks 1 + 1 + 0
    assert n_sub in (2, 3)
