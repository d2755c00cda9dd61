"""K16 without a GPU: the struct layout of spc_les_advect_args, the host-side refusals of spc_les_advect_*, advection.coefficients
and the substep rule, properties of the NumPy oracle of tests/les_advect_ref.py (a constant keeps its bits, the local maximum
principle, conservation under winds uniform per level, the reach of a special value), and models.DeviceLESEnsemble's advection
mode on an oracle-backed engine against its host twins."""
import ctypes
import os
import subprocess

import numpy
import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd import advection as adv
from tests import les_advect_ref as lar
from tests.gpu_util import assert_bits
from tests.les_harness import f32_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {numpy.float64: 2.0 ** -52, numpy.float32: 2.0 ** -23}
PLANES = [(1, 1), (1, 5), (2, 2), (3, 5), (9, 8), (64, 64)]


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


def test_struct_layout_of_the_advection_arguments(tmp_path):
    """sizeof / offsetof as gcc sees include/spc.h == the ctypes mirror"""
    cls, cname = _abi.LesAdvectArgs, "spc_les_advect_args"
    fields = ["n_les", "itot", "jtot", "ktot", "n_fields", "u", "v", "fields", "out", "hx", "hy", "cmax"]
    assert [f[0] for f in cls._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%%zu\\n", sizeof(%s));' % cname, 'printf("%d\\n", SPC_ABI_VERSION);', 'printf("%d\\n", SPC_ADVECT_MAX_FIELDS);']
    want = [ctypes.sizeof(cls), 4, _abi.SPC_ADVECT_MAX_FIELDS]
    for f in fields:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
        want.append(getattr(cls, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and _abi.ABI_VERSION == 4 and _abi.SPC_ADVECT_MAX_FIELDS == 6


def _args(n=4, itot=8, jtot=8, ktot=20, n_fields=4, fields=None, out=None, **ptrs):
    g = _abi.LesAdvectArgs()
    g.n_les, g.itot, g.jtot, g.ktot, g.n_fields = n, itot, jtot, ktot, n_fields
    for i, k in enumerate(("u", "v", "hx", "hy", "cmax")):        # distinct, 16-byte aligned, never dereferenced
        setattr(g, k, ptrs.get(k, 4096 * (i + 1)))
    for f in range(6):
        g.fields[f] = (fields or {}).get(f, 4096 * (f + 10))
        g.out[f] = (out or {}).get(f, 4096 * (f + 20))
    return g


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_advection_entry_points_validate_on_the_host(lib, sfx):
    """every refusal is made before any launch: none of these calls needs a device"""
    E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
    fn = getattr(lib, "spc_les_advect_" + sfx)

    def call(**kw):
        return fn(ctypes.byref(_args(**kw)), None), lib.spc_last_error()
    assert fn(None, None) == E and b"NULL" in lib.spc_last_error()
    for k in ("u", "v", "hx", "hy"):
        assert call(**{k: None}) == (E, b"required pointer %s is NULL" % k.encode())
    assert call(fields={1: None})[0] == E and b"fields" in lib.spc_last_error()
    assert call(out={3: None})[0] == E and b"out" in lib.spc_last_error()
    assert call(out={5: None}, fields={4: None}, n=1 << 40, ktot=3)[0] == U      # (beyond n_fields: not looked at; accepted up to the grid)
    assert call(n=-1)[0] == E
    for bad in (dict(itot=0), dict(jtot=-3), dict(ktot=0)):
        rc, text = call(**bad)
        assert rc == E and b">= 1" in text
    for nf in (7, -1):
        rc, text = call(n_fields=nf)
        assert rc == E and b"field count" in text
    rc, text = call(n_fields=0, cmax=None)
    assert rc == E and b"nothing to do" in text
    rc, text = call(out={3: 4096 * 20})
    assert rc == E and b"same array" in text
    for ptr in (4096, 2 * 4096, 3 * 4096, 4 * 4096, 5 * 4096, 4096 * 10, 4096 * 13):      # u, v, hx, hy, cmax, fields[0], fields[3]
        rc, text = call(out={2: ptr})
        assert rc == E and b"also an input" in text, ptr
    for k in ("u", "v", "hx", "hy"):
        rc, text = call(cmax=4096 * (1 + ("u", "v", "hx", "hy").index(k)))
        assert rc == E and b"cmax is also an input" in text
    rc, text = call(cmax=4096 * 11)
    assert rc == E and b"cmax is also an input" in text
    rc, text = call(fields={0: 4100 if sfx == "f64" else 4098})
    assert rc == E and b"not aligned" in text
    assert call(fields={0: 4096, 1: 2 * 4096}, n=1 << 40, ktot=3)[0] == U      # (a field may be u or v: accepted up to the grid)
    rc, text = call(n=1 << 40, ktot=3)
    assert rc == U and b"too many workgroups" in text
    g = _args(n=0, u=None, v=None, hx=None, hy=None, cmax=None, fields={f: None for f in range(6)}, out={f: None for f in range(6)})
    assert fn(ctypes.byref(g), None) == 0                         # an empty ensemble is a no-op


def test_strip_and_rows(lib):
    """256 cells of the run of a row; 32 rows where that still leaves 1 024 workgroups, else 8"""
    f, r = lib.spc_les_advect_strip, lib.spc_les_advect_rows
    assert f(64, 160, 8) == f(1, 1, 4) == 256
    assert f(0, 160, 8) == 0 and f(64, 0, 8) == 0 and f(64, 160, 2) == 0 and f(64, 160, 16) == 0
    want = lambda n, i, j, k: 32 if -(-j * k // 256) * -(-i // 32) * n >= 1024 else 8              # noqa: E731
    for n, i, j, k in [(2, 64, 64, 160), (12, 64, 64, 160), (13, 64, 64, 160), (256, 64, 64, 160), (1023, 31, 1, 1), (1024, 32, 1, 1),
                       (512, 33, 1, 1), (511, 33, 256, 1), (4, 8, 257, 128), (0, 8, 8, 8), (1 << 40, 4, 5, 20)]:
        assert r(n, i, j, k) == want(n, i, j, k), (n, i, j, k)
    assert r(13, 64, 64, 160) == 32 and r(12, 64, 64, 160) == 8 and r(130, 4, 5, 20) == 8
    assert r(-1, 8, 8, 8) == 0 and r(2, 0, 8, 8) == 0 and r(2, 8, 0, 8) == 0 and r(2, 8, 8, 0) == 0
    shapes = lar.strip_shapes(256, 8, 32)
    assert {j * k for n, _, j, k in shapes if n == 2} >= {255, 256, 257, 511, 512, 513}
    assert {i for n, i, _, _ in shapes if n == 2} >= {7, 8, 9, 15, 16, 17} and {i for n, i, _, _ in shapes if n != 2} >= {31, 32, 33, 63, 64, 65}
    assert all(r(n, i, j, k) == (8 if n == 2 else 32) for n, i, j, k in shapes)


# -- advection.py -----------------------------------------------------------------------------------------------------------------
def test_coefficients_and_the_substep_rule():
    assert (adv.DX, adv.DY, adv.CFL, adv.MAX_SUBSTEPS) == (200.0, 200.0, 0.5, 256)
    hx, hy = adv.coefficients(900.0, n=3)
    assert hx.dtype == hy.dtype == numpy.float64 and hx.tolist() == [2.25] * 3 and hy.tolist() == [2.25] * 3
    hx, hy = adv.coefficients(60.0, [100.0, 300.0], 50.0)
    assert hx.tolist() == [0.5 * 60.0 / 100.0, 0.5 * 60.0 / 300.0] and hy.tolist() == [0.6, 0.6] and hx.flags.c_contiguous
    for bad in (0.0, -1.0, numpy.nan, numpy.inf):
        with pytest.raises(ValueError):
            adv.coefficients(60.0, bad)
    with pytest.raises(ValueError):
        adv.coefficients(60.0, [100.0, 200.0], n=3)
    assert adv.substeps(0.0) == 1 and adv.substeps(0.5) == 1 and adv.substeps(numpy.nextafter(0.5, 1.0)) == 2
    assert adv.substeps(1.0) == 2 and adv.substeps(1.01) == 3 and adv.substeps(128.0) == 256 and adv.substeps(0.3, cfl=0.1) == 3
    for bad in (numpy.nan, numpy.inf, 128.5, 1e9):
        with pytest.raises(RuntimeError, match="c = "):
            adv.substeps(bad)
    with pytest.raises(RuntimeError, match="c = 0.7"):
        adv.substeps(0.7, max_substeps=1)


# -- properties of the oracle -----------------------------------------------------------------------------------------------------
def bounded_case(plane, dtype, seed=0, uniform=False):
    """a case whose Courant sums stay below 1 (asserted); ``uniform``: winds that depend on (l, k) only"""
    c = lar.case((2,) + plane + (7,), dtype, seed=seed, dt=2.0, names=("THL", "QT"))
    if uniform:
        c["u"][...] = c["u"][:, :1, :1, :]
        c["v"][...] = c["v"][:, :1, :1, :]
    s = lar.faces(c["u"], c["v"], c["hx"], c["hy"])[4]
    assert 0 < s.max() <= 1.0, s.max()
    return c


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
@pytest.mark.parametrize("plane", PLANES)
def test_oracle_keeps_a_constant_and_the_local_maximum_principle(plane, dtype):
    """s <= 1: x' is a convex combination of the cell and its four neighbours, so it lies in their range within
    8 eps max|x| (four products and four additions, each rounded once); a constant field keeps every bit"""
    c = bounded_case(plane, dtype)
    new, cmax = lar.les_advect(c["fields"], c["u"], c["v"], c["hx"], c["hy"])
    for k, x in c["fields"].items():
        nb = numpy.stack([x, numpy.roll(x, 1, 1), numpy.roll(x, -1, 1), numpy.roll(x, 1, 2), numpy.roll(x, -1, 2)])
        e = 8 * EPS[dtype] * numpy.abs(x).max()
        assert (new[k] >= nb.min(axis=0) - e).all() and (new[k] <= nb.max(axis=0) + e).all() and new[k].dtype == dtype
        if plane != (1, 1):
            assert (new[k] != x).any()
    const = {"a": numpy.full_like(c["u"], 287.3), "b": numpy.full_like(c["u"], -1e-3), "z": numpy.full_like(c["u"], -0.0)}
    kept = lar.les_advect(const, c["u"], c["v"], c["hx"], c["hy"])[0]
    assert_bits("a", kept["a"], const["a"])
    assert_bits("b", kept["b"], const["b"])
    assert not kept["z"].any() and not numpy.signbit(kept["z"]).any()          # -0.0 + pw * 0 is +0.0
    assert cmax.dtype == dtype and (cmax > 0).all() and not numpy.isnan(cmax).any()


@pytest.mark.parametrize("plane", PLANES)
def test_oracle_conserves_the_plane_sum_under_uniform_winds(plane):
    """winds uniform on each level: sum_ij x is kept within itot jtot eps sum_ij |x| in float64"""
    c = bounded_case(plane, numpy.float64, seed=1, uniform=True)
    new = lar.les_advect(c["fields"], c["u"], c["v"], c["hx"], c["hy"])[0]
    for k, x in c["fields"].items():
        res = numpy.abs(new[k].sum(axis=(1, 2)) - x.sum(axis=(1, 2)))
        bound = plane[0] * plane[1] * EPS[numpy.float64] * numpy.abs(x).sum(axis=(1, 2))
        print("conservation %s %s: worst residual %.3f of the bound" % (plane, k, (res / bound).max()))
        assert (res <= bound).all()


def test_oracle_faces_are_shared_and_signs_flip_the_upwind_side():
    """ce of a cell is cw of its eastern neighbour bit for bit; a positive u takes from the west, a negative one from the east"""
    c = lar.case((2, 5, 4, 3), numpy.float32, seed=2)
    pw, pe, ps, pn, s = lar.faces(c["u"], c["v"], c["hx"], c["hy"])
    assert ((pw == 0) | (numpy.roll(pe, 1, axis=1) == 0)).all() and ((ps == 0) | (numpy.roll(pn, 1, axis=2) == 0)).all()
    assert (s >= 0).all() and (pw > 0).any() and (pe > 0).any() and (ps > 0).any() and (pn > 0).any()
    x = numpy.zeros((1, 4, 1, 1))
    x[0, 1] = 1.0
    one, h = numpy.ones_like(x), numpy.array([0.125])
    east = lar.les_advect({"x": x}, one, 0 * one, h, h)[0]["x"].ravel()
    west = lar.les_advect({"x": x}, -one, 0 * one, h, h)[0]["x"].ravel()
    assert east.tolist() == [0.0, 0.75, 0.25, 0.0] and west.tolist() == [0.25, 0.75, 0.0, 0.0]
    y = x.reshape(1, 1, 4, 1)
    north = lar.les_advect({"x": y}, 0 * y, numpy.ones_like(y), h, 2 * h)[0]["x"].ravel()
    assert north.tolist() == [0.0, 0.5, 0.5, 0.0]


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.float32])
def test_oracle_special_values_reach_one_step(dtype):
    c, s, mask = lar.special_case(dtype)
    clean, got = lar.oracle(c)[0], lar.oracle(s)[0]
    for k in ("THL", "QT"):
        assert_bits(k, got[k][~mask], clean[k][~mask])
    assert numpy.isnan(got["THL"][0, 0, 0, 1]) and numpy.isnan(got["THL"][0, 1, 0, 1]) + numpy.isnan(got["THL"][0, 8, 0, 1]) >= 1
    assert not numpy.isnan(got["QT"]).any() and not numpy.array_equal(got["QT"][mask], clean["QT"][mask])
    assert numpy.isfinite(lar.oracle(s)[1]).all()


def test_engines_have_the_method():
    from sp_coupler_amd.engine import Engine
    from sp_coupler_amd.multi import MultiDeviceEngine
    assert callable(Engine.les_advect) and callable(MultiDeviceEngine.les_advect) and callable(Engine.advect_strip)
    assert not hasattr(lar.ldr.DiffuseOracleEngine, "les_advect")


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def _counted(engine, calls):
    inner = engine.les_advect
    engine.les_advect = lambda fields, *a, **kw: (calls.append((sorted(fields), int(a[1].shape[0]))), inner(fields, *a, **kw))[1]
    return engine


@pytest.mark.parametrize("thermo,micro,diffuse", [(False, False, False), (False, False, True), (True, False, False), (True, True, True),
                                                  (False, True, True)])
def test_ensemble_on_one_engine_equals_the_host_twin(thermo, micro, diffuse):
    calls = []
    n_sub = lar.check_ensemble(lar.AdvectOracleEngine(), [_counted(lar.AdvectOracleEngine(), calls)], 4, thermo, micro=micro, diffuse=diffuse)
    keys = ["QT", "THL", "U", "V"] + (["QR"] if micro else [])
    probes = [c for c in calls if not c[0]]
    assert n_sub in (2, 3) and len(probes) == 3 and all(c == (sorted(keys), 4) for c in calls if c[0])
    assert calls[:1 + n_sub] == [([], 4)] + [(sorted(keys), 4)] * n_sub               # one probe, then the substeps


def test_ensemble_with_one_substep():
    calls = []
    assert lar.check_ensemble(lar.AdvectOracleEngine(), [_counted(lar.AdvectOracleEngine(), calls)], 3, False, dx=lar.DX_ONE) == 1
    assert calls == [([], 3), (["QT", "THL", "U", "V"], 3)] * 3


@pytest.mark.parametrize("thermo", [False, True])
def test_ensemble_as_row_blocks_with_an_empty_device(thermo):
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(lar.AdvectOracleEngine(), calls) for _ in range(3)], min_cols_per_device=1)
    n_sub = lar.check_ensemble(lar.AdvectOracleEngine(), [multi], 2, thermo, micro=thermo, diffuse=True)
    assert all(c[1] == 1 for c in calls) and len([c for c in calls if not c[0]]) == 6      # blocks 1 + 1 + 0: two probes per step
    assert n_sub in (2, 3)


def test_fused_step_then_advection(monkeypatch):
    """K11 steps the fields (FUSED_MIN_LES patched to 0), K16 follows: the same bits as the twin"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    steps = []
    eng = lar.AdvectOracleEngine()
    inner = eng.les_advance
    eng.les_advance = lambda *a, **kw: (steps.append(kw.get("sat")), inner(*a, **kw))[1]
    lar.check_ensemble(lar.AdvectOracleEngine(), [eng], 3, False)
    assert steps == ["QT"] * 3


def test_without_the_call_every_path_keeps_its_bits():
    """enable_advection() is opt-in: an ensemble that never calls it evolves as the twin of the parent's path"""
    calls = []
    host = lar.ldr.ensemble_run(lar.ldr.DiffuseOracleEngine(), 3, False, False)[1]
    ens, dev = lar.ldr.ensemble_run(_counted(lar.AdvectOracleEngine(), calls), 3, False, True)
    lar.lmr.same_logs(host, dev)
    assert not ens.advection and ens._advect_coef is None and calls == [] and ens.advect_substeps is None


def _small(eng, n=2, nL=6):
    spcpl.set_engine(eng)
    gcm, src = models.make_batched_models(n, nL=nL)
    ens = models.DeviceLESEnsemble(src.grid_indices, src.zf_cache, src.zh_cache, src.p, itot=2, jtot=3, engine=eng)
    return ens


def test_enable_advection_refusals_the_grid_getters_and_the_uploads():
    eng = lar.AdvectOracleEngine()
    ens = _small(eng)
    assert (ens[0].dx, ens[1].get_dy(), ens[0].get_xsize(), ens[0].get_ysize()) == (200.0, 200.0, 400.0, 600.0)
    ens.set_fields_batched("U", numpy.full((2, 2, 3, 6), 4.0))
    with pytest.raises(ValueError, match="U and V"):
        ens.enable_advection()
    ens.set_fields_batched("V", numpy.full((2, 2, 3, 6), -1.0))
    ens.set_fields_batched("THL", 290.0 + numpy.random.default_rng(0).random((2, 2, 3, 6)))
    for bad in (dict(dx=0.0), dict(dy=-5.0), dict(dx=[1.0, 2.0, 3.0]), dict(cfl=0.0), dict(max_substeps=0)):
        with pytest.raises(ValueError):
            ens.enable_advection(**bad)
    assert not ens.advection
    ens.enable_advection(dx=[4000.0, 8000.0], dy=5000.0)
    assert ens.advection and ens.advect_par == {"cfl": 0.5, "max_substeps": 256}
    assert (ens[0].get_dx(), ens[1].get_dx(), ens[1].dy, ens[1].get_xsize(), ens[0].get_ysize()) == (4000.0, 8000.0, 5000.0, 16000.0, 15000.0)
    ens.evolve_model_batched(100.0)                               # c = 8 * 50 / 4000 + 2 * 50 / 5000 = 0.12
    assert ens.advect_substeps == 1 and ens.advect_courant == 8 * (0.5 * 100.0 / 4000.0) + 2 * (0.5 * 100.0 / 5000.0)
    first = ens._advect_coef
    coefs = dict(first[1])
    ens.evolve_model_batched(200.0)
    assert ens._advect_coef is first and first[1] == coefs and sorted(first[1]) == [1]      # same dt, n_sub, dx, dy: nothing uploaded again
    ens.evolve_model_batched(1200.0)                              # dt = 1000: c = 1.2 -> 3 substeps
    assert ens.advect_substeps == 3 and ens._advect_coef is not first and sorted(ens._advect_coef[1]) == [1, 3]
    assert abs(ens.advect_courant - 0.4) < 1e-12
    second = ens._advect_coef
    ens.dx = 2000.0
    ens.evolve_model_batched(2200.0)
    assert ens._advect_coef is not second and ens.advect_substeps == 5
    old = models.DeviceLESEnsemble(ens.grid_indices, ens.zf_cache, ens.zh_cache, ens.p, engine=lar.ldr.DiffuseOracleEngine())
    old.set_fields_batched("U", numpy.zeros((2, 2, 2, 6)))
    old.set_fields_batched("V", numpy.zeros((2, 2, 2, 6)))
    with pytest.raises(ValueError, match="les_advect"):
        old.enable_advection()


def test_a_refused_step_leaves_the_fields_untouched():
    """n_sub above max_substeps, and a wind that is not finite: RuntimeError naming c, every field bit-equal, the time not advanced"""
    eng = lar.AdvectOracleEngine()
    ens = _small(eng)
    rng = numpy.random.default_rng(1)
    start = {k: rng.standard_normal((2, 2, 3, 6)) + m for k, m in (("U", 5.0), ("V", -2.0), ("THL", 290.0), ("QT", 5.0))}
    ens.attach_fields({k: v.copy() for k, v in start.items()})
    ens.enable_advection(max_substeps=4)
    with pytest.raises(RuntimeError, match=r"c = \d"):
        ens.evolve_model_batched(900.0)                           # c of about 0.5 * 900 / 200 * 14: hundreds of substeps
    assert ens.model_time == 0.0
    for k, v in start.items():
        assert_bits(k, ens.get_fields_batched(k).numpy(), v)
    assert_bits("p THL", ens.p["THL"], lar.slab_ref.slab_means(start["THL"]))
    ens.enable_advection(dx=50000.0, dy=50000.0)
    bad = start["U"].copy()
    bad[1, 0, 2, 3] = numpy.inf
    ens.set_fields_batched("U", bad)
    with pytest.raises(RuntimeError, match="c = inf"):
        ens.evolve_model_batched(900.0)
    assert_bits("U", ens.get_fields_batched("U").numpy(), bad)
    assert_bits("THL", ens.get_fields_batched("THL").numpy(), start["THL"])
    bad[1, 0, 2, 3] = numpy.nan                                   # a NaN wind closes its faces: the step goes through
    ens.set_fields_batched("U", bad)
    ens.evolve_model_batched(900.0)
    assert ens.model_time == 900.0 and ens.advect_substeps == 1


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("thermo,micro,diffuse", [(False, False, False), (False, False, True), (True, False, False), (True, True, True),
                                                  (False, True, True)])
def test_float32_ensemble_on_one_engine_equals_the_host_twin(thermo, micro, diffuse):
    """test_ensemble_on_one_engine_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    calls = []
    n_sub = lar.check_ensemble(f32_of(lar.AdvectOracleEngine)(), [_counted(f32_of(lar.AdvectOracleEngine)(), calls)], 4, thermo, micro=micro, diffuse=diffuse)
    keys = ["QT", "THL", "U", "V"] + (["QR"] if micro else [])
    probes = [c for c in calls if not c[0]]
    assert n_sub in (2, 3) and len(probes) == 3 and all(c == (sorted(keys), 4) for c in calls if c[0])
    assert calls[:1 + n_sub] == [([], 4)] + [(sorted(keys), 4)] * n_sub               # one probe, then the substeps


def test_float32_ensemble_with_one_substep():
    """test_ensemble_with_one_substep on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    calls = []
    assert lar.check_ensemble(f32_of(lar.AdvectOracleEngine)(), [_counted(f32_of(lar.AdvectOracleEngine)(), calls)], 3, False, dx=lar.DX_ONE) == 1
    assert calls == [([], 3), (["QT", "THL", "U", "V"], 3)] * 3


@pytest.mark.parametrize("thermo", [False, True])
def test_float32_ensemble_as_row_blocks_with_an_empty_device(thermo):
    """test_ensemble_as_row_blocks_with_an_empty_device on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    from sp_coupler_amd.multi import MultiDeviceEngine
    calls = []
    multi = MultiDeviceEngine([_counted(f32_of(lar.AdvectOracleEngine)(), calls) for _ in range(3)], min_cols_per_device=1)
    n_sub = lar.check_ensemble(f32_of(lar.AdvectOracleEngine)(), [multi], 2, thermo, micro=thermo, diffuse=True)
    assert all(c[1] == 1 for c in calls) and len([c for c in calls if not c[0]]) == 6      # blocks 1 + 1 + 0: two probes per step
    assert n_sub in (2, 3)


def test_float32_fused_step_then_advection(monkeypatch):
    """test_fused_step_then_advection on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    steps = []
    eng = f32_of(lar.AdvectOracleEngine)()
    inner = eng.les_advance
    eng.les_advance = lambda *a, **kw: (steps.append(kw.get("sat")), inner(*a, **kw))[1]
    lar.check_ensemble(f32_of(lar.AdvectOracleEngine)(), [eng], 3, False)
    assert steps == ["QT"] * 3
