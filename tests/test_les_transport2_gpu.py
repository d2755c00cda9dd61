"""K23 on the MI355X: Engine.les_transport2 against the NumPy oracle of tests/les_transport2_ref.py, bit for bit
(gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero), in float64 and float32, with both limiters,
every array the leading part of a buffer poisoned with NaN whose other bytes are checked afterwards, the inputs compared with
what was uploaded; DeviceLESEnsemble's enable_advection(vertical=True, conservative=True, order=2) against its host twins.  The
bodies live in tests/les_transport2_ref.py: tools/mutation_control.py --transport2 runs them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_transport2_ref as lt2

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", lt2.DTYPES)
@pytest.mark.parametrize("ktot", lt2.KTOTS)
@pytest.mark.parametrize("plane", lt2.PLANES)
def test_transport2_equals_the_oracle(plane, ktot, dtype):
    """n = 3 at the extents where the distance-2 neighbours fold onto each other or the boundary slopes meet, both limiters"""
    lt2.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", lt2.DTYPES)
def test_cmax_and_mtop_are_those_of_the_first_order_kernel(dtype):
    """from a full launch and from the probe (n_fields == 0), against a K22 launch on the same arrays and against the oracle"""
    lt2.check_outputs(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lt2.DTYPES)
@pytest.mark.parametrize("ktot", [1, 65, 160])
def test_coefficients_and_profiles_that_differ_per_les(ktot, dtype):
    """n = 1, 2, 5: another dx, dy, g and r per LES, with and without a pitch"""
    lt2.check_rows(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", lt2.DTYPES)
def test_every_boundary_of_the_tiles(dtype):
    """C - 1, C, C + 1 and 2 C + 1 columns for every C of spc_les_transport2_cols_per_block, ktot on both sides of every change of
    it, 17 columns at the last supported ktot, and the first unsupported ktot refused; the edges are derived from the LDS budget
    and compared with the query"""
    first, changes, bad = lt2.check_tiles(Engine("cuda:0", dtype=dtype))
    wide = dtype == torch.float64
    assert (first, changes, bad) == ({64: 1, 32: 128 if wide else 256, 16: 256 if wide else 512}, [128, 256] if wide else [256, 512], 1280 if wide else 2560)


@pytest.mark.parametrize("dtype", lt2.DTYPES)
def test_zero_to_six_fields_with_and_without_cmax_mtop_and_ftop(dtype):
    lt2.check_fields(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lt2.DTYPES)
@pytest.mark.parametrize("lead,ktot", [(1, 65), (3, 64), (1, 160), (2, 7)])
def test_views_off_the_16_byte_grid(lead, ktot, dtype):
    lt2.check_alignment(Engine("cuda:0", dtype=dtype), lead, ktot)


@pytest.mark.parametrize("dtype", lt2.DTYPES)
def test_winds_of_either_sign_and_zero_winds(dtype):
    lt2.check_signs(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lt2.DTYPES)
def test_a_constant_field_equals_the_oracle(dtype):
    """(how far a constant moves is bounded in tests/test_les_transport2_cpu.py)"""
    lt2.check_constant(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lt2.DTYPES)
def test_special_values(dtype):
    """NaN, +-inf and -0.0 planted in single field cells reach what the oracle says, at most two cells along each axis"""
    lt2.check_special(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lt2.DTYPES)
def test_refusals(dtype):
    """K22's refusals and the limiter that is neither, through the C ABI and through the engine"""
    lt2.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert lt2.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "buoyancy", "all"])
@pytest.mark.parametrize("n", [4, 130])
def test_ensemble_equals_the_host_twin(monkeypatch, n, variant):
    """three steps and one constantT nudge before the last, on one engine and on two engines sharing the card, plain, with the
    pressure force, and with diffusion + radiation + thermo + microphysics: every profile, field and lid flux bit-equal to the
    host twin after each of them, W within a few roundings; per step and device ONE K22 probe, then per substep K21 where
    enabled and ONE K23 -- no K16, no K17 and no K22 field launch; the run with order=1 is bit-equal to today's conservative
    run"""
    launches = []
    for name in ("les_advect", "les_vadvect", "les_transport", "les_transport2"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, fields, out, u, *a, _n=name, _f=inner, **kw: (
            launches.append((id(self), _n, int(u.shape[0]), len(fields))), _f(self, fields, out, u, *a, **kw))[1])
    inner_b = Engine.les_buoyancy
    monkeypatch.setattr(Engine, "les_buoyancy", lambda self, thl, *a, **kw: (
        launches.append((id(self), "les_buoyancy", int(thl.shape[0]), -1)), inner_b(self, thl, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    subs = lt2.check_ensemble(Engine("cuda:0"), [one, multi], n, variant)
    assert len(subs) == 3 and all(s >= 1 for s in subs)
    kw = lt2.VARIANTS[variant]
    nf = 5 if kw.get("micro") else 4
    for eng, rows in [(one, n)] + [(e, n // 2) for e in multi.engines]:
        mine = [(k, r, f) for i, k, r, f in launches if i == id(eng)]
        assert all(r == rows for _, r, _ in mine)
        want = []
        for n_sub in subs:                                            # the probe, then (K21 and) K23 per substep
            want += [("les_transport", rows, 0)] + (([("les_buoyancy", rows, -1)] if kw.get("buoyancy") else []) + [("les_transport2", rows, nf)]) * n_sub
        assert mine[:len(want)] == want                               # the second-order run came first
        if eng is one:                                                # then the runs with order=1 and without the arguments: K22's
            rest = mine[len(want):]
            assert rest and all(m[0] in ("les_transport", "les_buoyancy") for m in rest) and any(m[0] == "les_transport" and m[2] for m in rest)
        else:
            assert len(mine) == len(want)


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "buoyancy", "all"])
@pytest.mark.parametrize("n", [4, 130])
def test_float32_ensemble_equals_the_host_twin(monkeypatch, n, variant):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    launches = []
    for name in ("les_advect", "les_vadvect", "les_transport", "les_transport2"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, fields, out, u, *a, _n=name, _f=inner, **kw: (
            launches.append((id(self), _n, int(u.shape[0]), len(fields))), _f(self, fields, out, u, *a, **kw))[1])
    inner_b = Engine.les_buoyancy
    monkeypatch.setattr(Engine, "les_buoyancy", lambda self, thl, *a, **kw: (
        launches.append((id(self), "les_buoyancy", int(thl.shape[0]), -1)), inner_b(self, thl, *a, **kw))[1])
    one = Engine("cuda:0", dtype=torch.float32)
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=torch.float32, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    subs = lt2.check_ensemble(Engine("cuda:0", dtype=torch.float32), [one, multi], n, variant)
    assert len(subs) == 3 and all(s >= 1 for s in subs)
    kw = lt2.VARIANTS[variant]
    nf = 5 if kw.get("micro") else 4
    for eng, rows in [(one, n)] + [(e, n // 2) for e in multi.engines]:
        mine = [(k, r, f) for i, k, r, f in launches if i == id(eng)]
        assert all(r == rows for _, r, _ in mine)
        want = []
        for n_sub in subs:                                            # the probe, then (K21 and) K23 per substep
            want += [("les_transport", rows, 0)] + (([("les_buoyancy", rows, -1)] if kw.get("buoyancy") else []) + [("les_transport2", rows, nf)]) * n_sub
        assert mine[:len(want)] == want                               # the second-order run came first
        if eng is one:                                                # then the runs with order=1 and without the arguments: K22's
            rest = mine[len(want):]
            assert rest and all(m[0] in ("les_transport", "les_buoyancy") for m in rest) and any(m[0] == "les_transport" and m[2] for m in rest)
        else:
            assert len(mine) == len(want)
