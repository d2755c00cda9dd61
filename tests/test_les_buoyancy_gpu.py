"""K21 on the MI355X: Engine.les_buoyancy against the NumPy oracle of tests/les_buoyancy_ref.py, bit for bit
(gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero), in float64 and float32, every array the
leading part of a poisoned buffer whose other bytes are checked afterwards, the read-only inputs compared with what was
uploaded; models.DeviceLESEnsemble's enable_buoyancy() against its host twins.  The bodies live in tests/les_buoyancy_ref.py:
tools/mutation_control.py --buoyancy runs them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_buoyancy_ref as lbr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", lbr.DTYPES)
@pytest.mark.parametrize("ktot", lbr.KTOTS)
@pytest.mark.parametrize("plane", lbr.PLANES)
def test_pressure_force_equals_the_oracle(plane, ktot, dtype):
    """with ql, psfc and amax, and without all three"""
    lbr.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", lbr.DTYPES)
@pytest.mark.parametrize("ktot", [1, 2, 65, 160])
def test_profiles_and_coefficients_that_differ_per_les(ktot, dtype):
    """n = 1, 2, 5: another t0, lex, s, hx and hy per LES, with and without a pitch between the rows of the profiles"""
    lbr.check_rows(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", lbr.DTYPES)
def test_every_boundary_of_the_tiles(dtype):
    """C - 1, C, C + 1 and 2 C + 1 columns for every C of spc_les_buoyancy_cols_per_block, ktot on both sides of every change of
    it, 17 columns at the last supported ktot, and the first unsupported ktot refused through its return code; the thresholds
    are the ones 160 KiB of LDS and the pitch ktot | 1 give (derived in check_tiles, and stated here)"""
    first, changes, bad = lbr.check_tiles(Engine("cuda:0", dtype=dtype))
    wide = dtype == torch.float64
    assert (first, changes, bad) == ({64: 1, 32: 128 if wide else 256, 16: 256 if wide else 512}, [128, 256] if wide else [256, 512], 1280 if wide else 2560)


@pytest.mark.parametrize("dtype", lbr.DTYPES)
def test_the_column_tile_cases(dtype):
    """tiles that span three and five LES, ktot 1 ... 17 and at every change of C, every lead off the 16-byte grid"""
    lbr.check_coltile(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lbr.DTYPES)
def test_strip_seams_of_the_gradient_kernel(dtype):
    """jtot * ktot one below, at and one above a strip of k_les_pgrad, at itot = 1, 2, 3, 8, 9, 33"""
    strip, rows = lbr.check_strips(Engine("cuda:0", dtype=dtype))
    assert (strip, rows) == (256, 8)


@pytest.mark.parametrize("dtype", lbr.DTYPES)
def test_with_and_without_ql_psfc_and_amax(dtype):
    lbr.check_outputs(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lbr.DTYPES)
@pytest.mark.parametrize("leads,ktot,pad", [((1, 1, 1, 1), 65, 0), ((3, 3, 3, 3), 64, 0), ((1, 1, 1, 0), 160, 2), ((2, 2, 2, 1), 7, 0),
                                            ((1, 0, 0, 0), 65, 0), ((0, 1, 3, 2), 160, 5), ((0, 0, 1, 3), 63, 0)])
def test_views_off_the_16_byte_grid(leads, ktot, pad, dtype):
    """thl, qt and ql equally off the grid (the 16-byte mover with a head and a tail) and each differently (single elements); phi
    on a grid of its own"""
    lbr.check_alignment(Engine("cuda:0", dtype=dtype), leads, ktot, pad)


@pytest.mark.parametrize("dtype", lbr.DTYPES)
def test_special_values(dtype):
    """the uniform state keeps every wind's bits; a NaN in one thl cell reaches its own column from its level down, the winds of
    its neighbours there and amax of its LES, and nothing else"""
    lbr.check_special(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lbr.DTYPES)
def test_refusals(dtype):
    """n = 0; pitch_prof < ktot, a NULL required pointer, phi, u, v, psfc or amax equal to an input or to each other: through the C
    ABI and through the engine"""
    lbr.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert lbr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(lbr.VARIANTS))
@pytest.mark.parametrize("n", [4, 130])
def test_ensemble_equals_the_host_twin(monkeypatch, n, variant):
    """three steps and one constantT nudge before the last, on one engine and on two engines sharing the card, plain and with
    diffusion + radiation + thermo + microphysics: every profile, every field and phi bit-equal to the host twin after each of
    them; per step and device the two probes, then K21, K16, K17 per substep in that order (asserted); U differs from the run
    without enable_buoyancy() (asserted on the twin's logs), whose device run is bit-equal to today's twin"""
    launches = []
    for name in ("les_buoyancy", "les_advect", "les_vadvect"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, *a, _n=name, _f=inner, **kw: (launches.append((id(self), _n)), _f(self, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    subs = lbr.check_ensemble(Engine("cuda:0"), [one, multi], n, variant)
    want = []
    for n_sub in subs[:2] + subs[3:]:                                 # (the record after the nudge repeats the second step's)
        want += ["les_advect", "les_vadvect"] + ["les_buoyancy", "les_advect", "les_vadvect"] * n_sub
    for eng in multi.engines:
        assert [k for i, k in launches if i == id(eng)] == want
    mine = [k for i, k in launches if i == id(one)]                   # (then the run without enable_buoyancy(): on `one` only)
    assert mine[:len(want)] == want and len(mine) > len(want) and "les_buoyancy" not in mine[len(want):]


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(lbr.VARIANTS))
@pytest.mark.parametrize("n", [4, 130])
def test_float32_ensemble_equals_the_host_twin(monkeypatch, n, variant):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    launches = []
    for name in ("les_buoyancy", "les_advect", "les_vadvect"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, *a, _n=name, _f=inner, **kw: (launches.append((id(self), _n)), _f(self, *a, **kw))[1])
    one = Engine("cuda:0", dtype=torch.float32)
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=torch.float32, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    subs = lbr.check_ensemble(Engine("cuda:0", dtype=torch.float32), [one, multi], n, variant)
    want = []
    for n_sub in subs[:2] + subs[3:]:                                 # (the record after the nudge repeats the second step's)
        want += ["les_advect", "les_vadvect"] + ["les_buoyancy", "les_advect", "les_vadvect"] * n_sub
    for eng in multi.engines:
        assert [k for i, k in launches if i == id(eng)] == want
    mine = [k for i, k in launches if i == id(one)]                   # (then the run without enable_buoyancy(): on `one` only)
    assert mine[:len(want)] == want and len(mine) > len(want) and "les_buoyancy" not in mine[len(want):]
