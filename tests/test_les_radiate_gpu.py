"""K18 on the MI355X: Engine.les_radiate against the NumPy oracle of tests/les_radiate_ref.py, bit for bit
(gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero), in float64 and float32, every array the
leading part of a poisoned buffer whose other bytes are checked afterwards, the read-only inputs compared with what was
uploaded; models.DeviceLESEnsemble's enable_radiation() against its host twins.  The bodies live in tests/les_radiate_ref.py:
tools/mutation_control.py --radiate runs them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_radiate_ref as lrr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", lrr.DTYPES)
@pytest.mark.parametrize("ktot", lrr.KTOTS)
@pytest.mark.parametrize("plane", lrr.PLANES)
def test_radiation_equals_the_oracle(plane, ktot, dtype):
    lrr.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", lrr.DTYPES)
@pytest.mark.parametrize("ktot", [1, 2, 65, 160])
def test_profiles_and_flux_scales_that_differ_per_les(ktot, dtype):
    """n = 1, 2, 5: another w, c, f0 and f1 per LES, with and without a pitch between the rows of w and c"""
    lrr.check_rows(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", lrr.DTYPES)
def test_every_boundary_of_the_tiles(dtype):
    """C - 1, C, C + 1 and 2 C + 1 columns for every C of spc_les_radiate_cols_per_block, ktot on both sides of every change of
    it, 17 columns at the last supported ktot, and the first unsupported ktot refused"""
    first, changes, bad = lrr.check_tiles(Engine("cuda:0", dtype=dtype))
    wide = dtype == torch.float64
    assert (first, changes, bad) == ({64: 1, 32: 63 if wide else 127, 16: 127 if wide else 255}, [63, 127] if wide else [127, 255], 639 if wide else 1279)


@pytest.mark.parametrize("dtype", lrr.DTYPES)
def test_the_column_tile_cases(dtype):
    """tiles that span three and five LES, ktot 1 ... 17 and at every change of C, every lead off the 16-byte grid"""
    lrr.check_coltile(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lrr.DTYPES)
def test_with_and_without_flux_and_fsfc(dtype):
    lrr.check_outputs(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lrr.DTYPES)
@pytest.mark.parametrize("leads,ktot,pad", [((1, 1, 1), 65, 0), ((3, 3, 3), 64, 0), ((1, 1, 1), 160, 2), ((2, 2, 2), 7, 0), ((1, 0, 0), 65, 0), ((0, 1, 3), 160, 5)])
def test_views_off_the_16_byte_grid(leads, ktot, pad, dtype):
    """ql, thl and flux equally off the grid (the 16-byte mover with a head and a tail) and each differently (single elements)"""
    lrr.check_alignment(Engine("cuda:0", dtype=dtype), leads, ktot, pad)


@pytest.mark.parametrize("dtype", lrr.DTYPES)
def test_clear_sky_cloud_placements_and_their_signs(dtype):
    lrr.check_clouds(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lrr.DTYPES)
def test_table_nodes_and_the_clamp(dtype):
    lrr.check_lookup(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lrr.DTYPES)
def test_special_values(dtype):
    """a negative ql; NaN, +-inf and -0.0 in one ql cell and in one thl cell each; every other column keeps the bits of the run
    without them"""
    lrr.check_special(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lrr.DTYPES)
def test_refusals(dtype):
    """n = 0; n_tab < 2, inv_step not positive, pitch_prof < ktot, a NULL input, thl, flux or fsfc equal to an input or to each
    other: through the C ABI and through the engine"""
    lrr.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert lrr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(lrr.VARIANTS))
@pytest.mark.parametrize("n", [4, 130])
def test_ensemble_equals_the_host_twin(monkeypatch, n, variant):
    """three steps and one constantT nudge before the last, on one engine and on two engines sharing the card, plain, with
    diffusion and with diffusion + thermo + microphysics + vertical advection: every profile, every field and the flux bit-equal
    to the host twin after each of them; ONE K18 launch per device and step (asserted); THL at the cloud top differs from the
    run without enable_radiation() (asserted on the twin's logs), whose device run is bit-equal to its own twin"""
    launches = []
    inner = Engine.les_radiate
    monkeypatch.setattr(Engine, "les_radiate", lambda self, ql, *a, **kw: (launches.append((id(self), int(ql.shape[0]))), inner(self, ql, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    lrr.check_ensemble(Engine("cuda:0"), [one, multi], n, variant)
    for eng, rows in [(one, n)] + [(e, n // 2) for e in multi.engines]:
        assert [r for i, r in launches if i == id(eng)] == [rows] * 3          # three steps: three launches


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(lrr.VARIANTS))
@pytest.mark.parametrize("n", [4, 130])
def test_float32_ensemble_equals_the_host_twin(monkeypatch, n, variant):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    launches = []
    inner = Engine.les_radiate
    monkeypatch.setattr(Engine, "les_radiate", lambda self, ql, *a, **kw: (launches.append((id(self), int(ql.shape[0]))), inner(self, ql, *a, **kw))[1])
    one = Engine("cuda:0", dtype=torch.float32)
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=torch.float32, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    lrr.check_ensemble(Engine("cuda:0", dtype=torch.float32), [one, multi], n, variant)
    for eng, rows in [(one, n)] + [(e, n // 2) for e in multi.engines]:
        assert [r for i, r in launches if i == id(eng)] == [rows] * 3          # three steps: three launches
