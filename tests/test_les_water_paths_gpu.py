"""K13 on the MI355X: Engine.les_water_paths against the NumPy oracle of tests/les_water_paths_ref.py, bit for bit (every water
path, top and cover; gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero), every array the leading
part of a poisoned buffer whose other bytes are checked afterwards, the inputs compared with what was uploaded; the water-path
methods of models.DeviceLESEnsemble against their host twin.  The bodies live in tests/les_water_paths_ref.py:
tools/mutation_control.py --waterpath runs them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_water_paths_ref as wpr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", wpr.DTYPES)
@pytest.mark.parametrize("ktot", wpr.KTOTS)
@pytest.mark.parametrize("plane", wpr.PLANES)
def test_water_paths_equal_the_oracle(plane, ktot, dtype):
    wpr.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", wpr.DTYPES)
def test_row_counts_off_the_workgroup_and_one_les(dtype):
    wpr.check_rows(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", wpr.DTYPES)
def test_cover_of_fewer_than_eight_rows_over_several_les(dtype):
    """2 ... 7 LES of 1 x 1 and 2 LES of 1 x 3: one wave holds live rows of several LES and dead groups behind them"""
    wpr.check_few_rows(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", wpr.DTYPES)
def test_four_fields_in_one_launch(dtype):
    wpr.check_four_fields(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", wpr.DTYPES)
@pytest.mark.parametrize("lead,lead_w,pad", [(1, 0, 0), (0, 1, 0), (3, 3, 0), (0, 0, 3), (3, 1, 5)])
def test_views_off_the_16_byte_grid_and_a_pitched_w(lead, lead_w, pad, dtype):
    wpr.check_alignment(Engine("cuda:0", dtype=dtype), lead, lead_w, pad)


@pytest.mark.parametrize("dtype", wpr.DTYPES)
def test_cloud_top_and_cover(dtype):
    """cloudy only at k = 0, only at k = ktot - 1, nowhere; NaN and -0.0 cells; cover 0 and 1"""
    wpr.check_cloud(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", wpr.DTYPES)
def test_non_finite_values_and_rows_of_negative_zero(dtype):
    wpr.check_nonfinite(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", wpr.DTYPES)
def test_refusals_and_the_empty_ensemble(dtype):
    """ktot = 8193 is refused, 8192 is summed; n = 0 returns empties; the engine's argument checks"""
    wpr.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert wpr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thermo", [False, True])
@pytest.mark.parametrize("n", [4, 130])
def test_ensemble_water_paths_equal_the_host_twin(monkeypatch, n, thermo):
    """LWP, TWP, RWP, top, cover, the means and two rows' get_field at the start, after one evolve_model_batched and after one
    variability nudge, on one engine and on two engines sharing the card: equal bits with the host twin; one launch per device
    and state of the fields"""
    launches = []
    inner = Engine.les_water_paths
    monkeypatch.setattr(Engine, "les_water_paths", lambda self, fields, *a, **kw: (launches.append((tuple(fields), int(next(iter(fields.values())).shape[0]))), inner(self, fields, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    wpr.check_ensemble(Engine("cuda:0"), [one, multi], n, thermo)
    assert launches == [(("LWP", "TWP", "RWP"), n)] * 3 + [(("LWP", "TWP", "RWP"), n // 2)] * 6


@pytest.mark.parametrize("dtype", wpr.DTYPES)
@pytest.mark.parametrize("thermo", [False, True])
@pytest.mark.parametrize("n", [4, 130])
def test_ensemble_water_paths_in_the_engines_dtype(n, thermo, dtype):
    """the ensemble on a float64 and on a float32 engine against the oracle on its own fields in that dtype (the weights'
    .astype(T), the cover's division in T), at the start, after one step and after one nudge"""
    wpr.check_ensemble_dtype(Engine("cuda:0", dtype=dtype), n, thermo)
