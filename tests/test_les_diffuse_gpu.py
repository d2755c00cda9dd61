"""K15 on the MI355X: Engine.les_diffuse against the NumPy oracle of tests/les_diffuse_ref.py, bit for bit
(gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero), in float64 and float32, every array the
leading part of a poisoned buffer whose other bytes are checked afterwards, the inputs compared with what was uploaded;
models.DeviceLESEnsemble's diffusion mode against its host twins.  The bodies live in tests/les_diffuse_ref.py:
tools/mutation_control.py --diffuse runs them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import models, spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_diffuse_ref as ldr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", ldr.DTYPES)
@pytest.mark.parametrize("ktot", ldr.KTOTS)
@pytest.mark.parametrize("plane", ldr.PLANES)
def test_diffusion_equals_the_oracle(plane, ktot, dtype):
    ldr.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", ldr.DTYPES)
@pytest.mark.parametrize("ktot", [1, 7, 64, 160])
def test_coefficient_rows_that_differ_per_les(ktot, dtype):
    """n = 1, 2, 5: another density and another mixed layer per LES"""
    ldr.check_rows(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", ldr.DTYPES)
def test_every_boundary_of_cols_per_block(dtype):
    """the last ktot of 64, 32 and 16 columns per workgroup, the first of the next, and one above the largest: refused"""
    bounds = ldr.check_boundaries(Engine("cuda:0", dtype=dtype))
    assert bounds[-2][0] >= 1024 and bounds[-1][1] == 0


@pytest.mark.parametrize("dtype", ldr.DTYPES)
@pytest.mark.parametrize("ktot", [7, 160, 300, 600])
def test_whole_and_partial_tiles(ktot, dtype):
    """C q + r columns, r in {0, 1, C - 1}, at 64, 32 and 16 columns per workgroup"""
    ldr.check_tiles(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", ldr.DTYPES)
def test_the_column_tile_cases(dtype):
    """tiles that span three and five LES, ktot 1 ... 17 and at every change of C, every lead off the 16-byte grid"""
    ldr.check_coltile(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", ldr.DTYPES)
def test_field_counts_and_optional_fluxes(dtype):
    ldr.check_fields(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", ldr.DTYPES)
@pytest.mark.parametrize("lead,lead_rows,pad,ktot", [(1, 0, 0, 65), (0, 1, 0, 65), (3, 3, 0, 64), (0, 0, 3, 64), (2, 1, 5, 7), (1, 1, 1, 160)])
def test_views_off_the_16_byte_grid_and_pitched_rows(lead, lead_rows, pad, ktot, dtype):
    ldr.check_alignment(Engine("cuda:0", dtype=dtype), lead, lead_rows, pad, ktot)


@pytest.mark.parametrize("dtype", ldr.DTYPES)
def test_a_step_of_an_hour(dtype):
    ldr.check_long_step(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", ldr.DTYPES)
def test_special_values_stay_in_their_column(dtype):
    """-0.0, NaN and +-inf planted in single columns; the neighbours' bits equal a run without them; the identity keeps every bit"""
    ldr.check_special(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", ldr.DTYPES)
def test_refusals(dtype):
    """n = 0; two equal fields, a field that is a profile, a flux without s0"""
    ldr.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert ldr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thermo,micro", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("n", [4, 130])
def test_ensemble_equals_the_host_twin(monkeypatch, n, thermo, micro):
    """three steps with non-zero wt and wq and one constantT nudge before the last, on one engine and on two engines sharing
    the card, plain, with enable_thermo() and with thermo + microphysics: every profile and field bit-equal to the host twin
    after each of them; one K15 launch per device and step; p["THL"] at level 0 differs from the run without enable_diffusion()
    (asserted on the twin's logs)"""
    launches = []
    dif = Engine.les_diffuse
    monkeypatch.setattr(Engine, "les_diffuse", lambda self, fields, *a, **kw: (launches.append((int(fields["THL"].shape[0]), sorted(kw["flux"]))),
                                                                              dif(self, fields, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    ldr.check_ensemble(Engine("cuda:0"), [one, multi], n, thermo, micro=micro)
    assert launches == [(n, ["QT", "THL"])] * 3 + [(n // 2, ["QT", "THL"])] * 6


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("thermo,micro", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("n", [4, 130])
def test_float32_ensemble_equals_the_host_twin(monkeypatch, n, thermo, micro):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    launches = []
    dif = Engine.les_diffuse
    monkeypatch.setattr(Engine, "les_diffuse", lambda self, fields, *a, **kw: (launches.append((int(fields["THL"].shape[0]), sorted(kw["flux"]))),
                                                                              dif(self, fields, *a, **kw))[1])
    one = Engine("cuda:0", dtype=torch.float32)
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=torch.float32, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    ldr.check_ensemble(Engine("cuda:0", dtype=torch.float32), [one, multi], n, thermo, micro=micro)
    assert launches == [(n, ["QT", "THL"])] * 3 + [(n // 2, ["QT", "THL"])] * 6
