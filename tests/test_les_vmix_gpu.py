"""K25 on the MI355X: Engine.les_vmix against the NumPy oracle of tests/les_vmix_ref.py, bit for bit (gpu_util.assert_bits: equal
values, NaN at the same places, equal sign of zero), in float64 and float32, every array the leading part of a poisoned buffer
whose other bytes are checked afterwards, the read-only inputs compared with what was uploaded; models.DeviceLESEnsemble's
enable_vertical_mixing() against its host twins.  The bodies live in tests/les_vmix_ref.py: tools/mutation_control.py --vmix runs
them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_vmix_ref as lvr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", lvr.DTYPES)
@pytest.mark.parametrize("ktot", lvr.KTOTS)
def test_vertical_mixing_equals_the_oracle(ktot, dtype):
    """six fields with the fluxes and the drag, 1 to 3 LES of 3 x 5 and 8 x 8 columns"""
    lvr.check_parity(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_the_column_tile_cases(dtype):
    """tiles that span three and five LES, ktot 1 ... 17 and at every change of C, every lead off the 16-byte grid"""
    lvr.check_coltile(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_tiles_of_64_32_and_16_columns(dtype):
    """42 columns in LES of 6 around every change of the columns per workgroup, the largest supported ktot, the refusal above it"""
    first, changes, bad = lvr.check_tiles(Engine("cuda:0", dtype=dtype))
    assert (changes, bad) == (([64, 128], 640) if dtype == torch.float64 else ([128, 256], 1280))


@pytest.mark.parametrize("dtype", lvr.DTYPES)
@pytest.mark.parametrize("leads,ktot,pad", lvr.ALIGNMENTS)
def test_views_off_the_16_byte_grid(leads, ktot, pad, dtype):
    """every 4-D array 1 to 3 elements off the grid, differently per array; an odd ktot; pitch_prof > ktot"""
    lvr.check_alignment(Engine("cuda:0", dtype=dtype), leads, ktot, pad)


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_special_viscosities_and_calm_columns_beside_a_plume(dtype):
    """km NaN, negative, infinite and at the cap; km = 0 with kb = 0 keeps every value; calm columns beside one column of large
    km keep every value"""
    lvr.check_viscosity(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_fluxes_drag_and_the_speed_plane(dtype):
    """with and without flux and drag; zero wind gives sp = +0; a NaN wind stays in its column"""
    lvr.check_boundary(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_special_values_stay_in_their_column(dtype):
    lvr.check_special(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_one_to_six_fields_of_mixed_classes(dtype):
    lvr.check_fields(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_refusals(dtype):
    """through the C ABI and through the engine, with the fields and the speed plane untouched"""
    lvr.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert lvr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant,cap", [(4, "plain", None), (4, "plain", 1e6), (4, "all", None), (4, "forced", None), (130, "plain", None)])
def test_ensemble_equals_the_host_twin(monkeypatch, n, variant, cap):
    """three steps and one constantT nudge before the last, on one engine and on two engines sharing the card, plain and with
    radiation + thermo + microphysics + conservative second-order transport, and ("forced") with K19 in front of the step and K21
    in front of every substep: every profile, every field and both viscosities bit-equal to the host twin after each of them; per
    step and device one les_vmix behind the step's last les_mix, which is the second one (without fields) exactly where the cap
    bound (asserted)"""
    launches = []
    for name in ("les_mix", "les_vmix"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, *a, _n=name, _f=inner, **kw: (launches.append((id(self), _n)), _f(self, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    host, capped = lvr.check_ensemble(Engine("cuda:0"), [one, multi], n, variant, cap=cap)
    steps = [capped[0], capped[1], capped[3]]                         # (capped[2]: the record behind the nudge repeats step 2)
    assert all(steps) if cap is None and variant == "plain" else cap is None or not any(steps)
    want = [k for c in steps for k in (["les_mix"] * (2 if c else 1) + ["les_vmix"])]
    for eng in multi.engines + [one]:
        assert [k for i, k in launches if i == id(eng)] == want


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant,cap", [(4, "plain", None), (4, "plain", 1e6), (4, "all", None), (4, "forced", None), (130, "plain", None)])
def test_float32_ensemble_equals_the_host_twin(monkeypatch, n, variant, cap):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    launches = []
    for name in ("les_mix", "les_vmix"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, *a, _n=name, _f=inner, **kw: (launches.append((id(self), _n)), _f(self, *a, **kw))[1])
    one = Engine("cuda:0", dtype=torch.float32)
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=torch.float32, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    host, capped = lvr.check_ensemble(Engine("cuda:0", dtype=torch.float32), [one, multi], n, variant, cap=cap)
    steps = [capped[0], capped[1], capped[3]]                         # (capped[2]: the record behind the nudge repeats step 2)
    assert all(steps) if cap is None and variant == "plain" else cap is None or not any(steps)
    want = [k for c in steps for k in (["les_mix"] * (2 if c else 1) + ["les_vmix"])]
    for eng in multi.engines + [one]:
        assert [k for i, k in launches if i == id(eng)] == want
