"""K26 on the MI355X: Engine.les_hmix against the NumPy oracle of tests/les_hmix_ref.py, bit for bit (gpu_util.assert_bits: equal
values, NaN at the same places, equal sign of zero), in float64 and float32, every array the leading part of a poisoned buffer
whose other bytes are checked afterwards, the read-only inputs compared with what was uploaded; models.DeviceLESEnsemble's
enable_mixing(implicit=True) against its host twin.  The bodies live in tests/les_hmix_ref.py: tools/mutation_control.py --hmix
runs them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_hmix_ref as lhr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", lhr.DTYPES)
@pytest.mark.parametrize("ktot", lhr.KTOTS)
def test_horizontal_mixing_equals_the_oracle(ktot, dtype):
    """six fields of both classes, 1 to 3 LES of 3 x 5, 8 x 8 and 4 x 7 columns"""
    lhr.check_parity(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", lhr.DTYPES)
def test_lines_of_1_to_33_cells_along_each_axis(dtype):
    """both sweeps and each alone; 777 lines: a partial last workgroup, and workgroups that span two LES"""
    lhr.check_lines(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lhr.DTYPES)
@pytest.mark.parametrize("leads,ktot", lhr.ALIGNMENTS)
def test_views_off_the_16_byte_grid(leads, ktot, dtype):
    """every 4-D array 1 to 3 elements off the grid, differently per array; an odd ktot"""
    lhr.check_alignment(Engine("cuda:0", dtype=dtype), leads, ktot)


@pytest.mark.parametrize("dtype", lhr.DTYPES)
def test_special_viscosities_and_calm_lines_beside_a_violent_one(dtype):
    """km NaN, negative, infinite, at the bound and zero; calm lines beside one line of large km keep every value"""
    lhr.check_viscosity(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lhr.DTYPES)
def test_special_values_stay_in_their_line_then_in_their_plane(dtype):
    lhr.check_special(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lhr.DTYPES)
def test_one_to_six_fields_of_mixed_classes(dtype):
    lhr.check_fields(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lhr.DTYPES)
def test_two_calls_of_one_sweep_equal_one_call_of_both(dtype):
    lhr.check_sweeps(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lhr.DTYPES)
def test_refusals(dtype):
    """through the C ABI and through the engine, with the fields untouched"""
    lhr.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lhr.DTYPES)
def test_lines_per_workgroup(dtype):
    """the flagship planes and the longest lines the issue asks for"""
    eng = Engine("cuda:0", dtype=dtype)
    f64 = dtype == torch.float64
    assert [eng.hmix_lines_per_block(n) for n in (8, 64, 256)] == ([256, 64, 32] if f64 else [256, 128, 32])
    assert eng.hmix_lines_per_block(641 if f64 else 1281) == 16 and eng.hmix_lines_per_block(642 if f64 else 1282) == 0


@pytest.mark.parametrize("dtype", lhr.DTYPES)
def test_a_line_of_256_cells(dtype):
    """the longest line that must be supported, along i and along j: 32 lines per workgroup in more than 64 KiB of LDS"""
    eng = Engine("cuda:0", dtype=dtype)
    for shape in ((1, 256, 2, 3), (1, 2, 256, 3)):
        lhr.Run(eng, lhr.case(shape, lhr.np_of(eng), seed=14), ("U", "QT")).check("shape %s" % (shape,))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert lhr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant", [(4, "plain"), (4, "all"), (4, "forced"), (4, "k15"), (130, "plain")])
def test_ensemble_equals_the_host_twin(monkeypatch, n, variant):
    """three steps and one constantT nudge before the last, on one engine and on two engines sharing the card: every profile, every
    field and the viscosity bit-equal to the host twin after each of them; per step and device one les_mix WITHOUT fields, one
    les_hmix, then les_vmix where enabled, and never a second les_mix (asserted)"""
    launches = []
    for name in ("les_mix", "les_hmix", "les_vmix"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, *a, _n=name, _f=inner, **kw: (
            launches.append((id(self), _n, len(a[0]) if _n == "les_mix" else None)), _f(self, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    lhr.check_ensemble(Engine("cuda:0"), [one, multi], n, variant)
    vmix = lhr.VARIANTS[variant].get("vmix", False)
    want = ([("les_mix", 0), ("les_hmix", None)] + ([("les_vmix", None)] if vmix else [])) * 3
    for eng in multi.engines + [one]:
        assert [(k, c) for i, k, c in launches if i == id(eng)] == want


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant", [(4, "plain"), (4, "all"), (4, "forced"), (4, "k15"), (130, "plain")])
def test_float32_ensemble_equals_the_host_twin(monkeypatch, n, variant):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    launches = []
    for name in ("les_mix", "les_hmix", "les_vmix"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, *a, _n=name, _f=inner, **kw: (
            launches.append((id(self), _n, len(a[0]) if _n == "les_mix" else None)), _f(self, *a, **kw))[1])
    one = Engine("cuda:0", dtype=torch.float32)
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=torch.float32, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    lhr.check_ensemble(Engine("cuda:0", dtype=torch.float32), [one, multi], n, variant)
    vmix = lhr.VARIANTS[variant].get("vmix", False)
    want = ([("les_mix", 0), ("les_hmix", None)] + ([("les_vmix", None)] if vmix else [])) * 3
    for eng in multi.engines + [one]:
        assert [(k, c) for i, k, c in launches if i == id(eng)] == want
