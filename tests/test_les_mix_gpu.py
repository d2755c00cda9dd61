"""K24 on the MI355X: Engine.les_mix against the NumPy oracle of tests/les_mix_ref.py, bit for bit (gpu_util.assert_bits: equal
values, NaN at the same places, equal sign of zero), in float64 and float32, every array the leading part of a poisoned buffer
whose other bytes are checked afterwards, the read-only inputs compared with what was uploaded; models.DeviceLESEnsemble's
enable_mixing() against its host twins.  The bodies live in tests/les_mix_ref.py: tools/mutation_control.py --mix runs them on
wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_mix_ref as lxr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", lxr.DTYPES)
@pytest.mark.parametrize("ktot", lxr.KTOTS)
@pytest.mark.parametrize("plane", lxr.PLANES)
def test_mixing_equals_the_oracle(plane, ktot, dtype):
    """0, 1, 2, 5 and 6 fields with theta and kmax, and two fields without both"""
    lxr.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", lxr.DTYPES)
@pytest.mark.parametrize("ktot", [1, 2, 65, 160])
def test_coefficients_and_profiles_that_differ_per_les(ktot, dtype):
    """n = 1, 2, 5: another gx, gy, kcap, ax, ay, gz, bz and l2 per LES, with and without a pitch between the rows of the profiles"""
    lxr.check_rows(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", lxr.DTYPES)
def test_strip_seams_of_both_kernels(dtype):
    """jtot * ktot one below, at and one above a strip, at itot = 1, 2, 3, 8, 9, 33, and the smallest launch that reaches 1 024
    workgroups, which walks the other number of rows"""
    assert lxr.check_strips(Engine("cuda:0", dtype=dtype)) == (256, 8, 32)


@pytest.mark.parametrize("dtype", lxr.DTYPES)
def test_the_vertical_index_is_clamped(dtype):
    """shear and stratification only at k = 0, then only at k = ktot - 1"""
    lxr.check_clamp(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lxr.DTYPES)
@pytest.mark.parametrize("leads,ktot,pad", [((1, 2, 3), 65, 0), ((3, 3, 3), 64, 0), ((1, 0, 2, 3), 160, 2), ((2, 1), 7, 0), ((3, 0, 1, 2, 0), 63, 5)])
def test_views_off_the_16_byte_grid(leads, ktot, pad, dtype):
    """every 4-D array 1 to 3 elements off the grid, differently per array"""
    lxr.check_alignment(Engine("cuda:0", dtype=dtype), leads, ktot, pad)


@pytest.mark.parametrize("dtype", lxr.DTYPES)
def test_special_values(dtype):
    """the uniform stable state keeps every bit with km = +0; an unstable theta at rest gives km > 0; a NaN in u, theta or a field
    reaches the cells whose stencil reads it and nothing else; an infinite kk is capped"""
    lxr.check_special(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lxr.DTYPES)
def test_a_known_share_of_cells_is_capped(dtype):
    assert 0.1 < lxr.check_cap(Engine("cuda:0", dtype=dtype)) < 0.9


@pytest.mark.parametrize("dtype", lxr.DTYPES)
def test_refusals(dtype):
    """n = 0; pitch_prof < ktot, a NULL required pointer, theta without bz, km, kmax or an out[f] equal to an input or to each
    other, n_fields outside 0 ... 6: through the C ABI and through the engine, with the outputs untouched"""
    lxr.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert lxr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant,vertical", [(4, "plain", False), (4, "all", False), (4, "all", True), (4, "forced", True), (130, "plain", False),
                                                 (130, "all", True)])
def test_ensemble_equals_the_host_twin(monkeypatch, n, variant, vertical):
    """three steps and one constantT nudge before the last, on one engine and on two engines sharing the card, plain and with
    diffusion + radiation + thermo + microphysics + conservative second-order transport, with K15 taking K24's viscosity and
    without, and ("forced") with K19 in front of the step and K21 in front of every substep: every profile, every field and km
    bit-equal to the host twin after each of them; per step and device the
    transport's launches, then les_mix, then les_diffuse (asserted); U differs from the run without enable_mixing() (asserted on
    the twin's logs), whose device run is bit-equal to the twin of tests/les_full_ref.py"""
    launches = []
    for name in ("les_transport", "les_transport2", "les_mix", "les_diffuse"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, *a, _n=name, _f=inner, **kw: (launches.append((id(self), _n)), _f(self, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    lxr.check_ensemble(Engine("cuda:0"), [one, multi], n, variant, vertical)
    for eng in multi.engines:
        mine = [k for i, k in launches if i == id(eng)]
        steps = [i for i, k in enumerate(mine) if k == "les_mix"]
        assert len(steps) == 3
        if variant != "plain":                                        # per step: the probe (K22), the substeps (K23), K24, K15
            for i in steps:
                assert mine[i - 1] == "les_transport2" and mine[i + 1] == "les_diffuse"
            assert mine[0] == "les_transport" and mine.count("les_diffuse") == 3 and mine.count("les_transport") == 3
        else:
            assert mine == ["les_mix"] * 3
    mine = [k for i, k in launches if i == id(one)]                   # (then the run without enable_mixing(): on `one` only)
    assert mine.count("les_mix") == 3 and (variant == "plain" or mine.count("les_diffuse") == 6)


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant,vertical", [(4, "plain", False), (4, "all", False), (4, "all", True), (4, "forced", True), (130, "plain", False),
                                                 (130, "all", True)])
def test_float32_ensemble_equals_the_host_twin(monkeypatch, n, variant, vertical):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    launches = []
    for name in ("les_transport", "les_transport2", "les_mix", "les_diffuse"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, *a, _n=name, _f=inner, **kw: (launches.append((id(self), _n)), _f(self, *a, **kw))[1])
    one = Engine("cuda:0", dtype=torch.float32)
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=torch.float32, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    lxr.check_ensemble(Engine("cuda:0", dtype=torch.float32), [one, multi], n, variant, vertical)
    for eng in multi.engines:
        mine = [k for i, k in launches if i == id(eng)]
        steps = [i for i, k in enumerate(mine) if k == "les_mix"]
        assert len(steps) == 3
        if variant != "plain":                                        # per step: the probe (K22), the substeps (K23), K24, K15
            for i in steps:
                assert mine[i - 1] == "les_transport2" and mine[i + 1] == "les_diffuse"
            assert mine[0] == "les_transport" and mine.count("les_diffuse") == 3 and mine.count("les_transport") == 3
        else:
            assert mine == ["les_mix"] * 3
    mine = [k for i, k in launches if i == id(one)]                   # (then the run without enable_mixing(): on `one` only)
    assert mine.count("les_mix") == 3 and (variant == "plain" or mine.count("les_diffuse") == 6)
