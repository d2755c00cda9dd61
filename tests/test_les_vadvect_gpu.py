"""K17 on the MI355X: Engine.les_vadvect against the NumPy oracle of tests/les_vadvect_ref.py, bit for bit
(gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero), in float64 and float32, every array the
leading part of a poisoned buffer whose other bytes are checked afterwards, the inputs compared with what was uploaded;
models.DeviceLESEnsemble's enable_advection(vertical=True) against its host twins.  The bodies live in
tests/les_vadvect_ref.py: tools/mutation_control.py --vadvect runs them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_vadvect_ref as lvr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", lvr.DTYPES)
@pytest.mark.parametrize("ktot", lvr.KTOTS)
@pytest.mark.parametrize("plane", lvr.PLANES)
def test_vertical_advection_equals_the_oracle(plane, ktot, dtype):
    lvr.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", lvr.DTYPES)
@pytest.mark.parametrize("ktot", [1, 65, 160])
def test_coefficients_and_profiles_that_differ_per_les(ktot, dtype):
    """n = 1, 2, 5: another hx, hy, g and r per LES"""
    lvr.check_rows(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_every_boundary_of_the_tiles(dtype):
    """C - 1, C, C + 1 and 2 C + 1 columns for every C of spc_les_vadvect_cols_per_block, ktot on both sides of every change of
    it, 17 columns at the last supported ktot, and the first unsupported ktot refused"""
    first, changes, bad = lvr.check_tiles(Engine("cuda:0", dtype=dtype))
    wide = dtype == torch.float64
    assert (first, changes, bad) == ({64: 1, 32: 128 if wide else 256, 16: 256 if wide else 512}, [128, 256] if wide else [256, 512], 1280 if wide else 2560)


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_zero_to_six_fields_with_and_without_cmax_and_mtop(dtype):
    lvr.check_fields(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_the_probe_returns_what_a_full_launch_returns(dtype):
    lvr.check_probe(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lvr.DTYPES)
@pytest.mark.parametrize("lead,ktot", [(1, 65), (3, 64), (1, 160), (2, 7)])
def test_views_off_the_16_byte_grid(lead, ktot, dtype):
    lvr.check_alignment(Engine("cuda:0", dtype=dtype), lead, ktot)


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_convergent_and_divergent_columns_and_no_divergence(dtype):
    lvr.check_columns(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_special_values(dtype):
    """NaN, +-inf and -0.0 planted in single field cells; a NaN in one wind cell reaches the three columns that read it, from
    its level upward"""
    lvr.check_special(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lvr.DTYPES)
def test_refusals(dtype):
    """n = 0; nothing to do, a NULL g or r, pitch_prof < ktot, an output that is an input or another output, an extent below 1"""
    lvr.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert lvr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diffuse,thermo,micro", [(False, False, False), (True, False, False), (True, True, True)])
@pytest.mark.parametrize("n", [4, 130])
def test_ensemble_equals_the_host_twin(monkeypatch, n, diffuse, thermo, micro):
    """three steps and one constantT nudge before the last, on one engine and on two engines sharing the card, plain, with
    diffusion and with diffusion + thermo + microphysics, U raised in one column, 2 or 3 substeps in the first step (asserted):
    every profile and field bit-equal to the host twin after each of them; 2 + 2 n_sub launches per device and step; THL in and
    next to the raised column differs from the run with vertical=False (asserted on the twin's logs), and that run is bit-equal
    to enable_advection() without the argument"""
    launches = []
    for name in ("les_advect", "les_vadvect"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, fields, out, u, *a, _n=name, _f=inner, **kw: (
            launches.append((id(self), _n, int(u.shape[0]), len(fields))), _f(self, fields, out, u, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    n_sub = lvr.check_ensemble(Engine("cuda:0"), [one, multi], n, thermo, micro=micro, diffuse=diffuse)
    assert n_sub in (2, 3)
    nf = 5 if micro else 4
    for eng, rows in [(one, n)] + [(e, n // 2) for e in multi.engines]:
        mine = [(k, r, f) for i, k, r, f in launches if i == id(eng)]
        assert all(r == rows for _, r, _ in mine)
        want = [("les_advect", rows, 0), ("les_vadvect", rows, 0)] + [("les_advect", rows, nf), ("les_vadvect", rows, nf)] * n_sub
        assert mine[:2 + 2 * n_sub] == want                           # the two probes, then K16 and K17 per substep
        last = max(k for k, m in enumerate(mine) if m[0] == "les_vadvect")
        assert len([m for m in mine[:last + 1] if m == ("les_vadvect", rows, 0)]) == 3      # the run with vertical=True came first
        assert len([m for m in mine[:last + 1] if m[0] == "les_advect"]) == len([m for m in mine[:last + 1] if m[0] == "les_vadvect"])


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("diffuse,thermo,micro", [(False, False, False), (True, False, False), (True, True, True)])
@pytest.mark.parametrize("n", [4, 130])
def test_float32_ensemble_equals_the_host_twin(monkeypatch, n, diffuse, thermo, micro):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    launches = []
    for name in ("les_advect", "les_vadvect"):
        inner = getattr(Engine, name)
        monkeypatch.setattr(Engine, name, lambda self, fields, out, u, *a, _n=name, _f=inner, **kw: (
            launches.append((id(self), _n, int(u.shape[0]), len(fields))), _f(self, fields, out, u, *a, **kw))[1])
    one = Engine("cuda:0", dtype=torch.float32)
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=torch.float32, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    n_sub = lvr.check_ensemble(Engine("cuda:0", dtype=torch.float32), [one, multi], n, thermo, micro=micro, diffuse=diffuse)
    assert n_sub in (2, 3)
    nf = 5 if micro else 4
    for eng, rows in [(one, n)] + [(e, n // 2) for e in multi.engines]:
        mine = [(k, r, f) for i, k, r, f in launches if i == id(eng)]
        assert all(r == rows for _, r, _ in mine)
        want = [("les_advect", rows, 0), ("les_vadvect", rows, 0)] + [("les_advect", rows, nf), ("les_vadvect", rows, nf)] * n_sub
        assert mine[:2 + 2 * n_sub] == want                           # the two probes, then K16 and K17 per substep
        last = max(k for k, m in enumerate(mine) if m[0] == "les_vadvect")
        assert len([m for m in mine[:last + 1] if m == ("les_vadvect", rows, 0)]) == 3      # the run with vertical=True came first
        assert len([m for m in mine[:last + 1] if m[0] == "les_advect"]) == len([m for m in mine[:last + 1] if m[0] == "les_vadvect"])
