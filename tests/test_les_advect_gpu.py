"""K16 on the MI355X: Engine.les_advect against the NumPy oracle of tests/les_advect_ref.py, bit for bit
(gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero), in float64 and float32, every array the
leading part of a poisoned buffer whose other bytes are checked afterwards, the inputs compared with what was uploaded;
models.DeviceLESEnsemble's advection mode against its host twins.  The bodies live in tests/les_advect_ref.py:
tools/mutation_control.py --advect runs them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_advect_ref as lar

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", lar.DTYPES)
@pytest.mark.parametrize("ktot", lar.KTOTS)
@pytest.mark.parametrize("plane", lar.PLANES)
def test_advection_equals_the_oracle(plane, ktot, dtype):
    lar.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", lar.DTYPES)
@pytest.mark.parametrize("ktot", [1, 65, 160])
def test_coefficients_that_differ_per_les(ktot, dtype):
    """n = 1, 2, 5: another dx and another dy per LES"""
    lar.check_rows(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", lar.DTYPES)
def test_every_boundary_of_the_workgroups(dtype):
    """the flat run of a row at spc_les_advect_strip - 1, + 0, + 1 and the rows at spc_les_advect_rows - 1, + 0, + 1, for launches
    of few and of many workgroups"""
    assert lar.check_strips(Engine("cuda:0", dtype=dtype)) == (256, 8, 32)


@pytest.mark.parametrize("dtype", lar.DTYPES)
def test_one_to_six_fields_with_and_without_the_winds_among_them(dtype):
    lar.check_fields(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lar.DTYPES)
def test_the_probe_returns_the_courant_sums_of_a_full_launch(dtype):
    lar.check_probe(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lar.DTYPES)
@pytest.mark.parametrize("lead,ktot", [(1, 65), (3, 64), (1, 160), (2, 7)])
def test_views_off_the_16_byte_grid(lead, ktot, dtype):
    lar.check_alignment(Engine("cuda:0", dtype=dtype), lead, ktot)


@pytest.mark.parametrize("dtype", lar.DTYPES)
def test_winds_of_either_sign_and_no_wind(dtype):
    lar.check_signs(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lar.DTYPES)
def test_special_values_reach_one_step(dtype):
    """NaN, +-inf and -0.0 planted in single field cells, NaN in one wind cell; the cells further away equal a run without them"""
    lar.check_special(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lar.DTYPES)
def test_refusals(dtype):
    """n = 0; no field and no cmax, an output that is an input, cmax or another output, an extent below 1"""
    lar.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert lar.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diffuse,thermo,micro,dx", [(False, False, False, lar.DX_FEW), (True, False, False, lar.DX_FEW),
                                                     (True, True, True, lar.DX_FEW), (False, False, False, lar.DX_ONE)])
@pytest.mark.parametrize("n", [4, 130])
def test_ensemble_equals_the_host_twin(monkeypatch, n, diffuse, thermo, micro, dx):
    """three steps and one constantT nudge before the last, on one engine and on two engines sharing the card, plain, with
    diffusion and with diffusion + thermo + microphysics, with 2 or 3 substeps in the first step (asserted) and with one:
    every profile and field bit-equal to the host twin after each of them; 1 + n_sub launches per device and step; a QT raised
    in one column differs from the run without enable_advection() (asserted on the twin's logs)"""
    launches = []
    inner = Engine.les_advect
    monkeypatch.setattr(Engine, "les_advect", lambda self, fields, out, u, *a, **kw: (launches.append((id(self), int(u.shape[0]), len(fields))),
                                                                                    inner(self, fields, out, u, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    n_sub = lar.check_ensemble(Engine("cuda:0"), [one, multi], n, thermo, micro=micro, diffuse=diffuse, dx=dx)
    assert (n_sub == 1) if dx == lar.DX_ONE else n_sub in (2, 3)
    nf = 5 if micro else 4
    for eng, rows in [(one, n)] + [(e, n // 2) for e in multi.engines]:
        mine = [(r, f) for i, r, f in launches if i == id(eng)]
        probes = [k for k, (r, f) in enumerate(mine) if f == 0]
        assert len(probes) == 3 and all(r == rows for r, _ in mine)                       # one probe per device and step ...
        assert mine[:1 + n_sub] == [(rows, 0)] + [(rows, nf)] * n_sub                     # ... and n_sub launches behind it
        assert all(f == nf for k, (r, f) in enumerate(mine) if k not in probes)


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("diffuse,thermo,micro,dx", [(False, False, False, lar.DX_FEW), (True, False, False, lar.DX_FEW),
                                                     (True, True, True, lar.DX_FEW), (False, False, False, lar.DX_ONE)])
@pytest.mark.parametrize("n", [4, 130])
def test_float32_ensemble_equals_the_host_twin(monkeypatch, n, diffuse, thermo, micro, dx):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    launches = []
    inner = Engine.les_advect
    monkeypatch.setattr(Engine, "les_advect", lambda self, fields, out, u, *a, **kw: (launches.append((id(self), int(u.shape[0]), len(fields))),
                                                                                    inner(self, fields, out, u, *a, **kw))[1])
    one = Engine("cuda:0", dtype=torch.float32)
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=torch.float32, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    n_sub = lar.check_ensemble(Engine("cuda:0", dtype=torch.float32), [one, multi], n, thermo, micro=micro, diffuse=diffuse, dx=dx)
    assert (n_sub == 1) if dx == lar.DX_ONE else n_sub in (2, 3)
    nf = 5 if micro else 4
    for eng, rows in [(one, n)] + [(e, n // 2) for e in multi.engines]:
        mine = [(r, f) for i, r, f in launches if i == id(eng)]
        probes = [k for k, (r, f) in enumerate(mine) if f == 0]
        assert len(probes) == 3 and all(r == rows for r, _ in mine)                       # one probe per device and step ...
        assert mine[:1 + n_sub] == [(rows, 0)] + [(rows, nf)] * n_sub                     # ... and n_sub launches behind it
        assert all(f == nf for k, (r, f) in enumerate(mine) if k not in probes)
