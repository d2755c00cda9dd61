"""K12 on the MI355X: Engine.les_thermo against the NumPy oracle of tests/les_thermo_ref.py, bit for bit (qsat, ql, temp and
both means; gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero), every array the leading part of
a poisoned buffer whose other bytes are checked afterwards, thl and qt compared with what was uploaded;
models.DeviceLESEnsemble's thermo mode in the Coupler's closed loop against its host twin.  The bodies live in
tests/les_thermo_ref.py: tools/mutation_control.py --thermo runs them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import _abi, models, spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_thermo_ref as ltr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", ltr.DTYPES)
@pytest.mark.parametrize("ktot", ltr.KTOTS)
@pytest.mark.parametrize("plane", ltr.PLANES)
def test_thermo_equals_the_oracle(plane, ktot, dtype):
    ltr.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", ltr.DTYPES)
@pytest.mark.parametrize("n_iter", [0, 1, None])
@pytest.mark.parametrize("ktot", [7, 64])
def test_thermo_of_the_mixed_field(ktot, n_iter, dtype):
    """unsaturated and saturated cells, qt == qs, Tl outside the table and on its knots, NaN, qt = -0.0, in one field"""
    ltr.check_special(Engine("cuda:0", dtype=dtype), ktot, n_iter)


@pytest.mark.parametrize("dtype", ltr.DTYPES)
@pytest.mark.parametrize("lead,lead_rows,pad", [(1, 0, 0), (0, 1, 0), (3, 3, 0), (0, 0, 4), (0, 0, 3), (2, 1, 5)])
def test_thermo_with_views_off_the_16_byte_grid_and_pitched_rows(lead, lead_rows, pad, dtype):
    ltr.check_alignment(Engine("cuda:0", dtype=dtype), lead, lead_rows, pad)


@pytest.mark.parametrize("dtype", ltr.DTYPES)
def test_thermo_options(dtype):
    """n_iter 0, 1 and the default; temp NULL; no means; both places of the table"""
    ltr.check_options(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", ltr.DTYPES)
def test_thermo_with_tables_of_the_caller(dtype):
    """through the C ABI: a Newton step that lands on a knot where qs == qt exactly; dq == -0.0"""
    ltr.check_table(Engine("cuda:0", dtype=dtype))


def test_thermo_argument_checks_of_the_engine():
    eng = Engine("cuda:0")
    f = torch.full((2, 4, 4, 8), 290.0, dtype=torch.float64, device=eng.device)
    q = torch.full_like(f, 1e-2)
    p = torch.full((2, 8), 1e5, dtype=torch.float64, device=eng.device)
    e = torch.ones_like(p)
    for bad in (lambda: eng.les_thermo(f, q[:, :, :, ::2], p, e),                                   # another shape / not contiguous
                lambda: eng.les_thermo(f.float(), q, p, e),                                         # not the engine's dtype
                lambda: eng.les_thermo(f.cpu(), q, p, e),
                lambda: eng.les_thermo(f, q, p[:, :4], e),
                lambda: eng.les_thermo(f, q, p, e, n_iter=-1),
                lambda: eng.les_thermo(f, q, p, e, means={"U": p}),
                lambda: eng.les_thermo(f, q, p, e, qsat=f),                                         # an output that is an input
                lambda: eng.les_thermo(f, q, p, e, temp=q),
                lambda: eng.les_thermo(f, q, p, e, table_mode=7)):
        with pytest.raises(ValueError):
            bad()
    one = torch.zeros((2, 4, 4, 1), dtype=torch.float64, device=eng.device)
    with pytest.raises(_abi.SpcError) as err:
        eng.les_thermo(one, one.clone(), p[:, :1], e[:, :1])
    assert err.value.code == _abi.SPC_ERR_UNSUPPORTED and "ktot == 1" in str(err.value)
    res = eng.les_thermo(f[:0], q[:0], p[:0], e[:0])                                               # an empty ensemble: no launch
    assert res["QL"].shape == (0, 8) and res["T"].shape == (0, 8)
    torch.cuda.synchronize()
    assert bool((f == 290.0).all()) and bool((q == 1e-2).all())


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert ltr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 130])
def test_closed_loop_of_the_thermo_ensemble_equals_the_host_twin(monkeypatch, n):
    """Coupler(qt_forcing="variance"), spin-up, 3 steps and one constantT nudge, on one engine and on two engines sharing the
    card: every tendency, profile and field bit-equal to the host twin after each step.  130 LES on one engine are above
    FUSED_MIN_LES: K11 steps the fields there (without its own saturation), K12 follows"""
    steps, launches = [], []
    adv, thm = Engine.les_advance, Engine.les_thermo
    monkeypatch.setattr(Engine, "les_advance", lambda self, *a, **kw: (steps.append((int(next(iter(a[0].values())).shape[0]), kw.get("sat"))), adv(self, *a, **kw))[1])
    monkeypatch.setattr(Engine, "les_thermo", lambda self, *a, **kw: (launches.append(int(a[0].shape[0])), thm(self, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    ltr.check_closed_loop(Engine("cuda:0"), [one, multi], n)
    assert launches.count(n) >= 5 and launches.count(n // 2) >= 10
    assert models.DeviceLESEnsemble.FUSED_MIN_LES == 128
    assert steps == ([] if n < 128 else [(n, None)] * len(steps)) and (n < 128 or len(steps) >= 3)


@pytest.mark.parametrize("dtype", ltr.DTYPES)
def test_the_chain_cases(dtype):
    """the cases of the lane's walk that spc_chain.hpp's kernels share, held together (les_thermo_ref.check_chain)"""
    ltr.check_chain(Engine("cuda:0", dtype=dtype))
