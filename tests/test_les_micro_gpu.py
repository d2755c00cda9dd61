"""K14 on the MI355X: Engine.les_microphysics against the NumPy oracle of tests/les_micro_ref.py, bit for bit (qt, thl, qr_new,
rain and the four means; gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero), every array the
leading part of a poisoned buffer whose other bytes are checked afterwards, the inputs compared with what was uploaded;
models.DeviceLESEnsemble's microphysics mode against its host twin.  The bodies live in tests/les_micro_ref.py:
tools/mutation_control.py --micro runs them on wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import models, spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_micro_ref as lmr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", lmr.DTYPES)
@pytest.mark.parametrize("ktot", lmr.KTOTS)
@pytest.mark.parametrize("plane", lmr.PLANES)
def test_microphysics_equals_the_oracle(plane, ktot, dtype):
    lmr.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", lmr.DTYPES)
@pytest.mark.parametrize("n", lmr.NS)
@pytest.mark.parametrize("ktot", [2, 3, 8, 63, 64, 65, 66, 128, 129, 160])
def test_the_top_level_reads_nothing_above_it(ktot, n, dtype):
    """level 0 of the column (of the LES) that follows in memory holds large qr; n = 1, 2, 5"""
    lmr.check_neighbour(Engine("cuda:0", dtype=dtype), ktot, n)


@pytest.mark.parametrize("dtype", lmr.DTYPES)
@pytest.mark.parametrize("ktot", [160, 33])
def test_row_counts_with_every_remainder_of_the_look_ahead(ktot, dtype):
    lmr.check_rows(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", lmr.DTYPES)
@pytest.mark.parametrize("lead,lead_rows,pad", [(1, 0, 0), (0, 1, 0), (3, 3, 0), (0, 0, 4), (0, 0, 3), (2, 1, 5)])
def test_views_off_the_16_byte_grid_and_pitched_rows(lead, lead_rows, pad, dtype):
    lmr.check_alignment(Engine("cuda:0", dtype=dtype), lead, lead_rows, pad)


@pytest.mark.parametrize("dtype", lmr.DTYPES)
def test_optional_arguments(dtype):
    """thl, temp, rain NULL, no means, constants of the caller; each optional pointer NULL on its own through the C ABI"""
    lmr.check_optional(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lmr.DTYPES)
def test_special_values(dtype):
    """NaN, +-inf and -0.0 in ql, qr and temp; temp exactly t_up and t_dn; ql = qt = -0.0; a NaN threshold"""
    lmr.check_special(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lmr.DTYPES)
def test_the_cap(dtype):
    lmr.check_cap(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lmr.DTYPES)
def test_launches_of_more_than_one_wave_per_simd(dtype):
    """the kernels with 2 rows per batch (one compute unit counted, so the small launches of a test take them)"""
    lmr.check_many_waves(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", lmr.DTYPES)
def test_refusals(dtype):
    """n = 0, ktot = 1, aliasing, wrong dtype / device / shape"""
    lmr.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert lmr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thermo", [False, True])
@pytest.mark.parametrize("n", [4, 130])
def test_ensemble_equals_the_host_twin(monkeypatch, n, thermo):
    """three steps with one constantT nudge before the last, on one engine and on two engines sharing the card, K11 stepping
    the fields (FUSED_MIN_LES patched to 0): every profile, field, rain2d and RWP bit-equal to the host twin after each of
    them; one K14 launch per device and step; p["Rain"], p["QR"] and RWP change (asserted on the twin's log)"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    launches, steps = [], []
    mic, adv = Engine.les_microphysics, Engine.les_advance
    monkeypatch.setattr(Engine, "les_microphysics", lambda self, qt, *a, **kw: (launches.append((int(qt.shape[0]), kw.get("temp") is not None)), mic(self, qt, *a, **kw))[1])
    monkeypatch.setattr(Engine, "les_advance", lambda self, *a, **kw: (steps.append(kw.get("sat")), adv(self, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    lmr.check_ensemble(Engine("cuda:0"), [one, multi], n, thermo)
    assert launches == [(n, thermo)] * 3 + [(n // 2, thermo)] * 6
    assert steps == [None if thermo else "QT"] * 9


@pytest.mark.parametrize("dtype", lmr.DTYPES)
def test_the_chain_cases(dtype):
    """the cases of the lane's walk that spc_chain.hpp's kernels share, held together, for both batch sizes (les_micro_ref.check_chain)"""
    lmr.check_chain(Engine("cuda:0", dtype=dtype))


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("thermo", [False, True])
@pytest.mark.parametrize("n", [4, 130])
def test_float32_ensemble_equals_the_host_twin(monkeypatch, n, thermo):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    monkeypatch.setattr(models.DeviceLESEnsemble, "FUSED_MIN_LES", 0)
    launches, steps = [], []
    mic, adv = Engine.les_microphysics, Engine.les_advance
    monkeypatch.setattr(Engine, "les_microphysics", lambda self, qt, *a, **kw: (launches.append((int(qt.shape[0]), kw.get("temp") is not None)), mic(self, qt, *a, **kw))[1])
    monkeypatch.setattr(Engine, "les_advance", lambda self, *a, **kw: (steps.append(kw.get("sat")), adv(self, *a, **kw))[1])
    one = Engine("cuda:0", dtype=torch.float32)
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=torch.float32, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    lmr.check_ensemble(Engine("cuda:0", dtype=torch.float32), [one, multi], n, thermo)
    assert launches == [(n, thermo)] * 3 + [(n // 2, thermo)] * 6
    assert steps == [None if thermo else "QT"] * 9
