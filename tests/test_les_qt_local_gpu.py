"""K19 on the MI355X: Engine.les_qt_local against the NumPy oracle of tests/les_qt_local_ref.py, bit for bit
(gpu_util.assert_bits: equal values, NaN at the same places, equal sign of zero) with exact integer counts, in float64 and
float32, every array the leading part of a poisoned buffer whose other bytes are checked afterwards, the read-only inputs compared
with what was uploaded; models.DeviceLESEnsemble's enable_qt_forcing() against its host twins, and driver.Coupler with
qt_forcing 'local' / 'strong'.  The bodies live in tests/les_qt_local_ref.py: tools/mutation_control.py --qtlocal runs them on
wrong kernels."""
import numpy
import pytest
import torch

from sp_coupler_amd import models, spcpl
from sp_coupler_amd import qt_forcing as qf
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import les_qt_local_ref as qlr
from tests.gpu_util import assert_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


@pytest.mark.parametrize("dtype", qlr.DTYPES)
@pytest.mark.parametrize("ktot", qlr.KTOTS)
@pytest.mark.parametrize("plane", qlr.PLANES)
def test_forcing_equals_the_oracle(plane, ktot, dtype):
    qlr.check_parity(Engine("cuda:0", dtype=dtype), plane, ktot)


@pytest.mark.parametrize("dtype", qlr.DTYPES)
@pytest.mark.parametrize("ktot", [1, 2, 65, 160])
def test_profiles_that_differ_per_les(ktot, dtype):
    """n = 1, 2, 5: another A and QTM per LES, with and without a pitch between the rows of the profiles and of count"""
    qlr.check_rows(Engine("cuda:0", dtype=dtype), ktot)


@pytest.mark.parametrize("dtype", qlr.DTYPES)
def test_every_launch_shape_gives_the_same_bits(dtype):
    """forced split factors 1, 2, 3 and one above the number of rows against the unforced launch, the oracle and each other;
    the split the library chooses on its own"""
    qlr.check_shapes(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", qlr.DTYPES)
def test_skipped_levels_keep_every_byte(dtype):
    """-0.0, NaN and infinities in qt on untouched levels; a NaN qt cell on a mixed level stays NaN and counts as dry"""
    qlr.check_skipped(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", qlr.DTYPES)
def test_cells_on_the_threshold_are_dry(dtype):
    qlr.check_ties(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("dtype", qlr.DTYPES)
@pytest.mark.parametrize("leads,ktot,pad", [((1, 1), 65, 0), ((3, 3), 64, 0), ((1, 1), 160, 2), ((2, 2), 7, 0), ((1, 0), 64, 0), ((0, 1), 160, 5),
                                            ((2, 0), 160, 0), ((0, 0), 160, 3)])
def test_views_off_the_16_byte_grid(leads, ktot, pad, dtype):
    """qt and ql equally off the grid and each differently (single elements whatever ktot), and on it (16-byte accesses)"""
    qlr.check_alignment(Engine("cuda:0", dtype=dtype), leads, ktot, pad)


@pytest.mark.parametrize("dtype", qlr.DTYPES)
def test_refusals(dtype):
    """n = 0; N > 2^24, a pitch below ktot, a NULL pointer, qt == ql, a negative split: through the C ABI and through the engine"""
    qlr.check_refusals(Engine("cuda:0", dtype=dtype))


@pytest.mark.parametrize("engines,n", [(2, 7), (3, 2)])
def test_engines_sharing_the_card_equal_one_engine(engines, n):
    """Sharded row blocks 4 + 3, and 1 + 1 + 0 (a device without rows)"""
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(engines)], min_cols_per_device=1)
    assert qlr.check_multi(one, multi, n) == ([4, 3] if engines == 2 else [1, 1, 0])


# -- the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", qf.KINDS)
@pytest.mark.parametrize("variant", list(qlr.VARIANTS))
@pytest.mark.parametrize("n", [4, 130])
def test_ensemble_equals_the_host_twin(monkeypatch, n, variant, kind):
    """three steps and one constantT nudge before the last, on one engine and on two engines sharing the card, plain and with
    diffusion + thermo + microphysics + horizontal and vertical advection + radiation: every profile, every field and the counts
    bit-equal to the host twin after each of them; ONE K19 launch per device and step (asserted); the QT field differs from the
    run without enable_qt_forcing() (asserted on the twin's logs), whose device run is bit-equal to its own twin"""
    launches = []
    inner = Engine.les_qt_local
    monkeypatch.setattr(Engine, "les_qt_local", lambda self, qt, *a, **kw: (launches.append((id(self), int(qt.shape[0]))), inner(self, qt, *a, **kw))[1])
    one = Engine("cuda:0")
    multi = MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    qlr.check_ensemble(Engine("cuda:0"), [one, multi], n, variant, kind)
    for eng, rows in [(one, n)] + [(e, n // 2) for e in multi.engines]:
        assert [r for i, r in launches if i == id(eng)] == [rows] * 3          # three steps: three launches


# -- the coupler ---------------------------------------------------------------------------------------------------------------
def test_coupler_with_a_local_qt_forcing_is_not_sp():
    """one spin-up step and one coupled step of driver.Coupler(qt_forcing=kind) on a DeviceLESEnsemble: the mode is enabled, QT
    differs from the "sp" run inside the mixed planes only while its slab mean follows it to rounding, the cloud water moves
    with the forcing; every record is bit-equal to the host twin's under the same coupler"""
    dev = qlr.check_coupler(Engine("cuda:0"), models.DeviceLESEnsemble)
    host = qlr.check_coupler(Engine("cuda:0"), qlr.HostQtLocalLESEnsemble)
    for kind in ("sp",) + qf.KINDS:
        for a, b in zip(host[kind], dev[kind]):
            assert set(a) == set(b)
            for k in a:
                assert_bits("%s %s" % (kind, k), b[k], a[k])


# -- the same on float32 engines against the float32 twin -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", qf.KINDS)
@pytest.mark.parametrize("variant", list(qlr.VARIANTS))
@pytest.mark.parametrize("n", [4, 130])
def test_float32_ensemble_equals_the_host_twin(monkeypatch, n, variant, kind):
    """test_ensemble_equals_the_host_twin on float32 engines against the float32 twin (tests/slab_ref.py: the rule of T)"""
    launches = []
    inner = Engine.les_qt_local
    monkeypatch.setattr(Engine, "les_qt_local", lambda self, qt, *a, **kw: (launches.append((id(self), int(qt.shape[0]))), inner(self, qt, *a, **kw))[1])
    one = Engine("cuda:0", dtype=torch.float32)
    multi = MultiDeviceEngine([Engine("cuda:0", dtype=torch.float32, stream=torch.cuda.Stream("cuda:0")) for _ in range(2)], min_cols_per_device=1)
    qlr.check_ensemble(Engine("cuda:0", dtype=torch.float32), [one, multi], n, variant, kind)
    for eng, rows in [(one, n)] + [(e, n // 2) for e in multi.engines]:
        assert [r for i, r in launches if i == id(eng)] == [rows] * 3          # three steps: three launches
