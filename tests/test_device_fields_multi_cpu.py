"""The sharding arithmetic of models.DeviceLESEnsemble under a multi.MultiDeviceEngine, without a GPU: two or three
oracle-backed engines (tests/fake_engine.OracleEngine: K9 by numpy.random.RandomState, K10 by tests/slab_ref.py, K6 by
oracle/vnudge_oracle.py) stand for the devices, as in tests/test_multi_device.py.  The bodies are those of
tests/test_device_fields_multi_gpu.py (tests/device_fields_multi.py); the host twin runs on one such engine."""
import numpy
import pytest

from sp_coupler_amd import spcpl
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import device_fields_multi as dfm
from tests.fake_engine import OracleEngine


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


def _multi(ndev, min_cols=1):
    return MultiDeviceEngine([OracleEngine() for _ in range(ndev)], min_cols_per_device=min_cols)


def test_the_oracle_engine_draws_the_initial_state_as_the_reference_loop():
    """OracleEngine.les_state against spcpl.set_les_state's own draws from the global generator"""
    from sp_coupler_amd import spcpl as sp
    shapes = [(3, 2, 5)] * 2
    prof = [numpy.arange(10.0).reshape(2, 5) + j for j in range(4)]
    numpy.random.seed(3)
    start = numpy.random.get_state()
    want = []

    class Les:
        get_itot, get_jtot, get_ktot = (lambda s: 3), (lambda s: 2), (lambda s: 5)

        def set_field(self, name, v):
            want.append(numpy.array(v))
    for l in range(2):
        sp.set_les_state(Les(), *[p[l] for p in prof])
    fields, (key, pos) = OracleEngine().les_state(shapes, *prof, start)
    end = numpy.random.get_state()
    assert numpy.array_equal(key, end[1]) and pos == end[2]
    for j, name in enumerate(("U", "V", "THL", "QT")):
        assert numpy.array_equal(fields[name].numpy(), numpy.stack([want[j], want[4 + j]])), name


@pytest.mark.parametrize("part", dfm.PARTITIONS)
def test_initial_state_in_row_blocks_equals_the_host_twin(part):
    dfm.check_initial_state(OracleEngine(), _multi(part[0], part[2]), part)


@pytest.mark.parametrize("constantT", [False, True])
@pytest.mark.parametrize("part", dfm.PARTITIONS)
def test_variability_nudge_in_row_blocks_equals_the_host_twin(part, constantT):
    dfm.check_variability_nudge(OracleEngine(), _multi(part[0], part[2]), part, constantT)


@pytest.mark.parametrize("constantT", [False, True])
def test_variability_nudge_split_at_the_column_limit(monkeypatch, constantT):
    dfm.check_chunked_nudge(monkeypatch, OracleEngine(), _multi(3), 7, constantT)


@pytest.mark.parametrize("ndev,n", [(2, 5), (3, 7)])
def test_closed_loop_with_variance_forcing_in_row_blocks_equals_the_host_twin(ndev, n):
    dfm.check_closed_loop(OracleEngine(), _multi(ndev), ndev, n)
