"""models.DeviceLESEnsemble with its fields in row blocks (transfer.Sharded) under a multi.MultiDeviceEngine, on the MI355X:
several Engine objects with streams of their own share the one card (as tests/test_slab_gpu.py::
test_two_engines_on_one_card_equal_one_engine), against the host twin slab_ref.HostFieldLESEnsemble on ONE engine -- the
executable definition.  Initial state, variability nudge (whole and split at the column limit) and a closed loop of coupled
steps give the same bits and leave numpy's generator in the same state; the blocks stay where they are.  The bodies live in
tests/device_fields_multi.py; tests/test_device_fields_multi_cpu.py runs them on oracle-backed engines without a GPU."""
import numpy
import pytest
import torch

from sp_coupler_amd import spcpl
from sp_coupler_amd.engine import Engine
from sp_coupler_amd.multi import MultiDeviceEngine
from tests import device_fields_multi as dfm

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    saved = numpy.random.get_state()
    yield
    spcpl.set_engine(None)
    numpy.random.set_state(saved)


def _multi(ndev, min_cols=1):
    return MultiDeviceEngine([Engine("cuda:0", stream=torch.cuda.Stream("cuda:0")) for _ in range(ndev)], min_cols_per_device=min_cols)


@pytest.mark.parametrize("part", dfm.PARTITIONS)
def test_initial_state_in_row_blocks_equals_the_host_twin(part):
    dfm.check_initial_state(Engine("cuda:0"), _multi(part[0], part[2]), part, nG=91, nL=160, itot=8, jtot=8)


@pytest.mark.parametrize("constantT", [False, True])
@pytest.mark.parametrize("part", dfm.PARTITIONS)
def test_variability_nudge_in_row_blocks_equals_the_host_twin(part, constantT):
    dfm.check_variability_nudge(Engine("cuda:0"), _multi(part[0], part[2]), part, constantT, itot=16, jtot=12, nL=40)


@pytest.mark.parametrize("constantT", [False, True])
def test_variability_nudge_split_at_the_column_limit(monkeypatch, constantT):
    dfm.check_chunked_nudge(monkeypatch, Engine("cuda:0"), _multi(3), 7, constantT, itot=16, jtot=12, nL=40)


@pytest.mark.parametrize("ndev,n", [(2, 5), (3, 7)])
def test_closed_loop_with_variance_forcing_in_row_blocks_equals_the_host_twin(ndev, n):
    dfm.check_closed_loop(Engine("cuda:0"), _multi(ndev), ndev, n, nG=91, nL=160, itot=12, jtot=10, steps=3)
