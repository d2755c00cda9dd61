"""K7 on the MI355X where a workgroup owns a slab of several rows: the bodies of tests/sputils_slabs.py on both engines, bit for bit
against NumPy / the oracle (float64) and tests/f32_ref.py (float32).  Every launch of a body asserts the slab height the library's
own description gives it (one compute unit counted: a few dozen rows get the slabs of thousands); the last test requires that the
instantiation names the bodies launched are the reachable ones.  tools/mutation_control.py --sputils runs the same bodies on its
mutant libraries (profiles/mutation_control_sputils.log)."""
import pytest

from tests import sputils_slabs as ss

pytestmark = pytest.mark.gpu
IDS = ["f64", "f32"]
RAN = {8: set(), 4: set()}


@pytest.fixture(scope="module")
def engines():
    from sp_coupler_amd.engine import Engine
    return {dtype: Engine("cuda:0", dtype=dtype) for dtype in ss.DTYPES}


@pytest.mark.parametrize("dtype", ss.DTYPES, ids=IDS)
@pytest.mark.parametrize("body", ss.BODIES)
def test_body(engines, body, dtype):
    dict(ss.jobs(engines[dtype]))[body]()
    RAN[ss.ES[dtype]].add(body)


@pytest.mark.parametrize("dtype", ss.DTYPES, ids=IDS)
def test_every_reachable_instantiation_was_launched_in_a_slab(engines, dtype):
    """as tests/test_dispatch_gpu.py for K1-K5: the names are the description's, so a new SL, PD or WT instantiation cannot ship
    without a launch here (bodies that have not run in this process, e.g. deselected, run now)"""
    for body, job in ss.jobs(engines[dtype]):
        if body not in RAN[ss.ES[dtype]]:
            job()
    ss.check_coverage(engines[dtype])
