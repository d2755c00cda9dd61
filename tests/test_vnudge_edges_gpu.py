"""K6 at the edges of its kernels: the bodies of tests/vnudge_edges.py on the shipped library, one case per body and dtype
(tests/test_vnudge_edges_cpu.py states on the CPU that the inputs reach what the bodies claim; tools/mutation_control.py
--vnudge runs the same bodies on the mutant libraries, profiles/mutation_control_vnudge.log)."""
import pytest

from tests import vnudge_edges as ve


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ve.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("body", ve.BODIES)
def test_vnudge_edge_body(body, dtype):
    from sp_coupler_amd.engine import Engine
    getattr(ve, "check_" + body)(Engine("cuda:0", dtype=dtype))
