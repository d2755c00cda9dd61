"""K8 on the GPU: spc_point_in_polygon_f64 / spc_haversine_f64 and sputils.get_mask_indices (splib/sputils.py:46-73).

Location codes are compared bit for bit with the exact oracle of tests/geo_ref.py (itself checked against a pure-Fraction
brute force on the CPU, test_geometry_cpu.py); get_mask_indices element for element, in order, with the reference loop
restated over that oracle.  The bodies that tools/mutation_control.py --geo also runs on its mutant libraries live in
tests/geo_edges.py."""
import numpy
import pytest
import torch

from sp_coupler_amd import geometry
from tests import geo_edges, geo_ref

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def eng():
    from sp_coupler_amd.engine import Engine
    return Engine("cuda:0")


@pytest.fixture(params=[torch.float64, torch.float32], ids=["f64", "f32"])
def su(request):
    from sp_coupler_amd import spcpl, sputils
    from sp_coupler_amd.engine import Engine
    spcpl.set_engine(Engine("cuda:0", dtype=request.param))
    yield sputils
    spcpl.set_engine(None)


@pytest.mark.parametrize("case", geo_ref.adversarial(), ids=lambda c: c[0])
def test_adversarial_codes_equal_exact_oracle(eng, case):
    geo_edges.check_adversarial(eng, case[0])


def test_exact_path_decides_where_the_naive_determinant_is_wrong(eng):
    geo_edges.check_naive_flips(eng)


def test_scale_reduced_gaussian_against_star_polygon(eng):
    geo_edges.check_scale(eng)


def test_haversine_matches_reference_formula(eng):
    geo_edges.check_haversine(eng)


def test_exact_stage_decides_by_the_tails_of_its_differences(eng):
    """orientations that only the tail x head and tail x tail products of the exact stage get right, one of them collinear"""
    geo_edges.check_exact_tails(eng)


def test_rings_whose_edges_end_on_the_lds_tile(eng):
    """rings of 1024, 1025, 2048, 2049 edges, as shells and as holes: the seam vertex, the edges on either side of it, a
    last tile of one edge"""
    geo_edges.check_tile_seams(eng)


def test_image_longitude_at_and_next_to_the_multiples_of_180(eng):
    geo_edges.check_image_lon(eng)


@pytest.mark.parametrize("n", geo_edges.POINT_COUNTS)
def test_point_counts_around_the_workgroup_size(eng, n):
    """two polygons in one launch, a polygon id that comes back; nothing behind the output is written"""
    geo_edges.check_point_counts(eng, (n,))


def test_non_finite_points_are_exterior(eng):
    """NaN / +-inf in lon or lat: exterior of every polygon as p and as q, never selected through an area mask"""
    geo_edges.check_non_finite_points(eng)


def _expected(points, masks, nmax):
    pts = numpy.asarray(points, dtype=numpy.float64).reshape(-1, 2)
    keyed, areas = [], {}
    for k, g in enumerate(masks):
        m = geometry.as_mask(g)
        if isinstance(m, geometry.Point):
            keyed.append(("point", m.x, m.y))
        else:
            areas[k] = geo_ref.contains(geo_ref.locations(pts[:, 0], pts[:, 1], *geometry.pack(*m)))
            keyed.append(("area", k))
    return geo_ref.reference_mask_indices(list(map(tuple, pts)), keyed, nmax, lambda k: (areas[k][:, 0], areas[k][:, 1]),
                                          lambda x, y: geo_ref.haversine(pts[:, 0], pts[:, 1], x, y))


def _grid():
    lon, lat = numpy.meshgrid(numpy.arange(0.0, 360.0, 2.5), numpy.arange(-80.0, 81.0, 2.5))
    return list(zip(lon.ravel().tolist(), lat.ravel().tolist()))


MASKS = {
    "polygon_whole_degrees": [geometry.Polygon([(-30, -20), (10, -20), (10, 25), (-30, 25)])],
    "polygon_with_hole": [geometry.Polygon([(100, -40), (160, -40), (160, 40), (100, 40)], [[(120, -10), (140, -10), (140, 10), (120, 10)]])],
    "mixed": [geometry.Point((12.0, 31.0)), geometry.shape({"type": "Polygon", "coordinates": [[[-60, 0], [-20, 0], [-40, 30], [-60, 0]]]}),
              geometry.Point((200.0, -41.0)), geometry.box(100, 0, 130, 30)],
    "multipolygon": [geometry.shape({"type": "MultiPolygon", "coordinates": [[[[0, -10], [20, -10], [20, 10], [0, 10], [0, -10]]],
                                                                             [[[20, -10], [40, -10], [40, 10], [20, 10], [20, -10]]]]})],
    "all": [geometry.box(-INF, -INF, INF, INF)],
    "empty": [],
}


@pytest.mark.parametrize("name", sorted(MASKS))
@pytest.mark.parametrize("form", ["tuples", "array", "device"])
def test_get_mask_indices_equals_reference_loop(su, name, form):
    pts = _grid()
    arg = pts if form == "tuples" else numpy.asarray(pts) if form == "array" else torch.tensor(pts, dtype=torch.float64, device="cuda:0")
    got = su.get_mask_indices(arg, MASKS[name])
    want = _expected(pts, MASKS[name], -1)
    assert got == want and all(type(i) is int for i in got)
    if name == "all":
        assert sorted(got) == list(range(len(pts)))


@pytest.mark.parametrize("form", ["tuples", "device"])
def test_get_mask_indices_single_point_nmax(su, form):
    pts = _grid() + [(42.5, 10.0), (42.5, 10.0)]                        # exact duplicates of a grid point
    arg = pts if form == "tuples" else torch.tensor(pts, dtype=torch.float64, device="cuda:0")
    p = [geometry.Point((42.4, 10.1))]
    assert su.get_mask_indices(arg, p, nmax=0) == []
    first = su.get_mask_indices(arg, p)
    assert first == _expected(pts, p, -1) and first[0] < len(pts) - 2          # the lowest of the equal indices
    for nmax in (1, 5, len(pts) + 10):
        got = su.get_mask_indices(arg, p, nmax=nmax)
        got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
        assert got.dtype == numpy.int64 and got.tolist() == list(_expected(pts, p, nmax))
    dup = su.get_mask_indices(arg, [geometry.Point((42.5, 10.0))], nmax=3)
    dup = dup.cpu().numpy() if isinstance(dup, torch.Tensor) else dup
    assert dup.tolist() == sorted(dup.tolist())                               # stable among exactly equal distances


def test_reference_fixture_closest_point(su):
    """splib/test/sputils_test.py:42-45, restated with one Point as the mask"""
    points = [(52.314970, 4.824198), (52.379932, 4.897997), (52.387264, 5.082968), (52.278097, 5.021635)]
    target = (52.356591, 4.954541)
    assert su.get_mask_indices(points, [geometry.Point(target)], nmax=4)[0] == 1
    assert su.get_mask_indices(points, [geometry.Point(target)]) == [1]
