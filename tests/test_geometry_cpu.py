"""CPU tests of the K8 geometry (sputils.get_mask_indices): the shapely stand-ins of sp_coupler_amd.geometry, the test
oracle against its exact brute force, the C ABI of spc_point_in_polygon_f64 / spc_haversine_f64 (layout, symbols,
argument checks), and the assembly of get_mask_indices (splib/sputils.py:50-73) driven through a CPU stand-in engine that
computes with the oracle.  The kernels themselves are checked on the GPU (test_geo_gpu.py)."""
import ctypes
import math
import os
import subprocess
from types import SimpleNamespace

import numpy
import pytest
import torch

import __graft_entry__ as ge
from sp_coupler_amd import _abi, geometry
from tests import geo_edges, geo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


# ---- sp_coupler_amd.geometry ----------------------------------------------------------------------
def test_point_forms():
    assert (geometry.Point((3.5, -2)).x, geometry.Point((3.5, -2)).y) == (3.5, -2.0)
    assert (geometry.Point(1, 2).x, geometry.Point(1, 2).y) == (1.0, 2.0)
    with pytest.raises(ValueError):
        geometry.Point((float("nan"), 0))
    with pytest.raises(ValueError):
        geometry.Point((INF, 0))


def test_polygon_closes_rings_and_keeps_holes():
    p = geometry.Polygon([(0, 0), (4, 0), (4, 4)], holes=[[(1, 1), (2, 1), (2, 2)]])
    assert p.exterior.coords == [(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 0.0)]
    assert p.interiors[0].coords[-1] == (1.0, 1.0) and len(p.interiors[0].coords) == 4
    closed = geometry.Polygon([(0, 0), (4, 0), (4, 4), (0, 0)])
    assert len(closed.exterior.coords) == 4                     # an already closed ring is not closed twice


@pytest.mark.parametrize("ring", [[(0, 0), (1, 1)], [(0, 0), (1, 1), (0, 0), (1, 1)], [(0, 0), (float("nan"), 1), (1, 0)]])
def test_polygon_rejects_degenerate_and_nan_rings(ring):
    with pytest.raises(ValueError):
        geometry.Polygon(ring)


def test_non_finite_only_in_a_rectangle():
    b = geometry.box(-INF, -INF, INF, INF)
    assert b.exterior.coords == [(INF, -INF), (INF, INF), (-INF, INF), (-INF, -INF), (INF, -INF)]
    with pytest.raises(ValueError):
        geometry.Polygon([(0, 0), (INF, 0), (0, 5)])
    with pytest.raises(ValueError):                               # a rectangle inside a MultiPolygon takes the ray rule
        geometry.pack(*geometry.as_mask(geometry.MultiPolygon([b, geometry.box(0, 0, 1, 1)])))


def test_is_rectangle_is_geos_rule():
    assert geometry.is_rectangle(geometry.box(0, 0, 2, 1).exterior.xy_array)
    assert geometry.is_rectangle(geometry.box(0, 0, 2, 1, ccw=False).exterior.xy_array)
    assert not geometry.is_rectangle(geometry.Polygon([(0, 0), (2, 0), (2, 1), (0, 1), (0, 0.5)]).exterior.xy_array)
    assert not geometry.is_rectangle(geometry.Polygon([(0, 0), (2, 1), (2, 0), (0, 1)]).exterior.xy_array)   # bow tie
    assert not geometry.is_rectangle(geometry.box(0, 0, 2, 1).exterior.xy_array, [numpy.zeros((4, 2))])


def test_shape_reads_geojson():
    pt = geometry.shape({"type": "Point", "coordinates": [4.9, 52.3]})
    assert (pt.x, pt.y) == (4.9, 52.3)
    poly = geometry.shape({"type": "Polygon", "coordinates": [[[0, 0], [3, 0], [3, 3], [0, 3], [0, 0]],
                                                              [[1, 1], [2, 1], [2, 2], [1, 1]]]})
    assert poly.geom_type == "Polygon" and len(poly.interiors) == 1
    mp = geometry.shape({"type": "MultiPolygon", "coordinates": [[[[0, 0], [1, 0], [1, 1], [0, 0]]], [[[5, 5], [6, 5], [6, 6], [5, 5]]]]})
    assert mp.geom_type == "MultiPolygon" and len(mp.geoms) == 2
    assert geometry.shape(poly).geom_type == "Polygon"            # __geo_interface__ round trip
    with pytest.raises(ValueError):
        geometry.shape({"type": "LineString", "coordinates": [[0, 0], [1, 1]]})


def _duck_polygon(shell, holes=()):
    ring = lambda c: SimpleNamespace(coords=list(c) + [c[0]])          # noqa: E731  (shapely: closed coordinate sequences)
    return SimpleNamespace(geom_type="Polygon", exterior=ring(shell), interiors=[ring(h) for h in holes])


def test_duck_typed_shapely_objects():
    assert isinstance(geometry.as_mask(SimpleNamespace(geom_type="Point", x=1.0, y=2.0)), geometry.Point)
    polys, single = geometry.as_mask(_duck_polygon([(0, 0), (3, 0), (3, 3)], [[(1, 1), (2, 1), (1, 2)]]))
    assert single and len(polys) == 1 and len(polys[0].interiors) == 1
    mp = SimpleNamespace(geom_type="MultiPolygon", geoms=[_duck_polygon([(0, 0), (1, 0), (1, 1)]), _duck_polygon([(5, 5), (6, 5), (6, 6)])])
    polys, single = geometry.as_mask(mp)
    assert not single and len(polys) == 2
    with pytest.raises(ValueError):
        geometry.as_mask(SimpleNamespace(geom_type="LineString"))


def test_pack_layout():
    vx, vy, start, role, poly, n = geometry.pack(*geometry.as_mask(geometry.Polygon([(0, 0), (4, 0), (4, 4), (0, 4)], [[(1, 1), (2, 1), (2, 2)]])))
    assert start.tolist() == [0, 5, 9] and role.tolist() == [geometry.SHELL, geometry.HOLE] and poly.tolist() == [0, 0] and n == 1
    assert (vx[0], vy[0]) == (vx[4], vy[4])
    _, _, _, role, _, _ = geometry.pack(*geometry.as_mask(geometry.box(0, 0, 1, 1)))
    assert role.tolist() == [geometry.RECTANGLE]


# ---- the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", geo_ref.adversarial(), ids=lambda c: c[0])
def test_numpy_oracle_equals_fraction_brute_force(case):
    name, lon, lat, lay = case
    assert numpy.array_equal(geo_ref.locations(lon, lat, *lay), geo_ref.brute_locations(lon, lat, *lay)), name


def test_adversarial_set_covers_the_rules():
    cases = {c[0]: c for c in geo_ref.adversarial()}
    # the naive double determinant is wrong for these points, and that changes a decision
    a, b = (0.5, 0.5), (17.3, 24.25)
    pts = geo_ref.naive_flips(a, b)
    assert any(geo_ref.naive_sign(*a, *b, x, y) == -geo_ref._orient_fraction(*a, *b, x, y) for x, y in pts)
    codes = geo_ref.locations(*cases["naive_determinant_wrong"][1:3], *cases["naive_determinant_wrong"][3])
    assert set(numpy.unique(codes)) == {geo_ref.EXT, geo_ref.INT}
    # Mod-2: the shared edge of two squares (both components' boundary: even) is interior, a point on one component's
    # boundary only (odd) is not -- also at the shared edge's end vertices, which GEOS's Mod-2 rule counts twice
    name, lon, lat, lay = cases["multipolygon_shared_edge"]
    inside = geo_ref.contains(geo_ref.locations(lon, lat, *lay))[:, 0]
    at = lambda x, y: inside[numpy.flatnonzero((lon == x) & (lat == y))[0]]     # noqa: E731
    assert at(0.0, 0.0) and at(0.0, 1.5) and at(0.0, 3.0) and not at(1.5, 3.0) and not at(-6.0, 0.0) and at(-3.0, 0.0)
    # the image: points 330 ... 350 E fall in the polygon drawn at -30 ... -10
    name, lon, lat, lay = cases["antimeridian_image"]
    inside = geo_ref.contains(geo_ref.locations(lon, lat, *lay))
    assert not inside[:, 0].any() and inside[:, 1].any() and set(lon[inside[:, 1]]) == set(numpy.arange(332.5, 350.0, 2.5))
    assert geo_ref.contains(geo_ref.locations(*cases["infinite_box"][1:3], *cases["infinite_box"][3])).all()


# ---- the inputs of tests/geo_edges.py: the oracle pinned by the brute force, and what they were built to hold --------------
def _brute_equals(lon, lat, lay, want, pick):
    pick = numpy.asarray(pick)
    assert numpy.array_equal(geo_ref.brute_locations(lon[pick], lat[pick], *lay), want[:, pick, :])


def test_exact_tails_case_conditions_and_oracle():
    a, b, apex, pts, exact, head, tails = geo_edges.exact_tails_case()
    deciding = tails & (exact != 0) & (head != exact)
    assert deciding.sum() >= 32                                   # the sign of the head-only expansion is wrong there
    col = numpy.flatnonzero(tails & (exact == 0))
    assert len(col) >= 1 and (head[col] != 0).all()               # exactly collinear, and the head-only expansion denies it
    assert all(not geo_edges.filter_decides(*a, *b, x, y) for x, y in pts)
    want = geo_edges.exact_tails_want()
    assert numpy.array_equal(want[0, :, 0] == geo_ref.INT, exact > 0) and numpy.array_equal(want[0, :, 0] == geo_ref.BND, exact == 0)
    lay = geo_ref.layout([geo_ref.rings_of([a, b, apex, a])])
    _brute_equals(pts[:, 0], pts[:, 1], lay, want, list(range(0, len(pts), 7)) + col.tolist())
    print(geo_edges.exact_tails_counts())


def test_tile_seam_rings_and_points():
    for edges in geo_edges.SEAM_EDGES:
        ring, of_edge = geo_edges.seam_ring(edges)
        assert len(ring) == edges + 1 and (ring[0] == ring[-1]).all() and (ring * 2 == numpy.round(ring * 2)).all()
        assert len({tuple(v) for v in ring[:-1]}) == edges      # no repeated vertex
        assert of_edge[-geo_edges.SEAM_START:] == list(range(geo_edges.SEAM_START))     # the last ring edges are chain edges
        for s in range(geo_edges.TILE, edges, geo_edges.TILE):   # the edges on both sides of a seam are chain edges
            assert of_edge[s - 1] >= 0 and of_edge[s] >= 0
    assert geo_edges.seam_ring(1025)[1][1024] == 3 and geo_edges.seam_ring(2049)[1][2048] == 3   # the one-edge last tiles
    lon, lat, lay, want = geo_edges.tile_seams_case()
    assert 250 <= len(lon) <= 350 and lay[5] == 8
    assert (numpy.diff(lay[2])[[0, 1, 2, 3]] == numpy.array(geo_edges.SEAM_EDGES) + 1).all()
    for k, edges in enumerate(geo_edges.SEAM_EDGES):
        ring, of_edge = geo_edges.seam_ring(edges)
        at = lambda x, y: want[k, numpy.flatnonzero((lon == x) & (lat == y))[0], 0]       # noqa: E731
        for r in [s + d for s in range(geo_edges.TILE, edges + 1, geo_edges.TILE) for d in (-1, 0)] + [edges - 1]:
            if r < edges:
                y = 0.5 * of_edge[r] + 0.25
                # inside: the ray crosses ring edge r only; left of the ring: the left side and edge r; right: nothing
                assert (at(50.0, y), at(-5.0, y), at(150.0, y)) == (geo_ref.INT, geo_ref.EXT, geo_ref.EXT), (edges, r)
                assert at(*((ring[r] + ring[r + 1]) / 2)) == geo_ref.BND
        for s in range(geo_edges.TILE, edges, geo_edges.TILE):
            assert at(*ring[s]) == geo_ref.BND                    # the seam vertex
        # as the hole of the square: interior and exterior change places, the boundary stays
        swap = numpy.array([geo_ref.INT, geo_ref.BND, geo_ref.EXT])
        inside_square = (lon > -100) & (lon < 2000) & (lat > -100) & (lat < 2000)
        assert inside_square.all() and numpy.array_equal(want[4 + k], swap[want[k]])
    _brute_equals(lon, lat, lay, want, range(0, len(lon), 23))


def test_image_lon_case():
    for lon in geo_edges.IMAGE_LONS:
        assert float(geo_ref.image_lon(lon)) == (lon - 180) % 360 - 180
        assert -180.0 <= float(geo_ref.image_lon(lon)) <= 180.0
    assert len(geo_edges.IMAGE_LONS) == 15
    lon, lat, lay, want = geo_edges.image_lon_case()
    _brute_equals(lon, lat, lay, want, range(len(lon)))
    at = lambda k, x, img: want[k, numpy.flatnonzero((lon == x) & (lat == 0.0))[0], img]      # noqa: E731
    up, down = math.nextafter(180.0, INF), math.nextafter(180.0, -INF)
    assert (at(2, up, 1), at(2, 180.0, 1), at(2, down, 1)) == (geo_ref.INT, geo_ref.BND, geo_ref.EXT)   # the strip -180 ... -170
    assert at(0, 720.5, 1) == geo_ref.INT and at(0, 720.5, 0) == geo_ref.EXT and at(1, 360.0, 0) == geo_ref.BND
    assert set(numpy.unique(want)) == {geo_ref.EXT, geo_ref.BND, geo_ref.INT}


def test_point_counts_case():
    for n in geo_edges.POINT_COUNTS:
        lon, lat, two, want_two, inter, want_inter = geo_edges.point_counts_case(n)
        assert len(lon) == n and want_two.shape == want_inter.shape == (2, n, 2)
        pick = range(0, n, max(1, n // 12))
        _brute_equals(lon, lat, two, want_two, pick)
        _brute_equals(lon, lat, inter, want_inter, pick)
        assert inter[4].tolist() == [0, 1, 0]
        # row 0 of the interleaved layout is the square that came back under id 0, not the triangle
        sq = geo_ref.locations(lon, lat, *geo_ref.layout([geo_ref.rings_of([(-5, -5), (5, -5), (5, 5), (-5, 5), (-5, -5)])]))
        assert numpy.array_equal(want_inter[0], sq[0]) and want_two[1, -1, 0] == geo_ref.BND
    assert not numpy.array_equal(want_inter[0], want_two[0])


def test_non_finite_points_are_exterior_in_the_oracle():
    lon, lat, finite, cases = geo_edges.non_finite_case()
    assert (~finite).sum() == 18 and finite.sum() >= 5
    for name, lay, want in cases:
        assert (want[:, ~finite, :] == geo_ref.EXT).all(), name
        assert numpy.array_equal(geo_ref.brute_locations(lon, lat, *lay), want), name
        assert not geo_ref.contains(want)[~finite].any()
        assert geo_ref.contains(want)[finite].any()
    assert geo_ref.contains(dict((c[0], c[2]) for c in cases)["infinite_box"])[finite].all()
    # two parts of a MultiPolygon span latitude 0: were a NaN longitude "collinear" with an edge of each, the point would
    # be on two boundaries and GEOS's mod-2 rule would call it contained
    assert geo_ref.contains(numpy.full((2, 1, 2), geo_ref.BND)).all()


def test_non_finite_points_never_selected_through_the_stand_in_engine(su):
    lon, lat, finite, cases = geo_edges.non_finite_case()
    points = list(zip(lon.tolist(), lat.tolist()))
    for name, g in geo_edges.non_finite_masks().items():
        sel = su.get_mask_indices(points, [g])
        assert sel and all(finite[i] for i in sel), (name, sel)


# ---- the C ABI ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    return _abi.load_library()


def test_pip_struct_layout_matches_c_compiler(tmp_path):
    fields = ["n_points", "n_vertices", "n_rings", "n_polys", "lon", "lat", "vx", "vy", "ring_start", "ring_role", "ring_poly", "out"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spc.h"', 'int main(void){',
             'printf("%zu\\n", sizeof(spc_pip_args));'] + ['printf("%%zu\\n", offsetof(spc_pip_args, %s));' % f for f in fields]
    lines += ['printf("%d %d %d %d %d %d\\n", SPC_RING_SHELL, SPC_RING_HOLE, SPC_RING_RECTANGLE, SPC_LOC_EXTERIOR, SPC_LOC_BOUNDARY, SPC_LOC_INTERIOR);',
              'return 0;}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_abi.PipArgs)] + [getattr(_abi.PipArgs, f).offset for f in fields]
    want += [_abi.SPC_RING_SHELL, _abi.SPC_RING_HOLE, _abi.SPC_RING_RECTANGLE, _abi.SPC_LOC_EXTERIOR, _abi.SPC_LOC_BOUNDARY, _abi.SPC_LOC_INTERIOR]
    assert got == want
    assert (geometry.SHELL, geometry.HOLE, geometry.RECTANGLE) == (_abi.SPC_RING_SHELL, _abi.SPC_RING_HOLE, _abi.SPC_RING_RECTANGLE)


def test_geometry_symbols_exported(lib):
    for name in ("spc_point_in_polygon_f64", "spc_haversine_f64"):
        assert hasattr(lib, name) and name in _abi.PROTOTYPES


def test_geometry_arguments_rejected_on_the_host(lib):
    assert lib.spc_point_in_polygon_f64(None, None) == _abi.SPC_ERR_INVALID_ARGUMENT
    a = _abi.PipArgs(-1, 0, 1, 1)
    assert lib.spc_point_in_polygon_f64(ctypes.byref(a), None) == _abi.SPC_ERR_INVALID_ARGUMENT
    assert b"negative" in lib.spc_last_error()
    a = _abi.PipArgs(10, 5, 1, 1)                                  # every pointer NULL
    assert lib.spc_point_in_polygon_f64(ctypes.byref(a), None) == _abi.SPC_ERR_INVALID_ARGUMENT
    assert b"NULL" in lib.spc_last_error()
    a = _abi.PipArgs(10, 5, 0, 1)
    assert lib.spc_point_in_polygon_f64(ctypes.byref(a), None) == _abi.SPC_ERR_INVALID_ARGUMENT
    assert lib.spc_point_in_polygon_f64(ctypes.byref(_abi.PipArgs(0, 5, 1, 1)), None) == 0          # no points: no-op
    assert lib.spc_haversine_f64(-1, None, None, 0.0, 0.0, None, None) == _abi.SPC_ERR_INVALID_ARGUMENT
    assert lib.spc_haversine_f64(4, None, None, 0.0, 0.0, None, None) == _abi.SPC_ERR_INVALID_ARGUMENT
    assert lib.spc_haversine_f64(0, None, None, 0.0, 0.0, None, None) == 0


# ---- get_mask_indices on a CPU stand-in engine ----------------------------------------------------------
class OracleGeoEngine:
    """the engine interface get_mask_indices uses, computing with tests/geo_ref.py on CPU tensors"""
    device = torch.device("cpu")

    def on_stream(self):
        import contextlib
        return contextlib.nullcontext()

    def point_in_polygon(self, lon, lat, vx, vy, ring_start, ring_role, ring_poly, n_polys=None):
        return torch.from_numpy(geo_ref.locations(lon.numpy(), lat.numpy(), numpy.asarray(vx), numpy.asarray(vy), numpy.asarray(ring_start),
                                                  numpy.asarray(ring_role), numpy.asarray(ring_poly), n_polys))

    def haversine(self, lon, lat, lon0, lat0):
        return torch.from_numpy(geo_ref.haversine(lon.numpy(), lat.numpy(), lon0, lat0))


@pytest.fixture()
def su():
    from sp_coupler_amd import spcpl, sputils
    spcpl.set_engine(OracleGeoEngine())
    yield sputils
    spcpl.set_engine(None)


def _grid():
    lon, lat = numpy.meshgrid(numpy.arange(0.0, 360.0, 5.0), numpy.arange(-60.0, 61.0, 5.0))
    return list(zip(lon.ravel().tolist(), lat.ravel().tolist()))


def _expected(points, masks, nmax):
    """the reference loop over tests/geo_ref.py: masks as geometry objects"""
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


def test_assembly_mixed_masks_in_reference_order(su):
    pts = _grid()
    masks = [geometry.Point((12.0, 31.0)), geometry.Polygon([(-40, -20), (-5, -20), (-5, 25), (-40, 25)]),
             geometry.Point((200.0, -41.0)), geometry.box(100, 0, 130, 30)]
    got = su.get_mask_indices(pts, masks)
    want = _expected(pts, masks, -1)
    assert got == want and all(type(i) is int for i in got)
    assert su.get_mask_indices(pts, masks, nmax=3) == want          # nmax is ignored with several geometries (reference)


def test_assembly_nmax_and_empty(su):
    pts = _grid()
    p = [geometry.Point((42.0, 10.5))]
    assert su.get_mask_indices(pts, p, nmax=0) == []
    assert su.get_mask_indices(pts, [], nmax=5) == []
    assert su.get_mask_indices(pts, p) == _expected(pts, p, -1)
    assert su.get_mask_indices(pts, p, nmax=-3) == _expected(pts, p, -1)
    got = su.get_mask_indices(pts, p, nmax=7)
    assert isinstance(got, numpy.ndarray) and got.dtype == numpy.int64 and got.tolist() == list(_expected(pts, p, 7))
    assert len(su.get_mask_indices(pts, p, nmax=10 ** 6)) == len(pts)
    assert su.get_mask_indices(numpy.asarray(pts), [geometry.box(-INF, -INF, INF, INF)]) == list(range(len(pts)))


def test_assembly_stable_among_equal_distances(su):
    pts = [(10.0, 5.0), (3.0, 3.0), (10.0, 5.0), (3.0, 3.0), (10.0, 5.0)]
    assert su.get_mask_indices(pts, [geometry.Point((3.0, 3.0))]) == [1]
    assert su.get_mask_indices(pts, [geometry.Point((3.0, 3.0))], nmax=4).tolist() == [1, 3, 0, 2]


def test_reference_fixture_closest_point(su):
    """splib/test/sputils_test.py:42-45 (find_closest_points(points, target)[0] == 1), restated with one Point mask"""
    points = [(52.314970, 4.824198), (52.379932, 4.897997), (52.387264, 5.082968), (52.278097, 5.021635)]
    target = (52.356591, 4.954541)
    assert su.get_mask_indices(points, [geometry.Point(target)], nmax=1)[0] == 1
    assert su.get_mask_indices(points, [geometry.Point(target)]) == [1]
    assert su.find_closest_points(points, target)[0] == 1


def test_empty_points_with_a_point_mask(su):
    with pytest.raises(ValueError):
        su.get_mask_indices([], [geometry.Point((0, 0))])
    assert su.get_mask_indices([], [geometry.box(0, 0, 1, 1)]) == []


def test_haversine_oracle_is_the_reference_formula():
    lon, lat = numpy.array([4.8, 170.0, -33.3]), numpy.array([52.3, -10.0, 80.0])
    for i in range(3):
        lng1, lat1, lng2, lat2 = map(math.radians, (lon[i], lat[i], 5.0, 51.0))
        d = math.sin((lat2 - lat1) * 0.5) ** 2 + math.cos(lat1) * math.cos(lat2) * math.sin((lng2 - lng1) * 0.5) ** 2
        assert abs(geo_ref.haversine(lon[i:i + 1], lat[i:i + 1], 5.0, 51.0)[0] - 2 * 6371 * math.asin(math.sqrt(d))) <= 1e-12 * 6371
