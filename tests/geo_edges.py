"""K8 at the edges of its kernels (sp_coupler_amd/csrc/spc_geo.hpp): the inputs as NumPy arrays, built and checked on the CPU
(tests/test_geometry_cpu.py pins the oracle's answer to each of them with the Fraction brute force and states the conditions
the inputs were built to meet), and the bodies of the GPU tests, each taking an engine (tests/test_geo_gpu.py hands them
Engine("cuda:0"); tools/mutation_control.py hands them the engines of its mutant libraries).  Every comparison of location
codes asks for equal bytes against geo_ref.locations.  Inputs and oracle answers are computed once per process."""
import functools
import math
from fractions import Fraction

import numpy
import torch

from tests import geo_ref
from tests.les_harness import run_bodies

INF, NAN = float("inf"), float("nan")
TILE = 1024                      # GEO_TILE of spc_geo.hpp: edges per LDS tile


def codes(eng, lon, lat, lay):
    """the engine's [n_polys x n x 2] uint8 codes as a NumPy array"""
    return eng.point_in_polygon(torch.from_numpy(numpy.ascontiguousarray(lon, dtype=numpy.float64)).to(eng.device),
                                torch.from_numpy(numpy.ascontiguousarray(lat, dtype=numpy.float64)).to(eng.device), *lay).cpu().numpy()


def _same(name, got, want):
    assert got.dtype == numpy.uint8 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    assert numpy.array_equal(got, want), "%s: %d of %d codes differ, first at %s" % (
        name, (got != want).sum(), want.size, numpy.argwhere(got != want)[:4].tolist())


# ---- the bodies that tests/test_geo_gpu.py had before this module ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adversarial_cases():
    return tuple((name, lon, lat, lay, geo_ref.locations(lon, lat, *lay)) for name, lon, lat, lay in geo_ref.adversarial())


def check_adversarial(eng, name=None):
    """every case of geo_ref.adversarial() (or the one called ``name``): codes equal to the exact oracle's"""
    for cname, lon, lat, lay, want in adversarial_cases():
        if name is None or cname == name:
            got = codes(eng, lon, lat, lay)
            assert got.dtype == numpy.uint8 and got.shape == (lay[5], len(lon), 2)
            assert numpy.array_equal(got, want), "%s: %d of %d codes differ" % (cname, (got != want).sum(), want.size)


@functools.lru_cache(maxsize=None)
def naive_flips_case():
    a, b = (0.5, 0.5), (17.3, 24.25)
    pts = numpy.array(geo_ref.naive_flips(a, b))
    naive = numpy.array([geo_ref.naive_sign(*a, *b, x, y) for x, y in pts])
    exact = numpy.array([geo_ref._orient_fraction(*a, *b, x, y) for x, y in pts])
    return a, b, pts, naive, exact


def check_naive_flips(eng):
    """points a few ulps off a long edge where the plain double determinant has the wrong sign: the exact stage decides"""
    a, b, pts, naive, exact = naive_flips_case()
    assert (naive == -exact).any() and (naive != exact).all()
    lay = geo_ref.layout([geo_ref.rings_of([a, b, (-20.0, 30.0), a])])
    got = codes(eng, pts[:, 0], pts[:, 1], lay)[0, :, 0]
    # the point is inside the triangle exactly when it is left of a -> b (the triangle is counter-clockwise)
    assert numpy.array_equal(got == geo_ref.INT, exact > 0) and not (got == geo_ref.BND).any()


@functools.lru_cache(maxsize=None)
def haversine_case():
    rng = numpy.random.default_rng(7)
    lon, lat = rng.uniform(0, 360, 200_000), rng.uniform(-90, 90, 200_000)
    targets = ((4.9, 52.3), (-120.0, -45.0), (179.5, 0.0))
    return lon, lat, tuple((lon0, lat0, geo_ref.haversine(lon, lat, lon0, lat0)) for lon0, lat0 in targets)


def check_haversine(eng):
    lon, lat, targets = haversine_case()
    for lon0, lat0, want in targets:
        keep = want < numpy.pi * 6371 - 111.0                              # more than ~1 degree from the antipode
        got = eng.haversine(torch.from_numpy(lon).to(eng.device), torch.from_numpy(lat).to(eng.device), lon0, lat0).cpu().numpy()
        rel = numpy.abs(got - want)[keep] / numpy.maximum(want[keep], 1e-300)
        assert rel.max() <= 1e-12, rel.max()


@functools.lru_cache(maxsize=None)
def scale_case():
    lon, lat = geo_ref.reduced_gaussian(1 << 20)
    ring = geo_ref.star(4096)
    lay = geo_ref.layout([geo_ref.rings_of(ring)])
    return lon, lat, ring, lay, geo_ref.locations(lon, lat, *lay)


def check_scale(eng):
    """2^20 reduced-Gaussian points against a star of about 4 000 vertices (the size test of tests/test_geo_gpu.py)"""
    lon, lat, ring, lay, want = scale_case()
    assert len(lon) == 1 << 20
    assert len(ring) >= 4000
    got = codes(eng, lon, lat, lay)
    assert numpy.array_equal(got, want), "%d of %d codes differ" % ((got != want).sum(), want.size)
    counts = numpy.bincount(want.ravel(), minlength=3)
    assert counts[geo_ref.INT] > 1000 and counts[geo_ref.BND] > 0


# ---- exact_tails: the low-order half of the exact orientation -----------------------------------------------------------------
def two_diff_tail(a, b):
    """the part of a - b that the rounded difference loses (exact)"""
    return Fraction(a) - Fraction(b) - Fraction(a - b)


def head_only_sign(ax, ay, bx, by, cx, cy):
    """sign of the determinant of the four ROUNDED differences, multiplied out exactly: what the exact stage gives when the
    tails of its TwoDiff are lost"""
    d = Fraction(ax - cx) * Fraction(by - cy) - Fraction(ay - cy) * Fraction(bx - cx)
    return int(d > 0) - int(d < 0)


def filter_decides(ax, ay, bx, by, cx, cy):
    """whether Shewchuk's filter settles the sign from the plain double determinant; Python's floats round
    every operation once, as the kernel's build does (no contraction)"""
    detleft, detright = (ax - cx) * (by - cy), (ay - cy) * (bx - cx)
    det = detleft - detright
    if detleft > 0.0:
        if detright <= 0.0:
            return True
        detsum = detleft + detright
    elif detleft < 0.0:
        if detright >= 0.0:
            return True
        detsum = -detleft - detright
    else:
        return True
    return abs(det) >= 3.3306690738754716e-16 * detsum


def _step(x, k):
    for _ in range(abs(k)):
        x = math.nextafter(x, math.copysign(INF, k))
    return x


@functools.lru_cache(maxsize=None)
def exact_tails_case():
    """(a, b, apex, points, exact signs, head-only signs, tails-non-zero) for the edge a -> b of the counter-clockwise triangle
    a, b, apex.  a and b are near (-300, -250) and (300, 250), multiples of 2^-44; c0 near (2^-10, 2^-10) is EXACTLY on the
    line a-b and has bits down to 2^-60, so a - c0 and b - c0 are not doubles: with t = (2^15 + 1) / 2^16, c0 = a + t (b - a)
    in integers of 2^-60, b - a = 2^16 n with n odd, a = c0 - (2^15 + 1) n.  The points are c0 and the doubles up to 8 steps
    of nextafter from it in x and in y: their true determinants are about 2^-62 * 600, far below the 2^-46 * 300 that the
    lost tails amount to, so the head-only expansion gives ONE sign for all of them (or zero)."""
    unit, Q, p = Fraction(1, 2 ** 60), 2 ** 16, 2 ** 15 + 1

    def axis(extent):
        n = int(extent * 2 ** 60) // Q | 1                     # b - a = Q n units, n odd
        A = (p * n - 2 ** 50) // Q                             # a = -A Q units, so that c0 = p n - A Q = 2^50 + (a remainder < 2^16)
        c = p * n - A * Q
        assert c % 2 == 1                                      # odd x odd minus even: c0 has the bit 2^-60
        return -A * Q * unit, (n - A) * Q * unit, c * unit

    ax, bx, cx = axis(600)
    ay, by, cy = axis(500)
    for v in (ax, bx, cx, ay, by, cy):
        assert Fraction(float(v)) == v, v                      # every coordinate is a double
    assert (cx - ax) * (by - ay) == (cy - ay) * (bx - ax)      # c0 is on the line, exactly
    a, b, c0 = (float(ax), float(ay)), (float(bx), float(by)), (float(cx), float(cy))
    apex = (-400.0, 300.0)
    pts = [(_step(c0[0], kx), _step(c0[1], ky)) for kx in range(-8, 9) for ky in range(-8, 9)]
    exact = numpy.array([geo_ref._orient_fraction(*a, *b, x, y) for x, y in pts])
    head = numpy.array([head_only_sign(*a, *b, x, y) for x, y in pts])
    tails = numpy.array([any(two_diff_tail(u, v) != 0 for u, v in ((a[0], x), (b[1], y), (a[1], y), (b[0], x))) for x, y in pts])
    reach = numpy.array([not filter_decides(*a, *b, x, y) for x, y in pts])
    assert reach.all()                                          # every orientation against a -> b reaches the exact stage
    return a, b, apex, numpy.array(pts), exact, head, tails


def exact_tails_counts():
    a, b, apex, pts, exact, head, tails = exact_tails_case()
    deciding = tails & (exact != 0) & (head != exact)
    return ("%d points reach the exact stage of edge a -> b with a non-zero TwoDiff tail; at %d of them the sign of the head-only "
            "expansion differs from the exact sign (%d of these with the opposite sign); %d exactly collinear with a non-zero "
            "tail (head-only sign there: %s)" % (tails.sum(), deciding.sum(), (deciding & (head == -exact)).sum(),
                                                 (tails & (exact == 0)).sum(), sorted(set(head[tails & (exact == 0)].tolist()))))


def check_exact_tails(eng):
    """item 1: orientations that the tail x head and tail x tail products of the exact stage decide.  Conditions (checked here
    on the CPU before the launch): at least 32 points whose exact sign differs from the head-only sign, and an exactly
    collinear point with a non-zero tail, which must come out on the BOUNDARY."""
    a, b, apex, pts, exact, head, tails = exact_tails_case()
    assert (tails & (exact != 0) & (head != exact)).sum() >= 32
    assert (tails & (exact == 0)).sum() >= 1 and (head[tails & (exact == 0)] != 0).all()
    assert geo_ref._orient_fraction(*a, *b, *apex) > 0         # counter-clockwise: left of a -> b is the interior
    lay = geo_ref.layout([geo_ref.rings_of([a, b, apex, a])])
    got = codes(eng, pts[:, 0], pts[:, 1], lay)
    p = got[0, :, 0]
    assert numpy.array_equal(p == geo_ref.INT, exact > 0), "interior differs at %s" % numpy.flatnonzero((p == geo_ref.INT) != (exact > 0))[:8]
    assert numpy.array_equal(p == geo_ref.BND, exact == 0), "boundary differs at %s" % numpy.flatnonzero((p == geo_ref.BND) != (exact == 0))[:8]
    _same("exact_tails", got, exact_tails_want())


@functools.lru_cache(maxsize=None)
def exact_tails_want():
    a, b, apex, pts = exact_tails_case()[:4]
    return geo_ref.locations(pts[:, 0], pts[:, 1], *geo_ref.layout([geo_ref.rings_of([a, b, apex, a])]))


# ---- tile_seams: rings whose edge counts sit on the LDS tile ---------------------------------------------------------------
SEAM_EDGES = (1024, 1025, 2048, 2049)      # rings of 1025, 1026, 2049, 2050 vertices
SEAM_START = 4                             # the ring starts at chain vertex 4: its last 4 edges are the chain's first 4


def seam_ring(edges, start=SEAM_START):
    """a closed counter-clockwise ring of ``edges`` edges on half-integer vertices: a chain Q_j = (100 + (j mod 3) / 2, j / 2),
    j = 0 ... m, climbing on the right (every chain edge has a latitude band of its own: a ray from inside at latitude
    j / 2 + 1 / 4 crosses chain edge j and no other edge), closed over (0, m / 2) and (0, 0).  The ring starts at Q_start, so
    ring edge r is chain edge r + start for r < m - start, and the LAST ``start`` ring edges are chain edges 0 ... start - 1.
    Returns (ring [edges + 1 x 2], chain edge of every ring edge or -1)."""
    m = edges - 3
    chain = [(100.0 + 0.5 * (j % 3), 0.5 * j) for j in range(m + 1)]
    open_ring = chain[start:] + [(0.0, 0.5 * m), (0.0, 0.0)] + chain[:start]
    of_edge = list(range(start, m)) + [-1, -1, -1] + list(range(start))
    ring = numpy.array(open_ring + open_ring[:1])
    assert len(ring) == edges + 1 and len(of_edge) == edges
    return ring, of_edge


def seam_points(edges):
    """for the ring edges next to every tile seam, the first and the last ring edges that are chain edges: the seam vertex
    itself, and in each of these edges' latitude bands a point inside (its ray crosses this edge only), one left of the
    ring (its ray crosses the ring's left side and this edge), one right of it, and the edge's midpoint (on the boundary)"""
    ring, of_edge = seam_ring(edges)
    pts = []
    near = sorted({r for s in range(TILE, edges + 1, TILE) for r in (s - 2, s - 1, s, s + 1)} | {0, 1, edges - 3, edges - 2, edges - 1})
    for r in near:
        if 0 <= r < edges and of_edge[r] >= 0:
            y = 0.5 * of_edge[r] + 0.25
            pts += [(50.0, y), (-5.0, y), (150.0, y), tuple((ring[r] + ring[r + 1]) / 2)]
    pts += [tuple(ring[s]) for s in range(TILE, edges, TILE)]            # the seam vertices (also vertex 1024 of a 1025-edge ring)
    pts += [tuple(ring[edges - 1]), tuple(ring[0])]
    return pts


@functools.lru_cache(maxsize=None)
def tile_seams_case():
    """(lon, lat, layout, oracle codes, per-ring notes): the four rings as polygons 0 ... 3 and as the HOLE of a large square as
    polygons 4 ... 7, in one launch (so rings 1 ... also start at a vertex offset that is no multiple of the tile); the points
    of seam_points() of every ring plus a quarter-degree scatter: about 300"""
    rings = [seam_ring(e)[0] for e in SEAM_EDGES]
    square = [(-100.0, -100.0), (2000.0, -100.0), (2000.0, 2000.0), (-100.0, 2000.0), (-100.0, -100.0)]
    polys = [geo_ref.rings_of(r, poly=i) for i, r in enumerate(rings)]
    polys += [geo_ref.rings_of(square, [r], poly=len(rings) + i) for i, r in enumerate(rings)]
    lay = geo_ref.layout(polys)
    pts = [p for e in SEAM_EDGES for p in seam_points(e)]
    rng = numpy.random.default_rng(1025)
    pts += [(float(x), float(y)) for x, y in zip(rng.integers(-40, 480, 262) / 4, rng.integers(-8, 4200, 262) / 4)]
    pts = numpy.array(sorted(set(pts)))
    return pts[:, 0].copy(), pts[:, 1].copy(), lay, geo_ref.locations(pts[:, 0], pts[:, 1], *lay)


def check_tile_seams(eng):
    """item 2: rings of exactly 1024, 1025, 2048 and 2049 edges, as shells and as holes"""
    lon, lat, lay, want = tile_seams_case()
    _same("tile_seams", codes(eng, lon, lat, lay), want)


# ---- image_lon ---------------------------------------------------------------------------------------------------------------
IMAGE_LONS = (-540.0, -360.0, -180.0, math.nextafter(-180.0, -INF), math.nextafter(-180.0, INF), -0.0, 0.0, 180.0,
              math.nextafter(180.0, -INF), math.nextafter(180.0, INF), 360.0, math.nextafter(360.0, 0.0), 540.0, 720.5, 1e6 + 0.25)


@functools.lru_cache(maxsize=None)
def image_lon_case():
    """the longitudes of IMAGE_LONS at latitudes inside, on the lower edge of and above: a pentagon drawn in -180 ... 180, the
    same drawn in 0 ... 360, and a thin strip -180 ... -170 whose left edge is the image of 180 (the image of the double
    above 180 is inside it, that of the double below 180 is not)"""
    lat = numpy.repeat([0.0, -20.0, 22.5], len(IMAGE_LONS))
    lon = numpy.tile(IMAGE_LONS, 3)
    west = [(-180.0, -20.0), (180.0, -20.0), (180.0, 20.0), (0.0, 25.0), (-180.0, 20.0), (-180.0, -20.0)]
    east = [(x + 180.0, y) for x, y in west]
    strip = [(-180.0, -20.0), (-170.0, -20.0), (-170.0, 20.0), (-175.0, 21.0), (-180.0, 20.0), (-180.0, -20.0)]
    lay = geo_ref.layout([geo_ref.rings_of(west, poly=0), geo_ref.rings_of(east, poly=1), geo_ref.rings_of(strip, poly=2)])
    return lon, lat, lay, geo_ref.locations(lon, lat, *lay)


def check_image_lon(eng):
    """item 4: the image q = (lon - 180) % 360 - 180 at and next to the multiples of 180, for lon outside -180 ... 360, -0.0"""
    lon, lat, lay, want = image_lon_case()
    _same("image_lon", codes(eng, lon, lat, lay), want)


# ---- point_counts --------------------------------------------------------------------------------------------------------------
POINT_COUNTS = (1, 255, 256, 257, 513)
POISON = 0xA5C3


def raw_codes(eng, lon, lat, lay, pad=300):
    """spc_point_in_polygon_f64 through the C ABI with ``out`` the LEADING part of a buffer of POISON: returns the codes
    [n_polys x n x 2] and the ``pad`` 16-bit words behind them as the launch left them"""
    import ctypes
    from sp_coupler_amd import _abi
    vx, vy, start, role, poly, n_polys = lay
    n = len(lon)
    dev = lambda a, dt: torch.from_numpy(numpy.ascontiguousarray(a, dtype=dt)).to(eng.device)        # noqa: E731
    t = [dev(lon, numpy.float64), dev(lat, numpy.float64), dev(vx, numpy.float64), dev(vy, numpy.float64), dev(start, numpy.int64),
         dev(role, numpy.int32), dev(poly, numpy.int32)]
    buf = torch.full((n_polys * n + pad,), POISON - 65536, dtype=torch.int16, device=eng.device)
    a = _abi.PipArgs(n, len(vx), len(role), n_polys, *[x.data_ptr() for x in t], buf.data_ptr())
    torch.cuda.synchronize(eng.device)
    eng._call(eng.lib.spc_point_in_polygon_f64, ctypes.byref(a))
    eng.synchronize()
    host = buf.cpu().numpy().view(numpy.uint16)
    return host[:n_polys * n].copy().view(numpy.uint8).reshape(n_polys, n, 2), host[n_polys * n:]


@functools.lru_cache(maxsize=None)
def point_counts_case(n):
    """n points on a half-degree lattice around two polygons (a triangle with diagonal edges through lattice points, a
    square with a hole); the layouts: the two polygons, and three shells with the ids 0, 1, 0 (the square comes back under
    id 0: row 0 holds the codes of the last ring run written for it, as geo_ref.locations writes them)"""
    rng = numpy.random.default_rng(n)
    lon, lat = rng.integers(-24, 25, n) / 2.0, rng.integers(-24, 25, n) / 2.0
    lon[-1], lat[-1] = 5.0, 0.0                                   # the last point (the last live lane): on the square's edge
    tri = [(-8, -6), (8, -2), (0, 9), (-8, -6)]
    sq = [(-5, -5), (5, -5), (5, 5), (-5, 5), (-5, -5)]
    hole = [(-2, -2), (-2, 2), (2, 2), (2, -2), (-2, -2)]
    two = geo_ref.layout([geo_ref.rings_of(tri, poly=0), geo_ref.rings_of(sq, [hole], poly=1)])
    inter = geo_ref.layout([geo_ref.rings_of(tri, poly=0), geo_ref.rings_of(hole, poly=1), geo_ref.rings_of(sq, poly=0)])
    inter = inter[:5] + (2,)
    return lon, lat, two, geo_ref.locations(lon, lat, *two), inter, geo_ref.locations(lon, lat, *inter)


def check_point_counts(eng, counts=POINT_COUNTS):
    """item 5: 1, 255, 256, 257, 513 points (one lane, one short of, exactly, one more than a workgroup, two workgroups and
    one lane), two polygons in one launch; nothing behind the output is written"""
    for n in counts:
        lon, lat, two, want_two, inter, want_inter = point_counts_case(n)
        for name, lay, want in (("two polygons", two, want_two), ("ids 0, 1, 0", inter, want_inter)):
            got, tail = raw_codes(eng, lon, lat, lay)
            _same("point_counts n = %d, %s" % (n, name), got, want)
            assert (tail == POISON).all(), "n = %d, %s: %d words behind the output were written" % (n, name, (tail != POISON).sum())


# ---- non_finite_points -----------------------------------------------------------------------------------------------------------
def non_finite_points():
    """(lon, lat, finite): every pairing of NaN, +inf, -inf with a finite coordinate and with each other, between finite
    points; the finite latitude 0 is spanned by every polygon of non_finite_layouts()"""
    bad = (NAN, INF, -INF)
    pts = [(2.0, 0.0), (50.0, 0.0)]
    for v in bad:
        pts += [(v, 0.0), (3.0, 0.0), (2.0, v), (25.0, v)]
        pts += [(v, w) for w in bad]
    pts += [(25.0, 0.0), (2.5, 0.5)]
    lon, lat = numpy.array([p[0] for p in pts]), numpy.array([p[1] for p in pts])
    return lon, lat, numpy.isfinite(lon) & numpy.isfinite(lat)


def non_finite_masks():
    """name -> an area mask of sp_coupler_amd.geometry"""
    from sp_coupler_amd import geometry
    sq = lambda x0, x1: [(x0, -10.0), (x1, -10.0), (x1, 10.0), (x0, 10.0)]        # noqa: E731
    return {
        "polygon": geometry.Polygon(sq(0.0, 20.0)),
        "multipolygon": geometry.MultiPolygon([geometry.Polygon([(0.0, -10.0), (20.0, -8.0), (20.0, 10.0), (0.0, 10.0)]),
                                               geometry.Polygon([(21.0, -10.0), (40.0, -10.0), (40.0, 10.0), (21.0, 9.0)])]),
        "polygon_with_hole": geometry.Polygon(sq(0.0, 40.0), [[(10.0, -5.0), (10.0, 5.0), (30.0, 5.0), (30.0, -5.0)]]),
        "box": geometry.box(0.0, -10.0, 20.0, 10.0),
        "infinite_box": geometry.box(-INF, -INF, INF, INF),
    }


@functools.lru_cache(maxsize=None)
def non_finite_case():
    from sp_coupler_amd import geometry
    lon, lat, finite = non_finite_points()
    out = []
    for name, g in non_finite_masks().items():
        lay = geometry.pack(*geometry.as_mask(g))
        out.append((name, lay, geo_ref.locations(lon, lat, *lay)))
    return lon, lat, finite, tuple(out)


def check_non_finite_points(eng):
    """item 3: a point whose lon or lat is NaN or +-inf is EXTERIOR of every polygon, as p and as q, under the ray rule and
    under the rectangle rule; get_mask_indices selects no such point through an area mask"""
    from sp_coupler_amd import spcpl, sputils
    lon, lat, finite, cases = non_finite_case()
    for name, lay, want in cases:
        assert (want[:, ~finite, :] == geo_ref.EXT).all() and (want[:, finite, :] != geo_ref.EXT).any(), name
        got = codes(eng, lon, lat, lay)
        assert (got[:, ~finite, :] == geo_ref.EXT).all(), "%s: non-finite points with codes %s (p, q) at %s" % (
            name, got[:, ~finite, :].reshape(-1, 2)[(got[:, ~finite, :] != 0).any(axis=2).ravel()][:6].tolist(),
            [(lon[i], lat[i]) for i in numpy.flatnonzero(~finite)[(got[:, ~finite, :] != 0).any(axis=(0, 2))]][:6])
        _same("non_finite_points " + name, got, want)
    masks = non_finite_masks()
    points = list(zip(lon.tolist(), lat.tolist()))
    prev = spcpl._engine
    spcpl.set_engine(eng)
    try:
        for name, g in masks.items():
            sel = sputils.get_mask_indices(points, [g])
            assert all(finite[i] for i in sel), "%s: get_mask_indices selected the non-finite points %s" % (
                name, [points[i] for i in sel if not finite[i]])
            want = geo_ref.contains(dict((c[0], c[2]) for c in cases)[name]).any(axis=1)
            assert sorted(sel) == numpy.flatnonzero(want).tolist(), (name, sel)
    finally:
        spcpl.set_engine(prev)


# ---- everything ------------------------------------------------------------------------------------------------------------------
OLD_BODIES = ("adversarial", "naive_flips", "haversine")
NEW_BODIES = ("exact_tails", "tile_seams", "image_lon", "point_counts", "non_finite_points")


BODIES = OLD_BODIES + NEW_BODIES


def jobs(eng, names=BODIES):
    return [(name, lambda name=name: globals()["check_" + name](eng)) for name in names]


def check_everything(eng, names=BODIES, scale=False):
    """the bodies ``names`` (and the 2^20-point size test with ``scale``) on one engine: what tools/mutation_control.py runs on
    a mutant library.  Returns the names of the bodies that failed (AssertionError) in the order they ran."""
    names = tuple(names) + (("scale",) if scale else ())
    return run_bodies(names, jobs(eng, names))
