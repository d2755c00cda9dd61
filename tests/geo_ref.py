"""Test-only oracle of the K8 geometry (sputils.get_mask_indices), written from the rules of DESIGN.md section 7.1 and not
sharing code with the kernel or with sp_coupler_amd.geometry:

* ``locations``: the location codes of the C ABI (include/spc.h spc_pip_args: [n_polys x n x 2], 0 exterior, 1 boundary,
  2 interior; [..., 0] the point, [..., 1] its image ((lon - 180) % 360 - 180, lat)) in NumPy, one edge at a time over the
  points whose latitude the edge spans; orientations from the GEOS-form double determinant where a generous error bound
  proves its sign, else from ``fractions.Fraction``; a point whose lon or lat is NaN or +-inf is exterior (0) to every
  polygon, as p and as q, decided before any arithmetic touches it;
* ``brute_locations``: the same codes point by point, every orientation in ``Fraction`` (small inputs only);
* ``reference_mask_indices``: splib/sputils.py:50-73 restated loop for loop, with a ``contains`` predicate passed in;
* ``haversine``: splib/haversine.py:24-31 in NumPy.
"""
import math
from fractions import Fraction

import numpy

EXT, BND, INT = 0, 1, 2
SHELL, HOLE, RECT = 0, 1, 2


def image_lon(lon):
    """(lon - 180) % 360 - 180 with Python's float % (NumPy's float remainder has the same semantics)"""
    return (numpy.asarray(lon, dtype=numpy.float64) - 180) % 360 - 180


def _orient_fraction(x1, y1, x2, y2, qx, qy):
    F = Fraction
    d = (F(x2) - F(x1)) * (F(qy) - F(y1)) - (F(y2) - F(y1)) * (F(qx) - F(x1))
    return int(d > 0) - int(d < 0)


def orient(x1, y1, x2, y2, qx, qy):
    """sign of (p2 - p1) x (q - p1) for one edge and arrays of points q"""
    qx, qy = numpy.asarray(qx, dtype=numpy.float64), numpy.asarray(qy, dtype=numpy.float64)
    a = (x2 - x1) * (qy - y1)
    b = (y2 - y1) * (qx - x1)
    det = a - b
    sure = numpy.abs(det) > 1e-14 * (numpy.abs(a) + numpy.abs(b))
    o = numpy.sign(det).astype(numpy.int64)
    for k in numpy.flatnonzero(~sure):
        o[k] = _orient_fraction(x1, y1, x2, y2, qx[k], qy[k])
    return o


def ring_location(px, py, ring, order=None, pys=None):
    """codes of the points (px, py) against one closed ring [m x 2] (GEOS RayCrossingCounter)"""
    n = len(px)
    if order is None:
        order = numpy.argsort(py, kind="stable")
        pys = py[order]
    cnt = numpy.zeros(n, dtype=numpy.int64)
    onb = numpy.zeros(n, dtype=bool)
    for k in range(len(ring) - 1):
        x1, y1 = ring[k]
        x2, y2 = ring[k + 1]
        # only points with min(y1, y2) <= py <= max(y1, y2) can be on this edge, at its end vertex or crossed by it
        idx = order[numpy.searchsorted(pys, min(y1, y2), "left"):numpy.searchsorted(pys, max(y1, y2), "right")]
        if not len(idx):
            continue
        x, y = px[idx], py[idx]
        go = ~((x1 < x) & (x2 < x))
        vert = go & (x == x2) & (y == y2)
        go &= ~vert
        horiz = go & (y1 == y) & (y2 == y)
        on_h = horiz & (x >= min(x1, x2)) & (x <= max(x1, x2))
        go &= ~horiz
        go &= ((y1 > y) & (y2 <= y)) | ((y2 > y) & (y1 <= y))
        o = numpy.zeros(len(idx), dtype=numpy.int64)
        if go.any():
            o[go] = orient(x1, y1, x2, y2, x[go], y[go])
        col = go & (o == 0)
        up = numpy.where(y2 < y1, -o, o)
        onb[idx] |= vert | on_h | col
        cnt[idx] += (go & ~col & (up > 0)).astype(numpy.int64)
    return numpy.where(onb, BND, numpy.where(cnt % 2 == 1, INT, EXT))


def _fold(code, ring_code, role):
    if role != HOLE:
        return ring_code
    hole_decides = code == INT
    return numpy.where(hole_decides & (ring_code == INT), EXT, numpy.where(hole_decides & (ring_code == BND), BND, code))


def locations(lon, lat, vx, vy, ring_start, ring_role, ring_poly, n_polys):
    """[n_polys x n x 2] uint8 codes, the layout of spc_point_in_polygon_f64"""
    lon, lat = numpy.asarray(lon, dtype=numpy.float64), numpy.asarray(lat, dtype=numpy.float64)
    n = len(lon)
    out = numpy.zeros((n_polys, n, 2), dtype=numpy.uint8)
    finite = numpy.isfinite(lon) & numpy.isfinite(lat)
    if not finite.all():                 # the non-finite points stay exterior; only the finite ones reach the arithmetic
        keep = numpy.flatnonzero(finite)
        if len(keep):
            out[:, keep, :] = locations(lon[keep], lat[keep], vx, vy, ring_start, ring_role, ring_poly, n_polys)
        return out
    order = numpy.argsort(lat, kind="stable")
    pys = lat[order]
    for img, px in enumerate((lon, image_lon(lon))):
        code = numpy.zeros(n, dtype=numpy.int64)
        for r in range(len(ring_role)):
            ring = numpy.stack([vx[ring_start[r]:ring_start[r + 1]], vy[ring_start[r]:ring_start[r + 1]]], axis=1)
            if ring_role[r] == RECT:
                rc = numpy.where((ring[:, 0].min() < px) & (px < ring[:, 0].max()) & (ring[:, 1].min() < lat) & (lat < ring[:, 1].max()), INT, EXT)
            else:
                rc = ring_location(px, lat, ring, order, pys)
            code = _fold(code, rc, ring_role[r])
            if r + 1 == len(ring_role) or ring_poly[r + 1] != ring_poly[r]:
                out[ring_poly[r], :, img] = code
    return out


def brute_locations(lon, lat, vx, vy, ring_start, ring_role, ring_poly, n_polys):
    """the same codes point by point, every test in exact rational arithmetic"""
    F = Fraction
    out = numpy.zeros((n_polys, len(lon), 2), dtype=numpy.uint8)
    for i in range(len(lon)):
        if not (math.isfinite(lon[i]) and math.isfinite(lat[i])):
            continue                                                   # NaN / +-inf: exterior to everything
        for img, x in enumerate((float(lon[i]), (float(lon[i]) - 180) % 360 - 180)):
            y = float(lat[i])
            code = EXT
            for r in range(len(ring_role)):
                vs = [(float(vx[k]), float(vy[k])) for k in range(ring_start[r], ring_start[r + 1])]
                if ring_role[r] == RECT:
                    xs, ys = [v[0] for v in vs], [v[1] for v in vs]
                    rc = INT if min(xs) < x < max(xs) and min(ys) < y < max(ys) else EXT
                else:
                    crossings, on = 0, False
                    for (x1, y1), (x2, y2) in zip(vs[:-1], vs[1:]):
                        if x1 < x and x2 < x:
                            continue
                        if x == x2 and y == y2:
                            on = True
                            continue
                        if y1 == y and y2 == y:
                            on = on or min(x1, x2) <= x <= max(x1, x2)
                            continue
                        if (y1 > y and y2 <= y) or (y2 > y and y1 <= y):
                            d = (F(x2) - F(x1)) * (F(y) - F(y1)) - (F(y2) - F(y1)) * (F(x) - F(x1))
                            if d == 0:
                                on = True
                                continue
                            upward_left = (d > 0) if y2 > y1 else (d < 0)
                            crossings += upward_left
                    rc = BND if on else INT if crossings % 2 else EXT
                if ring_role[r] != HOLE:
                    code = rc
                elif code == INT:
                    code = EXT if rc == INT else BND if rc == BND else INT
                if r + 1 == len(ring_role) or ring_poly[r + 1] != ring_poly[r]:
                    out[ring_poly[r], i, img] = code
    return out


def contains(codes):
    """[n x 2] bool from the codes of ONE geometry's polygons: GEOS's Mod-2 boundary rule, contains == interior"""
    codes = numpy.asarray(codes)
    nb = (codes == BND).sum(axis=0)
    return (nb % 2 == 0) & (((codes == INT).any(axis=0)) | (nb > 0))


def rings_of(shell, holes=(), rect=False, poly=0):
    """ring arrays for one polygon given as closed vertex lists: (rings, roles, polys)"""
    rings = [numpy.asarray(shell, dtype=numpy.float64)] + [numpy.asarray(h, dtype=numpy.float64) for h in holes]
    return rings, [RECT if rect else SHELL] + [HOLE] * len(holes), [poly] * len(rings)


def layout(polys):
    """(vx, vy, ring_start, ring_role, ring_poly, n_polys) from a list of rings_of() triples"""
    rings = [r for p in polys for r in p[0]]
    roles = [x for p in polys for x in p[1]]
    ids = [x for p in polys for x in p[2]]
    xy = numpy.concatenate(rings)
    start = numpy.concatenate([[0], numpy.cumsum([len(r) for r in rings])]).astype(numpy.int64)
    return (xy[:, 0].copy(), xy[:, 1].copy(), start, numpy.array(roles, dtype=numpy.int32), numpy.array(ids, dtype=numpy.int32),
            max(ids) + 1)


def haversine(lon, lat, lon0, lat0):
    """splib/haversine.py:24-31 with point 1 the grid points, point 2 the target, in NumPy"""
    deg = numpy.pi / 180
    lat1, lng1 = numpy.asarray(lat, dtype=numpy.float64) * deg, numpy.asarray(lon, dtype=numpy.float64) * deg
    lat2, lng2 = lat0 * deg, lon0 * deg
    d = numpy.sin((lat2 - lat1) * 0.5) ** 2 + numpy.cos(lat1) * numpy.cos(lat2) * numpy.sin((lng2 - lng1) * 0.5) ** 2
    return 2 * 6371 * numpy.arcsin(numpy.sqrt(d))


def reference_mask_indices(points, masks, nmax, contains_pq, dists):
    """splib/sputils.py:50-73 loop for loop; ``masks`` entries are ('point', x, y) or ('area', key);
    ``contains_pq(key)`` -> ([n] bool for p, [n] bool for q); ``dists(x, y)`` -> [n] distances"""
    if nmax == 0:
        return []
    result = []
    if len(masks) == 1 and masks[0][0] == "point":
        d = dists(masks[0][1], masks[0][2])
        return numpy.argsort(d, kind="stable")[:nmax] if nmax > 0 else [int(numpy.argmin(d))]
    for g in masks:
        if g[0] == "point":
            result.append(int(numpy.argmin(dists(g[1], g[2]))))
        else:
            in_p, in_q = contains_pq(g[1])
            for i, p in enumerate(points):
                if in_p[i]:
                    result.append(i)
                if in_q[i]:
                    result.append(i)
    return list(set(result))


def naive_sign(ax, ay, bx, by, cx, cy):
    """the plain double determinant alone (what the kernel's filter computes first): NOT a valid decision"""
    ax, ay, bx, by, cx, cy = map(float, (ax, ay, bx, by, cx, cy))
    d = (ax - cx) * (by - cy) - (ay - cy) * (bx - cx)
    return int(d > 0) - int(d < 0)


def naive_flips(a, b, count=64):
    """points within a few ulps of the segment a-b (strictly between its end latitudes) where the naive determinant has
    the WRONG sign (both non-zero) or calls the point collinear when it is not"""
    pts = []
    for t in numpy.linspace(0.05, 0.95, count):
        cx, cy = float(a[0] + t * (b[0] - a[0])), float(a[1] + t * (b[1] - a[1]))
        for k in range(-6, 7):
            x = cx
            for _ in range(abs(k)):
                x = math.nextafter(x, math.copysign(math.inf, k))
            e = _orient_fraction(a[0], a[1], b[0], b[1], x, cy)
            if e != 0 and naive_sign(a[0], a[1], b[0], b[1], x, cy) != e:
                pts.append((x, cy))
    return pts


def star(nv, r0=20.0, r1=45.0, cx=10.0, cy=0.0, snap=0.5):
    """closed star polygon of nv vertices (alternating radii), vertices snapped to multiples of ``snap``"""
    k = numpy.arange(nv)
    r = numpy.where(k % 2 == 0, r1, r0)
    ang = 2 * numpy.pi * k / nv
    xy = numpy.stack([cx + r * numpy.cos(ang), cy + 0.9 * r * numpy.sin(ang)], axis=1)
    xy = numpy.round(xy / snap) * snap
    keep = numpy.ones(len(xy), dtype=bool)
    keep[1:] = (numpy.diff(xy, axis=0) != 0).any(axis=1)        # no repeated consecutive vertices
    xy = xy[keep]
    return numpy.vstack([xy, xy[:1]])


def reduced_gaussian(n_target, seed=0):
    """about n_target points on latitude rings (reduced-Gaussian-like: fewer points towards the poles), longitudes
    0 ... 360 in steps that land on whole and half degrees on some rings"""
    n_lat = int(numpy.sqrt(n_target / 1.3))
    lats = numpy.linspace(89.5, -89.5, n_lat)
    counts = numpy.maximum(4, numpy.round(numpy.cos(numpy.radians(lats)) * 2 * n_lat * 1.3 / 1.0)).astype(int)
    counts = numpy.round(counts * n_target / counts.sum()).astype(int)
    lon = numpy.concatenate([numpy.arange(c) * (360.0 / c) for c in counts])
    lat = numpy.concatenate([numpy.full(c, la) for c, la in zip(counts, lats)])
    return lon[:n_target], lat[:n_target]


def adversarial():
    """(name, lon, lat, layout) cases of DESIGN.md section 7.1's edge rules; layout as ``layout()`` returns it"""
    g = numpy.arange(-12.0, 12.5, 0.5)
    glon, glat = [a.ravel() for a in numpy.meshgrid(g, g)]
    sq = [(-5, -5), (5, -5), (5, 5), (-5, 5), (-5, -5)]                  # counter-clockwise
    tri = [(-8, -6), (8, -2), (0, 9), (-8, -6)]                           # diagonal edges through grid points
    hole = [(-2, -2), (-2, 2), (2, 2), (2, -2), (-2, -2)]
    cases = [
        ("square_ccw", glon, glat, layout([rings_of(sq)])),
        ("square_cw", glon, glat, layout([rings_of(sq[::-1])])),
        ("triangle", glon, glat, layout([rings_of(tri)])),
        ("concave_rays_through_vertices", glon, glat,
         layout([rings_of([(-6, -6), (0, -3), (6, -6), (6, 0), (3, 0), (6, 6), (0, 3), (-6, 6), (-3, 0), (-6, 0), (-6, -6)])])),
        ("square_with_hole", glon, glat, layout([rings_of(sq, [hole])])),
        ("square_with_two_holes", glon, glat,
         layout([rings_of(sq, [[(-4, -4), (-4, -1), (-1, -1), (-1, -4), (-4, -4)], [(1, 1), (4, 1), (3, 4), (1, 1)]])])),
        ("multipolygon_shared_edge", glon, glat,
         layout([rings_of([(-6, -3), (0, -3), (0, 3), (-6, 3), (-6, -3)], poly=0), rings_of([(0, -3), (6, -3), (6, 3), (0, 3), (0, -3)], poly=1)])),
        ("rectangle_rule", glon, glat, layout([rings_of(sq, rect=True)])),
    ]
    # a polygon drawn in -180 ... 180 over a 0 ... 360 grid: only the images q fall in it
    wlon, wlat = [a.ravel() for a in numpy.meshgrid(numpy.arange(0.0, 360.0, 2.5), numpy.arange(-30.0, 31.0, 2.5))]
    cases.append(("antimeridian_image", wlon, wlat, layout([rings_of([(-30, -20), (-10, -20), (-10, 20), (-30, 20), (-30, -20)])])))
    # the infinite box (spmaster.py's --all): rectangle rule
    inf = float("inf")
    cases.append(("infinite_box", wlon, wlat, layout([rings_of([(inf, -inf), (inf, inf), (-inf, inf), (-inf, -inf), (inf, -inf)], rect=True)])))
    # points a few ulps off a long diagonal edge, where the naive determinant is wrong
    a, b = (0.5, 0.5), (17.3, 24.25)
    fl = numpy.array(naive_flips(a, b))
    cases.append(("naive_determinant_wrong", fl[:, 0], fl[:, 1], layout([rings_of([a, b, (-20.0, 30.0), a])])))
    return cases
