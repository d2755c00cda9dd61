"""The four names of ``shapely.geometry`` that spmaster.py uses -- ``Point``, ``Polygon``, ``box`` and ``shape`` -- for
the masks of ``sputils.get_mask_indices``, so that ``import shapely.geometry`` can be replaced by
``from sp_coupler_amd import geometry`` where shapely is not installed.

These are plain containers of coordinates: no predicates, no area, no set operations.  Which grid points a mask selects is
decided on the GPU (``spc_point_in_polygon_f64``, include/spc.h) by GEOS's rules in exact arithmetic (DESIGN.md section
7.1).  ``as_mask`` also accepts shapely's own objects (anything with ``geom_type`` and shapely's attributes), so users who
have shapely can keep passing theirs.

As shapely does, a ring is closed automatically.  Beyond shapely, rings with fewer than 3 distinct vertices, NaN
coordinates, and non-finite coordinates anywhere but in an axis-aligned rectangle (``box(-inf, -inf, inf, inf)``: the
"all columns" mask of spmaster.py) raise ``ValueError``: no answer of the point locator would mean anything for them.
"""
import math

import numpy

SHELL, HOLE, RECTANGLE = 0, 1, 2          # include/spc.h SPC_RING_*


def _ring(coords, what="ring"):
    """[m x 2] float64 array of a ring's vertices, closed (last == first), checked"""
    a = numpy.array([tuple(c)[:2] for c in coords], dtype=numpy.float64).reshape(-1, 2)
    if numpy.isnan(a).any():
        raise ValueError("%s has NaN coordinates" % what)
    if len(a) and not (a[0] == a[-1]).all():
        a = numpy.vstack([a, a[:1]])
    if len(numpy.unique(a, axis=0)) < 3:
        raise ValueError("%s needs at least 3 distinct vertices, got %d" % (what, len(numpy.unique(a, axis=0))))
    return a


def is_rectangle(shell, holes=()):
    """GEOS's Polygon::isRectangle: no holes, 5 coordinates, every vertex on a corner of the envelope, and every side
    changes exactly one of x, y (so that the rectangle rule of RectangleContains applies)"""
    if len(holes) or len(shell) != 5:
        return False
    x0, x1 = shell[:, 0].min(), shell[:, 0].max()
    y0, y1 = shell[:, 1].min(), shell[:, 1].max()
    if not (((shell[:, 0] == x0) | (shell[:, 0] == x1)).all() and ((shell[:, 1] == y0) | (shell[:, 1] == y1)).all()):
        return False
    for k in range(1, 5):
        if (shell[k, 0] != shell[k - 1, 0]) == (shell[k, 1] != shell[k - 1, 1]):
            return False
    return True


class Point:
    """``shapely.geometry.Point(p)`` / ``Point(x, y)``: ``.x``, ``.y``"""
    geom_type = "Point"

    def __init__(self, *args):
        if len(args) == 1:
            a = args[0]
            args = (a.x, a.y) if hasattr(a, "x") and hasattr(a, "y") else tuple(a)
        if len(args) < 2:
            raise ValueError("Point needs two coordinates, got %r" % (args,))
        self.x, self.y = float(args[0]), float(args[1])
        if not (math.isfinite(self.x) and math.isfinite(self.y)):
            raise ValueError("Point has non-finite coordinates (%r, %r)" % (self.x, self.y))

    @property
    def coords(self):
        return [(self.x, self.y)]

    @property
    def __geo_interface__(self):
        return {"type": "Point", "coordinates": (self.x, self.y)}

    def __repr__(self):
        return "<POINT (%r %r)>" % (self.x, self.y)


class LinearRing:
    """a closed ring: ``.coords`` as shapely gives them (first vertex repeated at the end)"""

    def __init__(self, xy):
        self.xy_array = xy

    @property
    def coords(self):
        return [tuple(v) for v in self.xy_array.tolist()]


class Polygon:
    """``shapely.geometry.Polygon(shell, holes=None)``: ``.exterior``, ``.interiors``"""
    geom_type = "Polygon"

    def __init__(self, shell, holes=None):
        if hasattr(shell, "exterior"):               # Polygon(polygon)
            holes = [h.coords for h in shell.interiors] if holes is None else holes
            shell = shell.exterior.coords
        s = _ring(shell.coords if hasattr(shell, "coords") else shell, "shell")
        hs = [_ring(h.coords if hasattr(h, "coords") else h, "hole") for h in (holes or ())]
        if not all(numpy.isfinite(r).all() for r in [s] + hs) and not is_rectangle(s, hs):
            raise ValueError("non-finite coordinates are allowed in an axis-aligned rectangle only (box(-inf, -inf, inf, inf))")
        self.exterior = LinearRing(s)
        self.interiors = [LinearRing(h) for h in hs]

    @property
    def __geo_interface__(self):
        return {"type": "Polygon", "coordinates": tuple(tuple(r.coords) for r in [self.exterior] + self.interiors)}

    def __repr__(self):
        return "<POLYGON (%d vertices, %d holes)>" % (len(self.exterior.xy_array), len(self.interiors))


class MultiPolygon:
    """``shapely.geometry.MultiPolygon(polygons)``: ``.geoms``; components are Polygons or (shell, holes) pairs"""
    geom_type = "MultiPolygon"

    def __init__(self, polygons):
        self.geoms = [p if isinstance(p, Polygon) else Polygon(p) if hasattr(p, "exterior") else Polygon(*p) for p in polygons]
        if not self.geoms:
            raise ValueError("MultiPolygon needs at least one polygon")

    @property
    def __geo_interface__(self):
        return {"type": "MultiPolygon", "coordinates": tuple(g.__geo_interface__["coordinates"] for g in self.geoms)}


def box(minx, miny, maxx, maxy, ccw=True):
    """``shapely.geometry.box``: the rectangle with these bounds, vertices in shapely's order; infinite bounds allowed"""
    coords = [(maxx, miny), (maxx, maxy), (minx, maxy), (minx, miny)]
    return Polygon(coords if ccw else coords[::-1])


def shape(context):
    """``shapely.geometry.shape``: a GeoJSON geometry (a mapping, or an object with ``__geo_interface__``) of type
    Point, Polygon or MultiPolygon"""
    ob = getattr(context, "__geo_interface__", context)
    kind = ob.get("type")
    c = ob.get("coordinates")
    if kind == "Point":
        return Point(c)
    if kind == "Polygon":
        return Polygon(c[0], c[1:]) if len(c) else _empty()
    if kind == "MultiPolygon":
        return MultiPolygon([(p[0], p[1:]) for p in c]) if len(c) else _empty()
    raise ValueError("geometry type %r is not supported (Point, Polygon, MultiPolygon)" % kind)


def _empty():
    raise ValueError("an empty polygon selects nothing and is not supported")


def as_mask(g):
    """a mask geometry -- ours or shapely's (duck-typed: ``geom_type``, ``.x`` / ``.y``, ``.exterior.coords``,
    ``.interiors``, ``.geoms``) -- as a Point or as a list of ``(shell, holes)`` arrays (one per polygon) plus whether the
    geometry is ONE polygon (to which GEOS applies the rectangle rule); coordinates checked as the constructors check them"""
    kind = getattr(g, "geom_type", None)
    if kind == "Point":
        return Point(g.x, g.y)
    if kind == "Polygon":
        return [Polygon(g)], True
    if kind == "MultiPolygon":
        return [Polygon(p) for p in g.geoms], False
    raise ValueError("mask geometry %r is not supported (Point, Polygon, MultiPolygon)" % (kind or type(g).__name__))


def pack(polygons, single):
    """the ring arrays of spc_pip_args (include/spc.h) for ``as_mask``'s polygons: (vx, vy, ring_start, ring_role,
    ring_poly, n_polys).  A lone axis-aligned rectangle takes GEOS's rectangle rule (RectangleContains); every other ring
    the ray-crossing rule, which needs finite coordinates."""
    rings, roles, polys = [], [], []
    for k, p in enumerate(polygons):
        shell, holes = p.exterior.xy_array, [h.xy_array for h in p.interiors]
        rect = single and is_rectangle(shell, holes)
        if not rect and not all(numpy.isfinite(r).all() for r in [shell] + holes):
            raise ValueError("non-finite coordinates are allowed in a lone axis-aligned rectangle only")
        rings += [shell] + holes
        roles += [RECTANGLE if rect else SHELL] + [HOLE] * len(holes)
        polys += [k] * (1 + len(holes))
    xy = numpy.concatenate(rings)
    start = numpy.concatenate([[0], numpy.cumsum([len(r) for r in rings])]).astype(numpy.int64)
    return (numpy.ascontiguousarray(xy[:, 0]), numpy.ascontiguousarray(xy[:, 1]), start, numpy.array(roles, dtype=numpy.int32),
            numpy.array(polys, dtype=numpy.int32), len(polygons))
