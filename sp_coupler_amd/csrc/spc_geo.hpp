// spc_geo.hpp -- K8: the geometry of splib/sputils.py:46-73 (get_mask_indices) on the GPU (included by spc_hip.hip).
//   k_point_in_polygon  location of every grid point, and of its -180...180 image, in every polygon of a launch
//   k_haversine         great-circle distance of every grid point to one target (splib/haversine.py:12-36)
// Everything is fp64 whatever the engine's dtype: the decision "this column gets an LES" must not depend on it.
//
// Point in polygon follows GEOS's RayCrossingCounter and point locator in EXACT arithmetic: the
// orientation of a point against an edge is the sign of a 2x2 determinant, decided by the plain double determinant only
// where Shewchuk's error bound proves its sign, else by an exact expansion (TwoDiff / fma-TwoProduct / Grow-Expansion).
// The bound assumes the -ffp-contract=off of the build: no FMA may change a rounding of the filter.
//
// A point whose lon or lat is NaN or +-inf is EXTERIOR to every polygon, as p and as q (include/spc.h).
//
// One lane per grid point tests both of its images p = (lon, lat) and q = ((lon - 180) % 360 - 180, lat) against every
// edge.  The ring vertices are staged through LDS in tiles; every lane of a workgroup reads the same vertex at the same
// time (broadcast reads, no bank conflicts).
#pragma once

constexpr int GEO_THREADS = 256;
constexpr int GEO_TILE = 1024;                 // vertices per LDS tile: 2 x (1024 + 1) doubles = 16.0 KiB

enum { GEO_EXTERIOR = 0, GEO_BOUNDARY = 1, GEO_INTERIOR = 2 };

struct GeoP {
    int64_t n_points, n_vertices;
    int32_t n_rings, n_polys;
    const double *lon, *lat, *vx, *vy;
    const int64_t *ring_start;
    const int32_t *ring_role, *ring_poly;
    uint16_t *out;                 // [n_polys x n_points]: low byte the code of p, high byte the code of q
};

// ---- exact orientation ------------------------------------------------------------------------------
__device__ __forceinline__ void geo_two_sum(double a, double b, double &s, double &e)
{
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

__device__ __forceinline__ void geo_two_diff(double a, double b, double &d, double &e)
{
    d = a - b;
    const double bb = a - d;
    e = (a - (d + bb)) + (bb - b);
}

__device__ __forceinline__ void geo_two_prod(double a, double b, double &p, double &e)
{
    p = a * b;
    e = __builtin_fma(a, b, -p);   // the rounding error of a * b, exact (no underflow for lon / lat coordinates)
}

// sign of (ax - cx) (by - cy) - (ay - cy) (bx - cx) in exact arithmetic: the four differences as exact two-term sums,
// the eight products of their terms as exact two-term products, the 16 terms summed into a non-overlapping expansion by
// Grow-Expansion (Shewchuk 1997, section 2.5), whose largest non-zero component carries the sign.  Fully unrolled with
// compile-time indices so the expansion lives in registers.
__device__ __forceinline__ int geo_orient_exact(double ax, double ay, double bx, double by, double cx, double cy)
{
    double acx[2], bcy[2], acy[2], bcx[2];
    geo_two_diff(ax, cx, acx[0], acx[1]);
    geo_two_diff(by, cy, bcy[0], bcy[1]);
    geo_two_diff(ay, cy, acy[0], acy[1]);
    geo_two_diff(bx, cx, bcx[0], bcx[1]);
    double t[16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            geo_two_prod(acx[i], bcy[j], t[4 * i + 2 * j], t[4 * i + 2 * j + 1]);
            geo_two_prod(-acy[i], bcx[j], t[8 + 4 * i + 2 * j], t[8 + 4 * i + 2 * j + 1]);
        }
    double e[16];
    e[0] = t[0];
#pragma unroll
    for (int m = 1; m < 16; ++m) {          // e[0..m) + t[m] -> e[0..m]
        double q = t[m];
#pragma unroll
        for (int i = 0; i < m; ++i) {
            double s, h;
            geo_two_sum(q, e[i], s, h);
            e[i] = h;
            q = s;
        }
        e[m] = q;
    }
    int sign = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (e[i] != 0.0) sign = e[i] > 0.0 ? 1 : -1;
    return sign;
}

// GEOS Orientation::index(p1, p2, q): +1 q left of p1->p2, -1 right, 0 collinear.  Shewchuk's orient2d filter with
// ccwerrboundA = (3 + 16 eps) eps, eps = 2^-53, on det = (p1 - q) x (p2 - q), which has the sign of (p2 - p1) x (q - p1).
__device__ __forceinline__ int geo_orient(double ax, double ay, double bx, double by, double cx, double cy)
{
    const double detleft = (ax - cx) * (by - cy);
    const double detright = (ay - cy) * (bx - cx);
    const double det = detleft - detright;
    double detsum;
    if (detleft > 0.0) {
        if (detright <= 0.0) return det > 0.0 ? 1 : det < 0.0 ? -1 : 0;
        detsum = detleft + detright;
    } else if (detleft < 0.0) {
        if (detright >= 0.0) return det > 0.0 ? 1 : det < 0.0 ? -1 : 0;
        detsum = -detleft - detright;
    } else {
        return det > 0.0 ? 1 : det < 0.0 ? -1 : 0;
    }
    const double errbound = 3.3306690738754716e-16 * detsum;   // (3 + 16 * 2^-53) * 2^-53
    if (det >= errbound) return 1;
    if (-det >= errbound) return -1;
    return geo_orient_exact(ax, ay, bx, by, cx, cy);
}

// GEOS RayCrossingCounter::countSegment for the segment (x1, y1) -> (x2, y2) and the point (px, py)
__device__ __forceinline__ void geo_count_segment(double x1, double y1, double x2, double y2, double px, double py, int &crossings,
                                                  bool &on_boundary)
{
    if (x1 < px && x2 < px) return;                                    // wholly to the left of the point
    if (px == x2 && py == y2) { on_boundary = true; return; }          // the point is the segment's end vertex
    if (y1 == py && y2 == py) {                                        // horizontal at the point's y
        const double lo = x1 < x2 ? x1 : x2, hi = x1 < x2 ? x2 : x1;
        if (px >= lo && px <= hi) on_boundary = true;
        return;
    }
    // upward edges include their start and exclude their end, downward edges the reverse
    if ((y1 > py && y2 <= py) || (y2 > py && y1 <= py)) {
        int o = geo_orient(x1, y1, x2, y2, px, py);
        if (o == 0) { on_boundary = true; return; }
        if (y2 < y1) o = -o;                                           // orient the segment upwards
        if (o > 0) ++crossings;
    }
}

__device__ __forceinline__ int geo_ring_code(int crossings, bool on_boundary)
{
    return on_boundary ? GEO_BOUNDARY : (crossings & 1) ? GEO_INTERIOR : GEO_EXTERIOR;
}

// a polygon's location from its rings, in ring order (GEOS SimplePointInAreaLocator::locatePointInPolygon): the shell's
// exterior / boundary decide; the first hole that holds the point (interior: the polygon's exterior) or passes through
// it (boundary) decides; else interior
__device__ __forceinline__ int geo_fold(int poly_code, int ring_code, int role)
{
    if (role != SPC_RING_HOLE) return ring_code;
    if (poly_code != GEO_INTERIOR) return poly_code;
    return ring_code == GEO_INTERIOR ? GEO_EXTERIOR : ring_code == GEO_BOUNDARY ? GEO_BOUNDARY : GEO_INTERIOR;
}

// Python's float x % 360.0 (fmod, then + 360 when the remainder is non-zero and of the other sign); then - 180
__device__ __forceinline__ double geo_image_lon(double lon)
{
    const double x = lon - 180.0;
    double r = fmod(x, 360.0);
    if (r != 0.0) {
        if (r < 0.0) r += 360.0;
    } else {
        r = 0.0;                  // CPython: a zero remainder takes the divisor's sign (+0)
    }
    return r - 180.0;
}

__global__ __launch_bounds__(GEO_THREADS) void k_point_in_polygon(const GeoP p)
{
    __shared__ double sx[GEO_TILE + 1], sy[GEO_TILE + 1];
    const int64_t i = (int64_t)blockIdx.x * GEO_THREADS + threadIdx.x;
    const bool live = i < p.n_points;
    const double lon = live ? p.lon[i] : 0.0, lat = live ? p.lat[i] : 0.0;
    // a point with a NaN or infinite coordinate is exterior to every polygon, as p and as q (the image of +-inf is NaN):
    // decided here, before any arithmetic -- a NaN determinant would read as "collinear", that is as BOUNDARY
    const bool finite = isfinite(lon) && isfinite(lat);
    const double px = finite ? lon : 0.0, py = finite ? lat : 0.0;
    const double qx = geo_image_lon(px);
    int code_p = GEO_EXTERIOR, code_q = GEO_EXTERIOR;
    int cur_poly = -1;
    for (int r = 0; r < p.n_rings; ++r) {
        // ring metadata: the same for every lane; offsets clamped to the vertex array, whatever the caller passed
        int64_t s = p.ring_start[r], e = p.ring_start[r + 1];
        s = s < 0 ? 0 : s > p.n_vertices ? p.n_vertices : s;
        e = e < s ? s : e > p.n_vertices ? p.n_vertices : e;
        const int role = p.ring_role[r], poly = p.ring_poly[r];
        if (poly != cur_poly) {
            if (live && cur_poly >= 0 && cur_poly < p.n_polys)
                p.out[(int64_t)cur_poly * p.n_points + i] = finite ? (uint16_t)(code_p | (code_q << 8)) : (uint16_t)GEO_EXTERIOR;
            cur_poly = poly;
            code_p = code_q = GEO_EXTERIOR;
        }
        int rp, rq;
        if (role == SPC_RING_RECTANGLE) {
            // GEOS RectangleContains: strictly inside the envelope (the box of infinite bounds holds every finite point)
            double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
            for (int64_t k = s; k < e; ++k) {
                x0 = fmin(x0, p.vx[k]); x1 = fmax(x1, p.vx[k]);
                y0 = fmin(y0, p.vy[k]); y1 = fmax(y1, p.vy[k]);
            }
            const bool in_y = y0 < py && py < y1;
            rp = in_y && x0 < px && px < x1 ? GEO_INTERIOR : GEO_EXTERIOR;
            rq = in_y && x0 < qx && qx < x1 ? GEO_INTERIOR : GEO_EXTERIOR;
        } else {
            int cp = 0, cq = 0;
            bool bp = false, bq = false;
            for (int64_t t0 = s; t0 + 1 < e; t0 += GEO_TILE) {             // edges t0 ... t0 + n - 1 of this tile
                const int n = (int)(e - 1 - t0 < GEO_TILE ? e - 1 - t0 : GEO_TILE);
                __syncthreads();
                for (int k = threadIdx.x; k <= n; k += GEO_THREADS) {
                    sx[k] = p.vx[t0 + k];
                    sy[k] = p.vy[t0 + k];
                }
                __syncthreads();
                double x1 = sx[0], y1 = sy[0];
                for (int k = 1; k <= n; ++k) {
                    const double x2 = sx[k], y2 = sy[k];
                    geo_count_segment(x1, y1, x2, y2, px, py, cp, bp);
                    geo_count_segment(x1, y1, x2, y2, qx, py, cq, bq);
                    x1 = x2; y1 = y2;
                }
            }
            rp = geo_ring_code(cp, bp);
            rq = geo_ring_code(cq, bq);
        }
        code_p = geo_fold(code_p, rp, role);
        code_q = geo_fold(code_q, rq, role);
    }
    if (live && cur_poly >= 0 && cur_poly < p.n_polys)
        p.out[(int64_t)cur_poly * p.n_points + i] = finite ? (uint16_t)(code_p | (code_q << 8)) : (uint16_t)GEO_EXTERIOR;
}

// splib/haversine.py:24-31 in its order: radians(x) = x * (pi / 180), dlat = lat2 - lat1, dlng = lng2 - lng1,
// d = sin(dlat * 0.5)**2 + cos(lat1) * cos(lat2) * sin(dlng * 0.5)**2, h = 2 * 6371 * asin(sqrt(d)); point 1 the grid point
__global__ __launch_bounds__(GEO_THREADS) void k_haversine(int64_t n, const double *__restrict__ lon, const double *__restrict__ lat,
                                                          double lon0, double lat0, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * GEO_THREADS + threadIdx.x;
    if (i >= n) return;
    const double deg = 3.141592653589793 / 180.0;
    const double lat1 = lat[i] * deg, lng1 = lon[i] * deg, lat2 = lat0 * deg, lng2 = lon0 * deg;
    const double sl = sin((lat2 - lat1) * 0.5), sg = sin((lng2 - lng1) * 0.5);
    const double d = sl * sl + cos(lat1) * cos(lat2) * (sg * sg);
    out[i] = (2.0 * 6371.0) * asin(sqrt(d));
}
