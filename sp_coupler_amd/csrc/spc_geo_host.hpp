// spc_geo_host.hpp -- argument checks and launches of K8, the geometry of sputils.get_mask_indices (kernels: spc_geo.hpp);
// included by spc_hip.hip after spc_launch.hpp (fail, REQUIRE, launch_status).
#pragma once

int pip_impl(const spc_pip_args *a, void *stream)
{
    REQUIRE(a, "args");
    if (a->n_points < 0 || a->n_vertices < 0 || a->n_rings < 0 || a->n_polys < 0)
        return fail(SPC_ERR_INVALID_ARGUMENT, "%spoint_in_polygon: negative count");
    if (a->n_points == 0 || a->n_polys == 0) return SPC_OK;
    if (a->n_rings < 1) return fail(SPC_ERR_INVALID_ARGUMENT, "%spoint_in_polygon: %lld polygons but no ring", "", a->n_polys);
    REQUIRE(a->lon, "lon"); REQUIRE(a->lat, "lat"); REQUIRE(a->ring_start, "ring_start"); REQUIRE(a->ring_role, "ring_role");
    REQUIRE(a->ring_poly, "ring_poly"); REQUIRE(a->out, "out");
    if (a->n_vertices > 0) { REQUIRE(a->vx, "vx"); REQUIRE(a->vy, "vy"); }
    if ((uintptr_t)a->out % alignof(uint16_t) != 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%spoint_in_polygon: out is not 2-byte aligned");
    const int64_t grid = (a->n_points + GEO_THREADS - 1) / GEO_THREADS;
    if (grid > 0x7fffffff) return fail(SPC_ERR_UNSUPPORTED, "%spoint_in_polygon: more than 2^39 points");
    GeoP p;
    p.n_points = a->n_points; p.n_vertices = a->n_vertices; p.n_rings = a->n_rings; p.n_polys = a->n_polys;
    p.lon = a->lon; p.lat = a->lat; p.vx = a->vx; p.vy = a->vy;
    p.ring_start = a->ring_start; p.ring_role = a->ring_role; p.ring_poly = a->ring_poly; p.out = a->out;
    hipLaunchKernelGGL(k_point_in_polygon, dim3((unsigned)grid), dim3(GEO_THREADS), 0, (hipStream_t)stream, p);
    return launch_status("k_point_in_polygon");
}

int haversine_impl(int64_t n, const void *lon, const void *lat, double lon0, double lat0, void *out, void *stream)
{
    if (n < 0) return fail(SPC_ERR_INVALID_ARGUMENT, "%shaversine: n < 0");
    if (n == 0) return SPC_OK;
    REQUIRE(lon, "lon"); REQUIRE(lat, "lat"); REQUIRE(out, "out");
    const int64_t grid = (n + GEO_THREADS - 1) / GEO_THREADS;
    if (grid > 0x7fffffff) return fail(SPC_ERR_UNSUPPORTED, "%shaversine: more than 2^39 points");
    hipLaunchKernelGGL(k_haversine, dim3((unsigned)grid), dim3(GEO_THREADS), 0, (hipStream_t)stream, n, (const double *)lon,
                       (const double *)lat, lon0, lat0, (double *)out);
    return launch_status("k_haversine");
}
