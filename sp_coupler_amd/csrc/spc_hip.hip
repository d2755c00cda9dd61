// spc_hip.hip -- gfx950 (MI355X / CDNA4) kernels and C ABI of the batched SP coupling step: the ONE translation unit of
// libspc_hip.so.  This file is the include chain and the extern "C" block; every kernel family has a file of its own.
//
// Replaces the serial per-column Python loops of the reference (splib/splib.py:317-323, 330-332)
// and the NumPy helpers they call (splib/spcpl.py:171-246, 299-385, 388-555, 761-764;
// splib/sputils.py:28-34, 82-91) with three launches over ALL columns:
//   K1 k_forward   GCM state -> LES-level profiles + nudging forcings (+ fused K2 index map,
//                  surface fluxes, rain rate): spc_k1.hpp; float with 8-byte accesses: spc_f32v.hpp
//   K2 k_cloud_idx cloud-fraction level-index map (standalone form): spc_k1.hpp
//   K3 k_backward  LES slab means -> GCM tendencies, masked above the LES top: spc_k3.hpp
//   K4 k_backward_cons  the same with conservative (rho-weighted layer-mean) coarsening: spc_k4.hpp
//   K5 k_diag      spifs.nc diagnostics; k_surface: spc_k5.hpp
//   K6 k_vnudge_*  variability nudge (qt_forcing == 'variance'): spc_vnudge.hpp, spc_vnudge2.hpp; host: spc_vnudge_host.hpp
//   K7 k_exner, k_interp ...  the helpers of sputils.py as operators: spc_sputils.hpp; host: spc_sputils_host.hpp
//   K8 k_point_in_polygon, k_haversine  column selection of sputils.get_mask_indices: spc_geo.hpp; host: spc_geo_host.hpp
//   K9 k_mt_jump, k_les_state  initial LES state of spcpl.set_les_state (NumPy's MT19937, jump-ahead): spc_lesstate.hpp;
//                  host: spc_lesstate_host.hpp
//   K10 k_slab_means, k_slab_cloud_*  slab means and cloud fraction of device-resident LES fields (les.get_profile_*,
//                  les.get_cloudfraction): spc_slab.hpp, kernels and host side
//   K11 k_les_advance  one step of those fields in place (forcings, ql = max(qt - qsat, 0)) and the slab means of the stepped
//                  fields in one pass: spc_advance.hpp, kernel and host side
//   K12 k_les_thermo  saturation adjustment of those fields (Qsat, QL, T per cell by a Newton iteration over a
//                  saturation-pressure table) and the slab means of QL and T in one pass: spc_thermo.hpp, kernel and host side
//   K13 k_les_water_paths  column water paths of those fields (numpy.add.reduce(field * w) along k, pairwise as ndarray.sum()),
//                  with the cloud top and the cloud cover, in one pass: spc_waterpath.hpp, kernel and host side
//   K14 k_les_microphysics  warm-rain microphysics of those fields (autoconversion, accretion, one upwind step of sedimentation,
//                  the surface rain, the cloud ice) and the slab means of QT, THL, QR and QI in one pass: spc_micro.hpp, kernel
//                  and host side
//   K15 k_les_diffuse  one backward-Euler step of the vertical diffusion of those fields with the surface fluxes (Thomas sweeps
//                  of a tile of columns in LDS, the elimination done on the host): spc_diffuse.hpp, kernel and host side
//   K16 k_les_advect  one explicit upwind step of the horizontal advection of those fields on the periodic plane (neighbours
//                  along i and j, separate output buffers, the Courant sums): spc_advect.hpp, kernel and host side
//   K17 k_les_vadvect  one explicit upwind step of the vertical advection of those fields by the mass flux of continuity (K16's
//                  face numbers, a serial chain along k per column of a tile in LDS): spc_vadvect.hpp, kernel and host side
//   K18 k_les_radiate  the longwave flux that the liquid water of a column lets through and the THL tendency of its divergence
//                  (two opposed running sums along k per column of two tiles in LDS, a table of exp(-x)): spc_radiate.hpp,
//                  kernel and host side
//   K19 k_les_qt_local  the local cloud-water forcing of QT (qt_forcing == 'local' | 'strong': the wet cells of every plane
//                  counted, then moisture moved between them and the rest; integer counts through LDS, or through global
//                  atomics where a plane is split over workgroups): spc_qtlocal.hpp, kernels and host side
//   K20 k_les_moments  the second moments of those fields per (LES, level): means, variances, standard deviations and the
//                  covariances of pairs of fields (the resolved fluxes, W brought from the faces to the centres), NumPy's
//                  sequential order, one job per field or pair in one launch: spc_moments.hpp, kernel and host side
//   K21 k_les_hydrostatic, k_les_pgrad  the hydrostatic pressure force: the buoyancy of every column integrated downward to
//                  a pressure perturbation (one chain per column of a tile in LDS), whose horizontal gradient accelerates U
//                  and V in place (K16's neighbours along i and j): spc_buoyancy.hpp, kernels and host side
//   K22 k_les_transport  one unsplit donor-cell step in flux form of the transport of those fields along i, j and k (K16's face
//                  numbers, K17's chain and tile; every face flux formed alike by the two cells that share it, so the mass
//                  of a field changes only through the lid): spc_transport.hpp, kernel and host side
//   K23 k_les_transport2  K22's step with a second-order face value: every face adds to K22's donor flux a correction from the
//                  (MC-limited or unlimited) slope of its upwind cell, centred in time; 13 values per cell and field for 7, the
//                  same shared faces and lid budget: spc_transport2.hpp, kernel and host side
//   K24 k_les_eddy, k_les_hmix  the Smagorinsky-Lilly subgrid closure: an eddy viscosity per cell from the resolved deformation
//                  and the stratification (one sqrt per cell), and the horizontal mixing of the carried fields by it in flux
//                  form (K16's shape and neighbours, every face flux formed alike by its two cells): spc_mix.hpp, kernels and
//                  host side
//   K25 k_les_speed, k_les_vmix  one backward-Euler step of the vertical mixing by each column's own eddy viscosity: the Thomas
//                  elimination in the kernel (one division per level), K15's tile, surface fluxes and a neutral bulk drag on the
//                  lowest wind level from a plane of wind speeds: spc_vmix.hpp, kernels and host side
//   K26 k_les_hline  one backward-Euler step of the horizontal mixing by each line's own eddy viscosity, in place and without
//                  K24's cap: one lane eliminates one periodic grid line (a cyclic tridiagonal system, one division per cell),
//                  first every line along i, then every line along j: spc_hmix.hpp, kernel and host side
// Shared device code (constants, pow, searches, numpy.interp, parameter blocks): spc_device.hpp; the LDS column tile of the
// kernels with a serial chain along k (K15, K17, K18, K21, K22, K23, K25: its geometry, the run of a workgroup, the split of a
// run into 16-byte vectors, the plain mover, their host checks and launches): spc_coltile.hpp; the slab chain of the kernels
// that sum along (i, j) per (LES, level) (K10, K11, K12, K14, K20: the lane, the zero and the mean of a sum, their host checks
// and launch geometry): spc_chain.hpp.  Host side of K1-K5 (launch heuristics, kernel tables, launchers,
// spc_describe_launch's text): spc_launch.hpp.
// The path is 1-D interpolation over short columns: HBM-bound, no MFMA.  Design:
// a 256-thread workgroup owns CB consecutive columns; the source profiles of those columns are
// loaded with flat, fully coalesced accesses over the contiguous [CB x n_lev] slab, converted and
// staged in LDS (reversal of the top-down GCM arrays is index arithmetic while staging); then every
// thread produces output levels of the flat [CB x n_out] slab, searching its column's LDS copy.
// Arithmetic follows numpy.interp / numpy.searchsorted operation by operation, compiled with
// FP contraction OFF so no FMA changes a rounding: level indices are bit-exact, interpolated
// values differ from the CPU only through pow().
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// (the headers below are included inside the unnamed namespace, so what they need of the standard library is included here)
#include <initializer_list>   // spc_launch.hpp
#include <map>                // spc_lesstate.hpp
#include <mutex>              // spc_lesstate.hpp
#include <type_traits>
#include <unordered_map>      // spc_launch.hpp
#include <vector>             // spc_lesstate.hpp, spc_lesstate_host.hpp

#include "spc.h"

#pragma clang fp contract(off)

// spc_pow's coefficients as a __constant__ table with EXTERNAL linkage (file scope, outside the unnamed namespace below): the
// standalone exner kernel reads them into scalar registers (spc_pow.h: spc_pow_pos_tab); an internal table would be proved
// constant and folded back into literals
#include "spc_pow_coefs.h"
__constant__ double spc_pow_coef_table[21] = {SPC_POW_COEFS};
#define SPC_POW_TABLE spc_pow_coef_table

namespace {

#include "spc_device.hpp"
#include "spc_k1.hpp"
#include "spc_k3.hpp"
#include "spc_f32v.hpp"
#include "spc_vnudge.hpp"
#include "spc_vnudge2.hpp"
#include "spc_k4.hpp"
#include "spc_sputils.hpp"
#include "spc_geo.hpp"
#include "spc_lesstate.hpp"
#include "spc_chain.hpp"
#include "spc_slab.hpp"
#include "spc_advance.hpp"
#include "spc_thermo.hpp"
#include "spc_waterpath.hpp"
#include "spc_micro.hpp"
#include "spc_coltile.hpp"
#include "spc_diffuse.hpp"
#include "spc_advect.hpp"
#include "spc_vadvect.hpp"
#include "spc_transport.hpp"
#include "spc_transport2.hpp"
#include "spc_radiate.hpp"
#include "spc_qtlocal.hpp"
#include "spc_moments.hpp"
#include "spc_buoyancy.hpp"
#include "spc_mix.hpp"
#include "spc_vmix.hpp"
#include "spc_hmix.hpp"
#include "spc_k5.hpp"

#include "spc_launch.hpp"
#define SPC_COLTILE_HOST
#include "spc_coltile.hpp"
#undef SPC_COLTILE_HOST
#include "spc_sputils_host.hpp"
#include "spc_vnudge_host.hpp"
#include "spc_geo_host.hpp"
#include "spc_lesstate_host.hpp"
#define SPC_CHAIN_HOST
#include "spc_chain.hpp"
#undef SPC_CHAIN_HOST
#define SPC_SLAB_HOST
#include "spc_slab.hpp"
#undef SPC_SLAB_HOST
#define SPC_ADVANCE_HOST
#include "spc_advance.hpp"
#undef SPC_ADVANCE_HOST
#define SPC_THERMO_HOST
#include "spc_thermo.hpp"
#undef SPC_THERMO_HOST
#define SPC_WATERPATH_HOST
#include "spc_waterpath.hpp"
#undef SPC_WATERPATH_HOST
#define SPC_MICRO_HOST
#include "spc_micro.hpp"
#undef SPC_MICRO_HOST
#define SPC_DIFFUSE_HOST
#include "spc_diffuse.hpp"
#undef SPC_DIFFUSE_HOST
#define SPC_ADVECT_HOST
#include "spc_advect.hpp"
#undef SPC_ADVECT_HOST
#define SPC_VADVECT_HOST
#include "spc_vadvect.hpp"
#undef SPC_VADVECT_HOST
#define SPC_TRANSPORT_HOST
#include "spc_transport.hpp"
#undef SPC_TRANSPORT_HOST
#define SPC_TRANSPORT2_HOST
#include "spc_transport2.hpp"
#undef SPC_TRANSPORT2_HOST
#define SPC_RADIATE_HOST
#include "spc_radiate.hpp"
#undef SPC_RADIATE_HOST
#define SPC_QTLOCAL_HOST
#include "spc_qtlocal.hpp"
#undef SPC_QTLOCAL_HOST
#define SPC_MOMENTS_HOST
#include "spc_moments.hpp"
#undef SPC_MOMENTS_HOST
#define SPC_BUOYANCY_HOST
#include "spc_buoyancy.hpp"
#undef SPC_BUOYANCY_HOST
#define SPC_MIX_HOST
#include "spc_mix.hpp"
#undef SPC_MIX_HOST
#define SPC_VMIX_HOST
#include "spc_vmix.hpp"
#undef SPC_VMIX_HOST
#define SPC_HMIX_HOST
#include "spc_hmix.hpp"
#undef SPC_HMIX_HOST

}  // namespace

extern "C" {

int spc_forward_f64(const spc_dims *d, const spc_forward_args *a, void *s) { return forward_impl<double>(d, a, s); }
int spc_forward_f32(const spc_dims *d, const spc_forward_args *a, void *s) { return forward_impl<float>(d, a, s); }
int spc_cloud_indices_f64(const spc_dims *d, const void *zh, const void *Zh, int32_t *idx, void *s) { return cloud_idx_impl<double>(d, zh, Zh, idx, s); }
int spc_cloud_indices_f32(const spc_dims *d, const void *zh, const void *Zh, int32_t *idx, void *s) { return cloud_idx_impl<float>(d, zh, Zh, idx, s); }
int spc_backward_f64(const spc_dims *d, const spc_backward_args *a, void *s) { return backward_impl<double>(d, a, s); }
int spc_backward_f32(const spc_dims *d, const spc_backward_args *a, void *s) { return backward_impl<float>(d, a, s); }
int spc_diagnostics_f64(const spc_dims *d, const spc_diagnostics_args *a, void *s) { return diag_impl<double>(d, a, s); }
int spc_diagnostics_f32(const spc_dims *d, const spc_diagnostics_args *a, void *s) { return diag_impl<float>(d, a, s); }

#ifdef SPC_STAMPS
int spc_debug_set_stamps(void *buf)  // diagnostic build only
{
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &buf, sizeof(buf)) == hipSuccess ? 0 : SPC_ERR_LAUNCH;
}
#endif

int spc_exner_f64(int64_t n, const void *p, void *out, int32_t inv, void *s) { return exner_impl<double>(n, p, out, inv, s); }
int spc_exner_f32(int64_t n, const void *p, void *out, int32_t inv, void *s) { return exner_impl<float>(n, p, out, inv, s); }
int spc_interp_f64(const spc_interp_args *a, void *s) { return interp_impl<double>(a, s); }
int spc_interp_f32(const spc_interp_args *a, void *s) { return interp_impl<float>(a, s); }
int spc_searchsorted_f64(const spc_searchsorted_args *a, void *s) { return searchsorted_impl<double>(a, s); }
int spc_searchsorted_f32(const spc_searchsorted_args *a, void *s) { return searchsorted_impl<float>(a, s); }
int spc_interp_c_f64(const spc_interp_c_args *a, void *s) { return interp_c_impl<double>(a, s); }
int spc_interp_c_f32(const spc_interp_c_args *a, void *s) { return interp_c_impl<float>(a, s); }
int spc_rms_f64(int64_t nr, int64_t n, int64_t pitch, const void *a, void *out, void *s) { return rms_impl<double>(nr, n, pitch, a, out, s); }
int spc_rms_f32(int64_t nr, int64_t n, int64_t pitch, const void *a, void *out, void *s) { return rms_impl<float>(nr, n, pitch, a, out, s); }
int spc_sputils_describe_launch(int32_t op, int32_t es, const void *a, int64_t nr, int64_t n, int64_t pitch, char *buf, int32_t len)
{
    return sputils_describe_launch_impl(op, es, a, nr, n, pitch, buf, len);
}

int spc_point_in_polygon_f64(const spc_pip_args *a, void *s) { return pip_impl(a, s); }
int spc_haversine_f64(int64_t n, const void *lon, const void *lat, double lon0, double lat0, void *out, void *s)
{
    return haversine_impl(n, lon, lat, lon0, lat0, out, s);
}

int spc_surface_fluxes_f64(int64_t n, const void *Ph_s, const void *T_s, const void *QLflux, const void *QIflux,
                           const void *SHflux, const void *TSflux, void *wthl, void *wqt, void *stream)
{
    return surface_impl<double>(n, Ph_s, T_s, QLflux, QIflux, SHflux, TSflux, wthl, wqt, stream);
}
int spc_surface_fluxes_f32(int64_t n, const void *Ph_s, const void *T_s, const void *QLflux, const void *QIflux,
                           const void *SHflux, const void *TSflux, void *wthl, void *wqt, void *stream)
{
    return surface_impl<float>(n, Ph_s, T_s, QLflux, QIflux, SHflux, TSflux, wthl, wqt, stream);
}

int64_t spc_vnudge_workspace_bytes(int64_t n, int32_t itot, int32_t jtot, int32_t ktot) { return vnudge_workspace_bytes<double>(n, itot, jtot, ktot); }
int64_t spc_vnudge_workspace_bytes_f32(int64_t n, int32_t itot, int32_t jtot, int32_t ktot) { return vnudge_workspace_bytes<float>(n, itot, jtot, ktot); }
int spc_variability_nudge_f64(const spc_vnudge_args *a, void *stream) { return vnudge_impl<double>(a, stream); }
int spc_variability_nudge_f32(const spc_vnudge_args *a, void *stream) { return vnudge_impl<float>(a, stream); }

int spc_les_state_f64(const spc_les_state_args *a, void *s) { return les_state_impl(a, s); }
int64_t spc_les_state_workspace_bytes(int64_t n_les, int64_t n_elems, int32_t pos, int64_t gens) { return les_state_workspace_impl(n_les, n_elems, pos, gens); }
int spc_mt19937_jump(const uint32_t *key, int32_t pos, int64_t n_words, uint32_t *key_out, int32_t *pos_out) { return mt_jump_impl(key, pos, n_words, key_out, pos_out); }
int spc_mt19937_jump_poly(uint64_t J, uint64_t *out) { return mt_jump_poly_impl(J, out); }

int spc_slab_means_f64(const spc_slab_means_args *a, void *s) { return slab_means_impl<double>(a, s); }
int spc_slab_means_f32(const spc_slab_means_args *a, void *s) { return slab_means_impl<float>(a, s); }
int spc_slab_cloud_fraction_f64(const spc_slab_cloud_args *a, void *s) { return slab_cloud_impl<double>(a, s); }
int spc_slab_cloud_fraction_f32(const spc_slab_cloud_args *a, void *s) { return slab_cloud_impl<float>(a, s); }

int spc_les_advance_f64(const spc_les_advance_args *a, void *s) { return les_advance_impl<double>(a, s); }
int spc_les_advance_f32(const spc_les_advance_args *a, void *s) { return les_advance_impl<float>(a, s); }

int spc_les_thermo_f64(const spc_les_thermo_args *a, void *s) { return les_thermo_impl<double>(a, s); }
int spc_les_thermo_f32(const spc_les_thermo_args *a, void *s) { return les_thermo_impl<float>(a, s); }

int spc_les_water_paths_f64(const spc_water_path_args *a, void *s) { return water_paths_impl<double>(a, s); }
int spc_les_water_paths_f32(const spc_water_path_args *a, void *s) { return water_paths_impl<float>(a, s); }

int spc_les_microphysics_f64(const spc_les_micro_args *a, void *s) { return les_micro_impl<double>(a, s); }
int spc_les_microphysics_f32(const spc_les_micro_args *a, void *s) { return les_micro_impl<float>(a, s); }

int spc_les_diffuse_f64(const spc_les_diffuse_args *a, void *s) { return les_diffuse_impl<double>(a, s); }
int spc_les_diffuse_f32(const spc_les_diffuse_args *a, void *s) { return les_diffuse_impl<float>(a, s); }
int spc_les_diffuse_cols_per_block(int ktot, int elem_size) { return col_cols(ktot, elem_size, 1, 0); }

int spc_les_advect_f64(const spc_les_advect_args *a, void *s) { return les_advect_impl<double>(a, s); }
int spc_les_advect_f32(const spc_les_advect_args *a, void *s) { return les_advect_impl<float>(a, s); }
int spc_les_advect_strip(int jtot, int ktot, int elem_size) { return advect_strip(jtot, ktot, elem_size); }
int spc_les_advect_rows(int64_t n_les, int itot, int jtot, int ktot) { return advect_rows(n_les, itot, jtot, ktot); }

int spc_les_vadvect_f64(const spc_les_vadvect_args *a, void *s) { return les_vadvect_impl<double>(a, s); }
int spc_les_vadvect_f32(const spc_les_vadvect_args *a, void *s) { return les_vadvect_impl<float>(a, s); }
int spc_les_vadvect_cols_per_block(int ktot, int elem_size) { return col_cols(ktot, elem_size, 1, 0); }
int spc_les_transport_f64(const spc_les_transport_args *a, void *s) { return les_transport_impl<double>(a, s); }
int spc_les_transport_f32(const spc_les_transport_args *a, void *s) { return les_transport_impl<float>(a, s); }
int spc_les_transport_cols_per_block(int ktot, int elem_size) { return col_cols(ktot, elem_size, 1, 0); }
int spc_les_transport2_f64(const spc_les_transport2_args *a, void *s) { return les_transport2_impl<double>(a, s); }
int spc_les_transport2_f32(const spc_les_transport2_args *a, void *s) { return les_transport2_impl<float>(a, s); }
int spc_les_transport2_cols_per_block(int ktot, int elem_size) { return col_cols(ktot, elem_size, 1, 0); }

int spc_les_radiate_f64(const spc_les_radiate_args *a, void *s) { return les_radiate_impl<double>(a, s); }
int spc_les_radiate_f32(const spc_les_radiate_args *a, void *s) { return les_radiate_impl<float>(a, s); }
int spc_les_radiate_cols_per_block(int ktot, int elem_size) { return col_cols(ktot, elem_size, 2, 1); }

int spc_les_qt_local_f64(const spc_les_qt_local_args *a, void *s) { return les_qt_local_impl<double>(a, s); }
int spc_les_qt_local_f32(const spc_les_qt_local_args *a, void *s) { return les_qt_local_impl<float>(a, s); }
int spc_les_qt_local_split(int64_t n_les, int itot, int jtot, int ktot, int elem_size) { return qtl_split(n_les, itot, jtot, ktot, elem_size); }

int spc_les_buoyancy_f64(const spc_les_buoyancy_args *a, void *s) { return les_buoyancy_impl<double>(a, s); }
int spc_les_buoyancy_f32(const spc_les_buoyancy_args *a, void *s) { return les_buoyancy_impl<float>(a, s); }
int spc_les_buoyancy_cols_per_block(int ktot, int elem_size) { return col_cols(ktot, elem_size, 1, 0); }

int spc_les_mix_f64(const spc_les_mix_args *a, void *s) { return les_mix_impl<double>(a, s); }
int spc_les_mix_f32(const spc_les_mix_args *a, void *s) { return les_mix_impl<float>(a, s); }
int spc_les_vmix_f64(const spc_les_vmix_args *a, void *s) { return les_vmix_impl<double>(a, s); }
int spc_les_vmix_f32(const spc_les_vmix_args *a, void *s) { return les_vmix_impl<float>(a, s); }
int spc_les_vmix_cols_per_block(int ktot, int elem_size) { return col_cols(ktot, elem_size, 2, 0); }
int spc_les_hmix_f64(const spc_les_hmix_args *a, void *s) { return les_hmix_impl<double>(a, s); }
int spc_les_hmix_f32(const spc_les_hmix_args *a, void *s) { return les_hmix_impl<float>(a, s); }
int spc_les_hmix_lines_per_block(int n, int elem_size) { return hline_lines(n, elem_size); }

int spc_les_moments_f64(const spc_les_moments_args *a, void *s) { return les_moments_impl<double>(a, s); }
int spc_les_moments_f32(const spc_les_moments_args *a, void *s) { return les_moments_impl<float>(a, s); }

int spc_abi_version(void) { return SPC_ABI_VERSION; }
const char *spc_last_error(void) { return g_err; }

int spc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int spc_describe_launch(const spc_dims *d, int pass, int flags, int esize, char *buf, int len) { return describe_launch_impl(d, pass, flags, esize, buf, len); }
int spc_pick_cols_per_block(const spc_dims *d, int pass) { return pick_cols_per_block_impl(d, pass); }

}  // extern "C"
