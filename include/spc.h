/*
 * spc.h -- C ABI of the MI355X-native batched superparameterization coupling step.
 *
 * The reference (CloudResolvingClimateModeling/sp-coupler) is pure Python and defines no FFI; its
 * boundary for this path is the Python call contract of splib/spcpl.py.  Each entry point below
 * replaces the *arithmetic* of one group of reference functions for ALL SP columns at once; the
 * Python host mirror (sp_coupler_amd/spcpl.py) keeps the reference's function names on top of it.
 *
 *   spc_forward_*        <- spcpl.convert_profiles        splib/spcpl.py:171-246
 *                           spcpl.set_les_forcings        splib/spcpl.py:299-385 (arithmetic 316-333)
 *                           spcpl.convert_surface_fluxes  splib/spcpl.py:136-167 (optional)
 *                           index map of get_les_profiles splib/spcpl.py:761-764 (optional, fused)
 *                           sputils.interp / iexner       splib/sputils.py:82-86, 33-34
 *   spc_cloud_indices_*  <- spcpl.get_cloud_fraction      splib/spcpl.py:22-29 (line 26)
 *                           spcpl.get_les_profiles        splib/spcpl.py:761-764
 *                           sputils.searchsorted          splib/sputils.py:88-91
 *   spc_backward_*       <- spcpl.set_gcm_tendencies      splib/spcpl.py:388-555 (arithmetic 402-533)
 *                           sputils.interp_c / integral   splib/sputils.py:94-189 (conservative=1)
 *   spc_surface_fluxes_* <- spcpl.convert_surface_fluxes  splib/spcpl.py:136-167 (columns without LES)
 *   spc_variability_nudge_f64 <- spcpl.variability_nudge  splib/spcpl.py:613-744 (qt_forcing == 'variance')
 *   spc_variability_nudge_f32    (the same on float32 fields)
 *   spc_diagnostics_*    <- spifs.nc diagnostics          splib/spcpl.py:176,214-215,408-409;
 *                           spcpl.output_column_conversion splib/spcpl.py:251-267
 *   spc_slab_means_* / spc_slab_cloud_fraction_*
 *                        <- les.get_profile_U/V/THL/QT/QL/... and les.get_cloudfraction(indices) as get_les_profiles calls
 *                           them (splib/spcpl.py:748-765, 629-630), from device-resident 3-D fields
 *   spc_les_advance_*    <- the step of a device-resident LES ensemble: forcings applied to the 3-D fields in place,
 *                           ql = max(qt - qsat, 0), and the slab means of the stepped fields, in one pass
 *   spc_les_thermo_*     <- the saturation adjustment of that ensemble (nothing of it is in the reference): Qsat, QL and
 *                           T of every cell from THL, QT and the pressure by a Newton iteration over a
 *                           saturation-pressure table, with the slab means of QL and T, in one pass
 *   spc_les_water_paths_* <- les.get_field("LWP" | "TWP" | "RWP") (splib/spdummy.py:243-251): the column water paths of
 *                           those fields, with the cloud top and the cloud cover, in one pass
 *   spc_les_radiate_*    <- the longwave cooling of that ensemble's cloud tops (nothing of it is in the reference): the
 *                           GCSS / DYCOMS-II parametrised flux of every column from its liquid water and the THL tendency
 *                           of its divergence, in one pass (kernel family K18)
 *   spc_les_buoyancy_*   <- the hydrostatic pressure force of that ensemble (nothing of it is in the reference): the buoyancy
 *                           of every column integrated downward to a pressure perturbation, whose horizontal gradient
 *                           accelerates U and V in place, in two launches (kernel family K21)
 *   spc_les_mix_*        <- the Smagorinsky-Lilly subgrid closure of that ensemble (nothing of it is in the reference): an eddy
 *                           viscosity per cell from the resolved deformation and the stratification, and the horizontal
 *                           mixing of the carried fields by it in flux form, in two launches (kernel family K24)
 *   spc_les_vmix_*       <- the implicit vertical mixing of that ensemble by each column's own eddy viscosity (nothing of it is
 *                           in the reference): the Thomas elimination per column in the kernel, K15's surface fluxes and a
 *                           neutral bulk drag on the lowest wind level, in two launches (kernel family K25)
 *   spc_les_hmix_*       <- the implicit horizontal mixing of that ensemble by each line's own eddy viscosity (nothing of it is
 *                           in the reference), without K24's cap: a cyclic tridiagonal elimination per periodic grid line in
 *                           the kernel, along i and then along j, in place, in two launches (kernel family K26)
 *   spc_exner_* / spc_interp_* / spc_searchsorted_* / spc_interp_c_* / spc_rms_*
 *                        <- the helpers of splib/sputils.py on their own (exner, iexner :28-34; interp :82-86;
 *                           searchsorted :88-91; integral, interp_c, interp_rho :94-197; rms :23-24), batched over rows
 *
 * Conventions
 *   - All data pointers are DEVICE pointers (HBM) owned by the caller; the library never allocates,
 *     frees or copies them and keeps no global state except the last-error string (thread local).
 *   - Element type is double for *_f64 and float for *_f32; index outputs are int32_t.
 *   - Arrays are row-major [n_cols x n_lev] with an explicit element pitch between columns.
 *       GCM full-level arrays   [n_cols x nG]     pitchG  (index 0 = model top, nG-1 = lowest level)
 *       GCM half-level arrays   [n_cols x (nG+1)] pitchGh (index nG = surface)
 *       LES arrays              [n_cols x nL]     pitchL  (index 0 = lowest level, ascending)
 *       per-column scalars      [n_cols]
 *     The LES grids zf / zh are [nL] shared by all columns when les_grid_shared != 0, else
 *     [n_cols x nL] with pitchL.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls only enqueue work.
 *   - Optional pointers may be NULL; the corresponding work/outputs are skipped.
 *   - Every function returns 0 on success or a negative spc_status; spc_last_error() gives the text.
 *     No C++ exception crosses the ABI.
 */
#ifndef SPC_H
#define SPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPC_ABI_VERSION 4

typedef enum spc_status {
    SPC_OK = 0,
    SPC_ERR_INVALID_ARGUMENT = -1, /* NULL required pointer, bad dims or pitches              */
    SPC_ERR_UNSUPPORTED = -2,      /* level counts exceed what the kernels' LDS staging holds */
    SPC_ERR_LAUNCH = -3,           /* hipLaunchKernel / runtime error (see spc_last_error)    */
    SPC_ERR_NO_DEVICE = -4         /* no HIP device available                                 */
} spc_status;

typedef struct spc_dims {
    int64_t n_cols;          /* number of SP columns in the batch (0 is allowed: no-op)          */
    int32_t nG;              /* GCM full levels (19 / 91 / 137 ...)                              */
    int32_t nL;              /* LES levels (160 / 512 ...)                                       */
    int64_t pitchG;          /* elements between columns of [n_cols x nG] arrays,   >= nG        */
    int64_t pitchGh;         /* elements between columns of [n_cols x nG+1] arrays, >= nG+1      */
    int64_t pitchL;          /* elements between columns of [n_cols x nL] arrays,   >= nL        */
    int32_t les_grid_shared; /* 1: zf/zh are [nL]; 0: zf/zh are [n_cols x nL]                    */
    int32_t cols_per_block;  /* tuning: columns per 256-thread workgroup (0 = library heuristic) */
} spc_dims;

/* ---- forward: GCM state -> LES profiles + nudging forcings (kernel K1, K2 fused) ------------- */
typedef struct spc_forward_args {
    /* GCM inputs, spcpl.gather_gcm_data var list (spcpl.py:32). `A` is not used by this pass. */
    const void *U, *V, *T, *SH, *QL, *QI, *Pf; /* [n_cols x nG]                                  */
    const void *Ph;                            /* [n_cols x nG+1]; only Ph[nG] (surface) is read */
    const void *Zgfull;                        /* [n_cols x nG]   geopotential, full levels      */
    const void *Zghalf;                        /* [n_cols x nG+1] geopotential, half levels      */
    /* LES grid and slab means (profile[...] of spcpl.py:310-315)                               */
    const void *zf;                            /* LES full-level heights (les.zf_cache)          */
    const void *zh;                            /* LES half-level heights; only needed for `idx`  */
    const void *u_d, *v_d, *thl_d, *qt_d, *ql_d; /* [n_cols x nL]                                */
    const void *ps_d;                          /* [n_cols]                                       */
    const void *rain, *rain_last;              /* [n_cols], optional (both or neither)           */
    double factor;                             /* les_forcing_factor                             */
    double dt;                                 /* dt_gcm in seconds                              */
    /* required outputs (what the 7 setters of spcpl.py:341-347 receive)                        */
    void *f_u, *f_v, *f_thl, *f_qt, *f_ql, *ql_ref; /* [n_cols x nL]                            */
    void *f_ps;                                /* [n_cols]                                       */
    /* optional outputs                                                                         */
    void *u, *v, *thl, *qt;                    /* [n_cols x nL] interpolated profiles (return value
                                                  of convert_profiles; ql == ql_ref)            */
    void *ps;                                  /* [n_cols] Ph[nG]                                */
    void *Zf;                                  /* [n_cols x nG]   les.gcm_Zf (spcpl.py:200)      */
    void *Zh;                                  /* [n_cols x nG+1] les.gcm_Zh (spcpl.py:201)      */
    void *rainrate;                            /* [n_cols] (rain-rain_last)/dt (spcpl.py:325)    */
    int32_t *idx;                              /* [n_cols x nG] pitchG: cloud-fraction level map,
                                                  searchsorted(zh,Zh,'right')[:-1][::-1]         */
    /* optional surface coupling (cplsurf): inputs [n_cols], outputs [n_cols]                   */
    const void *Z0M, *Z0H, *QLflux, *QIflux, *SHflux, *TSflux;
    void *z0m, *z0h, *wthl, *wqt;
} spc_forward_args;

int spc_forward_f64(const spc_dims *dims, const spc_forward_args *args, void *stream);
int spc_forward_f32(const spc_dims *dims, const spc_forward_args *args, void *stream);

/* ---- index map only (kernel K2 standalone) --------------------------------------------------- */
/* Zh: [n_cols x nG+1] heights of GCM half levels (descending, Zh[nG] = 0), as cached by forward.
 * idx[c][m] = searchsorted(zh, Zh[c], side='right')[nG-1-m], m = 0..nG-1; values in 0..nL.       */
int spc_cloud_indices_f64(const spc_dims *dims, const void *zh, const void *Zh, int32_t *idx, void *stream);
int spc_cloud_indices_f32(const spc_dims *dims, const void *zh, const void *Zh, int32_t *idx, void *stream);

/* ---- backward: LES slab means -> GCM tendencies (kernel K3; K4 when conservative) ------------ */
typedef struct spc_backward_args {
    const void *T, *SH, *QL, *QI, *U, *V, *A; /* [n_cols x nG] GCM state                        */
    const void *Zf;                           /* [n_cols x nG] les.gcm_Zf; may be NULL when
                                                 Zgfull and Zghalf are given (recomputed)       */
    const void *Zgfull, *Zghalf;              /* optional, see Zf                               */
    const void *zf;                           /* LES full-level heights                         */
    const void *t_d, *qt_d, *ql_d, *ql_ice_d, *u_d, *v_d; /* [n_cols x nL] profile[T,QT,QL,QL_ice,U,V] */
    const void *A_prof;                       /* [n_cols x nG] pitchG: profile["A"] in the order
                                                 get_cloudfraction(indices) returns it (ascending
                                                 height); reversed in-kernel (spcpl.py:404)     */
    /* conservative coarsening (sputils.interp_c); required only when conservative != 0        */
    const void *zh;                           /* LES half-level heights                         */
    const void *Zh;                           /* [n_cols x nG+1] or NULL with Zghalf given      */
    const void *rhobf_d;                      /* [n_cols x nL] profile["Rhobf"]                 */
    int32_t conservative;
    int32_t reserved;
    double factor;                            /* gcm_forcing_factor                             */
    double dt;                                /* dt_gcm in seconds                              */
    void *f_T, *f_SH, *f_QL, *f_QI, *f_U, *f_V, *f_A; /* [n_cols x nG] outputs                  */
    int32_t *start_index;                     /* [n_cols] optional                              */
} spc_backward_args;

int spc_backward_f64(const spc_dims *dims, const spc_backward_args *args, void *stream);
int spc_backward_f32(const spc_dims *dims, const spc_backward_args *args, void *stream);

/* ---- diagnostics for spifs.nc (kernel K5) ----------------------------------------------------- */
typedef struct spc_diagnostics_args {
    const void *T, *SH, *QL, *QI, *Pf;        /* [n_cols x nG]                                  */
    const void *Zgfull, *Zghalf;              /* geopotential                                   */
    const void *zf;                           /* LES heights; with thl_d, ql_d for `t`          */
    const void *thl_d, *ql_d, *ql_ice_d;      /* [n_cols x nL] optional                         */
    void *Tv, *THL, *QT;                      /* [n_cols x nG] optional outputs (spcpl.py:176,214,215) */
    void *Zf;                                 /* [n_cols x nG]   optional                       */
    void *Zh;                                 /* [n_cols x nG+1] optional                       */
    void *pf, *t, *ql_water;                  /* [n_cols x nL] optional (spcpl.py:408,409,402)  */
} spc_diagnostics_args;

int spc_diagnostics_f64(const spc_dims *dims, const spc_diagnostics_args *args, void *stream);
int spc_diagnostics_f32(const spc_dims *dims, const spc_diagnostics_args *args, void *stream);

/* ---- surface fluxes for columns without an LES (extra output columns) --------------------------- */
/* spcpl.convert_surface_fluxes (splib/spcpl.py:136-167) on per-column scalars [n]:
 *   rho = Ph_s/(rd*T_s); wqt = -(QLflux+QIflux+SHflux)/rho; wthl = -TSflux*iexner(Ph_s)/(cp*rho)
 * Ph_s = Phalf[:, nG], T_s = T[:, nG-1].  (z0m, z0h are passed through by the caller.)  For SP columns
 * the same arithmetic is fused into spc_forward_* (wthl / wqt outputs).                               */
int spc_surface_fluxes_f64(int64_t n, const void *Ph_s, const void *T_s, const void *QLflux, const void *QIflux,
                           const void *SHflux, const void *TSflux, void *wthl, void *wqt, void *stream);
int spc_surface_fluxes_f32(int64_t n, const void *Ph_s, const void *T_s, const void *QLflux, const void *QIflux,
                           const void *SHflux, const void *TSflux, void *wthl, void *wqt, void *stream);

/* ---- variability nudge (qt_forcing == 'variance'): spcpl.variability_nudge, splib/spcpl.py:613-744 ------------ */
/* 3-D LES fields in the reference's layout [n_cols][itot][jtot][ktot] (k fastest), float64 (float32: below).  For every level the
 * kernel finds beta (multiplicative, brentq on [0,5]) or a (additive noise a*R, brentq on [0,5]) such that the plane
 * mean of max(qt' - qsat, 0) equals ql_ref[k], updates qt in place (and thl with constantT), and returns beta, a,
 * qt.std(axis=(0,1)) and a status word per (column, level):
 *   bit 0 multiplicative root found, 1 "barely unsaturated" branch (spcpl.py:679-695), 2 additive root found,
 *   3 additive branch skipped (ql_ref <= ql_av), 4 no bracket -> beta_max; bit 8: brentq sign error (the reference
 *   raises ValueError there), bit 9: no convergence in 100 iterations (RuntimeError).
 * R: [n_cols][itot*jtot] the zero-mean Gaussian field of spcpl.py:620-621, drawn by the caller.  At most 32 767
 * columns per call.  With the workspace (`work`) planes of up to ~9 000 points (KT levels x itot*jtot x 16 B <= 150 KiB of
 * LDS, e.g. 64 x 64, 90 x 90) are solved from the CU's LDS and larger ones (96 x 96, 128 x 128, 256 x 256 ...) by one
 * workgroup per level streaming its contiguous transposed planes; the update and qt.std are two further launches.
 * Without the workspace planes that fit the LDS are loaded strided (slower) and larger ones are refused
 * (SPC_ERR_INVALID_ARGUMENT); results are bit-identical on every path.
 * spc_variability_nudge_f32: the same struct for float32 fields.  qt, qsat, thl, ql, ql_av, qt_av, presf, ql_ref and
 * qt_std point to float; R, beta and a_add stay double; status is int32_t.  It equals the reference's lines evaluated by
 * NumPy (2.x promotion rules) on float32 arrays: the multiplicative plane sums in float32 (brentq's iterate rounded to
 * float), the additive ones in float64 (a*R is float64), the qt increments in float64 rounded back to float, the constantT
 * correction and qt.std in float32.  beta, a, status, qt and qt_std are bit-identical to that; thl agrees to a few float
 * ulp (exner's powf).  Float planes take half the LDS: planes of up to ~18 000 points (128 x 128) are solved from LDS. */
typedef struct spc_vnudge_args {
    int64_t n_cols;
    int32_t itot, jtot, ktot;
    int32_t constantT;                 /* variability_nudge_constant_T */
    void *qt;                          /* [n][itot][jtot][ktot] in/out: les.get_field("QT") -> les.fields.QT  */
    const void *qsat;                  /* [n][itot][jtot][ktot] les.get_field("Qsat")                         */
    void *thl;                         /* in/out, constantT only: les.get_field("THL")                        */
    const void *ql;                    /* constantT only: les.get_field("QL")                                 */
    const void *R;                     /* [n][itot*jtot]                                                      */
    const void *ql_av, *qt_av, *presf; /* [n][ktot] les.get_profile("QL"/"QT"), les.get_presf()               */
    const void *ql_ref;                /* [n][ktot] les.ql_ref (K1's ql_ref output)                           */
    void *beta, *a_add, *qt_std;       /* [n][ktot] outputs                                                   */
    int32_t *status;                   /* [n][ktot] output                                                    */
    void *work;                        /* device scratch of work_bytes >= spc_vnudge_workspace_bytes(): qt and qsat as  */
    int64_t work_bytes;                /* contiguous planes; optional (NULL) only for planes that fit the LDS           */
} spc_vnudge_args;

int spc_variability_nudge_f64(const spc_vnudge_args *args, void *stream);
int spc_variability_nudge_f32(const spc_vnudge_args *args, void *stream);

/* ---- the helpers of splib/sputils.py as standalone batched operators (kernel family K7) ---------------------- */
/* The fused kernels above contain this arithmetic already; these entry points serve callers that use a helper on its
 * own (sp_coupler_amd/sputils.py keeps the reference's names on top of them).  A "row" is one independent 1-D problem
 * (one column); arrays are [n_rows x n] with an element pitch between rows; where stated a pitch of 0 means ONE row
 * shared by all rows (the LES grid).  Results are bit-identical to NumPy for interp / searchsorted / integral /
 * interp_c / interp_rho / rms; exner / iexner agree with numpy.power to <= 2 ulp.  Row pitches must stay below 2^24
 * elements (SPC_ERR_UNSUPPORTED otherwise): the kernels address a slab of rows with 24-bit multiplies.  A launch of ONE
 * row is exempt (its pitch is never multiplied), but the row itself must stay below 2^32 bytes, because elements are
 * addressed with 32-bit byte offsets: interp serves one row of up to 2^29 - 1 points (float: 2^30 - 1), searchsorted of up to
 * 2^29 - 1 keys (its indices are int64), interp_c of up to 2^29 - 2 layers (float: 2^30 - 2); SPC_ERR_UNSUPPORTED beyond.
 * spc_sputils_describe_launch (below, beside spc_describe_launch) tells which kernel and slab height a launch takes.   */

/* sputils.exner (inverse == 0) / iexner (inverse != 0), splib/sputils.py:28-34: out[i] = (p[i]/pref0)**(+-rd/cp)   */
int spc_exner_f64(int64_t n, const void *p, void *out, int32_t inverse, void *stream);
int spc_exner_f32(int64_t n, const void *p, void *out, int32_t inverse, void *stream);

/* sputils.interp, splib/sputils.py:82-86 == numpy.interp(x, xp, fp) per row (end-clamped, exact-hit shortcut, NaN
 * fallbacks; xp increasing; no left / right / period).  n_xp == 0 is refused as numpy does (ValueError).            */
typedef struct spc_interp_args {
    int64_t n_rows;
    int32_t n_x, n_xp;
    int64_t pitch_x, pitch_xp;     /* 0 = shared by all rows */
    int64_t pitch_fp, pitch_out;
    const void *x;                 /* [n_rows x n_x]  points to evaluate at   */
    const void *xp, *fp;           /* [n_rows x n_xp] sample points / values  */
    void *out;                     /* [n_rows x n_x]                          */
} spc_interp_args;
int spc_interp_f64(const spc_interp_args *args, void *stream);
int spc_interp_f32(const spc_interp_args *args, void *stream);

/* sputils.searchsorted, splib/sputils.py:88-91 == numpy.searchsorted(a, v, side) per row; NaN sorts to the end.    */
typedef struct spc_searchsorted_args {
    int64_t n_rows;
    int32_t n_a, n_v;
    int64_t pitch_a, pitch_v;      /* 0 = shared by all rows */
    int64_t pitch_out;
    const void *a;                 /* [n_rows x n_a] sorted ascending */
    const void *v;                 /* [n_rows x n_v]                  */
    int64_t *out;                  /* [n_rows x n_v] insertion indices (numpy's intp) */
    int32_t side_right;            /* 0: side='left', 1: side='right' */
    int32_t reserved;
} spc_searchsorted_args;
int spc_searchsorted_f64(const spc_searchsorted_args *args, void *stream);
int spc_searchsorted_f32(const spc_searchsorted_args *args, void *stream);

/* sputils.integral / interp_c / interp_rho, splib/sputils.py:94-197.  Per row: Zh [nG+1] coarse layer bounds
 * (descending in the reference's use), zh [nL] fine grid points (ascending; they bound nL-1 cells), q [>= nL-1] cell
 * values, rho cell weights.
 *   mode 0 interp_c  : out[k] = integral(Zh[k+1], Zh[k], zh, q, rho) where Zh[k] < zh[nL-1], else 0 (sputils.py:185-188)
 *   mode 1 interp_rho: out[k] = integral(Zh[k+1], Zh[k], zh, q) / (Zh[k] - Zh[k+1]) where Zh[k] < zh[nL-1], else 0
 *                      (sputils.py:191-197; q is the density, rho is ignored)
 *   mode 2 integral  : out[k] = integral(Zh[k+1], Zh[k], zh, q, rho or NULL), no test against the top
 * Where integral() returns None (an end point outside zh) the output is NaN (what Q[i] = None stores).  Sums in
 * numpy's ndarray.sum() order.                                                                                      */
typedef struct spc_interp_c_args {
    int64_t n_rows;
    int32_t nG, nL;
    int64_t pitch_Zh;
    int64_t pitch_zh;              /* 0 = shared by all rows */
    int64_t pitch_q;               /* of q and rho           */
    int64_t pitch_out;
    const void *Zh, *zh, *q, *rho;
    void *out;                     /* [n_rows x nG]          */
    int32_t mode;
    int32_t reserved;
} spc_interp_c_args;
int spc_interp_c_f64(const spc_interp_c_args *args, void *stream);
int spc_interp_c_f32(const spc_interp_c_args *args, void *stream);

/* sputils.rms, splib/sputils.py:23-24: out[r] = sqrt(mean(a[r]**2)), the mean in numpy's pairwise order             */
int spc_rms_f64(int64_t n_rows, int64_t n, int64_t pitch, const void *a, void *out, void *stream);
int spc_rms_f32(int64_t n_rows, int64_t n, int64_t pitch, const void *a, void *out, void *stream);

/* ---- geometry of sputils.get_mask_indices, splib/sputils.py:46-73 (kernel family K8) ------------------------- */
/* Which GCM columns get an LES.  Everything is double, whatever the engine's dtype.
 * spc_point_in_polygon_f64: the location of every point p = (lon, lat) and of its image q = ((lon - 180) % 360 - 180,
 * lat) (Python's float %) in every polygon of the launch, in exact arithmetic, by GEOS's ray-crossing and point-locator
 * rules.  The vertices of all rings are concatenated in vx / vy; ring r is vertices
 * ring_start[r] ... ring_start[r+1]-1, CLOSED (last vertex == first).  Rings are grouped by polygon: ring_poly is
 * non-decreasing, and every polygon's first ring is its shell (SPC_RING_SHELL, or SPC_RING_RECTANGLE for an axis-aligned
 * rectangle without holes: strictly-inside rule of GEOS's RectangleContains), its holes follow (SPC_RING_HOLE).
 * out[k * n_points + i] = code of p | code of q << 8 in polygon k, codes SPC_LOC_*.  A point whose lon or lat is NaN or
 * +-inf is SPC_LOC_EXTERIOR to every polygon, as p and as q, under the ray rule and under the rectangle rule alike (no
 * arithmetic is done on it).  A polygon id that comes back after another polygon's rings starts that polygon anew, shell
 * first, and its codes replace the ones written for the id before.  Any other layout that breaks these rules gives
 * undefined codes, never an access outside the arrays.  All arrays are device memory.
 * spc_haversine_f64: out[i] = great-circle distance in km from (lon[i], lat[i]) to (lon0, lat0), splib/haversine.py:12-36
 * operation by operation (R = 6371 km).                                                                              */
#define SPC_RING_SHELL 0
#define SPC_RING_HOLE 1
#define SPC_RING_RECTANGLE 2
#define SPC_LOC_EXTERIOR 0
#define SPC_LOC_BOUNDARY 1
#define SPC_LOC_INTERIOR 2
typedef struct spc_pip_args {
    int64_t n_points;
    int64_t n_vertices;
    int32_t n_rings, n_polys;
    const double *lon, *lat;       /* [n_points] grid point coordinates (degrees)                   */
    const double *vx, *vy;         /* [n_vertices] ring vertices, rings one after another, closed   */
    const int64_t *ring_start;     /* [n_rings + 1] first vertex of each ring; ring_start[n_rings] == n_vertices */
    const int32_t *ring_role;      /* [n_rings] SPC_RING_SHELL / SPC_RING_HOLE / SPC_RING_RECTANGLE  */
    const int32_t *ring_poly;      /* [n_rings] polygon id 0 ... n_polys-1, non-decreasing          */
    uint16_t *out;                 /* [n_polys x n_points] location codes                           */
} spc_pip_args;
int spc_point_in_polygon_f64(const spc_pip_args *args, void *stream);
int spc_haversine_f64(int64_t n, const void *lon, const void *lat, double lon0, double lat0, void *out, void *stream);

/* ---- initial LES state of spcpl.set_les_state, splib/spcpl.py:274-294 (kernel family K9) ------------------------- */
/* For every LES l in list order and every field f = U, V, THL, QT in that order:
 *   out[f][elem_off[l] + idx] = amp[f] * numpy.random.uniform(-1., 1.)[idx] + prof[f][l * pitch_prof + idx % ktot[l]]
 * for idx = 0 ... elem_off[l+1] - elem_off[l] - 1 (C order, ktot fastest), drawn from NumPy's legacy MT19937 state
 * (key_in, pos_in) exactly as the reference loop draws them, in float64, bit for bit.  Also returns the state NumPy holds
 * afterwards (key_out, pos_out; has_gauss / cached_gaussian are not touched).  The substream starts are computed on the
 * device by jump-ahead; the final state is the generation the launch twisted last, so it equals
 * NumPy's in every bit.  key_in / elem_off / ktot / key_out / pos_out are HOST memory, prof / out / work device memory.
 * The call is synchronous: it returns once the fields are written and the final state is on the host.
 * gens_per_substream: 0 = chosen from the device's compute units; > 0 forces it (tests: many substream boundaries).      */
typedef struct spc_les_state_args {
    int64_t n_les;
    const int64_t *elem_off;       /* host [n_les + 1], elem_off[0] == 0, non-decreasing: itot*jtot*ktot per LES  */
    const int32_t *ktot;           /* host [n_les] >= 1, dividing the LES's element count                         */
    const double *prof[4];         /* device [n_les x pitch_prof] u, v, thl, qt profiles (ktot[l] <= pitch_prof)   */
    int64_t pitch_prof;
    double amp[4];                 /* 0.5, 0.5, 0.1, 2.5e-5 in the reference (spcpl.py:285-287)                   */
    double *out[4];                /* device [elem_off[n_les]] each                                               */
    const uint32_t *key_in;        /* host [624] numpy.random.get_state()[1]                                      */
    int32_t pos_in;                /* 0 ... 624                                                                    */
    int32_t reserved;
    uint32_t *key_out;             /* host [624]                                                                   */
    int32_t *pos_out;              /* host                                                                         */
    int64_t gens_per_substream;
    void *work;                    /* device scratch of work_bytes >= spc_les_state_workspace_bytes()              */
    int64_t work_bytes;
} spc_les_state_args;
int spc_les_state_f64(const spc_les_state_args *args, void *stream);
/* Bytes of spc_les_state_args.work for n_les LES holding n_elems = elem_off[n_les] elements per field, on the current
 * device; negative spc_status on bad extents. */
int64_t spc_les_state_workspace_bytes(int64_t n_les, int64_t n_elems, int32_t pos_in, int64_t gens_per_substream);
/* NumPy's MT19937 state after drawing n_words 32-bit words from (key_in, pos_in), computed on the host by jump-ahead
 * (Berlekamp-Massey for the characteristic polynomial, x^J mod phi by square-and-multiply); no device needed.  Equal to
 * NumPy's state in every bit (the last generation is twisted for real).  pos_in 0 ... 624, n_words >= 0. */
int spc_mt19937_jump(const uint32_t *key_in, int32_t pos_in, int64_t n_words, uint32_t *key_out, int32_t *pos_out);
/* x^J mod phi as 312 little-endian 64-bit words (bit i = coefficient of x^i); J = 0 ... 2^63 - 1.  J = 19937 gives phi
 * minus its leading term: tests re-derive phi from it. */
int spc_mt19937_jump_poly(uint64_t J, uint64_t *out);

/* ---- horizontal reductions of the LES 3-D fields (kernel family K10) --------------------------------------------- */
/* What les.get_profile_U/V/THL/QT/QL/... (splib/spcpl.py:748-759, 629-630) and les.get_cloudfraction(indices)
 * (spcpl.py:764-765) return, computed from device-resident fields [n_les][itot][jtot][ktot] (C order, ktot contiguous,
 * element type of the entry point).  A field may exceed 4 GiB: offsets are 64-bit.
 * spc_slab_means_*: out[f][l * pitch_out + k] = numpy.mean(fields[f][l], axis=(0, 1))[k] for f < n_fields, bit for bit:
 * the sequential sum over (i, j) in row-major order in the element type, then one division by itot * jtot.  All fields of
 * a launch have one shape; 1 <= n_fields <= SPC_SLAB_MAX_FIELDS.
 * spc_slab_cloud_fraction_*: idx [n_les x nG] is K2's index map (spc_cloud_indices_*: idx[r] = LES half levels at or below
 * the upper boundary of GCM layer r counted from the ground).  Layer r holds the LES levels [hi[r-1], hi[r]),
 * hi[r] = clip(idx[r], 0, ktot), hi[-1] = 0, and
 *   out[l * pitch_out + r] = (number of (i, j) with ql[l][i][j][k] > 0 for some k of layer r) / (itot * jtot), 0 for an empty
 * layer; NaN and -0.0 are not cloudy.  The count is an integer: the result is exact.  At most 65 535 LES, 2 048 layers per
 * launch.  This rule is the project's definition (the reference reaches DALES's routine through OMUSE).   */
#define SPC_SLAB_MAX_FIELDS 16
typedef struct spc_slab_means_args {
    int64_t n_les;                 /* 0 is allowed: no-op                                                  */
    int32_t itot, jtot, ktot;
    int32_t n_fields;
    const void *fields[SPC_SLAB_MAX_FIELDS]; /* device [n_les][itot][jtot][ktot] each                      */
    void *out[SPC_SLAB_MAX_FIELDS];          /* device [n_les x ktot] each, rows pitch_out apart           */
    int64_t pitch_out;             /* >= ktot                                                              */
} spc_slab_means_args;
int spc_slab_means_f64(const spc_slab_means_args *args, void *stream);
int spc_slab_means_f32(const spc_slab_means_args *args, void *stream);

typedef struct spc_slab_cloud_args {
    int64_t n_les;
    int32_t itot, jtot, ktot;
    int32_t nG;
    const void *ql;                /* device [n_les][itot][jtot][ktot]                                     */
    const int32_t *idx;            /* device [n_les x nG], rows pitch_idx apart                            */
    void *out;                     /* device [n_les x nG], rows pitch_out apart, element type of the field */
    int64_t pitch_idx, pitch_out;  /* >= nG                                                                */
} spc_slab_cloud_args;
int spc_slab_cloud_fraction_f64(const spc_slab_cloud_args *args, void *stream);
int spc_slab_cloud_fraction_f32(const spc_slab_cloud_args *args, void *stream);

/* ---- one step of the device-resident LES fields, with the slab means of the stepped fields (kernel family K11) --- */
/* The forcings applied to fields [n_les][itot][jtot][ktot] of one shape (layout and offsets as K10), the saturation
 * adjustment of the ensemble (ql = max(qt - qsat, 0)) and the slab means of the NEW fields, in one pass over the fields:
 *   for f < n_fields, where tend[f] != NULL:                       (a field without a tendency keeps its bits)
 *       inc[l][k]             = tend[f][l * pitch_tend + k] * (T)dt             one rounding in the element type T
 *       fields[f][l][i][j][k] = fields[f][l][i][j][k] + inc[l][k]               one rounding, IN PLACE, never an fma
 *   if sat_field >= 0:                                             (fields[sat_field] is QT, AFTER its update)
 *       d = fields[sat_field][l][i][j][k] - qsat[l][i][j][k]
 *       q = d > 0 ? d : (d != d ? d : +0.0)                        NaN stays NaN; -0.0 and negatives give +0.0
 *       ql[l][i][j][k] = q  where ql != NULL
 *   mean[f][l * pitch_mean + k] = numpy.mean(new fields[f][l], axis=(0, 1))[k]  where mean[f] != NULL, and ql_mean of q:
 *       spc_slab_means_*'s rule, bit for bit (sequential sum from +0 over (i, j) in row-major order in T, one division).
 * qsat, ql and ql_mean are ignored when sat_field == -1.  ql must not be a field or qsat; qsat must not be a field; the
 * fields must differ.  ktot == 1 is SPC_ERR_UNSUPPORTED (numpy reduces a one-level plane pairwise: step the field and call
 * spc_slab_means_*).  The q rule is this library's definition; it equals numpy.maximum(d, 0) and differs from torch's
 * clamp_min on the CPU only for d == -0.0.  tend and mean are device pointers with a row pitch, so the
 * launch can read K1's outputs and write K1 / K3's inputs in place.                                                   */
#define SPC_ADVANCE_MAX_FIELDS 8
typedef struct spc_les_advance_args {
    int64_t n_les;                 /* 0 is allowed: no-op                                                  */
    int32_t itot, jtot, ktot;
    int32_t n_fields;              /* 1 ... SPC_ADVANCE_MAX_FIELDS                                         */
    void *fields[8];               /* device [n_les][itot][jtot][ktot] each, updated in place              */
    const void *tend[8];           /* device [n_les x ktot] each, rows pitch_tend apart, or NULL           */
    void *mean[8];                 /* device [n_les x ktot] each, rows pitch_mean apart, or NULL           */
    int64_t pitch_tend, pitch_mean; /* >= ktot                                                             */
    double dt;                     /* rounded to the element type once                                     */
    int32_t sat_field, reserved;   /* index of QT in fields, or -1: no saturation adjustment               */
    const void *qsat;              /* device [n_les][itot][jtot][ktot]; required when sat_field >= 0       */
    void *ql;                      /* device [n_les][itot][jtot][ktot], or NULL                            */
    void *ql_mean;                 /* device [n_les x ktot], rows pitch_mean apart, or NULL                */
} spc_les_advance_args;
int spc_les_advance_f64(const spc_les_advance_args *args, void *stream);
int spc_les_advance_f32(const spc_les_advance_args *args, void *stream);

/* ---- saturation adjustment of the device-resident LES fields, with the slab means of QL and T (kernel family K12) --- */
/* Per cell (l, i, j, k) of fields [n_les][itot][jtot][ktot] (layout and offsets as K10), in the element type T, one rounding
 * per operation, never an fma.  Constants: eps = T(rd) / T(rv), om = T(1) - eps, c = T(rlv) / T(cp) (rd 287.04, rv 461.5,
 * cp 1004, rlv 2.53e6), lo = T(t_lo), s = T(inv_step), hi = T(t_lo + (n_tab - 1) / inv_step) (formed in double);
 * p = presf[l * pitch_prof + k]:
 *   Tl = thl * ex[l * pitch_prof + k]
 *   sat(Tk):  Tc  = Tk < lo ? lo : (Tk > hi ? hi : Tk)                        (NaN passes through)
 *             x   = (Tc - lo) * s
 *             m   = x >= 0 ? min((int)x, n_tab - 2) : 0                       (truncation; NaN gives m = 0)
 *             w   = x - T(m);   d = es_tab[m + 1] - es_tab[m];   e = es_tab[m] + w * d
 *             den = p - om * e
 *             qs  = (eps * e) / den
 *             dqs = ((eps * p) * (d * s)) / (den * den)
 *   Tk = Tl
 *   n_iter times:  qs, dqs = sat(Tk)
 *                  Tk = qt > qs ? Tk - ((Tk - Tl) - c * (qt - qs)) / (T(1) + c * dqs) : Tl
 *   qs, _ = sat(Tk)
 *   dq = qt - qs;   q = dq > 0 ? dq : (dq != dq ? dq : +0.0)                   (the q rule of spc_les_advance_*)
 *   t  = Tl + (T(rlv) * q) / T(cp)
 *   qsat[l][i][j][k] = qs;   ql[l][i][j][k] = q;   temp[l][i][j][k] = t  where temp != NULL
 *   ql_mean, t_mean [l * pitch_mean + k] = the slab means of q and t by spc_slab_means_*'s rule, bit for bit (sequential sum
 *       from +0 over (i, j) in row-major order in T, one division); each where its pointer != NULL.
 * den <= 0 is not guarded: IEEE decides.  The kernel calls no transcendental function: es_tab (saturation pressure over
 * water at t_lo + m / inv_step, sp_coupler_amd/thermo.py) and ex (the Exner factor (presf / 1e5) ** (rd / cp)) are inputs.
 * thl and qt are read only; no output may be one of the inputs or another output.  ktot == 1 is SPC_ERR_UNSUPPORTED, as in
 * spc_les_advance_*.  The rule is this library's definition.                                           */
typedef struct spc_les_thermo_args {
    int64_t n_les;                 /* 0 is allowed: no-op                                                  */
    int32_t itot, jtot, ktot;
    int32_t n_iter;                /* >= 0 Newton iterations                                               */
    const void *thl, *qt;          /* device [n_les][itot][jtot][ktot], read only                          */
    const void *presf, *ex;        /* device [n_les x ktot] each, rows pitch_prof apart                    */
    int64_t pitch_prof;            /* >= ktot                                                              */
    const void *es_tab;            /* device [n_tab], element type of the fields                           */
    int32_t n_tab;                 /* >= 2                                                                 */
    int32_t table_mode;            /* tuning: 0 library's choice, 1 table staged in LDS, 2 read from global memory */
    double t_lo, inv_step;         /* temperature of es_tab[0]; entries per kelvin                         */
    void *qsat, *ql;               /* device [n_les][itot][jtot][ktot]                                     */
    void *temp;                    /* device [n_les][itot][jtot][ktot], or NULL                            */
    void *ql_mean, *t_mean;        /* device [n_les x ktot] each, rows pitch_mean apart, or NULL           */
    int64_t pitch_mean;            /* >= ktot                                                              */
} spc_les_thermo_args;
int spc_les_thermo_f64(const spc_les_thermo_args *args, void *stream);
int spc_les_thermo_f32(const spc_les_thermo_args *args, void *stream);

/* ---- column water paths, cloud top and cloud cover of the device-resident LES fields (kernel family K13) ----------- */
/* What les.get_field("LWP" | "TWP" | "RWP") (splib/spdummy.py:243-251) returns, for every LES at once, from fields
 * [n_les][itot][jtot][ktot] of one shape (layout and offsets as K10) and ONE weight profile w [n_les x ktot] (rho * dz):
 *   out[f][l][i][j] = numpy.add.reduce(fields[f][l, i, j, :] * w[l, :])       for f < n_fields, bit for bit:
 * the product rounded on its own in the element type T (never an fma), then the row of ktot products summed as
 * ndarray.sum() sums a contiguous run: 0 + pairwise blocks of at most 128 elements with eight accumulators, halves split
 * at multiples of 8, the remainder of a block added in order; rows of fewer than 8 elements sequentially.  NaN and
 * infinities propagate as NumPy's do (inf * 0 is NaN); a row of -0.0 products gives +0.0.
 * With cloud_field = c >= 0 the same pass over fields[c] also gives, each where its pointer != NULL:
 *   top[l][i][j] = the largest k with fields[c][l, i, j, k] > 0, else -1       NaN and -0.0 are not cloudy (K10's rule)
 *   cover[l]     = T(number of (i, j) with top >= 0) / T(itot * jtot)          an integer count, one IEEE division: exact
 * ktot > 8192 (NumPy's chunk boundary) is SPC_ERR_UNSUPPORTED.  No output may be an input or another output.          */
#define SPC_WP_MAX_FIELDS 4
typedef struct spc_water_path_args {
    int64_t n_les;                 /* 0 is allowed: no-op                                                  */
    int32_t itot, jtot, ktot;
    int32_t n_fields;              /* 1 ... SPC_WP_MAX_FIELDS                                              */
    const void *fields[SPC_WP_MAX_FIELDS]; /* device [n_les][itot][jtot][ktot] each, read only             */
    void *out[SPC_WP_MAX_FIELDS];          /* device [n_les][itot][jtot] each, contiguous                  */
    const void *w;                 /* device [n_les x ktot], rows pitch_w apart                            */
    int64_t pitch_w;               /* >= ktot                                                              */
    int32_t cloud_field;           /* -1, or the field the cloud outputs are taken from                    */
    int32_t reserved;              /* 0                                                                    */
    int32_t *top;                  /* device [n_les][itot][jtot], or NULL                                  */
    void *cover;                   /* device [n_les], element type of the fields, or NULL                  */
} spc_water_path_args;
typedef spc_water_path_args SpcWaterPathArgs;
int spc_les_water_paths_f64(const spc_water_path_args *args, void *stream);
int spc_les_water_paths_f32(const spc_water_path_args *args, void *stream);

/* ---- warm-rain microphysics of the device-resident LES fields, with the slab means of what it changes (kernel family K14) --- */
/* Cloud water turns into rain (autoconversion above the threshold qc0, accretion by the rain that is there), rain falls one
 * upwind step and what leaves the lowest level is added to the surface rain; the cloud ice is a share of the remaining cloud
 * water that is linear in the temperature between t_dn and t_up.  Fields are [n_les][itot][jtot][ktot] (layout and offsets as
 * K10), element type T; every operation is rounded once in T, never an fma.  Profiles are [n_les x ktot], rows pitch_prof
 * apart: sed_out (the share of a layer's rain that leaves it in dt, 0 ... 1), sed_in (the same flux expressed in the layer
 * below), lcpex ((rlv / cp) / exner) and w (rho * dz, K13's weight profile); sp_coupler_amd/microphysics.py builds them.
 * Scalars, rounded to T once: qc0 = T(qc0), ka = T(T(k_auto) * T(dt)), kc = T(T(k_acc) * T(dt)), tu = T(t_up), td = T(t_dn),
 * den = tu - td.  Per cell (l, i, j, k), with qr_up = k + 1 < ktot ? qr[l][i][j][k + 1] : +0.0 (the OLD qr):
 *   out  = sed_out[l][k] * qr
 *   qs   = (qr - out) + sed_in[l][k] * qr_up                  sedimentation, upwind, the old qr on both sides
 *   d    = ql - qc0;   x = d > 0 ? d : (d != d ? d : +0.0)    the q rule of spc_les_advance_*
 *   s    = ka * x + (kc * ql) * qs                            autoconversion + accretion: product, product, one add
 *   s    = s > ql ? ql : s                                    never more than the cloud water; NaN stays NaN
 *   qt   = qt - s                                             IN PLACE
 *   thl  = thl + lcpex[l][k] * s                              IN PLACE, where thl != NULL
 *   qr_new[l][i][j][k] = qs + s                               a SEPARATE buffer: the neighbour below reads the old qr
 *   rain[l][i][j] = rain[l][i][j] + (sed_out[l][0] * qr[l][i][j][0]) * w[l][0]      IN PLACE, where rain != NULL
 *   fi   = temp >= tu ? 0 : (temp <= td ? 1 : (tu - temp) / den)                    where temp != NULL
 *   qi   = (ql - s) * fi
 *   qt_mean, thl_mean, qr_mean, qi_mean [l * pitch_mean + k] = the slab means of the NEW qt, the NEW thl, qr_new and qi by
 *       spc_slab_means_*'s rule, bit for bit (sequential sum from +0 over (i, j) in row-major order in T, one division);
 *       each where its pointer != NULL.
 * ql, qr and temp are read only.  lcpex is required with thl, w with rain; thl_mean needs thl, qi_mean needs temp.  qr_new
 * must not be any other argument, no written array may be another written array or an input: SPC_ERR_INVALID_ARGUMENT
 * where two such pointers are EQUAL; arrays that overlap in part are not detected and must not be passed.
 * ktot == 1 is SPC_ERR_UNSUPPORTED, as in spc_les_advance_*.  The rule is this library's definition.     */
typedef struct spc_les_micro_args {
    int64_t n_les;                 /* 0 is allowed: no-op                                                  */
    int32_t itot, jtot, ktot;
    int32_t reserved;              /* 0                                                                    */
    void *qt;                      /* device [n_les][itot][jtot][ktot], updated in place                   */
    const void *ql, *qr;           /* device [n_les][itot][jtot][ktot], read only                          */
    void *qr_new;                  /* device [n_les][itot][jtot][ktot], written whole                      */
    void *thl;                     /* device [n_les][itot][jtot][ktot], updated in place, or NULL          */
    const void *temp;              /* device [n_les][itot][jtot][ktot], read only, or NULL                 */
    void *rain;                    /* device [n_les][itot][jtot], contiguous, updated in place, or NULL    */
    const void *sed_out, *sed_in;  /* device [n_les x ktot] each, rows pitch_prof apart                    */
    const void *lcpex, *w;         /* the same; lcpex may be NULL without thl, w without rain              */
    int64_t pitch_prof;            /* >= ktot                                                              */
    double dt, qc0, k_auto, k_acc, t_up, t_dn;   /* rounded to the element type as stated above            */
    void *qt_mean, *thl_mean, *qr_mean, *qi_mean; /* device [n_les x ktot] each, rows pitch_mean apart, or NULL */
    int64_t pitch_mean;            /* >= ktot                                                              */
} spc_les_micro_args;
int spc_les_microphysics_f64(const spc_les_micro_args *args, void *stream);
int spc_les_microphysics_f32(const spc_les_micro_args *args, void *stream);

/* ---- implicit vertical diffusion and surface fluxes of the device-resident LES fields (kernel family K15) -------------------- */
/* One backward-Euler step of d(x)/dt = (1 / (rho dz)) d/dz (rho_h K dx/dz) per column, the kinematic surface flux (positive
 * upward) entering the lowest layer, solved by the Thomas algorithm.  The matrix depends on (l, k) only, so the elimination is
 * done ONCE per LES on the host in float64 (sp_coupler_amd/diffusion.py: profiles): a is the lower diagonal, m the reciprocal
 * pivots, cp the eliminated upper diagonal, [n_les x ktot] each, rows pitch_prof apart; s0 = dt / dz[0], [n_les].  Fields are
 * [n_les][itot][jtot][ktot] (layout and offsets as K10), element type T; every operation is rounded once in T, never an fma,
 * and the kernel holds no division.  Per column (l, i, j) of each field f:
 *   d    = flux[f] != NULL ? x[0] + s0[l] * flux[f][l] : x[0]      the product rounded, then the add; no add without a flux
 *   y[0] = d * m[l][0]
 *   y[k] = (x[k] - a[l][k] * y[k-1]) * m[l][k]                     k = 1 ... ktot - 1: product, subtraction, product
 *   x'[ktot-1] = y[ktot-1]
 *   x'[k] = y[k] - cp[l][k] * x'[k+1]                              k = ktot - 2 ... 0: product, subtraction
 * x' replaces x IN PLACE.  ktot == 1 is allowed.  Special values get no rule of their own: a NaN or an infinity spreads through
 * its own column as the recurrence dictates and reaches no other column.  With a = 0, m = 1, cp = 0 and no flux a field keeps
 * its bits.  Two EQUAL fields pointers, a field equal to a profile, s0 or its flux, and a flux without s0 are
 * SPC_ERR_INVALID_ARGUMENT; arrays that overlap in part are not detected and must not be passed.  A workgroup takes
 * spc_les_diffuse_cols_per_block(ktot, sizeof(T)) columns into LDS; above the largest ktot of which 16 columns fit (1 279 levels
 * of 8 bytes, 2 559 of 4) the launch is SPC_ERR_UNSUPPORTED.  The rule is this library's definition.      */
#define SPC_DIFFUSE_MAX_FIELDS 4
typedef struct spc_les_diffuse_args {
    int64_t n_les;                      /* 0 is allowed: no-op                                               */
    int32_t itot, jtot, ktot, n_fields; /* n_fields 1 ... SPC_DIFFUSE_MAX_FIELDS                             */
    void *fields[SPC_DIFFUSE_MAX_FIELDS];      /* device [n_les][itot][jtot][ktot], updated in place         */
    const void *flux[SPC_DIFFUSE_MAX_FIELDS];  /* device [n_les], the kinematic surface flux, or NULL        */
    const void *a, *m, *cp;             /* device [n_les x ktot] each, rows pitch_prof apart                 */
    const void *s0;                     /* device [n_les]; may be NULL when every flux is NULL               */
    int64_t pitch_prof;                 /* >= ktot                                                           */
} spc_les_diffuse_args;
int spc_les_diffuse_f64(const spc_les_diffuse_args *args, void *stream);
int spc_les_diffuse_f32(const spc_les_diffuse_args *args, void *stream);
/* columns per workgroup of k_les_diffuse for ktot levels of elem_size (4 or 8) bytes: 64, 32 or 16; 0: unsupported */
int spc_les_diffuse_cols_per_block(int ktot, int elem_size);

/* ---- horizontal upwind advection of the device-resident LES fields on the doubly periodic plane (kernel family K16) ------------ */
/* One explicit first-order upwind step in advective form from face Courant numbers.  Fields, u and v are
 * [n_les][itot][jtot][ktot] (layout and offsets as K10), element type T; every operation is rounded once in T, never an fma, and
 * the kernel holds no division.  Per LES l the caller hands in hx[l] = 0.5 * dt / dx[l] and hy[l] = 0.5 * dt / dy[l]
 * (sp_coupler_amd/advection.py forms them in float64; they are rounded to T once).  The neighbours wrap: im = (i - 1 + itot) %
 * itot, ip = (i + 1) % itot, jm = (j - 1 + jtot) % jtot, jp = (j + 1) % jtot (an extent of 1: the cell itself; of 2: both
 * neighbours are the same cell).  Per cell (l, i, j, k), every array at level k of LES l:
 *   cw = (u[im][j] + u[i][j]) * hx[l];   ce = (u[i][j] + u[ip][j]) * hx[l]        the add rounded, then the product
 *   cs = (v[i][jm] + v[i][j]) * hy[l];   cn = (v[i][j] + v[i][jp]) * hy[l]
 *   pw = cw > 0 ? cw : 0;   pe = ce < 0 ? -ce : 0;   ps = cs > 0 ? cs : 0;   pn = cn < 0 ? -cn : 0     a NaN face gives +0
 *   out[f] = (((x + pw * (x[im][j] - x)) + pe * (x[ip][j] - x)) + ps * (x[i][jm] - x)) + pn * (x[i][jp] - x)     x = fields[f]
 *   s  = ((pw + pe) + ps) + pn;          cmax[l] = the maximum of s over the cells of LES l (the launch zeroes it first)
 * u, v and the fields are read only; a field may be u or v itself (the winds are advected by the old winds).  Every out[f] is
 * written whole.  s is never NaN and never negative, so cmax does not depend on the order of the cells.  With s <= 1 out[f] is
 * a convex combination of the cell and its four neighbours; a constant finite field keeps its bits (a -0.0 constant comes out
 * +0.0).  Special values get no rule of their own: a NaN or an infinity of a field reaches at most its four neighbours, a NaN
 * wind closes the faces it touches.  n_fields == 0 with cmax is the probe: only the winds are read.  n_fields == 0 without
 * cmax, an out[f] EQUAL to u, v, hx, hy, cmax, a field or another out, and cmax EQUAL to an input are
 * SPC_ERR_INVALID_ARGUMENT; arrays that overlap in part are not detected and must not be passed.  ktot == 1 is allowed.  A
 * workgroup owns spc_les_advect_strip(jtot, ktot, sizeof(T)) consecutive cells of the run [jtot][ktot] of one row i and
 * spc_les_advect_rows(n_les, itot, jtot, ktot) consecutive rows.  The rule is this library's definition.                          */
#define SPC_ADVECT_MAX_FIELDS 6
typedef struct spc_les_advect_args {
    int64_t n_les;                      /* 0 is allowed: no-op                                               */
    int32_t itot, jtot, ktot, n_fields; /* n_fields 0 ... SPC_ADVECT_MAX_FIELDS                              */
    const void *u, *v;                  /* device [n_les][itot][jtot][ktot], read only                       */
    const void *fields[SPC_ADVECT_MAX_FIELDS];  /* device [n_les][itot][jtot][ktot], read only               */
    void *out[SPC_ADVECT_MAX_FIELDS];   /* device [n_les][itot][jtot][ktot], written whole                   */
    const void *hx, *hy;                /* device [n_les]: 0.5 dt / dx and 0.5 dt / dy                       */
    void *cmax;                         /* device [n_les], or NULL where n_fields > 0                        */
} spc_les_advect_args;
int spc_les_advect_f64(const spc_les_advect_args *args, void *stream);
int spc_les_advect_f32(const spc_les_advect_args *args, void *stream);
/* cells of the flat run [jtot][ktot] of one row i that a workgroup of k_les_advect owns (elem_size 4 or 8); 0: bad arguments */
int spc_les_advect_strip(int jtot, int ktot, int elem_size);
/* consecutive rows i that a workgroup of k_les_advect walks: 32 where the launch has at least 1 024 workgroups even so, else 8;
 * 0: bad arguments */
int spc_les_advect_rows(int64_t n_les, int itot, int jtot, int ktot);

/* ---- vertical upwind advection of the device-resident LES fields from continuity (kernel family K17) -------------------------- */
/* One explicit first-order upwind step along k in advective form, by the mass flux that continuity gives K16's horizontal face
 * Courant numbers.  Fields, u and v are [n_les][itot][jtot][ktot] (layout and offsets as K10), element type T; every operation
 * is rounded once in T, never an fma, and the kernel holds no division.  hx, hy [n_les] are K16's.  g and r are profiles
 * [n_les x ktot], rows pitch_prof apart: g = rho * dz (DeviceLESEnsemble.water_path_weights()) and r = 1 / g, formed in float64
 * (sp_coupler_amd/advection.py: vertical_profiles) and rounded to T once; neither depends on dt.  Per cell (l, i, j, k), with
 * cw, ce, cs, cn EXACTLY K16's face numbers at level k:
 *   d    = (ce - cw) + (cn - cs)                                  the Courant divergence of the cell
 *   e    = g[l][k] * d
 *   M[0] = +0;   M[k+1] = M[k] - e                                SEQUENTIAL in k from the ground: the mass through the upper face
 *   cb   = M[k] * r[l][k];   ct = M[k+1] * r[l][k]
 *   pb   = cb > 0 ? cb : 0;  pt = ct < 0 ? -ct : 0                a NaN face gives +0
 *   km   = k ? k-1 : 0;      kp = k+1 < ktot ? k+1 : ktot-1
 *   out[f] = (x + pb * (x[km] - x)) + pt * (x[kp] - x)            x = fields[f]
 *   s    = pb + pt;          cmax[l] = the maximum of s over the cells of LES l (the launch zeroes it first)
 *   mtop[l][i][j][k] = M[k+1]
 * The ground is closed (M[0] = 0); the lid is open with zero gradient: air that enters through the top carries the top cell's
 * own value.  u, v and the fields are read only; a field may be u or v itself.  Every out[f] and mtop is written whole.  s is
 * never NaN and never negative.  With winds that are uniform per level every d is +0: M = 0, cmax = 0, and every finite field
 * keeps its bits; a constant finite field keeps its bits under any winds.  Special values get no rule of their own: a NaN wind
 * makes M NaN from its level upward in the columns whose divergence reads it, and a NaN M closes its face.  n_fields == 0 with
 * cmax and / or mtop is the probe: only the winds and the profiles are read.  Nothing to do (no field, no cmax, no mtop),
 * pitch_prof < ktot, and an out[f], mtop or cmax EQUAL to an input or to another output are SPC_ERR_INVALID_ARGUMENT; arrays
 * that overlap in part are not detected and must not be passed.  ktot == 1 is allowed.  A workgroup takes
 * spc_les_vadvect_cols_per_block(ktot, sizeof(T)) columns into LDS; above the largest ktot of which 16 columns fit (1 279 levels
 * of 8 bytes, 2 559 of 4) the launch is SPC_ERR_UNSUPPORTED.  The rule is this library's definition.      */
#define SPC_VADVECT_MAX_FIELDS 6
typedef struct spc_les_vadvect_args {
    int64_t n_les;                      /* 0 is allowed: no-op                                               */
    int32_t itot, jtot, ktot, n_fields; /* n_fields 0 ... SPC_VADVECT_MAX_FIELDS                             */
    const void *u, *v;                  /* device [n_les][itot][jtot][ktot], read only                       */
    const void *fields[SPC_VADVECT_MAX_FIELDS]; /* device [n_les][itot][jtot][ktot], read only               */
    void *out[SPC_VADVECT_MAX_FIELDS];  /* device [n_les][itot][jtot][ktot], written whole                   */
    const void *hx, *hy;                /* device [n_les]: 0.5 dt / dx and 0.5 dt / dy                       */
    void *cmax;                         /* device [n_les], or NULL                                           */
    const void *g, *r;                  /* device [n_les x ktot] each, rows pitch_prof apart: rho dz, 1 / g  */
    int64_t pitch_prof;                 /* >= ktot                                                           */
    void *mtop;                         /* device [n_les][itot][jtot][ktot], written whole, or NULL          */
} spc_les_vadvect_args;
int spc_les_vadvect_f64(const spc_les_vadvect_args *args, void *stream);
int spc_les_vadvect_f32(const spc_les_vadvect_args *args, void *stream);
/* columns per workgroup of k_les_vadvect for ktot levels of elem_size (4 or 8) bytes: 64, 32 or 16; 0: unsupported */
int spc_les_vadvect_cols_per_block(int ktot, int elem_size);

/* ---- conservative flux-form transport of the device-resident LES fields along i, j and k in one launch (kernel family K22) ---- */
/* One UNSPLIT first-order donor-cell step in FLUX form, consistent with K17's continuity: what K16 followed by K17 do in advective
 * form and two launches, done in one so that sum_ijk g x changes only by what passes the lid.  The layout, the offsets, hx, hy,
 * g = rho dz, r = 1 / g and pitch_prof are K17's; im, ip, jm, jp are the periodic neighbours as K16 forms them.  Element type T;
 * every operation is rounded once in T, never an fma, and the kernel holds no division.  Per cell (l, i, j, k), every array at
 * level k of LES l unless indexed otherwise:
 *   cw, ce, cs, cn                                                K16's face Courant numbers, bit for bit
 *   d    = (ce - cw) + (cn - cs);   e = g[l][k] * d
 *   M[0] = +0;   M[k+1] = M[k] - e                                K17's chain, bit for bit; mtop[l][i][j][k] = M[k+1] is K17's mtop
 *   pw   = cw > 0 ? cw : 0;   qw = cw < 0 ? cw : 0                likewise (pe, qe), (ps, qs), (pn, qn); a NaN face gives +0 twice
 *   Mb   = M[k];   Mt = M[k+1]
 *   pb   = Mb > 0 ? Mb : 0;   qb = Mb < 0 ? Mb : 0;               pt, qt of Mt likewise
 *   km   = k ? k-1 : 0;   kp = k+1 < ktot ? k+1 : ktot-1          closed ground; open lid with zero gradient
 *   Fw   = pw * x[im] + qw * x                                    two products, each rounded, then the add; x = fields[f]
 *   Fe   = pe * x     + qe * x[ip]
 *   Fs   = ps * x[jm] + qs * x
 *   Fn   = pn * x     + qn * x[jp]
 *   Fb   = pb * x[km] + qb * x
 *   Ft   = pt * x     + qt * x[kp]
 *   h    = (Fe - Fw) + (Fn - Fs)
 *   z    = r[l][k] * (Ft - Fb)
 *   out[f] = (x - h) - z
 *   s    = ((pe - qw) + (pn - qs)) + r[l][k] * (pt - qb)          the outflow Courant sum; cmax[l] = its maximum over the cells of
 *                                                                 LES l (the launch zeroes it first)
 *   ftop[f][l][i][j] = Ft at k = ktot-1                           optional: what left through the lid, in units of g x
 * Shared faces: the flux through a face has the same bits in both cells that share it -- Fe of (i) is Fw of (ip), Fn of (j) is
 * Fs of (jp), Ft of k is Fb of k + 1 (the ground face has M[0] = +0: Fb of k = 0 is +0 for a finite field).
 * Conservation: sum_ijk g x' + sum_ij ftop = sum_ijk g x to rounding, per LES and field.  A constant field stays constant TO
 * ROUNDING -- not bit for bit, unlike K16 and K17: the six fluxes of a constant cancel only as far as continuity holds in T.
 * With s <= 1 out[f] is a convex combination of the cell and its six neighbours.  Winds that are uniform per level give M = 0
 * and the rule reduces to horizontal transport.  An extent of 1 makes the two fluxes of that axis equal: their difference is +0.
 * Special values get no rule of their own: a NaN or an infinity of a field reaches at most itself and its six neighbours (a
 * closed face still multiplies it by +0); a NaN wind closes the faces it touches and makes M NaN from its level upward, as in
 * K17.  s is never NaN and never negative.  u, v and the fields are read only; a field may be u or v itself.  Every out[f], mtop
 * and ftop is written whole.  n_fields == 0 with cmax and / or mtop is the probe: only the winds and the profiles are read (an
 * ftop is then ignored).  Nothing to do (no field, no cmax, no mtop), pitch_prof < ktot, a required array that is NULL, an
 * out[f], mtop, cmax or ftop EQUAL to an input or to another output, and a pointer that is not aligned to T are
 * SPC_ERR_INVALID_ARGUMENT; arrays that overlap in part are not detected and must not be passed.  n_les == 0 is a no-op; ktot == 1
 * is allowed.  A workgroup takes spc_les_transport_cols_per_block(ktot, sizeof(T)) columns into LDS (K17's tile); above the
 * largest ktot of which 16 columns fit (1 279 levels of 8 bytes, 2 559 of 4) the call is SPC_ERR_UNSUPPORTED on the host, before
 * any launch.  The rule is this library's definition.                                                   */
#define SPC_TRANSPORT_MAX_FIELDS 6
typedef struct spc_les_transport_args {
    int64_t n_les;                      /* 0 is allowed: no-op                                               */
    int32_t itot, jtot, ktot, n_fields; /* n_fields 0 ... SPC_TRANSPORT_MAX_FIELDS                           */
    const void *u, *v;                  /* device [n_les][itot][jtot][ktot], read only                       */
    const void *fields[SPC_TRANSPORT_MAX_FIELDS]; /* device [n_les][itot][jtot][ktot], read only             */
    void *out[SPC_TRANSPORT_MAX_FIELDS];/* device [n_les][itot][jtot][ktot], written whole                   */
    const void *hx, *hy;                /* device [n_les]: 0.5 dt / dx and 0.5 dt / dy                       */
    void *cmax;                         /* device [n_les], or NULL                                           */
    const void *g, *r;                  /* device [n_les x ktot] each, rows pitch_prof apart: rho dz, 1 / g  */
    int64_t pitch_prof;                 /* >= ktot                                                           */
    void *mtop;                         /* device [n_les][itot][jtot][ktot], written whole, or NULL          */
    void *ftop;                         /* device [n_fields][n_les][itot][jtot], written whole, or NULL      */
} spc_les_transport_args;
int spc_les_transport_f64(const spc_les_transport_args *args, void *stream);
int spc_les_transport_f32(const spc_les_transport_args *args, void *stream);
/* columns per workgroup of k_les_transport for ktot levels of elem_size (4 or 8) bytes: 64, 32 or 16; 0: unsupported */
int spc_les_transport_cols_per_block(int ktot, int elem_size);

/* ---- second-order limited flux-form transport of the device-resident LES fields in one launch (kernel family K23) ------------- */
/* K22's step with a SECOND-ORDER face value.  The layout, hx, hy, g, r, pitch_prof, the face Courant numbers, the chain M, the
 * twelve numbers pw, qw, ..., pt, qt, the six donor fluxes Fw ... Ft, mtop and cmax are K22's, bit for bit (so cmax of K23 equals
 * cmax of K22, and n_fields == 0 is the same probe).  Every operation is rounded once in T, never an fma; there is no division and
 * no fmin / fmax: selects only, spelled as below, so that what a NaN does is defined.  Per field x and axis the SLOPE of a cell,
 * m / p its neighbours along that axis (periodic along i and j; along k the slope is +0 at k == 0 and at k == ktot-1):
 *   a  = x - x[m];   b = x[p] - x;   t = a + b;   c0 = 0.5 * t
 *   SPC_LIMITER_NONE:  s = c0
 *   SPC_LIMITER_MC:    a2 = 2 * a;   b2 = 2 * b
 *                      a > 0 && b > 0:  lo = a2 < b2 ? a2 : b2;   s = c0 < lo ? c0 : lo
 *                      a < 0 && b < 0:  hi = a2 > b2 ? a2 : b2;   s = c0 > hi ? c0 : hi
 *                      otherwise (an extremum, a zero or a NaN difference):  s = +0
 * Every face adds to K22's donor flux a correction from the slope of its upwind cell, centred in time (si, sj, sk the slopes
 * along i, j, k):
 *   tw = 1 - pw;   gw = pw * tw;   uw = 1 + qw;   hw = qw * uw
 *   m1 = gw * si[im];   m2 = hw * si[i];   dw = m1 - m2;   Aw = 0.5 * dw;   Fw2 = Fw + Aw
 *   Ae = 0.5 * (pe * (1 - pe) * si[i] - qe * (1 + qe) * si[ip]),   As and An likewise with sj, each in the order of Aw
 *   ct = pt * r[k];    dt = qt * r[kp];   gt = pt * (1 - ct);   ht = qt * (1 + dt)       the Courant number of the upwind cell
 *   At = 0.5 * (gt * sk[k] - ht * (k+1 < ktot ? sk[k+1] : +0))
 *   cb = pb * r[km];   db = qb * r[k];    gb = pb * (1 - cb);   hb = qb * (1 + db)
 *   Ab = 0.5 * (gb * (k ? sk[k-1] : +0) - hb * sk[k])
 *   out[f] = (x - ((Fe2 - Fw2) + (Fn2 - Fs2))) - r[l][k] * (Ft2 - Fb2)
 *   ftop[f][l][i][j] = Ft2 at k = ktot-1
 * As in K22 the two cells that share a face form its flux from the same operands in the same order (At of k is Ab of k+1, operand
 * for operand; the slope of a neighbour is formed as the neighbour forms its own), so sum_ijk g x' + sum_ij ftop = sum_ijk g x to
 * rounding, and a constant stays constant to rounding.  With SPC_LIMITER_MC and a Courant number of at most 1 a 1-D step creates no
 * value outside the range of the cell and its two neighbours; SPC_LIMITER_NONE (Fromm's scheme) is second order and not
 * monotone.  A cell reads x at distance up to 2 along each axis, 13 values per field; the neighbours of neighbours are periodic
 * again (imm of itot = 3 is ip, of itot = 2 the cell itself), so an extent of 1 or 2 gives a = -b or 0 and a zero MC slope.  Along
 * k every index is clamped before the load: nothing is read outside the field.  A NaN or an infinity of a field reaches at most
 * two cells along each axis.  The slope is taken in INDEX space: on a stretched vertical grid the scheme stays conservative and
 * limited, but is second order only where dz is uniform.  The refusals, the aliasing rules, the alignment, n_les == 0, the
 * columns per workgroup and the largest ktot are K22's; a limiter other than the two below is SPC_ERR_INVALID_ARGUMENT.  The rule
 * is this library's definition.                                                                         */
#define SPC_LIMITER_NONE 0
#define SPC_LIMITER_MC 1
typedef struct spc_les_transport2_args {
    int64_t n_les;                      /* 0 is allowed: no-op                                               */
    int32_t itot, jtot, ktot, n_fields; /* n_fields 0 ... SPC_TRANSPORT_MAX_FIELDS                           */
    const void *u, *v;                  /* device [n_les][itot][jtot][ktot], read only                       */
    const void *fields[SPC_TRANSPORT_MAX_FIELDS]; /* device [n_les][itot][jtot][ktot], read only             */
    void *out[SPC_TRANSPORT_MAX_FIELDS];/* device [n_les][itot][jtot][ktot], written whole                   */
    const void *hx, *hy;                /* device [n_les]: 0.5 dt / dx and 0.5 dt / dy                       */
    void *cmax;                         /* device [n_les], or NULL                                           */
    const void *g, *r;                  /* device [n_les x ktot] each, rows pitch_prof apart: rho dz, 1 / g  */
    int64_t pitch_prof;                 /* >= ktot                                                           */
    void *mtop;                         /* device [n_les][itot][jtot][ktot], written whole, or NULL          */
    void *ftop;                         /* device [n_fields][n_les][itot][jtot], written whole, or NULL      */
    int32_t limiter;                    /* SPC_LIMITER_NONE or SPC_LIMITER_MC                                */
} spc_les_transport2_args;
int spc_les_transport2_f64(const spc_les_transport2_args *args, void *stream);
int spc_les_transport2_f32(const spc_les_transport2_args *args, void *stream);
/* columns per workgroup of k_les_transport2 for ktot levels of elem_size (4 or 8) bytes: K22's; 0: unsupported */
int spc_les_transport2_cols_per_block(int ktot, int elem_size);

/* ---- longwave cooling and warming of the device-resident LES fields by their liquid water (kernel family K18) ----------------- */
/* The first two terms of the GCSS / DYCOMS-II parametrised longwave flux (Stevens et al. 2005): the flux that the liquid water
 * above and below a face lets through, and the THL tendency of its divergence.  ql and thl are [n_les][itot][jtot][ktot] (layout
 * and offsets as K10), element type T; every operation is rounded once in T, never an fma, and the kernel holds no division and
 * no transcendental function.  w and c are profiles [n_les x ktot], rows pitch_prof apart: w = kappa * rho * dz and
 * c = dt / (cp * rho * dz * exner), formed in float64 (sp_coupler_amd/radiation.py: profiles) and rounded to T once.  etab is a
 * table of exp(-x) at x = m / inv_step, m = 0 ... n_tab - 1 (radiation.py: exp_table), x_hi = (T)((n_tab - 1) / inv_step) formed
 * in double.  f0, f1 [n_les] are the flux scales in W/m2.  Per column (l, i, j):
 *   t[k]    = w[l][k] * ql[k]                         k = 0 ... ktot - 1
 *   B[0]    = +0;   B[k+1] = B[k] + t[k]              SEQUENTIAL upward:   the optical depth below face k + 1
 *   A[ktot] = +0;   A[k]   = A[k+1] + t[k]            SEQUENTIAL downward: the optical depth above face k
 *   E(x):   xc = x < 0 ? 0 : (x > x_hi ? x_hi : x)    (a NaN passes through)
 *           s  = xc * inv_step;  m = s >= 0 ? min((int)s, n_tab - 2) : 0;  fr = s - (T)m
 *           E  = etab[m] + fr * (etab[m+1] - etab[m])
 *   F[k]    = f0[l] * E(A[k]) + f1[l] * E(B[k])       k = 0 ... ktot: the net upward flux at face k; two products, one add
 *   thl'[k] = thl[k] - c[l][k] * (F[k+1] - F[k])      IN PLACE: the difference, the product, the subtraction
 *   flux[l][i][j][k] = F[k+1]                         optional, written whole
 *   fsfc[l][i][j]    = F[0]                           optional, written whole
 * ql is read only.  A column without liquid water (every ql +0) has F = f0 + f1 at every face and keeps the bits of every finite
 * thl, -0.0 included.  A NaN in ql makes every F and every thl' of its own column NaN and reaches no other column; infinities and
 * negative ql get no rule beyond the clamp in E.  n_tab < 2, inv_step not positive, pitch_prof < ktot, and thl, flux or fsfc
 * EQUAL to an input or to each other are SPC_ERR_INVALID_ARGUMENT; arrays that overlap in part are not detected and must not be
 * passed.  ktot == 1 is allowed.  A workgroup takes spc_les_radiate_cols_per_block(ktot, sizeof(T)) columns into two LDS tiles;
 * above the largest ktot of which 16 columns fit (638 levels of 8 bytes, 1 278 of 4) the launch is SPC_ERR_UNSUPPORTED.  The
 * third DYCOMS term (the cooling of the free troposphere above the inversion) is not part of the rule.  The rule is this
 * library's definition.                                                                             */
typedef struct spc_les_radiate_args {
    int64_t n_les;                      /* 0 is allowed: no-op                                               */
    int32_t itot, jtot, ktot, n_tab;    /* n_tab >= 2                                                        */
    const void *ql;                     /* device [n_les][itot][jtot][ktot], read only                       */
    void *thl;                          /* device [n_les][itot][jtot][ktot], updated in place                */
    const void *w, *c;                  /* device [n_les x ktot] each, rows pitch_prof apart                 */
    int64_t pitch_prof;                 /* >= ktot                                                           */
    const void *f0, *f1;                /* device [n_les]                                                    */
    const void *etab;                   /* device [n_tab]: exp(-m / inv_step)                                */
    double inv_step;                    /* > 0: the nodes of etab per unit of optical depth                  */
    void *flux;                         /* device [n_les][itot][jtot][ktot], written whole, or NULL          */
    void *fsfc;                         /* device [n_les][itot][jtot], written whole, or NULL                */
} spc_les_radiate_args;
int spc_les_radiate_f64(const spc_les_radiate_args *args, void *stream);
int spc_les_radiate_f32(const spc_les_radiate_args *args, void *stream);
/* columns per workgroup of k_les_radiate for ktot levels of elem_size (4 or 8) bytes: 64, 32 or 16; 0: unsupported */
int spc_les_radiate_cols_per_block(int ktot, int elem_size);

/* ---- local cloud-water forcing of the device-resident LES fields: qt_forcing 'local' | 'strong' (kernel family K19) ---------- */
/* What an LES does with the cloud-water forcing the coupler hands it (set_tendency_QL, set_ref_profile_QL: splib/spcpl.py:346-347;
 * Dales.QT_FORCING_LOCAL / QT_FORCING_STRONG, splib/modfac.py:70-73): it moves its cloud water towards the GCM's without moving
 * its mean moisture.  DALES's source is not part of the reference: the rule is this library's definition, shaped
 * on what the coupler passes in and on the option's help text ("stimulate ql alignment with ... local forcing").
 * Fields are [n_les][itot][jtot][ktot] with k contiguous and 64-bit offsets as in K10.  The element type is T.  Every operation
 * is rounded once and nothing contracts to an fma.  N = itot * jtot.
 * Per LES l and level k, the kernel reads a = A[l * pitch_prof + k] and m = QTM[l * pitch_prof + k].  a is the wanted change of
 * the slab-mean cloud water in this step.
 *   - If a is +0, -0 or NaN, the level keeps every bit of qt and count[l][k] = 0.
 *   - If a > 0, a cell is wet when qt > m.  If a < 0, a cell is wet when ql > 0.  A NaN compares false, so such a cell is dry.
 *   - c is the number of wet cells of the plane.  count[l][k] = c (int32, exact).
 *   - If c == 0 or c == N, the level keeps every bit of qt.  There is nothing to redistribute.  An overcast level with too much
 *     cloud is left to the uniform QT tendency.
 *   - Otherwise s = a * T(N), dw = s / T(c) and dd = s / T(N - c).  These are two true IEEE quotients.  There are two divisions
 *     per (LES, level) and none per cell.  Wet cells get qt' = qt + dw and dry cells get qt' = qt - dd, IN PLACE.
 * ql is read only, and only on levels with a < 0.  The slab mean of qt is conserved up to rounding: moisture moves between the
 * cloudy (or moister) cells and the rest.  Because c is an integer, the result does not depend on how the launch is cut: a plane
 * may be counted by one workgroup or by several (spc_les_qt_local_split) and the bits are the same.
 * SPC_ERR_INVALID_ARGUMENT: N > 2^24, which is not exact in float; pitch_prof < ktot or pitch_count < ktot; a NULL qt, a, qtm or
 * count; a NULL ql (required: the caller does not know the signs); qt == ql; split < 0.  n_les == 0 is a no-op and ktot == 1 is
 * allowed.  There is no upper limit on ktot: no whole column has to sit in LDS.  The levels between ktot and pitch_count of a
 * count row are not written.                                                                                             */
typedef struct spc_les_qt_local_args {
    int64_t n_les;                      /* 0 is allowed: no-op                                               */
    int32_t itot, jtot, ktot;
    int32_t split;                      /* workgroups that share a plane: 0 the library's choice, else forced (at most N are used) */
    void *qt;                           /* device [n_les][itot][jtot][ktot], updated in place                */
    const void *ql;                     /* device [n_les][itot][jtot][ktot], read only                       */
    const void *a, *qtm;                /* device [n_les x ktot] each, rows pitch_prof apart: A and QTM      */
    int64_t pitch_prof;                 /* >= ktot                                                           */
    int32_t *count;                     /* device [n_les x ktot], rows pitch_count apart, written whole      */
    int64_t pitch_count;                /* >= ktot                                                           */
} spc_les_qt_local_args;
int spc_les_qt_local_f64(const spc_les_qt_local_args *args, void *stream);
int spc_les_qt_local_f32(const spc_les_qt_local_args *args, void *stream);
/* the split factor the library chooses for these extents (elem_size 4 or 8): 1 = one workgroup counts and updates a tile of
 * levels of a whole plane in one launch; S > 1 = S workgroups take ceil(N / S) rows of it each, their integer counts meet in
 * `count` and a second launch updates (few LES with large planes); 0: bad arguments */
int spc_les_qt_local_split(int64_t n_les, int itot, int jtot, int ktot, int elem_size);

/* ---- second moments of the device-resident LES fields: variances, covariances, resolved fluxes (kernel family K20) ----------- */
/* Per LES and level: the mean, the variance and the standard deviation of every field of a set and the covariance of pairs of
 * them, in ONE launch, with the bits of the NumPy statements below.
 * Inputs and outputs:
 *   - Fields x_f, f < n_fields, 1 <= n_fields <= SPC_MOMENTS_MAX_FIELDS.  Each is [n_les][itot][jtot][ktot] in C order, ktot
 *     contiguous, 64-bit offsets as in K10, element type T of the entry point, read only.
 *   - Pairs (a_p, b_p) = (pair_a[p], pair_b[p]), p < n_pairs, 0 <= n_pairs <= SPC_MOMENTS_MAX_PAIRS.  They are indices into the
 *     fields with a_p != b_p.  A field may appear in several pairs, and (a, b) and (b, a) may both be asked for.
 *   - face_field is -1 or the index of one field given at the UPPER faces of the cells (K17's W).  That field is first brought
 *     to the cell centres: xc[k] = T(0.5) * (x[k - 1] + x[k]) with x[-1] := +0.0 (the closed ground; nothing in front of a row
 *     is read).  One add and one multiply, each rounded once.  Every output of that field, its mean included, is of xc.
 *   - Per LES l and level k, N = itot * jtot, rows r = (i, j) in row-major order:
 *       m_f    = (sum over r, sequential from +0.0, of x_f[r]) / T(N), which is K10's rule.
 *       d_f[r] = x_f[r] - m_f.
 *       var_f  = (sum over r, sequential from +0.0, of (d_f[r] * d_f[r])) / T(N).  The product is rounded on its own, never an
 *                fma.
 *       std_f  = sqrt(var_f), IEEE correctly rounded.
 *       cov_p  = (sum over r, sequential from +0.0, of (d_a[r] * d_b[r])) / T(N).
 *   - The outputs are mean[f], var[f], std[f] and cov[p].  Each is [n_les x ktot] with one common row pitch pitch_out >= ktot,
 *     and each is optional (NULL means not asked).  At least one must be non-NULL.
 *   - Levels between ktot and pitch_out are not written.
 *   - NaN and infinities follow IEEE.  A NaN cell makes that level's outputs of the fields it touches NaN and no other level's
 *     (a face field: the level above it too).  A plane of -0.0 has mean +0.0.
 * These equal, bit for bit in f64 and f32, x.mean(axis=(0, 1)), x.var(axis=(0, 1)), x.std(axis=(0, 1)) and
 * ((x - x.mean(axis=(0, 1))) * (y - y.mean(axis=(0, 1)))).mean(axis=(0, 1)) of NumPy for ktot > 1.
 * Refusals:
 *   - ktot == 1 is SPC_ERR_UNSUPPORTED, as in spc_les_advance_*, because NumPy reduces a one-level plane pairwise.
 *   - SPC_ERR_INVALID_ARGUMENT for N > 2^24; a pitch below ktot; a NULL field; no output asked for; a pair index out of range
 *     or a_p == b_p; face_field >= n_fields; an output pointer EQUAL to a field or to another output.
 *   - n_les == 0 is a no-op.                                                                                                  */
#define SPC_MOMENTS_MAX_FIELDS 8
#define SPC_MOMENTS_MAX_PAIRS 8
typedef struct spc_les_moments_args {
    int64_t n_les;                                  /* 0 is allowed: no-op                                              */
    int32_t itot, jtot, ktot;
    int32_t n_fields, n_pairs, face_field;
    const void *fields[SPC_MOMENTS_MAX_FIELDS];     /* device [n_les][itot][jtot][ktot] each                            */
    int32_t pair_a[SPC_MOMENTS_MAX_PAIRS], pair_b[SPC_MOMENTS_MAX_PAIRS];
    void *mean[SPC_MOMENTS_MAX_FIELDS], *var[SPC_MOMENTS_MAX_FIELDS], *std[SPC_MOMENTS_MAX_FIELDS];
    void *cov[SPC_MOMENTS_MAX_PAIRS];               /* device [n_les x ktot] each, rows pitch_out apart, or NULL        */
    int64_t pitch_out;                              /* >= ktot                                                          */
} spc_les_moments_args;
int spc_les_moments_f64(const spc_les_moments_args *args, void *stream);
int spc_les_moments_f32(const spc_les_moments_args *args, void *stream);

/* ---- hydrostatic pressure force of the device-resident LES fields: buoyancy drives the winds (kernel family K21) -------------- */
/* The model diagnoses W from continuity with a closed ground and an open lid, so its closure is the hydrostatic one: the buoyancy
 * of every column is integrated downward from the lid to a pressure perturbation, the horizontal gradient of that pressure
 * accelerates U and V, and continuity (K17) then turns the convergence into vertical motion.  Two launches behind one entry
 * point.  The rule is this library's definition.
 * General conventions:
 *   - Fields are [n_les][itot][jtot][ktot], k contiguous, with 64-bit offsets as in K10.  The element type T is f64 or f32.
 *   - Every operation is rounded once in T.  Nothing contracts to an fma.
 *   - The kernels hold no division and no transcendental function.
 *   - So every output is asked for bit for bit in both types, whatever the launch shape.
 * Profiles:
 *   - The profiles are [n_les x ktot], rows pitch_prof apart.
 *   - They are formed in float64 by sp_coupler_amd/buoyancy.py (profiles(...)) and rounded to T once.
 *   - The constants come from sputils where it has them: grav, rlv, cp, rd, rv.
 *   - t0  = thv of the slab means: (THL + lex QL) * ((1 + c1 QT) - c2 QL) of p["THL"], p["QT"], p["QL"]: the reference virtual
 *           potential temperature.
 *   - lex = rlv / (cp * exner(presf)).
 *   - s   = 0.5 * grav * dz / t0: half a layer's weight; dz from the half levels, as water_path_weights() takes it.
 * Scalars and per-LES values:
 *   - c1 = rv / rd - 1 and c2 = rv / rd are passed as doubles in the args and rounded to T once.
 *   - hx, hy [n_les] are K16's: 0.5 dt / dx and 0.5 dt / dy.
 * Per cell (l, i, j, k):
 *   e   = lex[l][k] * ql                 (ql == NULL: e = +0 and m = 1 + c1 * qt)
 *   tl  = thl + e
 *   m   = (1 + c1 * qt) - c2 * ql
 *   tv  = tl * m
 *   b   = (tv - t0[l][k]) * s[l][k]                      half-layer buoyancy integral, m2/s2
 *   q[ktot] = +0                                         the lid: no pressure perturbation
 *   phi[k]  = q[k+1] - b[k];   q[k] = phi[k] - b[k]      SEQUENTIAL downward, two subtractions per level
 *   psfc[l][i][j] = q[0]                                 optional: the perturbation at the ground
 * Then, with ip, im, jp, jm the periodic neighbours as K16 forms them:
 *   gx = phi[ip] - phi[im];   du = hx[l] * gx;   u' = u - du     IN PLACE
 *   gy = phi[jp] - phi[jm];   dv = hy[l] * gy;   v' = v - dv     IN PLACE
 *   a  = |du| + |dv|;         amax[l] = the maximum of a over the cells of LES l (optional; the launch zeroes it first;
 *                                       K16's atomicMax on the bit pattern)
 * phi is [n_les][itot][jtot][ktot] and is written whole.
 *   - It is required, because it is both the workspace between the two launches and a diagnostic.
 *   - thl, qt and ql are read only.
 * Consequences:
 *   - A state that is uniform on every level gives the same phi in every column.  Every gx and gy is +0, every finite u and v
 *     keeps its bits (-0.0 included), and amax = 0.
 *   - itot <= 2 makes every gx zero.  The same holds for jtot <= 2 and gy.
 *   - A NaN in one thl cell makes phi NaN in its own column from that level DOWN.  It makes u' (resp. v') NaN in the two
 *     i-neighbour (resp. j-neighbour) columns at those levels, and amax[l] a NaN (ask with isnan, not for its bits).  Every
 *     other cell of the launch keeps the bits of the run without it.
 *   - Infinities get no rule of their own.
 *   - These are SPC_ERR_INVALID_ARGUMENT:
 *       pitch_prof < ktot;
 *       a NULL thl, qt, u, v, phi, hx, hy, t0, lex or s;
 *       phi, u, v, psfc or amax equal to an input or to each other.
 *   - Arrays that overlap only in part are not detected and must not be passed.
 *   - n_les == 0 is a no-op.  ktot == 1 is allowed.
 *   - Above the largest ktot of which 16 columns fit in LDS (1 279 levels of 8 bytes, 2 559 of 4) the launch is
 *     SPC_ERR_UNSUPPORTED.  It is refused on the host and nothing is launched.
 * k_les_hydrostatic: a workgroup takes spc_les_buoyancy_cols_per_block(ktot, sizeof(T)) columns into one LDS tile.  k_les_pgrad: a
 * workgroup owns spc_les_advect_strip(...) cells of the run [jtot][ktot] of a row i and spc_les_advect_rows(...) rows.        */
typedef struct spc_les_buoyancy_args {
    int64_t n_les;                      /* 0 is allowed: no-op                                               */
    int32_t itot, jtot, ktot, reserved;
    const void *thl, *qt;               /* device [n_les][itot][jtot][ktot], read only                       */
    const void *ql;                     /* device [n_les][itot][jtot][ktot], read only, or NULL              */
    void *u, *v;                        /* device [n_les][itot][jtot][ktot], updated in place                */
    const void *hx, *hy;                /* device [n_les]: 0.5 dt / dx and 0.5 dt / dy                       */
    const void *t0, *lex, *s;           /* device [n_les x ktot] each, rows pitch_prof apart                 */
    int64_t pitch_prof;                 /* >= ktot                                                           */
    double c1, c2;                      /* rv / rd - 1 and rv / rd                                           */
    void *phi;                          /* device [n_les][itot][jtot][ktot], written whole                   */
    void *psfc;                         /* device [n_les][itot][jtot], written whole, or NULL                */
    void *amax;                         /* device [n_les], or NULL                                           */
} spc_les_buoyancy_args;
int spc_les_buoyancy_f64(const spc_les_buoyancy_args *args, void *stream);
int spc_les_buoyancy_f32(const spc_les_buoyancy_args *args, void *stream);
/* columns per workgroup of k_les_hydrostatic for ktot levels of elem_size (4 or 8) bytes: 64, 32 or 16; 0: unsupported */
int spc_les_buoyancy_cols_per_block(int ktot, int elem_size);

/* ---- Smagorinsky-Lilly subgrid mixing of the device-resident LES fields (kernel family K24) ----------------------------------- */
/* An eddy viscosity per cell from the resolved deformation and the stratification, and one explicit step in flux form of the
 * horizontal mixing of the carried fields by that viscosity.  Two launches behind one entry point.  The rule is this library's
 * definition.
 * General conventions:
 *   - Fields are [n_les][itot][jtot][ktot], k contiguous, with 64-bit offsets as in K10.  The element type T is f64 or f32.
 *   - Every operation is rounded once in T.  Nothing contracts to an fma.
 *   - There is no division and no transcendental function; there is one correctly rounded sqrt per cell, as K20's std.
 *   - So every output is asked for bit for bit in both types, whatever the launch shape.
 * Neighbours:
 *   - im, ip, jm, jp are K16's periodic neighbours: an extent of 1 is the cell itself, an extent of 2 has both neighbours the
 *     same cell.
 *   - kp = k + 1 < ktot ? k + 1 : k and kq = k > 0 ? k - 1 : k.  The index is clamped before the load.
 * Per-LES values and profiles (formed in float64 by sp_coupler_amd/mixing.py and rounded to T once):
 *   - gx = 0.5 / dx, gy = 0.5 / dy and kcap [n_les]; gz = 1 / (zf[kp] - zf[kq]), bz = grav / (prandtl theta_ref) * gz and
 *     l2 (the squared mixing length, > 0 and finite: the caller's duty) [n_les x ktot], rows pitch_prof apart.
 *   - ax[f], ay[f] [n_les]: 0.5 dt / dx^2 and 0.5 dt / dy^2 for a wind, the same divided by the Prandtl number for a scalar:
 *     one pointer per field, so that the kernel needs no extra rounding; fields may share a pointer.
 * Launch 1, k_les_eddy, per cell (l, i, j, k):
 *   ux = (u[ip] - u[im]) * gx[l];        vx = (v[ip] - v[im]) * gx[l]
 *   uy = (u[jp] - u[jm]) * gy[l];        vy = (v[jp] - v[jm]) * gy[l]
 *   uz = (u[kp] - u[kq]) * gz[l][k];     vz = (v[kp] - v[kq]) * gz[l][k]
 *   a  = ux * ux + vy * vy;   sh = uy + vx
 *   d  = (a + a) + sh * sh;   d = d + (uz * uz + vz * vz)
 *   d  = d - (theta[kp] - theta[kq]) * bz[l][k]          only where theta != NULL
 *   e  = d > 0 ? d : +0                                   a NaN gives +0
 *   kk = l2[l][k] * sqrt(e)
 *   kmax[l] = the maximum of kk over the cells of LES l   optional; K16's atomicMax on the bit pattern, zeroed by the launch
 *   km = kk < kcap[l] ? kk : kcap[l]                      written whole; required: the workspace between the launches AND a
 *                                                         diagnostic
 * The gradients of W are left out: W is diagnosed from continuity under the hydrostatic closure of K21.
 * Launch 2, k_les_hmix, per cell and per field f with x = fields[f]:
 *   kw = km[im] + km;  ke = km + km[ip];  ks = km[jm] + km;  kn = km + km[jp]
 *   fw = (kw * ax[f][l]) * (x - x[im]);   fe = (ke * ax[f][l]) * (x[ip] - x)
 *   fs = (ks * ay[f][l]) * (x - x[jm]);   fn = (kn * ay[f][l]) * (x[jp] - x)
 *   out[f] = x + ((fe - fw) + (fn - fs))
 * n_fields == 0 runs launch 1 only (the probe / the diagnostic).
 * Consequences:
 *   - km is never negative, never NaN and at most kcap[l], given l2 > 0 finite.  A NaN in u, v or theta makes km = +0 in the
 *     cells whose stencil reads it and touches nothing else.  A NaN in a field reaches that cell and its four neighbours.
 *   - Both cells of a face form its flux from the same operands: fe of a cell equals fw of its ip neighbour bit for bit, fn of
 *     a cell fs of its jp neighbour.  The plane sum of every field is conserved to rounding.
 *   - A constant finite field keeps its bits; a -0.0 constant comes out +0.0, as in K16.
 *   - Winds that are uniform on every level (and without shear from level to level) under a stable or neutral theta give
 *     km = +0 everywhere, and every field keeps its bits.
 *   - With (kw + ke) ax + (ks + kn) ay <= 1, which kcap = CAP / (4 max(ax + ay)), CAP <= 1, guarantees, out is a convex
 *     combination of the cell and its four neighbours.
 *   - These are SPC_ERR_INVALID_ARGUMENT: pitch_prof < ktot; a NULL u, v, gx, gy, kcap, gz, l2, km, or a NULL fields[f],
 *     out[f], ax[f], ay[f] of f < n_fields; theta without bz; km, kmax or an out[f] equal to an input or to each other;
 *     n_fields outside 0 ... SPC_MIX_MAX_FIELDS.
 *   - Arrays that overlap only in part are not detected and must not be passed.  n_les == 0 is a no-op.  ktot == 1 is allowed
 *     (gz = bz = 0).
 * Both kernels: a workgroup owns spc_les_advect_strip(...) cells of the run [jtot][ktot] of a row i and
 * spc_les_advect_rows(...) rows.                                                                                          */
#define SPC_MIX_MAX_FIELDS 6
typedef struct spc_les_mix_args {
    int64_t n_les;                      /* 0 is allowed: no-op                                               */
    int32_t itot, jtot, ktot, n_fields; /* n_fields 0 ... SPC_MIX_MAX_FIELDS                                 */
    const void *u, *v;                  /* device [n_les][itot][jtot][ktot], read only                       */
    const void *theta;                  /* device [n_les][itot][jtot][ktot], read only, or NULL              */
    const void *gx, *gy, *kcap;         /* device [n_les]                                                    */
    const void *gz, *bz, *l2;           /* device [n_les x ktot] each, rows pitch_prof apart; bz NULL only without theta */
    int64_t pitch_prof;                 /* >= ktot                                                           */
    void *km;                           /* device [n_les][itot][jtot][ktot], written whole                   */
    void *kmax;                         /* device [n_les], or NULL                                           */
    const void *fields[SPC_MIX_MAX_FIELDS]; /* device [n_les][itot][jtot][ktot], read only                   */
    void *out[SPC_MIX_MAX_FIELDS];      /* device [n_les][itot][jtot][ktot], written whole                   */
    const void *ax[SPC_MIX_MAX_FIELDS]; /* device [n_les] per field                                          */
    const void *ay[SPC_MIX_MAX_FIELDS]; /* device [n_les] per field                                          */
} spc_les_mix_args;
int spc_les_mix_f64(const spc_les_mix_args *args, void *stream);
int spc_les_mix_f32(const spc_les_mix_args *args, void *stream);

/* ---- implicit vertical mixing of the device-resident LES fields by each column's own eddy viscosity (kernel family K25) ------- */
/* One backward-Euler step of d(x)/dt = (1 / (rho dz)) d/dz (rho_h K dx/dz) per column, K at a face from THAT column's km (K24),
 * the kinematic surface fluxes of K15 entering the lowest layer and a neutral bulk drag on the lowest wind level.  The matrix
 * depends on the column, so the Thomas elimination runs in the kernel.  The rule is this library's definition.
 * General conventions:
 *   - Fields, km are [n_les][itot][jtot][ktot], k contiguous, with 64-bit offsets as in K10; speed is [n_les][itot][jtot].  The
 *     element type T is f64 or f32.
 *   - Every operation is rounded once in T.  Nothing contracts to an fma.
 *   - There is ONE correctly rounded IEEE division per level and ONE correctly rounded sqrt per column.
 *   - So every output is asked for bit for bit in both types, whatever the launch shape.
 * Per-LES values and profiles (formed in float64 by sp_coupler_amd/vertical_mixing.py and rounded to T once), profiles
 * [n_les x ktot] with rows pitch_prof apart, w = Rhobf dz, rho_h[k] the mean of Rhobf[k-1] and Rhobf[k]:
 *   - el[f], eu[f]: one pointer pair per field, as K24's ax / ay, so that the Prandtl number costs the kernel no rounding:
 *     el[k] = 0.5 dt rho_h[k] / (w[k] (zf[k] - zf[k-1])), eu[k] = 0.5 dt rho_h[k+1] / (w[k] (zf[k+1] - zf[k])) for a wind, the
 *     same divided by the Prandtl number for a scalar.  el[0] and eu[ktot-1] are never read by the elimination.
 *   - kb: twice the background diffusivity at face k (kb[0] is never read).
 *   - kv2 [n_les]: twice the largest face diffusivity allowed: a sanity bound that keeps the matrix finite, no stability cap.
 *   - s0 [n_les] = dt / dz[0]; flux[f] [n_les] or NULL, exactly as in K15.
 *   - dr[f] [n_les] or NULL: dt cd / dz[0] with cd = (kappa / ln(zf[0] / z0m))^2; NULL for scalars.
 * Launch 1, k_les_speed, only where some dr[f] != NULL, per column (l, i, j):
 *   sp = sqrt(u[0] * u[0] + v[0] * v[0])                  products, add, sqrt, each rounded; written whole into speed
 * (the winds are updated in place by other workgroups, so launch 2 must not read them).
 * Launch 2, k_les_vmix, per column and per field f with x = fields[f]:
 *   t     = (km[k-1] + km[k]) + kb[l][k]                  face k = 1 ... ktot-1
 *   s[k]  = t > 0 ? t : +0                                a NaN or a negative sum gives +0
 *   s[k]  = s[k] < kv2[l] ? s[k] : kv2[l]
 *   lo[k] = el[f][l][k] * s[k]    (lo[0] = +0)            up[k] = eu[f][l][k] * s[k+1]    (up[ktot-1] = +0)
 *   b[k]  = (1 + lo[k]) + up[k];  b[0] = b[0] + dr[f][l] * sp                  the drag only where dr[f] != NULL
 *   d[0]  = flux[f] != NULL ? x[0] + s0[l] * flux[f][l] : x[0];                d[k] = x[k]
 *   m[0]  = 1 / b[0];                     q[0] = up[0] * m[0];   y[0] = d[0] * m[0]
 *   m[k]  = 1 / (b[k] - lo[k] * q[k-1]);  q[k] = up[k] * m[k];   y[k] = (d[k] + lo[k] * y[k-1]) * m[k]
 *   x'[ktot-1] = y[ktot-1];               x'[k] = y[k] + q[k] * x'[k+1]
 * x' replaces x IN PLACE.
 * Consequences:
 *   - Both cells of a face form s[k] from the same operands.  The form is all positive: lo, up and q are never negative, the
 *     matrix is an M-matrix, and every pivot is at least about 1 (b[k] >= 1 + lo[k] while lo[k] q[k-1] < lo[k]), so the
 *     division is always safe.
 *   - ktot == 1 is allowed.  Special values in a field get no rule of their own: they stay in their own column, as in K15.
 *   - With km = 0, kb = 0, no flux and no drag a finite column keeps every value.
 *   - These are SPC_ERR_INVALID_ARGUMENT: n_fields outside 1 ... SPC_VMIX_MAX_FIELDS; pitch_prof < ktot; a NULL km, kb, kv2, or
 *     a NULL fields[f], el[f], eu[f] of f < n_fields; two EQUAL fields pointers; a field equal to km, speed, a profile, kv2, s0,
 *     a drag or a flux; a flux without s0; a dr without u, v and speed; speed equal to an input; a misaligned pointer.
 *   - Arrays that overlap only in part are not detected and must not be passed.  n_les == 0 is a no-op.
 * A workgroup takes spc_les_vmix_cols_per_block(ktot, sizeof(T)) columns of km and of one field into LDS; above the largest
 * ktot of which 16 columns fit twice (639 levels of 8 bytes, 1 279 of 4) the launch is SPC_ERR_UNSUPPORTED.                */
#define SPC_VMIX_MAX_FIELDS 6
typedef struct spc_les_vmix_args {
    int64_t n_les;                      /* 0 is allowed: no-op                                               */
    int32_t itot, jtot, ktot, n_fields; /* n_fields 1 ... SPC_VMIX_MAX_FIELDS                                */
    void *fields[SPC_VMIX_MAX_FIELDS];       /* device [n_les][itot][jtot][ktot], updated in place           */
    const void *flux[SPC_VMIX_MAX_FIELDS];   /* device [n_les], the kinematic surface flux, or NULL          */
    const void *dr[SPC_VMIX_MAX_FIELDS];     /* device [n_les], the drag of a wind, or NULL                  */
    const void *el[SPC_VMIX_MAX_FIELDS];     /* device [n_les x ktot] per field, rows pitch_prof apart       */
    const void *eu[SPC_VMIX_MAX_FIELDS];     /* device [n_les x ktot] per field, rows pitch_prof apart       */
    const void *km;                     /* device [n_les][itot][jtot][ktot], read only                       */
    const void *kb;                     /* device [n_les x ktot], rows pitch_prof apart                      */
    const void *kv2;                    /* device [n_les]                                                    */
    const void *s0;                     /* device [n_les]; may be NULL when every flux is NULL               */
    const void *u, *v;                  /* device [n_les][itot][jtot][ktot], read by launch 1; NULL without a dr */
    void *speed;                        /* device [n_les][itot][jtot], written whole by launch 1; NULL without a dr */
    int64_t pitch_prof;                 /* >= ktot                                                           */
} spc_les_vmix_args;
int spc_les_vmix_f64(const spc_les_vmix_args *args, void *stream);
int spc_les_vmix_f32(const spc_les_vmix_args *args, void *stream);
/* columns per workgroup of k_les_vmix for ktot levels of elem_size (4 or 8) bytes: 64, 32 or 16; 0: unsupported */
int spc_les_vmix_cols_per_block(int ktot, int elem_size);

/* ---- implicit horizontal mixing of the device-resident LES fields by each line's own eddy viscosity (kernel family K26) ------- */
/* One backward-Euler step of d(x)/dt = d/dx (K dx/dx) + d/dy (K dx/dy), K at a face the mean of K24's km of its two cells, IN
 * PLACE and without K24's stability cap: first every line along i, then every line along j, which reads what the first sweep
 * wrote (Lie splitting; each sweep is one backward-Euler step, unconditionally stable).  A line is periodic, so its system is a
 * cyclic tridiagonal one: the last cell is condensed out and the others are eliminated with two right-hand sides.  The matrix
 * differs from line to line, so the elimination runs in the kernel.  The rule is this library's definition.
 * General conventions:
 *   - Fields and km are [n_les][itot][jtot][ktot], k contiguous, with 64-bit offsets as in K10.  The element type T is f64 or f32.
 *   - Every operation is rounded once in T.  Nothing contracts to an fma.
 *   - There is ONE correctly rounded IEEE division per cell of a line and per sweep, plus ONE per line for the closing unknown.
 *     There is no transcendental function.
 *   - So every output is asked for bit for bit in both types, whatever the launch shape.
 * Per-LES values (formed in float64 by sp_coupler_amd/horizontal_mixing.py and rounded to T once):
 *   - ax[f], ay[f] [n_les]: K24's, 0.5 dt / dx^2 and 0.5 dt / dy^2 for a wind, the same divided by the Prandtl number for a
 *     scalar; one pointer per field, fields may share a pointer.
 *   - kh2 [n_les]: twice the largest face viscosity allowed: a sanity bound that keeps the matrix finite, no stability cap.
 * For one line of length n (itot in the first sweep, jtot in the second) with the cells x[0 .. n-1], the line's km[0 .. n-1],
 * a = ax[f][l] (ay[f][l] in the second sweep), ip = (i + 1) mod n and im = (i - 1) mod n:
 *   n == 1:  the line keeps every bit (nothing is loaded or stored)
 *   t[i]  = km[i] + km[ip]                                face between i and ip
 *   s[i]  = t[i] > 0 ? t[i] : +0                          a NaN or a negative sum decouples the face
 *   s[i]  = s[i] < kh2[l] ? s[i] : kh2[l]
 *   w[i]  = a * s[i];   up[i] = w[i];   lo[i] = w[im]
 *   b[i]  = (1 + lo[i]) + up[i]
 *   m = n - 1 unknowns 0 .. n-2 are condensed on x[n-1]:
 *   c[i]  = (i == 0 ? lo[0] : +0) + (i == n-2 ? up[n-2] : +0)            (n == 2: c[0] = lo[0] + up[0])
 *   p     = 1 / b[0];                     q[0] = up[0] * p;   y[0] = x[0] * p;   z[0] = c[0] * p
 *   p     = 1 / (b[i] - lo[i] * q[i-1]);  q[i] = up[i] * p
 *   y[i]  = (x[i] + lo[i] * y[i-1]) * p;  z[i] = (c[i] + lo[i] * z[i-1]) * p             i = 1 .. n-2
 *   y[i]  = y[i] + q[i] * y[i+1];         z[i] = z[i] + q[i] * z[i+1]                    i = n-3 .. 0
 *   num   = (x[n-1] + up[n-1] * y[0]) + lo[n-1] * y[n-2]
 *   den   = (b[n-1] - up[n-1] * z[0]) - lo[n-1] * z[n-2]
 *   x'[n-1] = num / den;                  x'[i] = y[i] + z[i] * x'[n-1]                  i = 0 .. n-2
 * x' replaces x IN PLACE.  axes: bit 0 runs the sweep along i, bit 1 the sweep along j; 3 runs both, i first.
 * Consequences:
 *   - w is the same number for both cells of a face: the matrix is symmetric with unit column sums, so the sum of a line is
 *     conserved to rounding, and after both sweeps the plane sum of every field.
 *   - The matrix is an M-matrix: lo, up, q and z are never negative, 0 <= z <= 1, every pivot and den are at least about 1, so
 *     every division is safe.
 *   - A mixed line stays within its minimum and maximum up to the rounding of the solve (tests/test_les_hmix_cpu.py derives
 *     the slack).  A constant finite line stays constant to rounding; it does not keep its bits.
 *   - With km = 0 a finite line keeps every value; the sign of a zero is not kept (a -0.0 whose neighbours in the walk are not
 *     all -0.0 comes out +0.0).
 *   - A NaN in a field stays in its line in the first sweep and spreads only along the j lines of those cells in the second.
 *     A NaN or negative km touches nothing but its two faces (per direction).
 *   - These are SPC_ERR_INVALID_ARGUMENT: n_fields outside 1 ... SPC_HMIX_MAX_FIELDS; axes outside 1 ... 3; a NULL km, kh2, or
 *     a NULL fields[f], ax[f], ay[f] of f < n_fields; two EQUAL fields pointers; a field equal to km, kh2 or a coefficient; a
 *     misaligned pointer.  SPC_ERR_UNSUPPORTED: a swept extent above the largest supported line (641 cells of 8 bytes, 1 281
 *     of 4); too many workgroups.  Both sweeps are checked before the first is launched.
 *   - Arrays that overlap only in part are not detected and must not be passed.  n_les == 0 is a no-op after the scalar checks.
 * One lane owns one line; a workgroup takes spc_les_hmix_lines_per_block(n, sizeof(T)) lines, whose q and z (2 (n - 1)
 * elements per line) live in LDS while y lives in the field itself.  Nothing is allocated inside the library.             */
#define SPC_HMIX_MAX_FIELDS 6
typedef struct spc_les_hmix_args {
    int64_t n_les;                      /* 0 is allowed: no-op                                               */
    int32_t itot, jtot, ktot, n_fields; /* n_fields 1 ... SPC_HMIX_MAX_FIELDS                                */
    int32_t axes, reserved;             /* axes: bit 0 the sweep along i, bit 1 along j; 1 ... 3             */
    void *fields[SPC_HMIX_MAX_FIELDS];       /* device [n_les][itot][jtot][ktot], updated in place           */
    const void *ax[SPC_HMIX_MAX_FIELDS];     /* device [n_les] per field                                     */
    const void *ay[SPC_HMIX_MAX_FIELDS];     /* device [n_les] per field                                     */
    const void *km;                     /* device [n_les][itot][jtot][ktot], read only                       */
    const void *kh2;                    /* device [n_les]                                                    */
} spc_les_hmix_args;
int spc_les_hmix_f64(const spc_les_hmix_args *args, void *stream);
int spc_les_hmix_f32(const spc_les_hmix_args *args, void *stream);
/* lines per workgroup of k_les_hline for lines of n cells of elem_size (4 or 8) bytes: 256 ... 16; 0: unsupported */
int spc_les_hmix_lines_per_block(int n, int elem_size);

/* ---- misc ----------------------------------------------------------------------------------- */
int spc_abi_version(void);          /* == SPC_ABI_VERSION                                          */
const char *spc_last_error(void);   /* text of the calling thread's last failure ("" if none)     */
int spc_device_count(void);         /* number of visible HIP devices (0 if none / no driver)      */
/* columns per workgroup the library would pick (pass 0 forward [lean, fused index map], 1 backward, 2 index, 3 diag,
 * 4 conservative backward): the `cb` of spc_describe_launch */
int spc_pick_cols_per_block(const spc_dims *dims, int pass);
/* WHICH kernel instantiation, slab size and grid the library launches for this batch, as text, e.g.
 *   "k_forward<f64,lean,91,160,wt=1,blk=1024,pre=1> cb=4 grid=256 block=1024 lds=17472 cus=256"
 * (template arguments: element type, lean / full output set, compile-time level counts [0,0 = run-time geometry],
 *  write-through stores, workgroup size, prologue prefetch; float batches of a compile-time geometry that take the
 *  8-byte-access forward kernel read "k_forward_f32v<91,160,wt=0>" -- pointers that are only 4-byte aligned fall back to
 *  the scalar kernel at launch time; pass 3: "k_diag<f64,91,160,wt=0>"; `cus` = the compute units of the current device
 *  the residency rules counted with, SPC_CUS overrides).  pass as above; flags (pass 0 only): bit 0 = the index
 * map is fused (idx != NULL), bit 1 = FULL variant (any optional output or surface coupling requested); elem_size 8
 * (f64) or 4 (f32).  The text comes from the very function the launchers use to choose, so a test can walk the
 * dispatch table and require that every instantiation it reaches is bit-checked (tests/test_dispatch_gpu.py).
 * Writes at most buflen-1 characters + NUL; returns the length of the full text or a negative spc_status. */
int spc_describe_launch(const spc_dims *dims, int pass, int flags, int elem_size, char *buf, int buflen);
/* The same for the K7 operators above: which instantiation a launch of spc_exner_* ... spc_rms_* takes, with how many rows per
 * workgroup (the slab height `rb`; 32 for rms, 0 for exner), e.g.
 *   "k_interp<f64,sl=7,wt=1> rb=8 grid=4465 lds=14144 cus=256"
 *   "k_interp_c<f64,pd=1,sl=8,w=1,wt=1> rb=9 ..."   "k_searchsorted<f32,sl=0,wt=0> ..."   "k_rms<f64,pd=2,wt=1> ..."   "k_exner<f32,wt=1> ..."
 * (template arguments as the kernel tables index them: sl = unrolled search depth, 0 run-time trip count, -1 rows read from
 *  global memory; pd = unrolled depth of numpy's pairwise sum, -1 explicit stack; w = weighted; wt = write-through stores;
 *  "none": nothing to launch).  op: SPC_SU_*; elem_size 8 or 4; args: the operator's own argument block (spc_interp_args,
 * spc_searchsorted_args, spc_interp_c_args; NULL for exner and rms), of which only the extents, pitches, mode and whether rho is
 * NULL are read -- no pointer is dereferenced and no device is needed; n_rows, n, pitch: the scalars of spc_rms_* (n: those of
 * spc_exner_*), ignored otherwise.  The text comes from the very functions the launchers choose with (tests/sputils_slabs.py
 * asserts the slab height of every launch it checks).  Refusals of the launchers that are no pointer checks are returned
 * here too.  Writes at most buflen-1 characters + NUL; returns the length of the full text or a negative spc_status. */
enum { SPC_SU_EXNER = 0, SPC_SU_INTERP = 1, SPC_SU_SEARCHSORTED = 2, SPC_SU_INTERP_C = 3, SPC_SU_RMS = 4 };
int spc_sputils_describe_launch(int32_t op, int32_t elem_size, const void *args, int64_t n_rows, int64_t n, int64_t pitch,
                                char *buf, int32_t buflen);
/* Bytes of spc_vnudge_args.work spc_variability_nudge_f64 wants for these extents (n_cols*2*itot*jtot*ktot*8: qt and
 * qsat transposed to contiguous planes; required for planes of more than ~9 000 points); negative spc_status on bad
 * extents. */
int64_t spc_vnudge_workspace_bytes(int64_t n_cols, int32_t itot, int32_t jtot, int32_t ktot);
/* The same for spc_variability_nudge_f32 (float planes: n_cols*2*itot*jtot*ktot*4, half the f64 value). */
int64_t spc_vnudge_workspace_bytes_f32(int64_t n_cols, int32_t itot, int32_t jtot, int32_t ktot);

#ifdef __cplusplus
}
#endif
#endif /* SPC_H */
