"""ctypes mirror of include/spc.h (struct layouts and prototypes) and the library loader.

The product path has NO CPU fallback: ``load_library()`` raises ``SpcLibraryError`` when
``libspc_hip.so`` has not been built (``python -c "import __graft_entry__ as g; g.build()"``).
"""
import ctypes
import os

ABI_VERSION = 4
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libspc_hip.so"
LIB_PATH = os.path.join(_HERE, LIB_NAME)

c_void_p, c_double, c_int32, c_int64 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.c_int64
c_int32_p = ctypes.POINTER(ctypes.c_int32)

SPC_OK, SPC_ERR_INVALID_ARGUMENT, SPC_ERR_UNSUPPORTED, SPC_ERR_LAUNCH, SPC_ERR_NO_DEVICE = 0, -1, -2, -3, -4


class SpcError(RuntimeError):
    """A C-ABI call returned a negative spc_status."""

    def __init__(self, code, text):
        super().__init__("spc error %d: %s" % (code, text))
        self.code = code


class SpcInvalidArgument(SpcError, ValueError):
    pass


class SpcLibraryError(ImportError):
    """The HIP extension is missing or does not match include/spc.h."""


class Dims(ctypes.Structure):
    _fields_ = [("n_cols", c_int64), ("nG", c_int32), ("nL", c_int32), ("pitchG", c_int64),
                ("pitchGh", c_int64), ("pitchL", c_int64), ("les_grid_shared", c_int32),
                ("cols_per_block", c_int32)]


def _ptrs(*names):
    return [(n, c_void_p) for n in names]


class ForwardArgs(ctypes.Structure):
    _fields_ = (_ptrs("U", "V", "T", "SH", "QL", "QI", "Pf", "Ph", "Zgfull", "Zghalf", "zf", "zh",
                      "u_d", "v_d", "thl_d", "qt_d", "ql_d", "ps_d", "rain", "rain_last")
                + [("factor", c_double), ("dt", c_double)]
                + _ptrs("f_u", "f_v", "f_thl", "f_qt", "f_ql", "ql_ref", "f_ps", "u", "v", "thl", "qt", "ps",
                        "Zf", "Zh", "rainrate", "idx", "Z0M", "Z0H", "QLflux", "QIflux", "SHflux", "TSflux",
                        "z0m", "z0h", "wthl", "wqt"))


class BackwardArgs(ctypes.Structure):
    _fields_ = (_ptrs("T", "SH", "QL", "QI", "U", "V", "A", "Zf", "Zgfull", "Zghalf", "zf",
                      "t_d", "qt_d", "ql_d", "ql_ice_d", "u_d", "v_d", "A_prof", "zh", "Zh", "rhobf_d")
                + [("conservative", c_int32), ("reserved", c_int32), ("factor", c_double), ("dt", c_double)]
                + _ptrs("f_T", "f_SH", "f_QL", "f_QI", "f_U", "f_V", "f_A", "start_index"))


class DiagnosticsArgs(ctypes.Structure):
    _fields_ = _ptrs("T", "SH", "QL", "QI", "Pf", "Zgfull", "Zghalf", "zf", "thl_d", "ql_d", "ql_ice_d",
                     "Tv", "THL", "QT", "Zf", "Zh", "pf", "t", "ql_water")


class VnudgeArgs(ctypes.Structure):
    _fields_ = ([("n_cols", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("constantT", c_int32)]
                + _ptrs("qt", "qsat", "thl", "ql", "R", "ql_av", "qt_av", "presf", "ql_ref", "beta", "a_add", "qt_std", "status", "work")
                + [("work_bytes", c_int64)])


class InterpArgs(ctypes.Structure):
    _fields_ = ([("n_rows", c_int64), ("n_x", c_int32), ("n_xp", c_int32), ("pitch_x", c_int64), ("pitch_xp", c_int64),
                 ("pitch_fp", c_int64), ("pitch_out", c_int64)] + _ptrs("x", "xp", "fp", "out"))


class SearchsortedArgs(ctypes.Structure):
    _fields_ = ([("n_rows", c_int64), ("n_a", c_int32), ("n_v", c_int32), ("pitch_a", c_int64), ("pitch_v", c_int64),
                 ("pitch_out", c_int64)] + _ptrs("a", "v", "out") + [("side_right", c_int32), ("reserved", c_int32)])


class InterpCArgs(ctypes.Structure):
    _fields_ = ([("n_rows", c_int64), ("nG", c_int32), ("nL", c_int32), ("pitch_Zh", c_int64), ("pitch_zh", c_int64),
                 ("pitch_q", c_int64), ("pitch_out", c_int64)] + _ptrs("Zh", "zh", "q", "rho", "out")
                + [("mode", c_int32), ("reserved", c_int32)])


class PipArgs(ctypes.Structure):
    _fields_ = ([("n_points", c_int64), ("n_vertices", c_int64), ("n_rings", c_int32), ("n_polys", c_int32)]
                + _ptrs("lon", "lat", "vx", "vy", "ring_start", "ring_role", "ring_poly", "out"))


class LesStateArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64)] + _ptrs("elem_off", "ktot") + [("prof", c_void_p * 4), ("pitch_prof", c_int64),
                ("amp", c_double * 4), ("out", c_void_p * 4)] + _ptrs("key_in") + [("pos_in", c_int32), ("reserved", c_int32)]
                + _ptrs("key_out", "pos_out") + [("gens_per_substream", c_int64)] + _ptrs("work") + [("work_bytes", c_int64)])


SLAB_MAX_FIELDS = 16      # SPC_SLAB_MAX_FIELDS


class SlabMeansArgs(ctypes.Structure):
    _fields_ = [("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_fields", c_int32),
                ("fields", c_void_p * SLAB_MAX_FIELDS), ("out", c_void_p * SLAB_MAX_FIELDS), ("pitch_out", c_int64)]


class SlabCloudArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("nG", c_int32)]
                + _ptrs("ql", "idx", "out") + [("pitch_idx", c_int64), ("pitch_out", c_int64)])


ADVANCE_MAX_FIELDS = 8    # SPC_ADVANCE_MAX_FIELDS


class LesAdvanceArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_fields", c_int32),
                 ("fields", c_void_p * ADVANCE_MAX_FIELDS), ("tend", c_void_p * ADVANCE_MAX_FIELDS),
                 ("mean", c_void_p * ADVANCE_MAX_FIELDS), ("pitch_tend", c_int64), ("pitch_mean", c_int64), ("dt", c_double),
                 ("sat_field", c_int32), ("reserved", c_int32)] + _ptrs("qsat", "ql", "ql_mean"))


class LesThermoArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_iter", c_int32)]
                + _ptrs("thl", "qt", "presf", "ex") + [("pitch_prof", c_int64)] + _ptrs("es_tab")
                + [("n_tab", c_int32), ("table_mode", c_int32), ("t_lo", c_double), ("inv_step", c_double)]
                + _ptrs("qsat", "ql", "temp", "ql_mean", "t_mean") + [("pitch_mean", c_int64)])


WP_MAX_FIELDS = 4         # SPC_WP_MAX_FIELDS
WP_MAX_KTOT = 8192        # rows NumPy sums in one chunk: spc_les_water_paths_* refuses longer ones


class WaterPathArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_fields", c_int32),
                 ("fields", c_void_p * WP_MAX_FIELDS), ("out", c_void_p * WP_MAX_FIELDS), ("w", c_void_p), ("pitch_w", c_int64),
                 ("cloud_field", c_int32), ("reserved", c_int32)] + _ptrs("top", "cover"))


class LesMicroArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("reserved", c_int32)]
                + _ptrs("qt", "ql", "qr", "qr_new", "thl", "temp", "rain", "sed_out", "sed_in", "lcpex", "w") + [("pitch_prof", c_int64)]
                + [(k, c_double) for k in ("dt", "qc0", "k_auto", "k_acc", "t_up", "t_dn")]
                + _ptrs("qt_mean", "thl_mean", "qr_mean", "qi_mean") + [("pitch_mean", c_int64)])


SPC_DIFFUSE_MAX_FIELDS = 4


class LesDiffuseArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_fields", c_int32),
                 ("fields", c_void_p * SPC_DIFFUSE_MAX_FIELDS), ("flux", c_void_p * SPC_DIFFUSE_MAX_FIELDS)]
                + _ptrs("a", "m", "cp", "s0") + [("pitch_prof", c_int64)])


SPC_ADVECT_MAX_FIELDS = 6


class LesAdvectArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_fields", c_int32)] + _ptrs("u", "v")
                + [("fields", c_void_p * SPC_ADVECT_MAX_FIELDS), ("out", c_void_p * SPC_ADVECT_MAX_FIELDS)] + _ptrs("hx", "hy", "cmax"))


SPC_VADVECT_MAX_FIELDS = 6


class LesVadvectArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_fields", c_int32)] + _ptrs("u", "v")
                + [("fields", c_void_p * SPC_VADVECT_MAX_FIELDS), ("out", c_void_p * SPC_VADVECT_MAX_FIELDS)]
                + _ptrs("hx", "hy", "cmax", "g", "r") + [("pitch_prof", c_int64), ("mtop", c_void_p)])


SPC_TRANSPORT_MAX_FIELDS = 6


class LesTransportArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_fields", c_int32)] + _ptrs("u", "v")
                + [("fields", c_void_p * SPC_TRANSPORT_MAX_FIELDS), ("out", c_void_p * SPC_TRANSPORT_MAX_FIELDS)]
                + _ptrs("hx", "hy", "cmax", "g", "r") + [("pitch_prof", c_int64), ("mtop", c_void_p), ("ftop", c_void_p)])


SPC_LIMITER_NONE, SPC_LIMITER_MC = 0, 1
LIMITERS = {"none": SPC_LIMITER_NONE, "mc": SPC_LIMITER_MC}


class LesTransport2Args(ctypes.Structure):
    _fields_ = LesTransportArgs._fields_ + [("limiter", c_int32)]


class LesRadiateArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_tab", c_int32)]
                + _ptrs("ql", "thl", "w", "c") + [("pitch_prof", c_int64)] + _ptrs("f0", "f1", "etab")
                + [("inv_step", c_double)] + _ptrs("flux", "fsfc"))


class LesBuoyancyArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("reserved", c_int32)]
                + _ptrs("thl", "qt", "ql", "u", "v", "hx", "hy", "t0", "lex", "s") + [("pitch_prof", c_int64), ("c1", c_double), ("c2", c_double)]
                + _ptrs("phi", "psfc", "amax"))


SPC_MIX_MAX_FIELDS = 6


class LesMixArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_fields", c_int32)]
                + _ptrs("u", "v", "theta", "gx", "gy", "kcap", "gz", "bz", "l2") + [("pitch_prof", c_int64)] + _ptrs("km", "kmax")
                + [("fields", c_void_p * SPC_MIX_MAX_FIELDS), ("out", c_void_p * SPC_MIX_MAX_FIELDS),
                   ("ax", c_void_p * SPC_MIX_MAX_FIELDS), ("ay", c_void_p * SPC_MIX_MAX_FIELDS)])


SPC_VMIX_MAX_FIELDS = 6


class LesVmixArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_fields", c_int32),
                 ("fields", c_void_p * SPC_VMIX_MAX_FIELDS), ("flux", c_void_p * SPC_VMIX_MAX_FIELDS),
                 ("dr", c_void_p * SPC_VMIX_MAX_FIELDS), ("el", c_void_p * SPC_VMIX_MAX_FIELDS), ("eu", c_void_p * SPC_VMIX_MAX_FIELDS)]
                + _ptrs("km", "kb", "kv2", "s0", "u", "v", "speed") + [("pitch_prof", c_int64)])


SPC_HMIX_MAX_FIELDS = 6


class LesHmixArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("n_fields", c_int32),
                 ("axes", c_int32), ("reserved", c_int32),
                 ("fields", c_void_p * SPC_HMIX_MAX_FIELDS), ("ax", c_void_p * SPC_HMIX_MAX_FIELDS), ("ay", c_void_p * SPC_HMIX_MAX_FIELDS)]
                + _ptrs("km", "kh2"))


class LesQtLocalArgs(ctypes.Structure):
    _fields_ = ([("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32), ("split", c_int32)]
                + _ptrs("qt", "ql", "a", "qtm") + [("pitch_prof", c_int64), ("count", c_void_p), ("pitch_count", c_int64)])


MOMENTS_MAX_FIELDS, MOMENTS_MAX_PAIRS = 8, 8               # SPC_MOMENTS_MAX_FIELDS, SPC_MOMENTS_MAX_PAIRS


class LesMomentsArgs(ctypes.Structure):
    _fields_ = [("n_les", c_int64), ("itot", c_int32), ("jtot", c_int32), ("ktot", c_int32),
                ("n_fields", c_int32), ("n_pairs", c_int32), ("face_field", c_int32),
                ("fields", c_void_p * MOMENTS_MAX_FIELDS),
                ("pair_a", c_int32 * MOMENTS_MAX_PAIRS), ("pair_b", c_int32 * MOMENTS_MAX_PAIRS),
                ("mean", c_void_p * MOMENTS_MAX_FIELDS), ("var", c_void_p * MOMENTS_MAX_FIELDS), ("std", c_void_p * MOMENTS_MAX_FIELDS),
                ("cov", c_void_p * MOMENTS_MAX_PAIRS), ("pitch_out", c_int64)]


THERMO_TABLE_LIBRARY, THERMO_TABLE_LDS, THERMO_TABLE_GLOBAL = 0, 1, 2      # spc_les_thermo_args.table_mode

SPC_RING_SHELL, SPC_RING_HOLE, SPC_RING_RECTANGLE = 0, 1, 2
SPC_LOC_EXTERIOR, SPC_LOC_BOUNDARY, SPC_LOC_INTERIOR = 0, 1, 2


#: every symbol include/spc.h declares: name -> (restype, argtypes)
PROTOTYPES = {
    "spc_forward_f64": (ctypes.c_int, [ctypes.POINTER(Dims), ctypes.POINTER(ForwardArgs), c_void_p]),
    "spc_forward_f32": (ctypes.c_int, [ctypes.POINTER(Dims), ctypes.POINTER(ForwardArgs), c_void_p]),
    "spc_cloud_indices_f64": (ctypes.c_int, [ctypes.POINTER(Dims), c_void_p, c_void_p, c_void_p, c_void_p]),
    "spc_cloud_indices_f32": (ctypes.c_int, [ctypes.POINTER(Dims), c_void_p, c_void_p, c_void_p, c_void_p]),
    "spc_backward_f64": (ctypes.c_int, [ctypes.POINTER(Dims), ctypes.POINTER(BackwardArgs), c_void_p]),
    "spc_backward_f32": (ctypes.c_int, [ctypes.POINTER(Dims), ctypes.POINTER(BackwardArgs), c_void_p]),
    "spc_diagnostics_f64": (ctypes.c_int, [ctypes.POINTER(Dims), ctypes.POINTER(DiagnosticsArgs), c_void_p]),
    "spc_diagnostics_f32": (ctypes.c_int, [ctypes.POINTER(Dims), ctypes.POINTER(DiagnosticsArgs), c_void_p]),
    "spc_surface_fluxes_f64": (ctypes.c_int, [c_int64] + [c_void_p] * 9),
    "spc_surface_fluxes_f32": (ctypes.c_int, [c_int64] + [c_void_p] * 9),
    "spc_variability_nudge_f64": (ctypes.c_int, [ctypes.POINTER(VnudgeArgs), c_void_p]),
    "spc_variability_nudge_f32": (ctypes.c_int, [ctypes.POINTER(VnudgeArgs), c_void_p]),
    "spc_exner_f64": (ctypes.c_int, [c_int64, c_void_p, c_void_p, c_int32, c_void_p]),
    "spc_exner_f32": (ctypes.c_int, [c_int64, c_void_p, c_void_p, c_int32, c_void_p]),
    "spc_interp_f64": (ctypes.c_int, [ctypes.POINTER(InterpArgs), c_void_p]),
    "spc_interp_f32": (ctypes.c_int, [ctypes.POINTER(InterpArgs), c_void_p]),
    "spc_searchsorted_f64": (ctypes.c_int, [ctypes.POINTER(SearchsortedArgs), c_void_p]),
    "spc_searchsorted_f32": (ctypes.c_int, [ctypes.POINTER(SearchsortedArgs), c_void_p]),
    "spc_interp_c_f64": (ctypes.c_int, [ctypes.POINTER(InterpCArgs), c_void_p]),
    "spc_interp_c_f32": (ctypes.c_int, [ctypes.POINTER(InterpCArgs), c_void_p]),
    "spc_rms_f64": (ctypes.c_int, [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "spc_rms_f32": (ctypes.c_int, [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "spc_point_in_polygon_f64": (ctypes.c_int, [ctypes.POINTER(PipArgs), c_void_p]),
    "spc_haversine_f64": (ctypes.c_int, [c_int64, c_void_p, c_void_p, c_double, c_double, c_void_p, c_void_p]),
    "spc_les_state_f64": (ctypes.c_int, [ctypes.POINTER(LesStateArgs), c_void_p]),
    "spc_les_state_workspace_bytes": (c_int64, [c_int64, c_int64, c_int32, c_int64]),
    "spc_mt19937_jump": (ctypes.c_int, [c_void_p, c_int32, c_int64, c_void_p, c_void_p]),
    "spc_mt19937_jump_poly": (ctypes.c_int, [ctypes.c_uint64, c_void_p]),
    "spc_slab_means_f64": (ctypes.c_int, [ctypes.POINTER(SlabMeansArgs), c_void_p]),
    "spc_slab_means_f32": (ctypes.c_int, [ctypes.POINTER(SlabMeansArgs), c_void_p]),
    "spc_slab_cloud_fraction_f64": (ctypes.c_int, [ctypes.POINTER(SlabCloudArgs), c_void_p]),
    "spc_slab_cloud_fraction_f32": (ctypes.c_int, [ctypes.POINTER(SlabCloudArgs), c_void_p]),
    "spc_les_advance_f64": (ctypes.c_int, [ctypes.POINTER(LesAdvanceArgs), c_void_p]),
    "spc_les_advance_f32": (ctypes.c_int, [ctypes.POINTER(LesAdvanceArgs), c_void_p]),
    "spc_les_thermo_f64": (ctypes.c_int, [ctypes.POINTER(LesThermoArgs), c_void_p]),
    "spc_les_thermo_f32": (ctypes.c_int, [ctypes.POINTER(LesThermoArgs), c_void_p]),
    "spc_les_water_paths_f64": (ctypes.c_int, [ctypes.POINTER(WaterPathArgs), c_void_p]),
    "spc_les_water_paths_f32": (ctypes.c_int, [ctypes.POINTER(WaterPathArgs), c_void_p]),
    "spc_les_microphysics_f64": (ctypes.c_int, [ctypes.POINTER(LesMicroArgs), c_void_p]),
    "spc_les_microphysics_f32": (ctypes.c_int, [ctypes.POINTER(LesMicroArgs), c_void_p]),
    "spc_les_diffuse_f64": (ctypes.c_int, [ctypes.POINTER(LesDiffuseArgs), c_void_p]),
    "spc_les_diffuse_f32": (ctypes.c_int, [ctypes.POINTER(LesDiffuseArgs), c_void_p]),
    "spc_les_diffuse_cols_per_block": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "spc_les_advect_f64": (ctypes.c_int, [ctypes.POINTER(LesAdvectArgs), c_void_p]),
    "spc_les_advect_f32": (ctypes.c_int, [ctypes.POINTER(LesAdvectArgs), c_void_p]),
    "spc_les_advect_strip": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "spc_les_advect_rows": (ctypes.c_int, [c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "spc_les_vadvect_f64": (ctypes.c_int, [ctypes.POINTER(LesVadvectArgs), c_void_p]),
    "spc_les_vadvect_f32": (ctypes.c_int, [ctypes.POINTER(LesVadvectArgs), c_void_p]),
    "spc_les_vadvect_cols_per_block": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "spc_les_transport_f64": (ctypes.c_int, [ctypes.POINTER(LesTransportArgs), c_void_p]),
    "spc_les_transport_f32": (ctypes.c_int, [ctypes.POINTER(LesTransportArgs), c_void_p]),
    "spc_les_transport_cols_per_block": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "spc_les_transport2_f64": (ctypes.c_int, [ctypes.POINTER(LesTransport2Args), c_void_p]),
    "spc_les_transport2_f32": (ctypes.c_int, [ctypes.POINTER(LesTransport2Args), c_void_p]),
    "spc_les_transport2_cols_per_block": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "spc_les_radiate_f64": (ctypes.c_int, [ctypes.POINTER(LesRadiateArgs), c_void_p]),
    "spc_les_radiate_f32": (ctypes.c_int, [ctypes.POINTER(LesRadiateArgs), c_void_p]),
    "spc_les_radiate_cols_per_block": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "spc_les_qt_local_f64": (ctypes.c_int, [ctypes.POINTER(LesQtLocalArgs), c_void_p]),
    "spc_les_qt_local_f32": (ctypes.c_int, [ctypes.POINTER(LesQtLocalArgs), c_void_p]),
    "spc_les_qt_local_split": (ctypes.c_int, [c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "spc_les_moments_f64": (ctypes.c_int, [ctypes.POINTER(LesMomentsArgs), c_void_p]),
    "spc_les_moments_f32": (ctypes.c_int, [ctypes.POINTER(LesMomentsArgs), c_void_p]),
    "spc_les_buoyancy_f64": (ctypes.c_int, [ctypes.POINTER(LesBuoyancyArgs), c_void_p]),
    "spc_les_buoyancy_f32": (ctypes.c_int, [ctypes.POINTER(LesBuoyancyArgs), c_void_p]),
    "spc_les_buoyancy_cols_per_block": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "spc_les_mix_f64": (ctypes.c_int, [ctypes.POINTER(LesMixArgs), c_void_p]),
    "spc_les_mix_f32": (ctypes.c_int, [ctypes.POINTER(LesMixArgs), c_void_p]),
    "spc_les_vmix_f64": (ctypes.c_int, [ctypes.POINTER(LesVmixArgs), c_void_p]),
    "spc_les_vmix_f32": (ctypes.c_int, [ctypes.POINTER(LesVmixArgs), c_void_p]),
    "spc_les_vmix_cols_per_block": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "spc_les_hmix_f64": (ctypes.c_int, [ctypes.POINTER(LesHmixArgs), c_void_p]),
    "spc_les_hmix_f32": (ctypes.c_int, [ctypes.POINTER(LesHmixArgs), c_void_p]),
    "spc_les_hmix_lines_per_block": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "spc_abi_version": (ctypes.c_int, []),
    "spc_last_error": (ctypes.c_char_p, []),
    "spc_device_count": (ctypes.c_int, []),
    "spc_pick_cols_per_block": (ctypes.c_int, [ctypes.POINTER(Dims), ctypes.c_int]),
    "spc_describe_launch": (ctypes.c_int, [ctypes.POINTER(Dims), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                           ctypes.c_int]),
    "spc_sputils_describe_launch": (ctypes.c_int, [c_int32, c_int32, c_void_p, c_int64, c_int64, c_int64, ctypes.c_char_p, c_int32]),
    "spc_vnudge_workspace_bytes": (c_int64, [c_int64, c_int32, c_int32, c_int32]),
    "spc_vnudge_workspace_bytes_f32": (c_int64, [c_int64, c_int32, c_int32, c_int32]),
}

_lib = None


def bind(lib, prototypes=PROTOTYPES):
    for name, (res, args) in prototypes.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise SpcLibraryError("%s does not export %s (declared in include/spc.h)" % (lib._name, name)) from e
        fn.restype, fn.argtypes = res, args
    return lib


def load_library(path=None):
    """dlopen libspc_hip.so and bind every prototype. Raises SpcLibraryError if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("SPC_LIB") or LIB_PATH   # SPC_LIB: A/B a variant build of the same ABI
    if not os.path.exists(p):
        raise SpcLibraryError(
            "HIP extension %s not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback on the product path." % p)
    try:
        lib = ctypes.CDLL(p)
    except OSError as e:
        raise SpcLibraryError("cannot load %s: %s" % (p, e)) from e
    bind(lib)
    v = lib.spc_abi_version()
    if v != ABI_VERSION:
        raise SpcLibraryError("%s has ABI version %d, python mirror expects %d" % (p, v, ABI_VERSION))
    if path is None:
        _lib = lib
    return lib


def describe_launch(lib, dims, pass_, flags=1, elem_size=8):
    """text of spc_describe_launch (include/spc.h): the kernel instantiation + launch shape chosen for ``dims``"""
    buf = ctypes.create_string_buffer(256)
    rc = lib.spc_describe_launch(ctypes.byref(dims), pass_, flags, elem_size, buf, len(buf))
    if rc < 0:
        check(lib, rc)
    return buf.value.decode()


SPC_SU_EXNER, SPC_SU_INTERP, SPC_SU_SEARCHSORTED, SPC_SU_INTERP_C, SPC_SU_RMS = range(5)


def sputils_describe_launch(lib, op, elem_size=8, args=None, n_rows=0, n=0, pitch=0):
    """text of spc_sputils_describe_launch (include/spc.h): the K7 kernel instantiation and slab height a launch takes; ``args``
    the operator's argument block (InterpArgs, SearchsortedArgs, InterpCArgs), or the scalars of rms (``n``: of exner)"""
    buf = ctypes.create_string_buffer(256)
    rc = lib.spc_sputils_describe_launch(op, elem_size, None if args is None else ctypes.cast(ctypes.pointer(args), c_void_p),
                                         n_rows, n, pitch, buf, len(buf))
    if rc < 0:
        check(lib, rc)
    return buf.value.decode()


def check(lib, rc):
    if rc == SPC_OK:
        return
    text = lib.spc_last_error().decode("utf-8", "replace")
    if rc == SPC_ERR_INVALID_ARGUMENT:
        raise SpcInvalidArgument(rc, text)
    raise SpcError(rc, text)


MT_N = 624          # words of NumPy's MT19937 key
MT_PW = 312         # 64-bit words of a jump polynomial (include/spc.h spc_mt19937_jump_poly)


def mt19937_jump(key, pos, n_words, lib=None):
    """NumPy's legacy MT19937 state (key, pos) after drawing ``n_words`` 32-bit words from (key, pos): the host jump-ahead
    of the library (spc_mt19937_jump), no device needed.  Returns (uint32 key [624], pos)."""
    import numpy
    lib = lib or load_library()
    k = numpy.ascontiguousarray(key, dtype=numpy.uint32)
    if k.shape != (MT_N,):
        raise ValueError("key must hold 624 words, got %s" % (k.shape,))
    out = numpy.empty(MT_N, dtype=numpy.uint32)
    p = ctypes.c_int32()
    check(lib, lib.spc_mt19937_jump(k.ctypes.data, int(pos), int(n_words), out.ctypes.data, ctypes.byref(p)))
    return out, int(p.value)


def mt19937_jump_poly(J, lib=None):
    """x^J mod phi (phi: MT19937's characteristic polynomial) as 312 uint64 words, bit i = coefficient of x^i"""
    import numpy
    lib = lib or load_library()
    out = numpy.empty(MT_PW, dtype=numpy.uint64)
    check(lib, lib.spc_mt19937_jump_poly(int(J), out.ctypes.data))
    return out
