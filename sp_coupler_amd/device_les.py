"""An LES ensemble whose 3-D fields live on the GPU (fields_on_device):
``DeviceLESEnsemble``, the stand-in of ``models.SyntheticLESEnsemble`` whose fields never leave the device, and its per-column
face.  ``models.DeviceLESEnsemble`` and ``models._DeviceLESRow`` are these same objects (``models`` imports this module when
one of the two names is first asked for; it stays pure NumPy until then)."""
import numpy
import torch

from . import advection as adv
from . import buoyancy as buo
from . import diffusion as df
from . import microphysics as mp
from . import horizontal_mixing as hmx
from . import mixing as mix
from . import vertical_mixing as vmix
from . import radiation as rad
from . import thermo as th
from .models import SyntheticLESEnsemble, _LESRow, _row_getter, _timed
from .transfer import Sharded


def _same(a, b):
    """the comparison of two cache keys: tuples element by element, arrays by shape and content, scalars with =="""
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, numpy.ndarray):
        return a.shape == b.shape and numpy.array_equal(a, b)
    return a is b or a == b


def _kept(old, key, make):
    """"upload again where the inputs changed": the cache entry ``old`` itself where there is one and its key ``old[0]`` is
    ``key``, else ``make()``, the new entry (whose first element is ``key``)"""
    return old if old is not None and _same(old[0], key) else make()


def _f64(*arrays):
    """host float64 copies: the array part of a cache key"""
    return tuple(numpy.array(a, dtype=numpy.float64) for a in arrays)


class _DeviceLESRow(_LESRow):
    """per-column face of a DeviceLESEnsemble: the field extents are the ensemble's; single rows of a device field are not
    handed out (the fields never leave the GPU through the library)"""

    def get_itot(self):
        return self._e.itot

    def get_jtot(self):
        return self._e.jtot

    @property
    def dx(self):
        """the grid spacing along i, m: the ensemble's after enable_advection(), else ``advection.DX``"""
        return float(numpy.broadcast_to(adv.DX if self._e.dx is None else self._e.dx, (self._e.n,))[self._i])

    @property
    def dy(self):
        return float(numpy.broadcast_to(adv.DY if self._e.dy is None else self._e.dy, (self._e.n,))[self._i])

    def get_dx(self):
        return self.dx

    def get_dy(self):
        return self.dy

    def get_xsize(self):
        """the extent of the periodic plane along i, m (splib/spio.py:104-111 asks an LES for it)"""
        return self.dx * self._e.itot

    def get_ysize(self):
        return self.dy * self._e.jtot

    def get_cloudfraction(self, indices, return_request=False):
        raise NotImplementedError("a DeviceLESEnsemble answers get_cloudfraction_batched (all columns, one launch)")

    def set_field(self, name, values):
        raise NotImplementedError("a DeviceLESEnsemble takes whole fields: set_fields_batched")

    def get_field(self, name):
        """les.get_field("LWP" | "TWP" | "RWP") (splib/spdummy.py:243-251): row i of the ensemble's water paths (K13) as a
        host [itot x jtot] array; the 3-D fields themselves are not handed out row by row"""
        if name not in DeviceLESEnsemble.WATER_PATHS:
            raise NotImplementedError("a DeviceLESEnsemble hands out the water paths LWP, TWP and RWP per LES; its 3-D fields "
                                      "stay on the GPU: get_fields_batched")
        return self._e._water_path_host(name)[self._i].copy()

    def get_statistics(self, names=None, pairs=None):
        """this LES's rows of the ensemble's ``get_statistics``: ``{"mean": {name: [nL]}, "var": ..., "std": ..., "cov": {(a, b):
        [nL]}, "TKE": [nL]}``, host float64"""
        host = self._e.get_statistics(names, pairs)
        return {kind: (v[self._i].copy() if kind == "TKE" else {k: a[self._i].copy() for k, a in v.items()}) for kind, v in host.items()}


def _device_row_getter(key):
    """the row getter of a DeviceLESEnsemble: row i of what ``get_profiles_batched((key,))`` returns at that moment.  The 3-D
    fields are the truth, so the profile is refreshed first (both refreshes are cached: a second read launches nothing)"""
    plain = _row_getter(key)

    def get(self, return_request=False):
        self._e._refresh_profile(key)
        return plain(self, return_request)
    return get


for _m, _k in (("get_profile_U", "U"), ("get_profile_V", "V"), ("get_profile_THL", "THL"), ("get_profile_QT", "QT"),
               ("get_profile_QL", "QL"), ("get_profile_QL_ice", "QL_ice"), ("get_profile_QR", "QR"), ("get_profile_T", "T")):
    setattr(_DeviceLESRow, _m, _device_row_getter(_k))


class DeviceLESEnsemble(SyntheticLESEnsemble):
    """SyntheticLESEnsemble whose 3-D fields are device tensors [n x itot x jtot x nL] in the engine's dtype
    (``transfer.Sharded`` row blocks under a ``multi.MultiDeviceEngine``) from ``set_les_state_batched`` through every
    variability nudge: the library never copies them to the host.  The 3-D state is the truth and the profiles follow from
    it: U, V, THL, QT, QL are the slab means of the fields (K10, ``Engine.slab_means``: ONE launch for all of them per
    change of the fields), the cloud fraction is ``Engine.slab_cloud_fraction`` of the QL field.  ``Qsat`` is an attached
    field, constant in time; the QL field is ``max(QT - Qsat, 0)``.  tests/slab_ref.py holds the NumPy twin of this class.
    After ``enable_thermo()`` Qsat and QL are instead the saturation adjustment of THL and QT at ``presf`` (K12,
    ``Engine.les_thermo``: DESIGN.md 7.3), redone whenever THL or QT has changed, and ``p["T"]`` is K12's slab mean of the
    cells' temperature; tests/les_thermo_ref.py holds the NumPy twin of that mode.
    ``get_water_paths_batched`` reduces the fields along k instead (K13, ``Engine.les_water_paths``): the column water paths
    LWP, TWP and RWP, [n x itot x jtot] device tensors, and the cloud cover; tests/les_water_paths_ref.py holds their twin.
    After ``enable_microphysics()`` every step ends with the warm-rain microphysics (K14, ``Engine.les_microphysics``): cloud
    water turns into rain, the QR field falls, ``rain2d`` collects what reaches the ground and ``p["Rain"]`` is its plane mean;
    tests/les_micro_ref.py holds the twin of that mode.
    After ``enable_diffusion()`` every step mixes U, V, THL and QT along k and lets the surface fluxes of the coupler into THL
    and QT (K15, ``Engine.les_diffuse``); tests/les_diffuse_ref.py holds the twin of that mode.
    After ``enable_advection()`` every step carries U, V, THL, QT and QR along i and j with the winds U and V on the periodic
    plane, in as many upwind substeps as the Courant sums ask for (K16, ``Engine.les_advect``); tests/les_advect_ref.py holds
    the twin of that mode.  With ``vertical=True`` every substep also carries them along k by the mass flux of continuity (K17,
    ``Engine.les_vadvect``) and ``get_vertical_wind_batched()`` returns W; tests/les_vadvect_ref.py holds that twin.
    After ``enable_radiation()`` every step cools THL at the top of the cloud water and warms it at its base (K18,
    ``Engine.les_radiate``) and ``get_radiative_flux_batched()`` returns the longwave flux; tests/les_radiate_ref.py holds the
    twin of that mode.
    After ``enable_qt_forcing(kind)`` every step moves QT between the wet and the dry cells of every plane by the cloud-water
    forcing the coupler handed over (K19, ``Engine.les_qt_local``: qt_forcing 'local' | 'strong'); tests/les_qt_local_ref.py
    holds the twin of that mode.
    After ``enable_buoyancy()`` every advective substep starts with the hydrostatic pressure force on U and V (K21,
    ``Engine.les_buoyancy``) and ``get_pressure_batched()`` returns the pressure perturbation; tests/les_buoyancy_ref.py holds
    the twin of that mode.
    After ``enable_mixing()`` every step mixes U, V, THL, QT and QR along i and j by the Smagorinsky-Lilly eddy viscosity of the
    flow (K24, ``Engine.les_mix``), after the advection and before K15, whose diffusivity it can supply (``vertical=True``);
    ``get_eddy_viscosity_batched()`` returns the viscosity; tests/les_mix_ref.py holds the twin of that mode.  With
    ``implicit=True`` the mixing is one backward-Euler step per grid line by the uncapped viscosity, in place (K26,
    ``Engine.les_hmix``); tests/les_hmix_ref.py holds the twin of that mode.
    After ``enable_vertical_mixing()`` (behind ``enable_mixing()``) every step mixes U, V, THL, QT and QR along k by each
    column's own uncapped eddy viscosity, with the surface fluxes into THL and QT and a neutral bulk drag on U and V (K25,
    ``Engine.les_vmix``), where K15 stands; ``get_vertical_viscosity_batched()`` returns that viscosity; tests/les_vmix_ref.py
    holds the twin of that mode.
    ``get_statistics_batched`` reduces the fields to their second moments per level (K20, ``Engine.les_moments``): means,
    variances, standard deviations and the covariances of ``statistics.PAIRS``; tests/les_moments_ref.py holds their twin."""

    fields_on_device = True
    MEAN_KEYS = ("U", "V", "THL", "QT", "QL")          # profiles that ARE slab means, where the field exists
    STEP_KEYS = ("U", "V", "THL", "QT")                # fields a step applies a tendency to
    fused_advance = True                               # evolve_model_batched: one K11 launch (False: torch ops + K10)
    FUSED_MIN_LES = 128                                # ... where a launch holds at least so many LES
    WATER_PATHS = {"LWP": "QL", "TWP": "QT", "RWP": "QR"}     # les.get_field(name) -> the 3-D field it is the column sum of

    def __init__(self, grid_indices, zf, zh, prof, itot=8, jtot=8, engine=None):
        super().__init__(grid_indices, zf, zh, prof)
        self.itot, self.jtot = int(itot), int(jtot)
        self.engine = engine                            # None: spcpl.get_engine() when first needed
        self.fields3d = {}
        self._means = None                              # host slab means of the fields as they are now, or None
        self._wp, self._wp_host, self._wp_w = None, {}, None      # K13's results of the fields as they are now; its weights
        self._stats, self._stats_host = None, {}        # K20's results of the fields as they are now

    # -- saturation adjustment (K12), opt-in -------------------------------------------------------------------------
    thermo = False                                     # enable_thermo(): Qsat and QL follow THL, QT and presf
    thermo_n_iter = None
    _thermo_stale = True                               # THL or QT changed since K12 last ran
    _thermo_prof = None                                # (host presf the upload was made from, device presf, device ex)
    _thermo_means = None                               # host slab means {"QL", "T"} of K12's last launch

    def enable_thermo(self, n_iter=None):
        """from now on the Qsat and QL fields are K12's saturation adjustment of THL and QT (``n_iter`` Newton iterations,
        default ``thermo.DEFAULT_N_ITER``), run again before their next use whenever THL or QT has changed, and ``p["T"]`` is
        the slab mean of the adjusted temperature.  Without this call every path of the ensemble is unchanged."""
        if self.nL == 1:
            raise ValueError("the saturation adjustment (K12) does not take LES of one level")
        if not self._has("les_thermo"):
            raise ValueError("the engine has no les_thermo (K12)")
        self.thermo, self.thermo_n_iter = True, n_iter
        self._thermo_stale, self._means = True, None

    def _ensure_thermo(self):
        """K12 where THL or QT has changed since its last launch: the Qsat and QL fields, p["QL"] and p["T"]"""
        f = self.fields3d
        if not self._thermo_stale or "THL" not in f or "QT" not in f:
            return
        eng = self._eng()
        presf = numpy.asarray(self.p["presf"], dtype=numpy.float64)
        self._thermo_prof = _kept(self._thermo_prof, presf, lambda: (presf.copy(), self._upload(presf), self._upload(th.exner(presf))))
        for k in ("Qsat", "QL"):
            if k not in f:
                f[k] = self._per_device(torch.empty_like, f["QT"])          # written whole by the launch
        if self.micro and "T" not in f:                 # K14 reads the cells' temperature for the cloud ice
            f["T"] = self._per_device(torch.empty_like, f["QT"])
        dev = eng.les_thermo(f["THL"], f["QT"], self._thermo_prof[1], self._thermo_prof[2], n_iter=self.thermo_n_iter,
                             qsat=f["Qsat"], ql=f["QL"], **({"temp": f["T"]} if self.micro else {}))
        self._thermo_means = self._to_host(dev)
        self.p.update(self._thermo_means)
        self._drop_water_paths()                        # QL is new
        self._drop_statistics()
        if self._means is not None:
            self._means["QL"] = self._thermo_means["QL"]
        self._thermo_stale = False

    # -- warm-rain microphysics (K14), opt-in -------------------------------------------------------------------------
    micro = False                                      # enable_microphysics(): QR, rain2d and p["Rain"] follow the cloud water
    micro_par = None                                   # v_fall, qc0, k_auto, k_acc
    rain2d = None                                      # device [n x itot x jtot]: the rain that has reached the ground, kg/m2
    _qr_spare = None                                   # the QR buffer K14 writes next (it reads the other one)
    _micro_prof = None                                 # ((dt, v_fall, host presf, Rhobf, zh, zf) of the upload, the four device profiles)

    def enable_microphysics(self, v_fall=None, qc0=None, k_auto=None, k_acc=None):
        """from now on every ``evolve_model_batched`` ends with ONE K14 launch per device (``Engine.les_microphysics``,
        DESIGN.md 7.3) on the stepped fields and the current QL: cloud water turns into rain (QT and THL in place), the QR
        field falls one upwind step, what reaches the ground is summed in ``rain2d`` [n x itot x jtot], whose plane mean is
        ``p["Rain"]``; p["QT"], p["THL"] and p["QR"] are the launch's slab means, and with ``enable_thermo()`` p["QL_ice"] is the
        mean of the cloud ice at the cells' temperature.  Needs a QT field and more than one level; a QR field is created,
        zero, where none is attached.  The cloud water must be able to follow the QT the launch changes: a step needs an
        attached Qsat field or ``enable_thermo()`` (ValueError otherwise, also with an attached QL alone).  The profiles are
        uploaded again whenever dt, v_fall, presf, Rhobf or the grid (zh, zf) changed.  The constants default to those of
        ``microphysics``.  Without this call every path of the ensemble is unchanged."""
        if self.nL == 1:
            raise ValueError("the microphysics (K14) does not take LES of one level")
        if "QT" not in self.fields3d:
            raise ValueError("the microphysics (K14) needs a QT field (set_fields_batched)")
        if not self._has("les_microphysics"):
            raise ValueError("the engine has no les_microphysics (K14)")
        f = self.fields3d
        if "QR" not in f:
            f["QR"] = self._per_device(torch.zeros_like, f["QT"])
        self._qr_spare = self._per_device(torch.empty_like, f["QT"])
        self.rain2d = self._per_device(lambda t: t.new_zeros(t.shape[:3]), f["QT"])
        self.micro_par = {"v_fall": mp.V_FALL if v_fall is None else float(v_fall), "qc0": mp.QC0 if qc0 is None else float(qc0),
                          "k_auto": mp.K_AUTO if k_auto is None else float(k_auto), "k_acc": mp.K_ACC if k_acc is None else float(k_acc)}
        self.micro, self._micro_prof = True, None
        self._thermo_stale = True                         # (K12's next launch also writes the cells' temperature)
        self._drop_water_paths()
        self._drop_statistics()

    def _microphysics(self, dt):
        """K14 on the stepped fields: QT, THL, QR, rain2d and their profiles; QL (and Qsat) are then those of the new QT and THL"""
        eng, f, p, par = self._eng(), self.fields3d, self.p, self.micro_par
        if self.n == 0:
            return
        if not (self.thermo or "Qsat" in f):              # (an attached QL without Qsat could not follow the QT this step changes)
            raise ValueError("the microphysics (K14) needs the cloud water of the current QT: a Qsat field, or enable_thermo()")
        self._ensure_ql()                                 # (thermo: K12 where stale, with the cells' temperature in f["T"])
        # everything the profiles are made of; the four [n x nL] / [nL] host arrays are copied and compared every step (kilobytes)
        key = (float(dt), par["v_fall"]) + _f64(p["presf"], p["Rhobf"], self.zh_cache, self.zf_cache)
        self._micro_prof = _kept(self._micro_prof, key, lambda: (
            key, [self._upload(a) for a in mp.profiles(key[4], key[5], key[3], key[2], dt, par["v_fall"])]))
        self._qr_spare = self._scratch(self._qr_spare, f["QT"], f["QR"])
        temp = f.get("T") if self.thermo else None
        dev = eng.les_microphysics(f["QT"], f["QL"], f["QR"], self._qr_spare, *self._micro_prof[1], dt, thl=f.get("THL"), temp=temp,
                                   rain=self.rain2d, qc0=par["qc0"], k_auto=par["k_auto"], k_acc=par["k_acc"])
        f["QR"], self._qr_spare = self._qr_spare, f["QR"]
        rain = eng.slab_means({"Rain": self._per_device(lambda t: t.unsqueeze(-1), self.rain2d)})["Rain"]
        m = self._to_host({**dev, "Rain": rain})
        p["Rain"] = m["Rain"][:, 0]
        p["QR"] = m["QR"]
        if "QI" in m:
            p["QL_ice"] = m["QI"]
        own = {k: m[k] for k in ("QT", "THL") if k in m}
        p.update(own)
        if self._means is not None:
            self._means.update(own)
        self._drop_water_paths()
        self._drop_statistics()
        self._thermo_stale = True                         # thermo: the tail of the step runs K12 on the new QT and THL
        if not self.thermo and "Qsat" in f:
            self._saturate()
            p["QL"] = self._to_host(eng.slab_means({"QL": f["QL"]}))["QL"]
            if self._means is not None:
                self._means["QL"] = p["QL"]

    # -- implicit vertical diffusion and surface fluxes (K15), opt-in ---------------------------------------------------------
    diffusion = False                                  # enable_diffusion(): the columns mix and take the surface fluxes
    diffuse_par = None                                 # k_max, h_mix, k_bg
    DIFFUSE_KEYS = ("U", "V", "THL", "QT")             # fields a step diffuses, where they exist
    DIFFUSE_FLUX = {"THL": "wt", "QT": "wq"}           # field -> the slot of ``tend`` that holds its kinematic surface flux
    _diffuse_prof = None                               # ((dt, k_max, h_mix, k_bg, host Rhobf, zh, zf) of the upload, device a, m, cp, s0)

    def enable_diffusion(self, k_max=None, h_mix=None, k_bg=None):
        """from now on every ``evolve_model_batched`` runs ONE K15 launch per device (``Engine.les_diffuse``)
        on the fields among U, V, THL and QT that exist, after the step and before K14 / K12: one backward-Euler step of the
        vertical diffusion with the profile of ``diffusion.diffusivity``.  THL takes the surface flux ``set_wt_surf`` /
        ``WT_surf`` handed over, QT that of ``set_wq_surf`` / ``WQ_surf`` (kinematic, positive upward; none where none was
        set); U and V take none (no surface drag).  The profiles then are K10's means of the diffused fields and QL follows
        the new QT.  The coefficients are uploaded again whenever dt, a parameter, Rhobf or the grid (zh, zf) changed.  The
        parameters default to those of ``diffusion``.  Without this call every path of the ensemble is unchanged."""
        if not any(k in self.fields3d for k in self.DIFFUSE_KEYS):
            raise ValueError("the diffusion (K15) needs one of the fields %s (set_fields_batched)" % (self.DIFFUSE_KEYS,))
        if not self._has("les_diffuse"):
            raise ValueError("the engine has no les_diffuse (K15)")
        if self.vertical_mixing:
            raise ValueError("the diffusion (K15) and the vertical mixing (K25) exclude each other: a step has one vertical diffusion")
        self.diffuse_par = {"k_max": df.K_MAX if k_max is None else float(k_max), "h_mix": df.H_MIX if h_mix is None else float(h_mix),
                            "k_bg": df.K_BG if k_bg is None else float(k_bg)}
        self.diffusion, self._diffuse_prof = True, None

    def _diffuse(self, dt):
        """K15 on the stepped fields; QL (without thermo) and the profiles are then those of the diffused fields"""
        eng, f, p, par = self._eng(), self.fields3d, self.p, self.diffuse_par
        keys = [k for k in self.DIFFUSE_KEYS if k in f]
        if self.n == 0 or not keys:
            return
        # everything the coefficients are made of; the host arrays are copied and compared every step (kilobytes)
        key = (float(dt), par["k_max"], par["h_mix"], par["k_bg"]) + _f64(p["Rhobf"], self.zh_cache, self.zf_cache)
        kd = self._mix_kd if self.mixing and self.mix_par["vertical"] else None      # K24's slab-mean viscosity at the faces
        if kd is not None:
            key += (kd,)
        self._diffuse_prof = _kept(self._diffuse_prof, key, lambda: (
            key, [self._upload(a) for a in df.profiles(key[5], key[6], key[4], dt, par["k_max"], par["h_mix"], par["k_bg"], kd=kd)]))
        a, m, cp, s0 = self._diffuse_prof[1]
        flux = {k: self._upload(numpy.asarray(self.tend[slot], dtype=numpy.float64).reshape(self.n))
                for k, slot in self.DIFFUSE_FLUX.items() if k in keys and slot in self.tend}
        eng.les_diffuse({k: f[k] for k in keys}, a, m, cp, s0=s0, flux=flux)
        self._follow_fields()                             # K12 stale, QL of the diffused QT, p[U, V, THL, QT, QL] = K10's means

    # -- horizontal upwind advection on the periodic plane (K16), opt-in --------------------------------------------------------
    advection = False                                  # enable_advection(): the winds carry the fields along i and j
    advect_par = None                                  # cfl, max_substeps
    dx = dy = None                                     # the grid spacings, m (scalars or [n]); None: those of ``advection``
    ADVECT_KEYS = ("U", "V", "THL", "QT", "QR")        # fields a step advects, where they exist
    advect_courant = None                              # the largest Courant sum any substep of the last step returned
    advect_substeps = None                             # the substeps of the last step
    _advect_spare = None                               # name -> the buffer K16 writes next (it reads the field)
    _advect_coef = None                                # ((dt, dx, dy) of the uploads, {substeps: device (hx, hy)})
    advect_vertical = False                            # enable_advection(vertical=True): K17 follows every K16 substep
    advect_courant_z = None                            # the largest vertical Courant sum any substep of the last step returned
    _vadvect_prof = None                               # (the host weights of the upload, device (g, r))
    _vadvect_mtop = None                               # the mass flux through the upper faces in the last substep, device
    _vadvect_dt = None                                 # the seconds of that substep
    advect_conservative = False                        # enable_advection(vertical=True, conservative=True): K22 is every substep
    _transport_ftop = None                             # what K22 writes per substep: [fields x n x itot x jtot], device
    _transport_lid = None                              # (the names of the transported fields, the sum of ftop over the substeps)
    advect_order = 1                                   # enable_advection(..., conservative=True, order=2): K23 is every substep
    advect_limiter = "mc"                              # the limiter of K23's slopes: "mc" or "none"

    def enable_advection(self, dx=None, dy=None, cfl=None, max_substeps=None, vertical=False, conservative=False, order=1, limiter="mc"):
        """from now on every ``evolve_model_batched`` advects the fields among U, V, THL, QT and QR that exist with the winds U
        and V on the doubly periodic plane (K16, ``Engine.les_advect``), after the step and before K15 / K14 /
        K12: ONE probe launch per device finds the largest Courant sum c of the whole step, n_sub = max(1, ceil(c / cfl))
        launches of dt / n_sub follow, each into spare buffers that are swapped in (RuntimeError, the fields as the step left
        them, where c is not finite or n_sub > max_substeps).  ``advect_substeps`` and ``advect_courant`` hold n_sub and the
        largest Courant sum of the substeps.  The profiles then are K10's means of the advected fields and QL follows the new
        QT.  ``dx`` and ``dy`` (m, scalars or one per LES) are also what the rows' get_dx / get_dy / get_xsize / get_ysize
        answer.  The coefficients are uploaded again whenever dt, n_sub, dx or dy changed.  The parameters default to those of
        ``advection``.  Needs U and V fields.  Without this call every path of the ensemble is unchanged.

        ``vertical=True`` adds the vertical advection by the mass flux of continuity (K17, ``Engine.les_vadvect``): a K17 probe
        follows K16's, both with the coefficients of the whole step, n_sub comes from the larger of their Courant sums, and
        every substep is K16, a swap, K17 on the same fields (with the winds K16 just produced) into the same spare buffers and
        a swap: 2 + 2 n_sub launches per device and step.  The profiles g = ``water_path_weights()`` and r = 1 / g are uploaded
        once.  ``advect_courant_z`` holds the largest vertical Courant sum of the substeps (it can grow during them, so it is
        recorded and refused only where it is not finite: RuntimeError), ``get_vertical_wind_batched()`` the vertical wind of
        the last substep.  With the default every path, launch count and result is what it is without the argument.

        ``conservative=True`` (with ``vertical=True``; ValueError otherwise, or where the engine has no ``les_transport``)
        replaces the split pair by K22 (``Engine.les_transport``): one unsplit donor-cell step in flux form that conserves
        sum(rho dz x) of every field up to what passes the lid.  Per step ONE K22 probe with the coefficients of the whole dt
        gives the largest outflow Courant sum c and n_sub = ``advection.substeps(c, cfl, max_substeps)`` (with
        ``enable_buoyancy()`` at least the gravity wave's); every substep is K21 where enabled, then ONE K22 on the fields
        into the spare buffers, then a swap: 1 + n_sub launches per device and step.  ``advect_courant`` holds the largest
        outflow sum of the substeps (RuntimeError where it is not finite), ``advect_courant_z`` is None,
        ``get_vertical_wind_batched()`` works from K22's mass flux and ``get_lid_flux_batched()`` returns what left through
        the lid.  With the default every path, launch count and result is what it is without the argument.

        ``order=2`` (with ``conservative=True``; ValueError otherwise, for an order other than 1 or 2, for a ``limiter`` other
        than ``"mc"`` or ``"none"``, or where the engine has no ``les_transport2``) gives every substep a second-order face value:
        K23 (``Engine.les_transport2``) with the limiter in K22's place.  The probe stays K22's (the outflow Courant sums are
        the same bits), the launch count stays 1 + n_sub, and everything else of the conservative mode is unchanged.  With the
        default ``order=1`` every path, launch and bit is what it is without the argument."""
        if "U" not in self.fields3d or "V" not in self.fields3d:
            raise ValueError("the advection (K16) needs the fields U and V (set_fields_batched)")
        if not self._has("les_advect"):
            raise ValueError("the engine has no les_advect (K16)")
        if vertical and not self._has("les_vadvect"):
            raise ValueError("the engine has no les_vadvect (K17)")
        if conservative and not vertical:
            raise ValueError("the conservative transport (K22) is the horizontal and the vertical advection in one: it needs vertical=True")
        if conservative and not self._has("les_transport"):
            raise ValueError("the engine has no les_transport (K22)")
        if order not in (1, 2):
            raise ValueError("the order of the advection is 1 (donor cell) or 2 (K23), not %r" % (order,))
        if limiter not in ("mc", "none"):
            raise ValueError("the limiter of the second-order transport (K23) is 'mc' or 'none', not %r" % (limiter,))
        if order == 2 and not conservative:
            raise ValueError("the second-order transport (K23) is the conservative transport with another face value: it needs conservative=True")
        if order == 2 and not self._has("les_transport2"):
            raise ValueError("the engine has no les_transport2 (K23)")
        dx, dy = adv.DX if dx is None else dx, adv.DY if dy is None else dy
        adv.coefficients(1.0, dx, dy, n=self.n)                       # (ValueError for a spacing that is not positive, or not [n])
        self.dx = numpy.array(dx, dtype=numpy.float64) if numpy.ndim(dx) else float(dx)
        self.dy = numpy.array(dy, dtype=numpy.float64) if numpy.ndim(dy) else float(dy)
        self.advect_par = {"cfl": adv.CFL if cfl is None else float(cfl),
                           "max_substeps": adv.MAX_SUBSTEPS if max_substeps is None else int(max_substeps)}
        if not self.advect_par["cfl"] > 0 or self.advect_par["max_substeps"] < 1:
            raise ValueError("the advection (K16) needs cfl > 0 and max_substeps >= 1")
        self.advection, self._advect_coef, self._advect_spare = True, None, {}
        self.advect_vertical, self._vadvect_prof, self._vadvect_mtop, self._vadvect_dt = bool(vertical), None, None, None
        self.advect_courant_z = None
        self.advect_conservative, self._transport_ftop, self._transport_lid = bool(conservative), None, None
        self.advect_order, self.advect_limiter = int(order), limiter
        self.buoyancy = False                                         # (K21 is enabled after, and for, the advection of this call)

    def _advect_coefs(self, dt, n_sub):
        """device (hx, hy) of the substeps dt / n_sub; uploaded where dt, n_sub, dx or dy are not those of the last step"""
        key = (float(dt),) + _f64(self.dx, self.dy)
        old = self._advect_coef = _kept(self._advect_coef, key, lambda: (key, {}))
        if n_sub not in old[1]:
            for m in [m for m in old[1] if m != 1]:               # the probe's and one other: n_sub changed
                del old[1][m]
            old[1][n_sub] = tuple(self._upload(a) for a in adv.coefficients(float(dt) / n_sub, self.dx, self.dy, n=self.n))
        return old[1][n_sub]

    def _device_max(self, t):
        """the largest element of a device vector (of the blocks of a Sharded one): one number per device to the host"""
        parts = [(e, part) for e, part in zip(self._engines(), getattr(t, "parts", [t])) if part.numel()]
        vals, out = [], []
        for e, part in parts:
            with e.on_stream():
                vals.append(part.max())
        for (e, _), v in zip(parts, vals):                # (read on the stream that made it: torch's current stream does not wait for an engine's own)
            with e.on_stream():
                out.append(float(v.item()))
        return max(out)

    def _advect(self, dt):
        """K16 on the stepped fields: the probe, then n_sub launches into the spare buffers; QL (without thermo) and the
        profiles are then those of the advected fields, unless K15 follows and does both"""
        if self.advect_conservative:
            return self._transport(dt)
        eng, f = self._eng(), self.fields3d
        if self.n == 0:
            return
        if "U" not in f or "V" not in f:
            raise ValueError("the advection (K16) needs the fields U and V (set_fields_batched)")
        keys = [k for k in self.ADVECT_KEYS if k in f]
        buoyant = self.buoyancy
        if buoyant:
            prof, ql = self._buoyancy_inputs()
        c = self._device_max(eng.les_advect({}, {}, f["U"], f["V"], *self._advect_coefs(dt, 1)))
        vertical = self.advect_vertical
        if vertical:                                      # K17's probe: the vertical Courant sums of the whole step
            g, r = self._vadvect_profiles()
            c = max(c, self._device_max(eng.les_vadvect({}, {}, f["U"], f["V"], *self._advect_coefs(dt, 1), g, r)))
        n_sub = self._advect_substeps(c, dt)
        hx, hy = self._advect_coefs(dt, n_sub)
        spare = self._advect_spare
        for k in keys:
            spare[k] = self._scratch(spare.get(k), f[k], f[k])
        if vertical:
            self._vadvect_mtop = self._scratch(self._vadvect_mtop, f["U"])
        if buoyant:
            self._buoyancy_phi = self._scratch(self._buoyancy_phi, f["U"])
        worst = worst_z = worst_b = None
        for _ in range(n_sub):
            if buoyant:                                   # forward-backward: the winds feel the pressure, then carry the fields
                am = eng.les_buoyancy(f["THL"], f["QT"], ql, f["U"], f["V"], hx, hy, *prof, self._buoyancy_phi)
                worst_b = am if worst_b is None else self._per_device(torch.maximum, worst_b, am)
            out = {k: spare[k] for k in keys}
            cm = eng.les_advect({k: f[k] for k in keys}, out, f["U"], f["V"], hx, hy)
            for k in keys:
                f[k], spare[k] = spare[k], f[k]
            worst = cm if worst is None else self._per_device(torch.maximum, worst, cm)
            if vertical:                                  # K17 reads the winds K16 just produced
                out = {k: spare[k] for k in keys}
                cz = eng.les_vadvect({k: f[k] for k in keys}, out, f["U"], f["V"], hx, hy, g, r, mtop=self._vadvect_mtop)
                for k in keys:
                    f[k], spare[k] = spare[k], f[k]
                worst_z = cz if worst_z is None else self._per_device(torch.maximum, worst_z, cz)
        self.advect_substeps, self.advect_courant = n_sub, self._device_max(worst)
        if vertical:
            self._vadvect_dt = float(dt) / n_sub
            self.advect_courant_z = self._device_max(worst_z)
        if buoyant:
            self.buoyancy_wind_change = self._device_max(worst_b)
        self._drop_water_paths()
        self._drop_statistics()
        self._thermo_stale = True                         # thermo: K12 runs on the advected THL and QT before their next use
        if not self.diffusion:                            # (else the QL field and the means follow the diffused fields: _diffuse)
            self._follow_fields()
        if vertical and not numpy.isfinite(self.advect_courant_z):
            raise RuntimeError("the vertical advection (K17) found the Courant sum c = %r: the mass flux is not finite" % self.advect_courant_z)
        if buoyant and not numpy.isfinite(self.buoyancy_wind_change):
            raise RuntimeError("the pressure force (K21) found the wind change %r: the pressure is not finite" % self.buoyancy_wind_change)

    def _buoyancy_inputs(self):
        """(device (t0, lex, s), the QL field or None) of K21 for this step: QL and p[THL, QT, QL] of the stepped fields, then
        the profiles of those means"""
        f = self.fields3d
        if "THL" not in f or "QT" not in f:
            raise ValueError("the pressure force (K21) needs the fields THL and QT (set_fields_batched)")
        self._follow_fields()
        return self._buoyancy_profiles(), f.get("QL")

    def _advect_substeps(self, c, dt):
        """the substeps of a step of ``dt`` whose probes found the Courant sum ``c``, at least the gravity wave's with
        enable_buoyancy(); RuntimeError, after QL and the profiles have followed the stepped fields (nothing has been advected),
        where c is not finite or more than max_substeps would be needed"""
        par = self.advect_par
        try:
            n_sub = adv.substeps(c, par["cfl"], par["max_substeps"])
            if self.buoyancy:                             # the fastest gravity wave asks for its own substeps
                n_wave = buo.wave_substeps(dt, self.dx, self.dy, par["cfl"], self.buoyancy_wave_speed)
                if n_wave > par["max_substeps"]:
                    raise RuntimeError("the pressure force (K21) needs %d substeps for waves of %g m/s at cfl %g, more than max_substeps = %d"
                                       % (n_wave, self.buoyancy_wave_speed, par["cfl"], par["max_substeps"]))
                n_sub = max(n_sub, n_wave)
        except RuntimeError:
            self._follow_fields()
            raise
        return n_sub

    def _transport(self, dt):
        """K22 on the stepped fields: the probe, then n_sub launches into the spare buffers, each the whole transport of its
        substep; what follows the substeps is what follows them in ``_advect``"""
        eng, f = self._eng(), self.fields3d
        if self.n == 0:
            return
        if "U" not in f or "V" not in f:
            raise ValueError("the advection (K22) needs the fields U and V (set_fields_batched)")
        keys = [k for k in self.ADVECT_KEYS if k in f]
        buoyant = self.buoyancy
        if buoyant:
            prof, ql = self._buoyancy_inputs()
        g, r = self._vadvect_profiles()
        c = self._device_max(eng.les_transport({}, {}, f["U"], f["V"], *self._advect_coefs(dt, 1), g, r))
        n_sub = self._advect_substeps(c, dt)
        hx, hy = self._advect_coefs(dt, n_sub)
        spare = self._advect_spare
        for k in keys:
            spare[k] = self._scratch(spare.get(k), f[k], f[k])
        self._vadvect_mtop = self._scratch(self._vadvect_mtop, f["U"])
        if buoyant:
            self._buoyancy_phi = self._scratch(self._buoyancy_phi, f["U"])
        shapes = lambda t, lead=(): [lead + tuple(part.shape) for part in getattr(t, "parts", [t])]          # noqa: E731
        if self._transport_ftop is None or shapes(self._transport_ftop) != [s[:4] for s in shapes(f["U"], (len(keys),))]:
            self._transport_ftop = self._per_device(lambda w: w.new_empty((len(keys),) + tuple(w.shape[:3])), f["U"])
        ftop = self._transport_ftop
        worst = worst_b = total = None
        for _ in range(n_sub):
            if buoyant:                                   # forward-backward: the winds feel the pressure, then carry the fields
                am = eng.les_buoyancy(f["THL"], f["QT"], ql, f["U"], f["V"], hx, hy, *prof, self._buoyancy_phi)
                worst_b = am if worst_b is None else self._per_device(torch.maximum, worst_b, am)
            out = {k: spare[k] for k in keys}
            if self.advect_order == 2:
                cm = eng.les_transport2({k: f[k] for k in keys}, out, f["U"], f["V"], hx, hy, g, r, limiter=self.advect_limiter,
                                        mtop=self._vadvect_mtop, ftop=ftop)
            else:
                cm = eng.les_transport({k: f[k] for k in keys}, out, f["U"], f["V"], hx, hy, g, r, mtop=self._vadvect_mtop, ftop=ftop)
            for k in keys:
                f[k], spare[k] = spare[k], f[k]
            worst = cm if worst is None else self._per_device(torch.maximum, worst, cm)
            # (elementwise adds in substep order: a NumPy twin has the same bits)
            total = self._per_device(torch.clone, ftop) if total is None else self._per_device(torch.add, total, ftop)
        self.advect_substeps, self.advect_courant, self.advect_courant_z = n_sub, self._device_max(worst), None
        self._vadvect_dt, self._transport_lid = float(dt) / n_sub, (tuple(keys), total)
        if buoyant:
            self.buoyancy_wind_change = self._device_max(worst_b)
        self._drop_water_paths()
        self._drop_statistics()
        self._thermo_stale = True                         # thermo: K12 runs on the transported THL and QT before their next use
        if not self.diffusion:                            # (else the QL field and the means follow the diffused fields: _diffuse)
            self._follow_fields()
        if not numpy.isfinite(self.advect_courant):
            raise RuntimeError("the conservative transport (%s) found the Courant sum c = %r: the winds or the mass flux are not finite"
                               % ("K23" if self.advect_order == 2 else "K22", self.advect_courant))
        if buoyant and not numpy.isfinite(self.buoyancy_wind_change):
            raise RuntimeError("the pressure force (K21) found the wind change %r: the pressure is not finite" % self.buoyancy_wind_change)

    def get_lid_flux_batched(self):
        """dict name -> device tensor [n x itot x jtot] (Sharded row blocks under a MultiDeviceEngine): per transported field
        the sum over the substeps of the last step of K22's ``ftop``, what left every column through the lid in units of
        rho dz x (negative: it entered); None before the first step of enable_advection(vertical=True, conservative=True)"""
        if not self.advect_conservative or self._transport_lid is None:
            return None
        keys, total = self._transport_lid
        if isinstance(total, Sharded):
            return {k: Sharded([part[q] for part in total.parts], total.bounds) for q, k in enumerate(keys)}
        return {k: total[q] for q, k in enumerate(keys)}

    def _vadvect_profiles(self):
        """device (g, r) of K17: g = water_path_weights(), r = 1 / g; uploaded once, and again where the weights changed"""
        w = numpy.ascontiguousarray(self.water_path_weights())
        self._vadvect_prof = _kept(self._vadvect_prof, w, lambda: (w, tuple(self._upload(a) for a in adv.vertical_profiles(w))))
        return self._vadvect_prof[1]

    def get_vertical_wind_batched(self):
        """the device tensor [n x itot x jtot x nL] (Sharded row blocks under a MultiDeviceEngine) of the vertical wind W in m/s
        at the UPPER faces of the cells, positive upward, that continuity gave the last substep of the last step
        (``advection.vertical_wind`` of K17's mass flux); None before the first step of enable_advection(vertical=True)"""
        if not self.advect_vertical or self._vadvect_mtop is None or self._vadvect_dt is None:
            return None
        rho = self._upload(numpy.asarray(self.p["Rhobf"], dtype=numpy.float64))
        return self._per_device(lambda m, rh: adv.vertical_wind(m, rh, self._vadvect_dt), self._vadvect_mtop, rho)

    # -- hydrostatic pressure force on the winds (K21), opt-in --------------------------------------------------------------------
    buoyancy = False                                   # enable_buoyancy(): K21 in front of every advective substep
    buoyancy_wave_speed = None                         # m/s: the gravity wave the substeps resolve
    buoyancy_wind_change = None                        # the largest |du| + |dv| any substep of the last step returned, m/s
    _buoyancy_prof = None                              # ((host means THL, QT, QL, presf, zh) of the upload, device (t0, lex, s))
    _buoyancy_phi = None                               # the pressure perturbation of the last substep, device

    def enable_buoyancy(self, wave_speed=None):
        """from now on every advective substep of ``evolve_model_batched`` is K21 (``Engine.les_buoyancy``) with
        the substep's hx and hy on the winds, then K16, then K17: the buoyancy of THL, QT and QL against the virtual potential
        temperature of their slab means is integrated downward to a pressure perturbation whose horizontal gradient
        accelerates U and V, and continuity turns the convergence into vertical motion (forward-backward: the order that is
        stable for gravity waves); after ``enable_advection(..., vertical=True, conservative=True)`` it is K21, then K22.  Needs ``enable_advection(..., vertical=True)`` (without continuity the pressure force has
        no feedback) and THL, QT, U and V fields (ValueError otherwise).  QL is used where the ensemble has one (K12 where
        stale, or max(QT - Qsat, 0)), formed once per step from the stepped fields, whose slab means p[THL, QT, QL] give the
        profiles t0, lex and s (``buoyancy.profiles``; uploaded again only where they changed): one K10 launch (and one K12
        with ``enable_thermo()``) more per step.  n_sub is the larger of what the Courant probes ask for and
        ceil(wave_speed * dt / (cfl * min(dx, dy))) (``wave_speed`` defaults to ``buoyancy.WAVE_SPEED``), refused above
        ``max_substeps`` like K16's.  ``get_pressure_batched()`` returns phi of the last substep, ``buoyancy_wind_change`` holds
        the largest wind change of the step; the step raises RuntimeError where that is not finite.  Without this call every
        path, launch count and result of the ensemble is unchanged."""
        if not (self.advection and self.advect_vertical):
            raise ValueError("the pressure force (K21) needs enable_advection(..., vertical=True): continuity is its feedback")
        missing = [k for k in ("THL", "QT", "U", "V") if k not in self.fields3d]
        if missing:
            raise ValueError("the pressure force (K21) needs the fields %s (set_fields_batched)" % missing)
        if not self._has("les_buoyancy"):
            raise ValueError("the engine has no les_buoyancy (K21)")
        speed = buo.WAVE_SPEED if wave_speed is None else float(wave_speed)
        if not (numpy.isfinite(speed) and speed >= 0):
            raise ValueError("the pressure force (K21) needs a finite wave_speed >= 0")
        self.buoyancy, self.buoyancy_wave_speed = True, speed
        self.buoyancy_wind_change, self._buoyancy_prof, self._buoyancy_phi = None, None, None

    def _buoyancy_profiles(self):
        """device (t0, lex, s) of K21 from the host means as they are now; uploaded again where anything they are made of changed"""
        p = self.p
        has_ql = "QL" in self.fields3d
        key = _f64(p["THL"], p["QT"], p["QL"] if has_ql else numpy.zeros(0), p["presf"], self.zh_cache)
        self._buoyancy_prof = _kept(self._buoyancy_prof, key, lambda: (key, tuple(self._upload(a) for a in buo.profiles(
            key[0], key[1], key[2] if has_ql else None, key[3], key[4], zf=self.zf_cache))))
        return self._buoyancy_prof[1]

    def get_pressure_batched(self):
        """the device tensor [n x itot x jtot x nL] (Sharded row blocks under a MultiDeviceEngine) of the hydrostatic pressure
        perturbation phi in m2/s2 that K21 found in the last substep of the last step; None before the first step of
        enable_buoyancy()"""
        return self._buoyancy_phi if self.buoyancy else None

    # -- Smagorinsky-Lilly subgrid mixing (K24), opt-in ---------------------------------------------------------------------------
    mixing = False                                     # enable_mixing(): an eddy viscosity of the flow mixes the fields along i and j
    mix_par = None                                     # cs, prandtl, cap, theta_ref, stability, vertical, dx, dy
    MIX_KEYS = ("U", "V", "THL", "QT", "QR")           # fields a step mixes, where they exist
    MIX_WINDS = ("U", "V")                             # ... with the winds' coefficients; the others take the scalars'
    mixing_k_max = None                                # the largest uncapped viscosity of the last step, m2/s
    mixing_capped = None                               # ... lies above the smallest cap: the cap bound somewhere
    _mix_prof = None                                   # ((cs, prandtl, theta_ref, dx, dy, zf, zh) of the upload, device (gz, bz, l2))
    _mix_coef = None                                   # ((dt, prandtl, cap, dx, dy) of the upload, device gx, gy, kcap, winds' and scalars' (ax, ay), min kcap)
    _mix_km = None                                     # the eddy viscosity of the last step, device
    _mix_spare = None                                  # name -> the buffer K24 writes next (it reads the field)
    _mix_kd = None                                     # vertical=True: host [n x nL], K15's face diffusivity of this step
    _hmix_huge = None                                  # implicit=True: device [n], the type's largest finite value, the cap of K24's probe
    _hmix_kh2 = None                                   # implicit=True: ((kh_cap,) of the upload, device kh2)

    def enable_mixing(self, cs=None, prandtl=None, cap=None, theta_ref=None, stability=True, dx=None, dy=None, vertical=False,
                      implicit=False, kh_cap=None):
        """from now on every ``evolve_model_batched`` runs ONE ``Engine.les_mix`` per device (K24, DESIGN.md 7.3: two launches)
        after K16 / K17 / K22 / K23 and before K15: the Smagorinsky-Lilly eddy viscosity km of the winds U and V and, with
        ``stability=True``, of theta = THL (the moist correction of the stability is left out), capped at
        ``mixing.cap`` so that a mixed value is a convex combination of a cell and its four neighbours, mixes the fields among
        U and V (the winds' coefficients) and THL, QT and QR (the scalars': the winds' divided by ``prandtl``) that exist along
        i and j in flux form, into scratch buffers that are swapped in.  The profiles then are K10's means of the mixed fields
        and QL follows the new QT.  ``dx`` and ``dy`` default to those of ``enable_advection()`` where it was called, else to
        ``advection.DX`` / ``DY``; ``cs``, ``prandtl``, ``cap`` and ``theta_ref`` to those of ``mixing``.  The profiles gz, bz
        and l2 are uploaded once, and again only where the grid, dx, dy or a parameter changed; the coefficients again where dt
        changed.  ``get_eddy_viscosity_batched()`` returns km, ``mixing_k_max`` holds the largest uncapped viscosity of the
        step and ``mixing_capped`` whether it lies above the smallest cap (no substeps: where the cap binds, the mixing is
        weaker than the closure asks for).  ``vertical=True`` (after ``enable_diffusion()``; ValueError otherwise) makes K15's
        face diffusivity of the step k_bg + 0.5 (m[k-1] + m[k]) with m the slab mean of km (one K10 launch more), in place of
        the profile of ``diffusion.diffusivity``.  ``implicit=True`` mixes by the closure's OWN viscosity instead (K26,
        ``Engine.les_hmix``; ValueError where the engine has none): ``les_mix`` runs without fields under a cap that never binds
        (the type's largest finite value), so km is uncapped and ``mixing_capped`` False, and ONE ``les_hmix`` per device takes
        one backward-Euler step of every periodic line along i and then along j IN PLACE (no scratch buffers are swapped), the
        face viscosity bounded by ``kh_cap`` (default ``horizontal_mixing.KH_CAP``: a sanity bound, no stability cap; uploaded
        again where it changed); ``cap`` is then not used.  Needs U and V fields.  Without this call, and with
        ``implicit=False``, every path, launch and bit of the ensemble is unchanged."""
        if "U" not in self.fields3d or "V" not in self.fields3d:
            raise ValueError("the mixing (K24) needs the fields U and V (set_fields_batched)")
        if not self._has("les_mix"):
            raise ValueError("the engine has no les_mix (K24)")
        if vertical and self.vertical_mixing:
            raise ValueError("the mixing (K24) with vertical=True and the vertical mixing (K25) exclude each other: a step has one vertical diffusion")
        if vertical and not self.diffusion:
            raise ValueError("the mixing (K24) with vertical=True hands its viscosity to K15: it needs enable_diffusion()")
        if implicit and not self._has("les_hmix"):
            raise ValueError("the engine has no les_hmix (K26)")
        if dx is None:
            dx = self.dx if self.advection else adv.DX
        if dy is None:
            dy = self.dy if self.advection else adv.DY
        par = {"cs": mix.CS if cs is None else float(cs), "prandtl": mix.PRANDTL if prandtl is None else float(prandtl),
               "cap": mix.CAP if cap is None else float(cap), "theta_ref": mix.THETA_REF if theta_ref is None else float(theta_ref),
               "stability": bool(stability), "vertical": bool(vertical), "implicit": bool(implicit),
               "kh_cap": hmx.KH_CAP if kh_cap is None else float(kh_cap),
               "dx": numpy.array(dx, dtype=numpy.float64) if numpy.ndim(dx) else float(dx),
               "dy": numpy.array(dy, dtype=numpy.float64) if numpy.ndim(dy) else float(dy)}
        _, _, wind, scalar = mix.coefficients(1.0, par["dx"], par["dy"], par["prandtl"], n=self.n)       # (ValueError for what is not positive, or not [n])
        mix.cap(wind, scalar, par["cap"])
        hmx.bound(self.n, par["kh_cap"])
        mix.profiles(self.zf_cache, self.zh_cache, par["dx"], par["dy"], par["cs"], par["prandtl"], par["theta_ref"], n=self.n)
        self.mixing, self.mix_par = True, par
        self.mixing_k_max = self.mixing_capped = None
        self._mix_prof = self._mix_coef = self._mix_km = self._mix_kd = None
        self._hmix_huge = self._hmix_kh2 = None
        self._mix_spare = {}

    def _mix(self, dt):
        """K24 on the stepped (and advected) fields; QL (without thermo) and the profiles are then those of the mixed fields,
        unless K15 follows and does both"""
        eng, f, par = self._eng(), self.fields3d, self.mix_par
        if self.n == 0:
            return
        if "U" not in f or "V" not in f:
            raise ValueError("the mixing (K24) needs the fields U and V (set_fields_batched)")
        keys = [k for k in self.MIX_KEYS if k in f]
        # everything the profiles and the coefficients are made of; the host arrays are copied and compared every step (kilobytes)
        key = (par["cs"], par["prandtl"], par["theta_ref"]) + _f64(par["dx"], par["dy"], self.zf_cache, self.zh_cache)
        self._mix_prof = _kept(self._mix_prof, key, lambda: (key, tuple(self._upload(a) for a in mix.profiles(
            key[5], key[6], key[3], key[4], par["cs"], par["prandtl"], par["theta_ref"], n=self.n))))
        ckey = (float(dt), par["prandtl"], par["cap"]) + _f64(par["dx"], par["dy"])

        def coefficients():
            gx, gy, wind, scalar = mix.coefficients(dt, ckey[3], ckey[4], par["prandtl"], n=self.n)
            kcap = self._upload(mix.cap(wind, scalar, par["cap"]))
            up = lambda pair: tuple(self._upload(a) for a in pair)                            # noqa: E731
            return ckey, self._upload(gx), self._upload(gy), kcap, up(wind), up(scalar), float(self._host(kcap).min())
        self._mix_coef = _kept(self._mix_coef, ckey, coefficients)
        _, gx, gy, kcap, wind, scalar, lowest = self._mix_coef
        gz, bz, l2 = self._mix_prof[1]
        theta = f["THL"] if par["stability"] and "THL" in f else None
        coef = {k: wind if k in self.MIX_WINDS else scalar for k in keys}
        if par["implicit"]:
            return self._mix_implicit(keys, theta, gx, gy, gz, bz, l2, coef)
        spare = self._mix_spare
        for k in keys:
            spare[k] = self._scratch(spare.get(k), f[k], f[k])
        self._mix_km = self._scratch(self._mix_km, f["U"])
        u, v = f["U"], f["V"]                             # (the swap below leaves them in the spare buffers, unchanged)
        top = eng.les_mix({k: f[k] for k in keys}, {k: spare[k] for k in keys}, f["U"], f["V"], theta, gx, gy, gz, bz if theta is not None else None,
                          l2, kcap, self._mix_km, {k: coef[k][0] for k in keys}, {k: coef[k][1] for k in keys})
        for k in keys:
            f[k], spare[k] = spare[k], f[k]
        self.mixing_k_max = self._device_max(top)
        self.mixing_capped = self.mixing_k_max > lowest
        if self.vertical_mixing and self.mixing_capped:   # K25 mixes by the UNCAPPED viscosity: the probe again under a cap that never binds
            self._vmix_km = self._scratch(self._vmix_km, self._mix_km, self._mix_km)
            if self._vmix_huge is None:
                self._vmix_huge = self._upload(numpy.full(self.n, float(torch.finfo(eng.dtype).max)))
            eng.les_mix({}, {}, u, v, theta, gx, gy, gz, bz if theta is not None else None, l2, self._vmix_huge, self._vmix_km, {}, {}, kmax=False)
        self._mix_tail()

    def _mix_implicit(self, keys, theta, gx, gy, gz, bz, l2, coef):
        """K26 for K24's second launch: km of the flow under a cap that never binds (one les_mix without fields), then ONE
        les_hmix on every field in place"""
        eng, f, par = self._eng(), self.fields3d, self.mix_par
        self._mix_km = self._scratch(self._mix_km, f["U"])
        if self._hmix_huge is None:
            self._hmix_huge = self._upload(numpy.full(self.n, float(torch.finfo(eng.dtype).max)))
        hkey = (par["kh_cap"],)
        self._hmix_kh2 = _kept(self._hmix_kh2, hkey, lambda: (hkey, self._upload(hmx.bound(self.n, par["kh_cap"]))))
        top = eng.les_mix({}, {}, f["U"], f["V"], theta, gx, gy, gz, bz if theta is not None else None, l2, self._hmix_huge, self._mix_km, {}, {})
        eng.les_hmix({k: f[k] for k in keys}, self._mix_km, {k: coef[k][0] for k in keys}, {k: coef[k][1] for k in keys}, self._hmix_kh2[1])
        self.mixing_k_max = self._device_max(top)
        self.mixing_capped = False                        # (so K25 mixes by this km, without a second probe)
        self._mix_tail()

    def _mix_tail(self):
        """what follows the horizontal mixing of a step, explicit or implicit"""
        eng, par = self._eng(), self.mix_par
        if par["vertical"]:
            m = self._to_host(eng.slab_means({"km": self._mix_km}))["km"]
            self._mix_kd = mix.face_diffusivity(m, self.diffuse_par["k_bg"])
        self._drop_water_paths()
        self._drop_statistics()
        self._thermo_stale = True                         # thermo: K12 runs on the mixed THL and QT before their next use
        if not (self.diffusion or self.vertical_mixing):  # (else the QL field and the means follow the diffused fields: _diffuse, _vmix)
            self._follow_fields()

    def get_eddy_viscosity_batched(self):
        """the device tensor [n x itot x jtot x nL] (Sharded row blocks under a MultiDeviceEngine) of the capped eddy viscosity
        km in m2/s that K24 found in the last step; behind a step of enable_mixing(implicit=True) the UNCAPPED km by which K26
        mixed (its probe runs under a cap that never binds; ``kh_cap`` bounds the face means inside K26 and is not applied to
        this tensor); None before the first step of enable_mixing(), and of every later call of it"""
        return self._mix_km if self.mixing else None

    # -- implicit vertical mixing by each column's own eddy viscosity (K25), opt-in ----------------------------------------------
    vertical_mixing = False                            # enable_vertical_mixing(): every column mixes along k by its own km
    vmix_par = None                                    # kv_cap, k_bg, drag
    VMIX_FLUX = DIFFUSE_FLUX                           # field -> the slot of ``tend`` that holds its kinematic surface flux
    VMIX_Z0M = "z0m"                                   # the slot of ``tend`` that holds the roughness length of the drag
    _vmix_coef = None                                  # ((dt, prandtl, k_bg, kv_cap, host Rhobf, zh, zf) of the upload, device winds' and scalars' (el, eu), kb, kv2, s0)
    _vmix_drag = None                                  # ((dt, host z0m, zh, zf) of the upload, device dr)
    _vmix_km = None                                    # the uncapped eddy viscosity of the last step where K24's cap bound, device
    _vmix_huge = None                                  # device [n]: the type's largest finite value, the cap of that probe
    _vmix_speed = None                                 # device [n x itot x jtot]: the wind speed of the lowest level, K25's workspace
    _vmix_stepped = False                              # K25 has run since enable_vertical_mixing(): there is a viscosity it mixed by

    def enable_vertical_mixing(self, kv_cap=None, k_bg=None, drag=True):
        """from now on every ``evolve_model_batched`` runs ONE ``Engine.les_vmix`` per device (K25, DESIGN.md 7.3: two launches)
        after K24 and where K15 stands: one backward-Euler step of the vertical mixing of every column by ITS OWN eddy viscosity,
        the UNCAPPED km of K24 (where this step's ``mixing_capped`` is True one more ``les_mix`` without fields writes it into a
        second buffer; else K24's km is that value bit for bit), plus the background ``k_bg``, bounded by ``kv_cap``.  U and V mix
        with the winds' coefficients and, with ``drag``, feel a neutral bulk drag at the lowest level where a roughness length
        was handed over (``set_z0m_surf`` / ``Z0M_surf``; none where none was set); THL, QT and QR mix with the scalars'
        coefficients, and THL and QT take K15's surface fluxes (``WT_surf``, ``WQ_surf``).  The profiles then are K10's means of
        the mixed fields and QL follows the new QT.  The coefficients are uploaded again whenever dt, ``prandtl`` (that of
        ``enable_mixing()``), a parameter, Rhobf or the grid changed; the drag whenever z0m or dt did.  Needs ``enable_mixing()``
        first; ValueError with ``enable_diffusion()`` in either order and with ``enable_mixing(vertical=True)``: a step has
        one vertical diffusion.  ``get_vertical_viscosity_batched()`` returns the viscosity.  Without this call every path,
        launch and bit of the ensemble is unchanged."""
        if not self.mixing:
            raise ValueError("the vertical mixing (K25) mixes by the eddy viscosity of K24: it needs enable_mixing() first")
        if self.diffusion:
            raise ValueError("the vertical mixing (K25) and the diffusion (K15) exclude each other: a step has one vertical diffusion")
        if self.mix_par["vertical"]:
            raise ValueError("the vertical mixing (K25) and enable_mixing(vertical=True) exclude each other: a step has one vertical diffusion")
        if not self._has("les_vmix"):
            raise ValueError("the engine has no les_vmix (K25)")
        par = {"kv_cap": vmix.KV_CAP if kv_cap is None else float(kv_cap), "k_bg": vmix.K_BG if k_bg is None else float(k_bg),
               "drag": bool(drag)}
        vmix.background(self.n, 1, par["k_bg"], par["kv_cap"])                                 # (ValueError for what is out of range)
        self.vertical_mixing, self.vmix_par = True, par
        self._vmix_coef = self._vmix_drag = self._vmix_km = self._vmix_huge = self._vmix_speed = None
        self._vmix_stepped = False                        # (K24's km of a step before this call is no viscosity K25 mixed by)

    def _vmix(self, dt):
        """K25 on the mixed fields; QL (without thermo) and the profiles are then those of the vertically mixed fields"""
        eng, f, p, par = self._eng(), self.fields3d, self.p, self.vmix_par
        keys = [k for k in self.MIX_KEYS if k in f]
        if self.n == 0 or not keys:
            return
        # everything the coefficients are made of; the host arrays are copied and compared every step (kilobytes)
        key = (float(dt), self.mix_par["prandtl"], par["k_bg"], par["kv_cap"]) + _f64(p["Rhobf"], self.zh_cache, self.zf_cache)

        def coefficients():
            wind, scalar, s0 = vmix.coefficients(key[5], key[6], key[4], dt, key[1])
            kb, kv2 = vmix.background(self.n, wind[0].shape[-1], key[2], key[3])
            up = lambda pair: tuple(self._upload(a) for a in pair)                            # noqa: E731
            return key, up(wind), up(scalar), self._upload(kb), self._upload(kv2), self._upload(s0)
        self._vmix_coef = _kept(self._vmix_coef, key, coefficients)
        _, wind, scalar, kb, kv2, s0 = self._vmix_coef
        coef = {k: wind if k in self.MIX_WINDS else scalar for k in keys}
        flux = {k: self._upload(numpy.asarray(self.tend[slot], dtype=numpy.float64).reshape(self.n))
                for k, slot in self.VMIX_FLUX.items() if k in keys and slot in self.tend}
        drag, speed = {}, None
        if par["drag"] and self.VMIX_Z0M in self.tend:
            dkey = (float(dt),) + _f64(numpy.asarray(self.tend[self.VMIX_Z0M], dtype=numpy.float64).reshape(self.n), self.zh_cache, self.zf_cache)
            self._vmix_drag = _kept(self._vmix_drag, dkey, lambda: (dkey, self._upload(vmix.drag(
                dkey[1], dkey[3], mp.layer_thickness(dkey[2], dkey[3]), dt))))
            drag = {k: self._vmix_drag[1] for k in self.MIX_WINDS if k in keys}
            if self._vmix_speed is None or tuple(self._vmix_speed.shape) != tuple(f["U"].shape[:3]):
                self._vmix_speed = self._per_device(lambda u: torch.empty(u.shape[:3], dtype=u.dtype, device=u.device), f["U"])
            speed = self._vmix_speed
        eng.les_vmix({k: f[k] for k in keys}, self._vmix_viscosity(), {k: coef[k][0] for k in keys},
                     {k: coef[k][1] for k in keys}, kb, kv2, s0=s0, flux=flux, drag=drag,
                     u=f["U"] if drag else None, v=f["V"] if drag else None, speed=speed)
        self._vmix_stepped = True
        self._follow_fields()                             # K12 stale, QL of the mixed QT, p[U, V, THL, QT, QL] = K10's means

    def _vmix_viscosity(self):
        """what K25 mixes by in this step: K24's km where its cap did not bind, else the second buffer"""
        return self._vmix_km if self.mixing_capped else self._mix_km

    def get_vertical_viscosity_batched(self):
        """the device tensor [n x itot x jtot x nL] (Sharded row blocks under a MultiDeviceEngine) of the UNCAPPED eddy viscosity
        in m2/s by which K25 mixed in the last step: K24's own km where its cap did not bind, else the second buffer; None
        before the first step of enable_vertical_mixing(), and of an enable_mixing() behind it"""
        if not (self.vertical_mixing and self._vmix_stepped) or self._mix_km is None:
            return None
        return self._vmix_viscosity()

    # -- longwave cooling and warming by the liquid water (K18), opt-in ---------------------------------------------------------
    radiation = False                                  # enable_radiation(): the cloud water acts on THL
    radiate_par = None                                 # f0, f1, kappa: float64 [n] each
    _radiate_prof = None                               # ((dt, host kappa, Rhobf, presf, zh) of the upload, device w, c)
    _radiate_scale = None                              # device (f0, f1)
    _radiate_flux = None                               # the flux at the upper faces in the last step, device

    def enable_radiation(self, f0=None, f1=None, kappa=None):
        """from now on every ``evolve_model_batched`` runs ONE K18 launch per device (``Engine.les_radiate``) on
        THL with the current QL and the whole step's dt, after K16 / K17 / K15 and before K14 / K12: the first two terms of the
        GCSS / DYCOMS-II parametrised longwave flux cool the air at the top of a cloud and warm it at its base.  ``f0``, ``f1``
        (W/m2) and ``kappa`` (m2/kg) are scalars or one value per LES and default to those of ``radiation``.  Needs a THL
        field, more than one level, and cloud water that follows the fields: a Qsat field or ``enable_thermo()`` (ValueError
        otherwise).  Launches per step and device: ONE K18, and one K10 for the means of the new fields; with
        ``enable_thermo()`` one K12 more than without this call (K12 runs on the fields K18 reads QL of, and again on the new
        THL before the means are formed).  w and c are uploaded again only where dt, kappa, Rhobf,
        presf or the half levels changed.  ``get_radiative_flux_batched()`` returns the flux.  Without this call every path,
        launch count and result of the ensemble is unchanged."""
        if self.nL == 1:
            raise ValueError("the radiation (K18) does not take LES of one level")
        if "THL" not in self.fields3d:
            raise ValueError("the radiation (K18) needs a THL field (set_fields_batched)")
        if not (self.thermo or "Qsat" in self.fields3d):
            raise ValueError("the radiation (K18) needs the cloud water of the current fields: a Qsat field, or enable_thermo()")
        if not self._has("les_radiate"):
            raise ValueError("the engine has no les_radiate (K18)")
        par = {}
        for name, v, d in (("f0", f0, rad.F0), ("f1", f1, rad.F1), ("kappa", kappa, rad.KAPPA)):
            a = numpy.asarray(d if v is None else v, dtype=numpy.float64)
            if a.ndim > 1 or (a.ndim == 1 and a.shape != (self.n,)) or not numpy.isfinite(a).all():
                raise ValueError("the radiation (K18) needs a finite %s: a scalar or one value per LES" % name)
            par[name] = numpy.array(numpy.broadcast_to(a, (self.n,)), order="C")
        self.radiate_par = par
        self.radiation, self._radiate_prof, self._radiate_scale, self._radiate_flux = True, None, None, None

    def _radiate(self, dt):
        """K18 on the stepped THL with the QL of the stepped fields; the profiles are then the means of the new fields"""
        eng, f, p, par = self._eng(), self.fields3d, self.p, self.radiate_par
        if self.n == 0:
            return
        if "THL" not in f or not (self.thermo or "Qsat" in f):
            raise ValueError("the radiation (K18) needs a THL field and a Qsat field or enable_thermo()")
        self._ensure_ql()                                 # (thermo: K12 where stale)
        # everything the profiles are made of; the host arrays are copied and compared every step (kilobytes)
        key = (float(dt),) + _f64(par["kappa"], p["Rhobf"], p["presf"], self.zh_cache)
        self._radiate_prof = _kept(self._radiate_prof, key, lambda: (
            key, [self._upload(a) for a in rad.profiles(key[2], key[4], key[3], dt, key[1])]))
        if self._radiate_scale is None:
            self._radiate_scale = (self._upload(par["f0"]), self._upload(par["f1"]))
        self._radiate_flux = self._scratch(self._radiate_flux, f["THL"])
        eng.les_radiate(f["QL"], f["THL"], *self._radiate_prof[1], *self._radiate_scale, flux=self._radiate_flux)
        self._follow_fields()                             # K12 stale, QL of the QT field, p[U, V, THL, QT, QL] = K10's means

    def get_radiative_flux_batched(self):
        """the device tensor [n x itot x jtot x nL] (Sharded row blocks under a MultiDeviceEngine) of the net upward longwave
        flux in W/m2 at the UPPER faces of the cells that the last step's K18 launch found; None before the first step of
        enable_radiation()"""
        return self._radiate_flux if self.radiation else None

    # -- local cloud-water forcing of QT (K19: qt_forcing 'local' | 'strong'), opt-in -------------------------------------------
    qt_forcing_kind = None                             # enable_qt_forcing(): "local" or "strong"
    _qt_counts = None                                  # device int32 [n x nL]: the wet cells per plane of the last K19 launch

    def enable_qt_forcing(self, kind):
        """from now on every ``evolve_model_batched`` runs ONE K19 launch per device (``Engine.les_qt_local``)
        directly after the step and before K16 / K17 / K15 / K18 / K14 / K12 (the forcings first, then the physics): per level
        the QT field takes ``qt_forcing.increments(kind, ...)`` -- ``"local"``: the cloud-water forcing ``set_tendency_QL`` /
        ``QL`` handed over times dt, ``"strong"``: the profile of ``set_ref_profile_QL`` / ``QLp`` minus the slab mean of QL --
        times N / c in its wet cells and gives it back in the dry ones, so the cloud water moves towards the GCM's and the slab
        mean of QT does not.  QTM is the slab mean of the stepped QT (the cached means, else one K10 launch).  Needs a QT field
        and cloud water that follows it: a Qsat field or ``enable_thermo()`` (ValueError otherwise).  No launch before the
        forcing the kind reads was handed over.  ``get_qt_forcing_counts_batched()`` returns the wet cells per plane.  Calling
        it again with the same kind changes nothing.  Without this call every path of the ensemble is unchanged."""
        from . import qt_forcing
        if kind not in qt_forcing.KINDS:
            raise ValueError("the local QT forcing (K19) is one of %s, got %r" % (qt_forcing.KINDS, kind))
        if "QT" not in self.fields3d:
            raise ValueError("the local QT forcing (K19) needs a QT field (set_fields_batched)")
        if not (self.thermo or "Qsat" in self.fields3d):
            raise ValueError("the local QT forcing (K19) needs the cloud water of the current QT: a Qsat field, or enable_thermo()")
        if not self._has("les_qt_local"):
            raise ValueError("the engine has no les_qt_local (K19)")
        if kind != self.qt_forcing_kind:
            self.qt_forcing_kind, self._qt_counts = kind, None

    def _qt_local(self, dt):
        """K19 on the stepped QT with the QL and the slab means of the stepped fields; QL and the profiles then follow the new
        QT, here or in the stages behind it"""
        from . import qt_forcing
        eng, f, p, kind = self._eng(), self.fields3d, self.p, self.qt_forcing_kind
        if self.n == 0 or {"local": "QL", "strong": "QL_ref"}[kind] not in self.tend:
            return
        if "QT" not in f or not (self.thermo or "Qsat" in f):
            raise ValueError("the local QT forcing (K19) needs a QT field and a Qsat field or enable_thermo()")
        self._ensure_ql()                                 # (thermo: K12 where stale)
        means = self._slab_means()                        # cached by the step (K11, or K10 behind the torch path), else one K10 launch
        a = qt_forcing.increments(kind, self.tend.get("QL"), self.tend.get("QL_ref"), p["QL"], dt)
        self._qt_counts = eng.les_qt_local(f["QT"], f["QL"], self._upload(a), self._upload(means["QT"]), count=self._qt_counts)
        self._drop_water_paths()
        self._drop_statistics()
        self._thermo_stale, self._means = True, None      # thermo: K12 runs on the new QT before its next use
        if not (self.advection or self.diffusion):        # (else the QL field and the means follow the advected / diffused fields)
            self._follow_fields()

    def get_qt_forcing_counts_batched(self):
        """the device int32 tensor [n x nL] (Sharded row blocks under a MultiDeviceEngine) of the wet cells per plane that the
        last step's K19 launch counted (0 on levels it left alone); None before the first such launch"""
        return self._qt_counts if self.qt_forcing_kind else None

    def _saturate(self):
        """the QL field = max(QT - Qsat, 0), in place: two torch operations on each device's stream"""
        def saturate(ql, qt, qs):
            torch.sub(qt, qs, out=ql)
            return ql.clamp_min_(0.0)
        self._per_device(saturate, self.fields3d["QL"], self.fields3d["QT"], self.fields3d["Qsat"])

    def _follow_fields(self):
        """QL = max(QT - Qsat, 0) of the QT field as it is now (without thermo) and p[U, V, THL, QT, QL] = K10's means"""
        f = self.fields3d
        self._drop_water_paths()
        self._drop_statistics()
        self._thermo_stale = True                         # thermo: K12 runs on the new THL and QT before their next use
        if not self.thermo and ("QL" in f or ("QT" in f and "Qsat" in f)):
            self._ensure_ql()
            self._saturate()
        self._means = None
        self._slab_means()

    @classmethod
    def for_gcm(cls, gcm, grid_indices, nL=160, seed=0, itot=8, jtot=8, engine=None):
        ens = super().for_gcm(gcm, grid_indices, nL, seed)
        ens.itot, ens.jtot, ens.engine = int(itot), int(jtot), engine
        return ens

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self.n))]
        if self._rows[i] is None:
            self._rows[i] = _DeviceLESRow(self, i)
        return self._rows[i]

    # -- plumbing: one engine or one engine per device ------------------------------------------------------------------
    def _eng(self):
        if self.engine is None:
            from . import spcpl                           # (here: spcpl may import models)
            self.engine = spcpl.get_engine()
        return self.engine

    def _engines(self):
        """the engine, or the engines of a MultiDeviceEngine: one per device"""
        eng = self._eng()
        return getattr(eng, "engines", [eng])

    def _has(self, method):
        """every engine has the kernel ``method``"""
        return all(callable(getattr(e, method, None)) for e in self._engines())

    def _per_device(self, fn, *xs):
        """``fn(x, ...)`` on the engine's stream; with Sharded arguments on every device's block, on that engine's stream"""
        eng = self._eng()
        ex = next((x for x in xs if isinstance(x, Sharded) and x.bounds is not None), None)
        if ex is None:
            with eng.on_stream():
                return fn(*xs)
        parts = []
        for d, e in enumerate(eng.engines):
            with e.on_stream():
                parts.append(fn(*[(x.parts[d] if isinstance(x, Sharded) else x) for x in xs]))
        return Sharded(parts, ex.bounds)

    def _upload(self, a, dtype=None):
        eng = self._eng()
        with eng.on_stream():
            return eng.to_devices(numpy.ascontiguousarray(a), rows=self.n, dtype=dtype or eng.dtype)

    @staticmethod
    def _host(t):
        return t.to_host() if isinstance(t, Sharded) else t.cpu().numpy()

    def _to_host(self, dev, dtype=numpy.float64):
        """a dict of device tensors as host arrays (float64, or as they are: ``dtype=None``), copied in the dict's order"""
        with self._eng().on_stream():
            return {k: numpy.asarray(self._host(v), dtype=dtype) for k, v in dev.items()}

    def _scratch(self, buf, like, field=None):
        """``buf`` where a launch can write it: there is one, it is not ``field`` (the tensor the launch reads) and it has the
        shape of ``like``; else a new uninitialised tensor like ``like``"""
        if buf is None or buf is field or tuple(buf.shape) != tuple(like.shape):
            return self._per_device(torch.empty_like, like)
        return buf

    # -- 3-D fields --------------------------------------------------------------------------------------------------
    def attach_fields(self, fields):
        for k, v in fields.items():
            self.set_fields_batched(k, v)

    def get_fields_batched(self, name):
        """the device tensor itself (no copy): what K6 and K10 work on"""
        if name == "QL" or (self.thermo and name == "Qsat"):
            self._ensure_ql()
        return self.fields3d[name]

    def set_fields_batched(self, name, values):
        """a device tensor (Sharded) of the engine's is kept as it is; a NumPy array is uploaded once"""
        values = getattr(values, "number", values)
        dt = self._eng().dtype
        if isinstance(values, (torch.Tensor, Sharded)):
            conv = lambda t: t if t.dtype == dt else t.to(dt)                              # noqa: E731
            values = self._per_device(conv, values)
        else:
            values = self._upload(numpy.asarray(values))
        shape = tuple(values.shape)
        if len(shape) != 4 or shape[0] != self.n or shape[3] != self.nL:
            raise ValueError("field %s must be [%d x itot x jtot x %d], got %s" % (name, self.n, self.nL, shape))
        self.itot, self.jtot = int(shape[1]), int(shape[2])
        self.fields3d[name] = values
        self._means = None
        self._drop_water_paths()
        self._drop_statistics()
        self._thermo_stale = True                       # (K12 writes Qsat and QL in place, not through here)

    def set_field_row(self, i, name, values):
        raise NotImplementedError("a DeviceLESEnsemble takes whole fields: set_fields_batched")

    def _ensure_ql(self):
        if self.thermo:
            return self._ensure_thermo()
        f = self.fields3d
        if "QL" not in f:
            f["QL"] = self._per_device(lambda qt, qs: torch.clamp_min(qt - qs, 0.0), f["QT"], f["Qsat"])
            self._means = None

    def _slab_means(self):
        """host [n x nL] slab means of every field in MEAN_KEYS: one launch, cached until a field changes"""
        if self.thermo:
            self._ensure_thermo()
        if self._means is None:
            if "QT" in self.fields3d and "Qsat" in self.fields3d:
                self._ensure_ql()
            own = self.thermo and self._thermo_means is not None      # the mean of QL came with K12's launch
            self._means = self._to_host(self._eng().slab_means(
                {k: self.fields3d[k] for k in self.MEAN_KEYS if k in self.fields3d and not (own and k == "QL")}))
            if own:
                self._means["QL"] = self._thermo_means["QL"]
            self.p.update(self._means)
        return self._means

    # -- second moments per level (K20) ---------------------------------------------------------------------------------------
    _stats_w = None                                    # ((the substep's seconds, host Rhobf) W was made of, W: the tensor handed to K20, or None)

    def _drop_statistics(self):
        self._stats, self._stats_host, self._stats_w = None, {}, None

    def _drop_w_statistics(self):
        """what depends on W alone: its moments and the pairs that hold it; the moments of the other fields stay cached"""
        from . import statistics as st
        holds = lambda key: st.FACE in (key if isinstance(key, tuple) else (key,))                # noqa: E731
        for d in (self._stats or {}).values():
            for key in [key for key in d if holds(key)]:
                del d[key]
        self._stats_host = {kk: a for kk, a in self._stats_host.items() if not holds(kk[1])}

    def _statistics_fields(self):
        """name -> device field of every field of ``statistics.FIELDS`` the ensemble holds now (QL after K12 where thermo is
        enabled and stale; W from the last step of enable_advection(vertical=True))"""
        from . import statistics as st
        f = self.fields3d
        if self.thermo or "QL" in f or ("QT" in f and "Qsat" in f):
            self._ensure_ql()
        have = {}
        for k in st.FIELDS:
            if k == st.FACE:
                # W is a torch expression of K17's mass flux (new only in a step, which drops everything), the substep's seconds
                # and p["Rhobf"]: keyed as get_water_paths_batched keys its weights
                key = (self._vadvect_dt,) + (_f64(self.p["Rhobf"]) if self.advect_vertical else ())
                old = self._stats_w
                self._stats_w = _kept(old, key, lambda: (key, self.get_vertical_wind_batched()))
                if self._stats_w is not old:
                    self._drop_w_statistics()                     # moments of another W (p["Rhobf"] was set) are stale
                if self._stats_w[1] is not None:
                    have[k] = self._stats_w[1]
            elif k in f:
                have[k] = f[k]
        return have

    def get_statistics_batched(self, names=None, pairs=None):
        """``{"mean": {name: t}, "var": {...}, "std": {...}, "cov": {(a, b): t}}`` of device tensors [n x nL] (Sharded row blocks
        under a MultiDeviceEngine): per LES and level the mean, the variance and the standard deviation over the plane of the
        fields ``names`` (default: those of ``statistics.FIELDS`` the ensemble holds; W is ``get_vertical_wind_batched()``
        brought to the cell centres) and the covariances of ``pairs`` (default: those of ``statistics.PAIRS`` whose two fields
        are present), by NumPy's rule bit for bit (include/spc.h).  A name or a pair whose field the ensemble does not hold is
        left out; KeyError where no name is left.  What is not cached goes through ONE launch per device; the results are
        cached until a field changes."""
        from . import statistics as st
        if not self._has("les_moments"):
            raise ValueError("the engine has no les_moments (K20)")
        names = list(st.FIELDS if names is None else names)
        unknown = [k for k in names if k not in st.FIELDS]
        if unknown:
            raise KeyError("no statistics of %s (there are %s)" % (unknown, list(st.FIELDS)))
        fields = self._statistics_fields()                # (K12 where stale: it drops what is cached)
        if self._stats is None:
            self._stats = {"mean": {}, "var": {}, "std": {}, "cov": {}}
        have = [k for k in names if k in fields]
        if not have:
            raise KeyError("the ensemble holds no field for %s" % (names,))
        pairs = [tuple(p) for p in (st.PAIRS if pairs is None else pairs)]
        pairs = [p for p in pairs if p[0] in fields and p[1] in fields]
        cache = self._stats
        need_pairs = [p for p in pairs if p not in cache["cov"]]
        need = [k for k in have if k not in cache["mean"]]
        need += [k for p in need_pairs for k in p if k not in need and k not in cache["mean"]]
        launch = need + [k for p in need_pairs for k in p if k not in need]
        if launch:
            launch = [k for k in st.FIELDS if k in launch]              # one order whatever was asked for
            todo = bool(need)
            res = self._eng().les_moments({k: fields[k] for k in launch}, need_pairs, mean=todo, var=todo, std=todo,
                                          face=st.FACE if st.FACE in launch else None)
            for kind, d in res.items():                               # (a cached field that only a new pair needed keeps its tensors)
                for key, t in d.items():
                    cache[kind].setdefault(key, t)
        return {"mean": {k: cache["mean"][k] for k in have}, "var": {k: cache["var"][k] for k in have},
                "std": {k: cache["std"][k] for k in have}, "cov": {p: cache["cov"][p] for p in pairs}}

    def get_statistics(self, names=None, pairs=None):
        """``get_statistics_batched`` as host float64 arrays [n x nL], plus ``"TKE"`` (``statistics.tke`` of the variances) where
        U and V are among the names"""
        from . import statistics as st
        dev = self.get_statistics_batched(names, pairs)
        host = {}
        with self._eng().on_stream():
            for kind, d in dev.items():
                host[kind] = {}
                for key, t in d.items():
                    if (kind, key) not in self._stats_host:
                        self._stats_host[(kind, key)] = numpy.asarray(self._host(t), dtype=numpy.float64)
                    host[kind][key] = self._stats_host[(kind, key)]
        if "U" in host["var"] and "V" in host["var"]:
            host["TKE"] = st.tke(host["var"])
        return host

    # -- column water paths (K13) ------------------------------------------------------------------------------------------
    def _drop_water_paths(self):
        self._wp, self._wp_host = None, {}

    def water_path_weights(self):
        """host float64 [n x nL]: Rhobf * dz, dz the thickness of the LES layers from the half levels zh (the lower faces):
        dz[k] = zh[k + 1] - zh[k]; the top layer has no upper half level and takes the thickness of the layer below it,
        dz[nL - 1] = dz[nL - 2]; an LES of one level takes twice the distance of its full level from its half level"""
        zh = numpy.asarray(self.zh_cache, dtype=numpy.float64)
        if self.nL > 1:
            dz = numpy.diff(zh, axis=-1)
            dz = numpy.concatenate([dz, dz[..., -1:]], axis=-1)
        else:
            dz = 2.0 * (numpy.asarray(self.zf_cache, dtype=numpy.float64) - zh)
        return numpy.asarray(self.p["Rhobf"], dtype=numpy.float64) * dz

    def get_water_paths_batched(self, names=("LWP", "TWP", "RWP"), cloud_cover=False):
        """dict name -> device tensor [n x itot x jtot] (Sharded row blocks under a MultiDeviceEngine) of the column water
        paths ``numpy.add.reduce(field * w[:, None, None, :], axis=3)``, w = ``water_path_weights()`` in the engine's dtype:
        LWP of the QL field (after K12 where thermo is enabled and stale), TWP of QT, RWP of an attached QR field.  A name
        whose field the ensemble does not hold is left out; KeyError where none is left.  ``cloud_cover`` adds ``"top"``
        (int32: the highest cloudy level of QL per column, -1 for none) and ``"cover"`` ([n]: the fraction of cloudy
        columns).  What is not cached goes through ONE launch per device; the results are cached until a field changes."""
        unknown = [k for k in names if k not in self.WATER_PATHS]
        if unknown:
            raise KeyError("no water path %s (there are %s)" % (unknown, sorted(self.WATER_PATHS)))
        f = self.fields3d
        if ("LWP" in names or cloud_cover) and (self.thermo or "QL" in f or ("QT" in f and "Qsat" in f)):
            self._ensure_ql()
        have = [k for k in names if self.WATER_PATHS[k] in f]
        if not have or (cloud_cover and "QL" not in f):
            raise KeyError("the ensemble holds no field for %s" % ("the cloud cover (QL)" if have else list(names)))
        w = numpy.ascontiguousarray(self.water_path_weights())
        old = self._wp_w
        self._wp_w = _kept(old, w, lambda: (w, self._upload(w)))    # .astype(T) of the float64 product
        if self._wp_w is not old:
            self._drop_water_paths()                                # results of other weights (p["Rhobf"] was set) are stale
        cache = self._wp if self._wp is not None else {}
        need = [k for k in have if k not in cache]
        cloud = cloud_cover and "cover" not in cache
        out = None
        if cloud and "LWP" not in need:                             # the cloud pass walks QL: LWP comes with it, ...
            need.insert(0, "LWP")
            if "LWP" in cache:                                      # ... again into its cached tensor where there is one
                out = {"LWP": cache["LWP"]}
        if need:
            cache.update(self._eng().les_water_paths({k: f[self.WATER_PATHS[k]] for k in need}, self._wp_w[1],
                                                     cloud="LWP" if cloud else None, out=out, top=cloud, cover=cloud))
            self._wp = cache
            for k in need:
                self._wp_host.pop(k, None)
        return {k: cache[k] for k in have + (["top", "cover"] if cloud_cover else [])}

    def _water_path_host(self, name):
        t = self.get_water_paths_batched((name,))[name]           # (cached; it drops the host copies where p["Rhobf"] changed the weights)
        if name not in self._wp_host:
            with self._eng().on_stream():
                self._wp_host[name] = numpy.asarray(self._host(t))
        return self._wp_host[name]

    def get_water_path_means(self, names=("LWP", "TWP", "RWP")):
        """host dict name -> [n]: ``wp[l].mean()`` of every LES, bit for bit: K10's slab means of the 2-D result viewed as
        [n x itot x jtot x 1] (a one-level field is one contiguous run per LES, which NumPy sums pairwise)"""
        wp = self.get_water_paths_batched(names)
        dev = self._eng().slab_means({k: self._per_device(lambda t: t.unsqueeze(-1), v) for k, v in wp.items()})
        return {k: v[:, 0] for k, v in self._to_host(dev, dtype=None).items()}

    # -- batched protocol ----------------------------------------------------------------------------------------------
    @_timed
    def get_profiles_batched(self, keys, out):
        if self.thermo:
            self._ensure_thermo()                         # p["T"] and p["QL"] of the fields as they are now
        means = self._slab_means() if any(k in self.MEAN_KEYS and k in self.fields3d for k in keys) else {}
        for k in keys:
            numpy.copyto(out[k], means[k] if k in means else self.p[k])

    def _refresh_profile(self, key):
        """p[key] of the fields as they are now, by the rule of get_profiles_batched (the rows' getters read p: a nudge or
        set_fields_batched leaves the means of the old fields there)"""
        if self.thermo:
            self._ensure_thermo()
        if key in self.MEAN_KEYS and key in self.fields3d:
            self._slab_means()

    @_timed
    def get_cloudfraction_batched(self, indices, out):
        self._ensure_ql()
        eng = self._eng()
        idx = self._upload(numpy.asarray(indices, dtype=numpy.int32), dtype=torch.int32)
        A = eng.slab_cloud_fraction(self.fields3d["QL"], idx)
        with eng.on_stream():
            numpy.copyto(out, self._host(A))

    def _fused_step(self, dt):
        """the step of the fields, the QL field and the slab means of the new fields from ONE launch per device (K11,
        ``Engine.les_advance``); False -- nothing done -- where the engine has no such method, the LES have one level (numpy
        reduces a one-level plane pairwise: K10's own kernel), nothing is stepped or saturated, or ``fused_advance`` is off"""
        eng, f = self._eng(), self.fields3d
        keys = [k for k in self.STEP_KEYS if k in f]
        sat = "QT" in f and "Qsat" in f and not self.thermo          # (thermo: QL is K12's, after the step)
        if not (self.fused_advance and self.nL > 1 and self.n > 0 and keys and (sat or any(k in self.tend for k in keys))):
            return False
        if max(int(part.shape[0]) for part in getattr(f[keys[0]], "parts", [f[keys[0]]])) < self.FUSED_MIN_LES:
            return False                                  # a launch of few LES is a latency chain: the torch path is faster
        if ("QL" in f and not sat and not self.thermo) or not self._has("les_advance"):
            return False
        tend = {k: self._upload(self.tend[k]) for k in keys if k in self.tend}
        if sat and "QL" not in f:
            f["QL"] = self._per_device(torch.empty_like, f["QT"])          # written whole by the launch
        dev = eng.les_advance({k: f[k] for k in keys}, tend, dt, qsat=f["Qsat"] if sat else None, sat="QT" if sat else None,
                              ql=f["QL"] if sat else None)
        self._means = self._to_host(dev)
        self.p.update(self._means)
        self._thermo_stale = True
        return True

    @_timed
    def evolve_model_batched(self, t):
        dt = float(t) - self.model_time
        if dt <= 0:
            return
        f, p = self.fields3d, self.p
        self._drop_water_paths()
        self._drop_statistics()
        if self._fused_step(dt):
            pass                                          # K11: fields, QL and p[U, V, THL, QT, QL] from one launch
        else:
            for key in self.STEP_KEYS:
                if key in self.tend and key in f:
                    def step(field, tend):
                        inc = tend * dt                   # two separate ops: nothing contracts to an fma
                        return field.add_(inc[:, None, None, :])
                    self._per_device(step, f[key], self._upload(self.tend[key]))
            self._thermo_stale = True
            # (with diffusion or advection the QL field and the means follow the diffused / advected fields; K19 reads those of
            # the stepped fields)
            if not (self.diffusion or self.advection) or self.qt_forcing_kind:
                self._follow_fields()                     # p[U, V, THL, QT, QL] = the slab means of the new fields
        if "PS" in self.tend:
            p["PS"] = p["PS"] + dt * self.tend["PS"]
        if self.qt_forcing_kind:
            self._qt_local(dt)                            # one K19 launch: QT moved between the wet and the dry cells of every plane; p[...]
        if self.advection:
            self._advect(dt)                              # 1 + n_sub K16 launches: U, V, THL, QT, QR carried along i and j; p[...]
                                                          # (vertical: a K17 probe and a K17 launch behind every K16 substep)
        if self.mixing:
            self._mix(dt)                                 # one K24 call, two launches: km of the flow; U, V, THL, QT, QR mixed along i and j; p[...]
        if self.diffusion:
            self._diffuse(dt)                             # one K15 launch: U, V, THL, QT mixed along k, the surface fluxes; p[...]
        if self.vertical_mixing:
            self._vmix(dt)                                # one K25 call, two launches: U, V, THL, QT, QR mixed along k by each column's km; p[...]
        if self.radiation:
            self._radiate(dt)                             # one K18 launch: THL cooled at the cloud tops, warmed at the bases; p[...]
        if self.micro:
            self._microphysics(dt)                        # one K14 launch: QT, THL, QR, rain2d; p[QT, THL, QR, Rain(, QL_ice)]
        if self.thermo:
            self._ensure_thermo()                         # one K12 launch: the Qsat and QL fields, p["QL"] and p["T"]
        p["QL_ice"] = numpy.minimum(p["QL_ice"], p["QL"])
        if not (self.thermo and self._thermo_means is not None):
            p["T"] = p["THL"] * (p["presf"] / 1e5) ** (287.04 / 1004.) + 2.53e6 * p["QL"] / 1004.
        if not self.micro:
            p["Rain"] = p["Rain"] + 1e-6 * dt
        self.model_time = float(t)
