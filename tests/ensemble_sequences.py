"""Random operation sequences of models.DeviceLESEnsemble (the class lives in sp_coupler_amd/device_les.py; the name in models
is the same object) against its eager NumPy twin (tests/les_hmix_ref.py: HostHmixLESEnsemble / HostThermoHmixLESEnsemble, the
top of the chain of twins; with implicit=False their step is that of tests/les_vmix_ref.py): the body of tests/test_ensemble_sequences_cpu.py (on oracle-backed engines) and
tests/test_ensemble_sequences_gpu.py (on the card).

The device ensemble is a lazy, cached state machine (_thermo_stale, _means, _wp / _wp_host / _wp_w, _thermo_means, the profile
uploads keyed on their inputs, the ping-pong buffers of K14 / K16 / K17 / K22, the fused K11 step, K19's count buffer and its wait
for the forcing, K20's partial cache _stats / _stats_host / _stats_w, K21's profiles and pressure, K22's lid flux summed over the
substeps, K24's profiles, coefficients, ping-pong buffers and viscosity, K25's coefficients, drag and second viscosity buffer
with the switch between the two on ``mixing_capped``, K26's path ``_mix_implicit`` behind enable_mixing(implicit=True): the probe under
``_hmix_huge``, ONE in-place ``les_hmix`` under the bound ``_hmix_kh2`` keyed on ``kh_cap``, ``mixing_capped`` False and the
shared ``_mix_tail``, and the switch between that path and K24's ping-pong buffers at every later enable_mixing); the twin computes
everything eagerly from its fields.
``generate`` draws a list of operations that are all valid in
the state they meet, mutations and sparse observations mixed; ``replay`` applies the list to both and compares every observation
bit for bit (gpu_util.assert_bits), with two exceptions: W within the bound of les_vadvect_ref.check_w (a torch expression), and
the moments that hold W (its mean, variance and standard deviation, its covariances, TKE with it) bit for bit against NumPy's
moments (the oracle of K20) of the device's OWN get_vertical_wind_batched() read at that operation, the rule of
les_moments_ref.ensemble_run: the twin's W differs in its last bits.

The modes: the six of the first version (thermo, diffuse, micro, advect, vertical, radiate), then "qt" (K19; the kind local /
strong comes from ``params``), "buoyancy" (K21; needs vertical), "conservative" (K22; needs vertical), "order2" (K23; needs
conservative; the limiter comes from ``params``) and "stats" (K20: statistics observations are drawn only with it), then "mix"
(K24, enable_mixing), "vmix" (K25, enable_vertical_mixing; needs mix, excludes diffuse) and "kmix" (enable_mixing once more with
vertical=True: K24's slab-mean viscosity in K15; needs mix and diffuse, excludes vmix); the cap, the stability switch, the
spacings of K24 and the drag of K25 come from ``params``; last "imix" (K26; needs mix): the first enable_mixing of the sequence, at
``build`` or at a late ("enable", "mix"), passes implicit=True and the ``kh_cap`` of ``params``; every later call (a late kmix, a
``remix``) passes the switch as it stands, and the mutation ("implicit", flag, kh_cap) calls enable_mixing with the switch flipped
or kept and a drawn bound.  Whether K26 is on now is "imix" in the set of enabled modes.  Every newer set of modes stands at the
END of MODES: the bit mask that seeds the generator, and so every sequence of the 48 old subsets, of the 55 combinations of
ELEVEN and of the 14 with the mixing modes, is what it was (tests/test_ensemble_sequences_cpu.py holds the three digests).

Conditions, asserted here and not left to the callers:
  * every sequence has its full length, runs to its end on both sides and ends with a full record: every profile (batched,
    raw and through every row), every field, the water paths with the cloud cover and their means, rain2d, the flux, W, the
    Courant numbers, the counts, the lid flux, the pressure, the wind change and the statistics (whole and through every row) of
    what is enabled;
  * every sequence holds a step that no read precedes and two consecutive mutations;
  * every mode a sequence enables launches its engine method at least once on the device side (``check_launched``); K19 launches
    only behind the ``qt_forcings`` that every "qt" sequence holds between two steps, and never before it;
  * a "vmix" sequence with the drag holds a ``z0m`` between two steps; in a step with K25 ``les_mix`` is called twice exactly where
    the step's ``mixing_capped`` is True, else once; between ``les_mix`` and K15 stands one ``slab_means`` (of km) with "kmix", else nothing;
  * a step with K26 on launches exactly one ``les_mix`` per engine that holds rows, K25 or not, one ``les_hmix`` directly behind it
    (it stands between ``les_mix`` and K15, in front of the ``slab_means``) and leaves ``mixing_capped`` False; a step with K26 off
    launches no ``les_hmix``; an "imix" sequence launches ``les_hmix`` at least once;
  * a ``refused`` call raises ValueError on both sides, and what follows it shows that it changed nothing;
  * over a set of cases every kind of operation occurs that their modes allow (``check_kinds``).
Properties of the device ensemble (and of the twin, where it has the method) that need no twin:
  (a) a row getter of key k returns row i of what get_profiles_batched((k,)) returns at that moment: checked at every ``row``
      operation, the row getter FIRST (so it has to refresh p itself), and for every row and key at the final record; a row's
      get_statistics returns row i of the ensemble's get_statistics: at every ``row_stats`` and for every row at the record;
  (b) reading anything twice in a row gives the same bits and launches nothing the second time: checked at every observation.
      Two readers hold no cache of their own and launch their own reduction every time, and only that: the cloud fraction
      (slab_cloud_fraction) and the water path means (slab_means of the cached paths);
  (c) statistics that were read since the last mutation launch nothing (K20's cache is partial: what is new goes through a
      launch, what is cached does not), and a new p["Rhobf"] alone costs only the moments that hold W."""
import itertools

import numpy

from sp_coupler_amd import diffusion as df
from sp_coupler_amd import horizontal_mixing as hmx
from sp_coupler_amd import models, spcpl
from sp_coupler_amd import qt_forcing as qf
from sp_coupler_amd import radiation as rad
from sp_coupler_amd import statistics as st
from tests import les_diffuse_ref as ldr
from tests import les_hmix_ref as lhr
from tests import les_moments_ref as lmo
from tests import les_vadvect_ref as lvr
from tests import les_vmix_ref as lvm
from tests.gpu_util import assert_bits
from tests.les_harness import host_of, twin_kw
from tests.test_vnudge import make_les_fields

OLD_MODES = ("thermo", "diffuse", "micro", "advect", "vertical", "radiate")
NEW_MODES = ("qt", "buoyancy", "conservative", "order2", "stats")
MIX_MODES = ("mix", "vmix", "kmix")
ELEVEN = OLD_MODES + NEW_MODES                                    # everything but the mixing: what "all modes" meant before K24
IMIX = "imix"                                                     # K26: the first enable_mixing of the sequence passes implicit=True
MODES = ELEVEN + MIX_MODES + (IMIX,)
# may be enabled mid-sequence (vertical, conservative and order2 come with advect; vmix and kmix behind mix, kmix behind diffuse)
LATE = ("diffuse", "micro", "advect", "radiate", "qt", "buoyancy") + MIX_MODES
AFTER = {"buoyancy": ("advect",), "vmix": ("mix",), "kmix": ("mix", "diffuse")}      # a late enable waits for the late enables of these
WITH_ADVECT = ("vertical", "conservative", "order2")
METHOD = {"thermo": "les_thermo", "diffuse": "les_diffuse", "micro": "les_microphysics", "advect": "les_advect",
          "vertical": "les_vadvect", "radiate": "les_radiate", "qt": "les_qt_local", "buoyancy": "les_buoyancy",
          "conservative": "les_transport", "order2": "les_transport2", "stats": "les_moments", "mix": "les_mix", "vmix": "les_vmix",
          "kmix": "les_mix", IMIX: "les_hmix"}
COUNTED = ("slab_means", "slab_cloud_fraction", "variability_nudge", "les_advance", "les_thermo", "les_water_paths", "les_microphysics",
           "les_diffuse", "les_advect", "les_vadvect", "les_radiate", "les_moments", "les_qt_local", "les_buoyancy", "les_transport",
           "les_transport2", "les_mix", "les_vmix", "les_hmix")
MUTATIONS = ("step", "step0", "row_step", "nudge", "forcings", "set_field", "presf", "rhobf", "enable", "qt_forcings", "qt_kind", "readvect",
             "remix", "revmix", "z0m", "set_wind", "refused", "implicit")
OBSERVATIONS = ("profiles", "row", "field", "wp", "wp_means", "row_wp", "cloudfrac", "flux", "w", "courant", "counts", "lid", "pressure",
                "stats", "row_stats", "viscosity")
KINDS = MUTATIONS + OBSERVATIONS + ("record",)
NEEDS = {"qt_forcings": "qt", "qt_kind": "qt", "readvect": "buoyancy", "counts": "qt", "lid": "conservative", "pressure": "buoyancy",
         "stats": "stats", "row_stats": "stats", "remix": "mix", "revmix": "vmix", "z0m": "vmix", "set_wind": "mix", "refused": "mix",
         "viscosity": "mix", "implicit": IMIX}                                   # the mode without which a kind of operation is never drawn
RELAUNCH = {"cloudfrac": {"slab_cloud_fraction"}, "wp_means": {"slab_means"}, "record": {"slab_means"}}      # property (b)
PROFILE_KEYS = ("U", "V", "THL", "QT", "QL", "T", "QL_ice", "QR", "presf", "Rhobf", "Rain", "PS")
ROW_GETTERS = {"get_profile_U": "U", "get_profile_V": "V", "get_profile_THL": "THL", "get_profile_QT": "QT", "get_profile_QL": "QL",
               "get_profile_QL_ice": "QL_ice", "get_profile_QR": "QR", "get_profile_T": "T", "get_rain": "Rain", "get_presf": "presf"}
DTS = (300.0, 450.0, 900.0, 900.0)
ITOT, JTOT, NL, NG = 4, 5, 20, 19
LENGTH = 14
LIMITERS = ("mc", "none")
ALWAYS = ("U", "V", "THL", "QT", "QL")                            # the fields of statistics.FIELDS every ensemble of ``build`` holds
# the gravity wave of K21 and the spacings and Courant limits of ``enable``: the most wave substeps a step of DTS asks for is
# ceil(30 * 900 / (0.3 * 24000)) = 4, far below advection.MAX_SUBSTEPS (tests/test_ensemble_sequences_cpu.py checks every case)
LATE_WAVE_SPEED = 24.0
READVECT = dict(dx=0.8 * lvr.DX, cfl=0.3)
DEFAULT = {"kind": "local", "limiter": "mc", "cap": None, "stability": True, "drag": True, "dx": None, "kh_cap": None}
# K24 and K25.  The spacings of enable_mixing: None (those of the advection at the moment of the call, else advection.DX: with the
# 200 m of the latter the cap binds in every step of DTS, with the 30 km of ``enable`` it does not), 250 m (binds) and 20 km (does
# not); the caps of ``remix`` lie on both sides of either (tests/test_ensemble_sequences_cpu.py asserts that both occur)
MIX_DX = (None, 250.0, 20000.0)
MIX_CAPS = (None, 0.25)
REMIX_CAPS = (1e-3, 0.1, 1.0)
REMIX_PRANDTL = (0.5, 0.8)
REVMIX = dict(k_bg=(0.05, 0.3), kv_cap=(50.0, 400.0))
REFUSED = ("diffusion", "kmix", "vmix")
# K26.  The bounds of the face viscosity: None (horizontal_mixing.KH_CAP, 1000 m2/s), 10 m2/s and 1e5 m2/s.  The twin's largest
# viscosity of a step is 3 to 121 m2/s at the 250 m spacing and at the default spacings without advection and up to about 2000 m2/s
# at 20 km: 10 binds in most steps of the former, 1e5 in none at all, the default only at 20 km (tests/test_ensemble_sequences_cpu.py
# asserts steps on both sides of the bound in force, measured on the twin by ``mixing_steps``)
KH_CAPS = (None, 10.0, 1e5)
KH_BINDS, KH_NEVER = KH_CAPS[1], KH_CAPS[2]
Z0M = lvm.Z0M


def valid(modes):
    m = set(modes)
    return m <= set(MODES) and ("advect" in m or "vertical" not in m) and ("vertical" in m or not m & {"buoyancy", "conservative"}) and \
        ("conservative" in m or "order2" not in m) and ("mix" in m or not m & {"vmix", "kmix"}) and \
        ("vmix" not in m or not m & {"diffuse", "kmix"}) and ("kmix" not in m or "diffuse" in m) and ("mix" in m or IMIX not in m)


def combinations():
    """the 48 valid subsets of the six old modes (vertical needs advect), in a fixed order"""
    out = [c for r in range(len(OLD_MODES) + 1) for c in itertools.combinations(OLD_MODES, r) if "advect" in c or "vertical" not in c]
    assert len(out) == 48
    return out


def new_combinations(background):
    """the non-empty subsets of the five new modes that are valid on top of ``background``, in a fixed order"""
    return [tuple(background) + c for r in range(1, len(NEW_MODES) + 1) for c in itertools.combinations(NEW_MODES, r)
            if valid(tuple(background) + c)]


def mix_combinations(background):
    """the non-empty subsets of the three mixing modes that are valid on top of ``background``, in a fixed order"""
    return [tuple(background) + c for r in range(1, len(MIX_MODES) + 1) for c in itertools.combinations(MIX_MODES, r)
            if valid(tuple(background) + c)]


def name_of(modes):
    return "+".join(modes) or "plain"


def _mask(modes):
    return sum(1 << MODES.index(m) for m in modes)


def params(seed, modes):
    """the kind of K19, the limiter of K23, the cap, the stability switch and the spacings of K24 (``dx``: dx = dy / 1.5, None for
    the default) and the drag of K25 of the sequence ``generate(seed, modes)``, and with "imix" the bound ``kh_cap`` of K26 of its first
    enable_mixing (a generator of its own: the four older draws are what they were): pure functions of (seed, modes)"""
    bits = bin(_mask(modes)).count("1")
    pick = numpy.random.default_rng([int(seed), _mask(modes), 24]).integers(0, 1 << 16, 4)
    kh_cap = KH_CAPS[int(numpy.random.default_rng([int(seed), _mask(modes), 26]).integers(0, 1 << 16)) % 3] if IMIX in modes else None
    return {"kh_cap": kh_cap, "kind": qf.KINDS[(int(seed) + bits) % 2], "limiter": LIMITERS[(int(seed) + bits // 2) % 2],
            "cap": MIX_CAPS[int(pick[0]) % 2], "stability": bool(pick[1] % 2), "drag": bool(pick[2] % 2), "dx": MIX_DX[int(pick[3]) % 3]}


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def enable(ens, mode, modes, late=False, par=DEFAULT, implicit=None):
    """one of the opt-in modes: with the parameters of les_radiate_ref.ensemble_run, or, ``late``, with others; ``implicit``: what
    enable_mixing passes as such (None: whether the sequence has "imix", which is what its first call passes)"""
    n = ens.n
    if mode == "diffuse":
        ens.enable_diffusion(**(dict(k_max=0.5 * df.K_MAX, h_mix=1.25 * df.H_MIX, k_bg=2.0 * df.K_BG) if late else {}))
    elif mode == "micro":
        ens.enable_microphysics(**(dict(qc0=8e-5, v_fall=0.04, k_acc=3.0) if late else dict(qc0=1e-4, v_fall=0.05)))
    elif mode in ("advect", "readvect"):
        dx = READVECT["dx"] if mode == "readvect" else 1.25 * lvr.DX if late else lvr.DX
        kw = dict(cfl=READVECT["cfl"]) if mode == "readvect" else dict(cfl=0.4) if late else {}
        if "conservative" in modes:
            kw["conservative"] = True
        if "order2" in modes:
            kw.update(order=2, limiter=par["limiter"])
        ens.enable_advection(dx=dx, dy=1.5 * dx, vertical="vertical" in modes, **kw)
    elif mode == "qt":
        ens.enable_qt_forcing(par["kind"])
    elif mode == "buoyancy":
        ens.enable_buoyancy(**(dict(wave_speed=LATE_WAVE_SPEED) if late else {}))
    elif mode in ("mix", "kmix"):                                  # (kmix: enable_mixing once more, now with K15 behind it)
        ens.enable_mixing(vertical=mode == "kmix", **mixing(par, IMIX in modes if implicit is None else implicit, **(dict(cs=0.2) if late else {})))
    elif mode == "vmix":
        ens.enable_vertical_mixing(drag=par["drag"], **(dict(k_bg=0.2, kv_cap=500.0) if late else {}))
    else:
        assert mode == "radiate", mode
        s = 0.9 if late else 1.0
        ens.enable_radiation(f0=s * rad.F0 * (1.0 + 0.05 * numpy.arange(n)), f1=rad.F1 * (1.0 + 0.1 * (numpy.arange(n) % 3)),
                             kappa=rad.KAPPA * (1.0 + 0.02 * (numpy.arange(n) % 5)))


def mixing(par, implicit=False, **kw):
    """the arguments of enable_mixing that ``params`` sets: the cap, the stability switch and, where given, the spacings; with
    ``implicit`` the switch of K26 and its bound (else neither is passed: the call is what it was before K26)"""
    kw.update(cap=par["cap"], stability=par["stability"])
    if implicit:
        kw.update(implicit=True, kh_cap=par["kh_cap"])
    if par["dx"] is not None:
        kw.update(dx=par["dx"], dy=1.5 * par["dx"])
    return kw


def _comes_with(mode, modes):
    """what an ``enable`` of ``mode`` switches on ("imix" in the set of enabled modes: enable_mixing was last called with implicit=True)"""
    return {mode} | ({m for m in WITH_ADVECT if m in modes} if mode == "advect" else {IMIX} & set(modes) if mode == "mix" else set())


def _on_at_start(modes, late):
    return set(modes) - set(late) - ({m for m in WITH_ADVECT} if "advect" in late else set()) - ({IMIX} if "mix" in late else set())


def build(engine, device, n, modes, late=(), par=DEFAULT):
    """the ensemble of les_radiate_ref.ensemble_run (fields of make_les_fields at 4 x 5 x 20, the thermo variant's THL and QT,
    U raised in lvr.RAISED with the vertical advection, QR with the microphysics, presf, ql_ref, model_time = 900) on
    ``engine``: the device ensemble or the twin (thermo is the twin's class, so it is enabled here), with every mode of
    ``modes`` enabled that is not in ``late``"""
    assert valid(modes) and set(late) <= set(LATE) & set(modes)
    spcpl.set_engine(engine)
    thermo = "thermo" in modes
    cls = models.DeviceLESEnsemble if device else (lhr.HostThermoHmixLESEnsemble if thermo else lhr.HostHmixLESEnsemble)
    fs = [make_les_fields(ITOT, JTOT, NL, seed=60 + (i % 7)) for i in range(n)]
    stack = lambda k: numpy.stack([f[k] for f in fs])                                      # noqa: E731
    gcm = models.BatchedSyntheticGCM(n + 4, NG, 21)
    ens = cls.for_gcm(gcm, numpy.arange(1, n + 1), nL=NL, seed=21, itot=ITOT, jtot=JTOT, **twin_kw(cls, engine))
    rng = numpy.random.default_rng(n + 100)
    fields = {"Qsat": stack("qsat"), "QT": stack("qt"), "THL": stack("thl"), "U": 5.0 + rng.standard_normal((n, ITOT, JTOT, NL)),
              "V": -2.0 + rng.standard_normal((n, ITOT, JTOT, NL))}
    if "vertical" in modes:
        fields["U"][:, lvr.RAISED[0], lvr.RAISED[1], :] += 2.0
    if thermo:
        del fields["Qsat"]
        fields["THL"] = fields["THL"] - 25.0
        fields["QT"] = fields["QT"] * 0.35
        fields["QT"][:, 2, 1, :] *= 2.0
    if "micro" in modes:
        fields["QR"] = numpy.random.default_rng(n).random((n, ITOT, JTOT, NL)) * 1e-5
    ens.attach_fields({k: v.copy() for k, v in fields.items()})
    ens.p["presf"] = stack("presf")
    ens.ql_ref = stack("ql_ref")
    ens.model_time = 900.0
    if thermo:
        ens.enable_thermo()
    for mode in LATE:
        if mode in modes and mode not in late:
            enable(ens, mode, modes, par=par)
    rng = numpy.random.default_rng(5)
    ens.set_forcings_batched(THL=rng.normal(0, 2e-4, (n, NL)), QT=rng.normal(0, 2e-7, (n, NL)), U=rng.normal(0, 1e-4, (n, NL)),
                             WT_surf=ldr.WT * (0.5 + rng.random(n)), WQ_surf=ldr.WQ * (0.5 + rng.random(n)))
    return ens


# -- the generator -----------------------------------------------------------------------------------------------------------
def _choose(rng, table):
    names = [k for k, w in table if w > 0]
    w = numpy.array([w for k, w in table if w > 0], dtype=numpy.float64)
    return names[int(rng.choice(len(names), p=w / w.sum()))]


def _reads(op):
    """an operation that reads a profile, a field or a derived quantity of the ensemble (the nudge reads the means)"""
    return op[0] in OBSERVATIONS or op[0] in ("nudge", "record")


def _is_step(op):
    return op[0] in ("step", "row_step")


def generate(seed, modes, length=LENGTH):
    """``length`` operations, the last a full record, every one valid in the state it meets (the generator tracks what exists:
    RWP needs the QR field, the flux, W and the Courant numbers a step of their mode).  Plain tuples of Python values: a
    printed list can be pasted into ``replay``.  A row is given as any integer, taken modulo n.  A kind of operation that
    belongs to a mode the sequence does not have has weight 0 and consumes no draw; the two branches of the loop that belong to
    "imix" (the switch of K26, and the kinds of single modes that its switches would crowd out) test for the mode first."""
    modes = tuple(m for m in MODES if m in modes)
    assert valid(modes), modes
    rng = numpy.random.default_rng([int(seed), _mask(modes)])
    pending = [m for m in LATE if m in modes and rng.random() < (0.35 if m in MIX_MODES else 0.5)]     # (the mixing more often from the start)
    if "buoyancy" in modes and "advect" in pending and "buoyancy" not in pending:
        pending.append("buoyancy")                                 # (K21 is enabled after, and for, the advection)
    for m in ("vmix", "kmix"):                                     # (K25 and K24's vertical=True come behind enable_mixing, the latter behind K15)
        if m in modes and m not in pending and any(a in pending for a in AFTER[m]):
            pending.append(m)
    par = params(seed, modes)
    rough = [0, True]                                              # the z0m drawn; a step has followed the last one
    on = _on_at_start(modes, pending)
    stepped = set()                                                # modes that have seen a step since they were enabled
    lag = [False]                                                  # without thermo the QL field follows a new QT at the next step only
    handed = [False]                                               # qt_forcings has been drawn
    counted = [False]                                              # K19 has launched: there are counts a change of kind has to drop
    dropped = [False]                                              # the last mutation was a readvect: a step now runs without the buoyancy
    wread = [False]                                                # the moments of W have been read since the last mutation but a new Rhobf
    hint = [None]                                                  # the observation that would notice a stale cache behind the last mutation
    mixed = [False]                                                # a step of the mixing has followed the last switch of K26 (at first: enable_mixing)
    flipped = [False]                                              # the switch of K26 has been flipped
    ops = []
    small = lambda: int(rng.integers(0, 1 << 16))                                         # noqa: E731
    wp_names = ("LWP", "TWP") + (("RWP",) if "micro" in modes else ())
    field_names = ("U", "V", "THL", "QT", "QL", "Qsat") + (("QR",) if "micro" in modes else ())

    def subset(names, most):
        k = int(rng.integers(1, min(most, len(names)) + 1))
        return tuple(names[i] for i in sorted(rng.choice(len(names), k, replace=False)))

    def todo():
        """the operations that are still to come whatever is drawn: the late enables and, with "qt", the forcing"""
        return len(pending) + (1 if "qt" in modes and not handed[0] else 0) + z0m_todo()

    def z0m_todo():
        """a sequence of K25 with the drag holds two roughness lengths with a step behind each: the drag's key has something to miss"""
        return {0: 3, 1: 1}.get(rough[0], 0) + (0 if rough[1] else 1) if "vmix" in modes and par["drag"] else 0

    def refusable():
        """the calls that have to raise now: K15 and vertical=True beside K25, K25 beside K15 or vertical=True"""
        return [] if "mix" not in modes else (["diffusion", "kmix"] if "vmix" in on else []) + (["vmix"] if on & {"diffuse", "kmix"} else [])

    def mutation(kind=None, room=True):
        # (a nudge whose ql_av is not that of its QT is refused, "f(a) and f(b) must have different signs": none is drawn there)
        # (readvect puts the buoyancy back among the late enables: it needs the room for one more forced operation)
        again = "buoyancy" in on and length - 1 - len(ops) >= todo() + 3
        kind = kind or _choose(rng, [("step", 5), ("step0", 1), ("row_step", 1), ("nudge", 0 if lag[0] else 2), ("forcings", 1.5), ("set_field", 1.5), ("presf", 1),
                                     ("rhobf", 1), ("enable", 2.5 if pending and room else 0), ("qt_forcings", 0 if "qt" not in modes or not room else 0.7 if handed[0] else 2),
                                     ("qt_kind", 0 if "qt" not in on else 2.5 if counted[0] else 0.5), ("readvect", 2.5 if again else 0),
                                     ("rhobf", 12 if wread[0] else 0),                               # (W and its moments are made of Rhobf, ...
                                     ("presf", 2.5 if "buoyancy" in stepped else 0),                 # ... K21's profiles of presf: more of both there)
                                     ("remix", 2.5 if "mix" in on else 0), ("revmix", 6 if "vmix" in on else 0),
                                     ("z0m", 0 if "vmix" not in on or not room else 2 if rough[1] else 0.5), ("set_wind", 1.5 if "mix" in modes else 0),
                                     ("refused", 3 if refusable() else 0), ("rhobf", 1.5 if "vmix" in stepped else 0),
                                     # (the mixing early, so that steps follow it, and more of what the older modes draw rarely)
                                     ("enable", 8 if room and set(pending) & set(MIX_MODES) else 0), ("readvect", 4 if again and "mix" in on else 0),
                                     ("qt_kind", 2 if "qt" in on and "mix" in modes else 0),
                                     ("step", 3 if "kmix" in on else 0),                             # (K15's key holds K24's viscosity: steps of one dt)
                                     # (K26: most "imix" sequences switch, and a step of the mixing stands between two switches: both
                                     # paths run, the implicit one first, so ``les_hmix`` is launched whatever follows)
                                     ("implicit", 8 if IMIX in modes and mixed[0] else 0), ("step", 5 if IMIX in modes and "mix" in on and not mixed[0] else 0)])
        if kind == "step" and "kmix" in on and ops and _is_step(ops[-1]) and rng.random() < 0.6:
            op = ("step", ops[-1][-1])                             # (K15's key holds K24's viscosity: two steps of one dt show a key without it)
        elif kind == "step":
            op = ("step", DTS[int(rng.integers(len(DTS)))])
        elif kind == "row_step":
            op = ("row_step", small(), DTS[int(rng.integers(len(DTS)))])
        elif kind == "nudge":
            op = ("nudge", bool(rng.integers(2)), 1 + small())
        elif kind in ("forcings", "cloudfrac", "qt_forcings", "z0m"):
            op = (kind, small())
            handed[0] = handed[0] or kind == "qt_forcings"
            if kind == "z0m":
                rough[:] = [rough[0] + 1, False]
        elif kind == "set_wind":
            op = ("set_wind", ("U", "V")[int(rng.integers(2))], small())
        elif kind == "remix":
            op = ("remix", REMIX_CAPS[int(rng.integers(len(REMIX_CAPS)))], REMIX_PRANDTL[int(rng.integers(len(REMIX_PRANDTL)))])
        elif kind == "revmix":
            op = ("revmix", REVMIX["k_bg"][int(rng.integers(2))], REVMIX["kv_cap"][int(rng.integers(2))], bool(rng.integers(2)))
        elif kind == "refused":
            able = refusable()
            op = ("refused", able[int(rng.integers(len(able)))])
        elif kind == "implicit":                                   # (the first flips the switch, of the later ones three in four; the others keep it: a new kh_cap alone)
            op = ("implicit", (IMIX in on) != (rng.random() < 0.75 or not flipped[0]), KH_CAPS[int(rng.integers(len(KH_CAPS)))])
            flipped[0] = flipped[0] or (IMIX in on) != op[1]
            (on.add if op[1] else on.discard)(IMIX)
            mixed[0] = False
        elif kind == "set_field":
            op = ("set_field", ("QT", "THL")[int(rng.integers(2))], small())
        elif kind == "enable":
            able = [m for m in pending if not any(a in pending for a in AFTER.get(m, ()))]
            able = [m for m in able if m in MIX_MODES] or able     # (the mixing first: the steps behind it are what its sequences are for)
            mode = able[int(rng.integers(len(able)))]
            pending.remove(mode)
            on.update(_comes_with(mode, modes))
            op = ("enable", mode)
        elif kind == "readvect":
            on.discard("buoyancy")
            stepped.difference_update(("advect", "buoyancy") + WITH_ADVECT)
            pending.append("buoyancy")
            op = ("readvect",)
        else:
            op = (kind,)
        hint[0] = ("counts",) if kind == "qt_kind" else ("lid",) if kind == "readvect" and "conservative" in on else \
            ("stats", ("U", "W"), (("W", "THL"),)) if kind == "rhobf" and wread[0] else \
            ("stats", ("W", "QT"), (("U", "W"),)) if kind == "step" and "stats" in modes and "vertical" in on else \
            ("viscosity",) if kind in ("remix", "revmix", "implicit") or (kind == "enable" and op[1] in MIX_MODES) else None
        wread[0] = wread[0] and kind == "rhobf"
        dropped[0] = kind in ("readvect", "z0m")                  # (and a step behind a new roughness length: the drag's key)
        if _is_step(op):
            stepped.update(on)
            mixed[0] = mixed[0] or (kind != "step0" and "mix" in on)
            rough[1] = True
            lag[0] = False
            counted[0] = counted[0] or ("qt" in on and handed[0])
        elif op[0] == "nudge" or op[:2] == ("set_field", "QT"):
            lag[0] = "thermo" not in modes
        return op

    def stat_args():
        """a drawn subset of statistics.FIELDS (fields the ensemble does not hold among them: they are left out) with at least one
        it holds, and a drawn subset of statistics.PAIRS; one draw in four asks for everything (None, None): TKE is among it"""
        if rng.random() < 0.25:
            return None, None
        names = subset(st.FIELDS, 4)
        if not set(names) & set(ALWAYS):
            names = ("U",) + names
        if rng.random() < 0.3:
            names = tuple(k for k in st.FIELDS if k in names or k in ("U", "V"))          # (TKE)
        return names, (subset(st.PAIRS, 3) if rng.random() < 0.7 else ())

    def unseen():
        """the observations and mutations of single modes that can be drawn now and have not been: the switches of K26 crowd them
        out of 14 operations, and ``check_kinds`` wants each of them over a few cases"""
        able = (("flux", "radiate" in stepped), ("w", "vertical" in stepped), ("courant", "advect" in stepped), ("pressure", "buoyancy" in on),
                ("lid", "conservative" in on), ("counts", "qt" in on), ("row_stats", "stats" in modes), ("qt_kind", "qt" in on), ("revmix", "vmix" in on),
                ("readvect", "buoyancy" in on and length - 1 - len(ops) >= todo() + 3))
        return [k for k, ok in able if ok and not any(op[0] == k for op in ops)]

    def observation(kind=None):
        kind = kind or _choose(rng, [("profiles", 3), ("row", 3), ("field", 1.5), ("wp", 3), ("wp_means", 1), ("row_wp", 1), ("cloudfrac", 1),
                             ("flux", 3 if "radiate" in stepped else 0), ("w", 3 if "vertical" in stepped else 0),
                             ("courant", 2 if "advect" in stepped else 0), ("counts", 3 if "qt" in on else 0),
                             ("lid", 3 if "conservative" in on else 0), ("pressure", 4 if "buoyancy" in on else 0),
                             ("stats", 5 if "stats" in modes else 0), ("row_stats", 1.5 if "stats" in modes else 0),
                             ("viscosity", 3 if "mix" in modes else 0)] + ([] if "mix" not in modes else [
                                 ("flux", 2 if "radiate" in stepped else 0), ("courant", 2 if "advect" in stepped else 0), ("counts", 4 if "qt" in on else 0),
                                 ("lid", 2 if "conservative" in on else 0), ("stats", 3 if "stats" in modes else 0), ("row_stats", 3 if "stats" in modes else 0)]))
        if kind == "profiles":
            return ("profiles", subset(PROFILE_KEYS, 3))
        if kind == "row":
            return ("row", small(), sorted(ROW_GETTERS)[int(rng.integers(len(ROW_GETTERS)))])
        if kind == "field":
            return ("field", field_names[int(rng.integers(len(field_names)))])
        if kind == "wp":
            return ("wp", subset(wp_names, 3), bool(rng.integers(2)))
        if kind == "wp_means":
            return ("wp_means", subset(wp_names, 3))
        if kind == "row_wp":
            return ("row_wp", small(), wp_names[int(rng.integers(len(wp_names)))])
        if kind == "cloudfrac":
            return ("cloudfrac", small())
        if kind in ("stats", "row_stats"):
            names, pairs = stat_args()
            wread[0] = wread[0] or ("vertical" in stepped and (names is None or st.FACE in names))
            return ((kind,) if kind == "stats" else (kind, small())) + (names, pairs)
        return (kind,)

    # the head: a step that no read precedes, and two consecutive mutations
    head = int(rng.integers(3))
    if head == 0:
        ops += [mutation("step")]
        ops += [mutation(room=False)]
    elif head == 1:
        ops += [mutation(("forcings", "set_field", "presf", "rhobf")[int(rng.integers(4))])]
        ops += [mutation("step")]
    else:
        ops += [mutation("enable" if pending else "forcings")]
        ops += [mutation("step")]
    while len(ops) < length - 1:
        room = len(ops) < length - 3
        if todo() and length - 1 - len(ops) <= todo() + 1:         # a mode that is to be enabled late is, with a step behind it
            ops.append(mutation("enable" if pending else "qt_forcings" if "qt" in modes and not handed[0] else "z0m" if rough[1] else "step"))
        elif hint[0] is not None and rng.random() < 0.7:           # (no mutation of the old modes leaves a hint: no draw there)
            ops.append(hint[0])
            wread[0] = wread[0] or (hint[0][0] == "stats" and "vertical" in stepped)
            hint[0] = None
        elif dropped[0] and rng.random() < 0.7:
            ops.append(mutation("step"))
        elif IMIX in modes and mixed[0] and (not flipped[0] or IMIX not in on) and rng.random() < 0.5:
            # (most sequences of K26 leave it once, behind a step of it, and come back behind a step of K24)
            ops.append(mutation("implicit"))
        elif IMIX in modes and unseen() and rng.random() < 0.4:
            ops.append(mutation(unseen()[0]) if unseen()[0] in MUTATIONS else observation(unseen()[0]))
        elif rng.random() < 0.4:
            ops.append(observation())
        else:
            ops.append(mutation(room=room))
    last = _last_forced(ops)
    if not any(_is_step(op) for op in ops[last + 1:]):
        assert last < len(ops) - 1
        ops[-1] = mutation("step")
    ops.append(("record",))
    assert not pending and todo() == 0
    check_sequence(ops, modes, length, par)
    return ops


def _last_forced(ops):
    """the index of the last operation that wants a step behind it: an enable, the cloud-water forcing, the first two roughness lengths"""
    return max([i for i, op in enumerate(ops) if op[0] in ("enable", "qt_forcings")] + [i for i, op in enumerate(ops) if op[0] == "z0m"][:2], default=-1)


def check_sequence(ops, modes, length=None, par=None):
    """the conditions every sequence meets, whoever made it; returns the modes that are enabled late (an enable of the buoyancy
    behind a ``readvect`` is the second one)"""
    assert length is None or len(ops) == length, (len(ops), length)
    assert ops[-1] == ("record",) and all(op[0] in KINDS for op in ops)
    assert all(NEEDS.get(op[0]) is None or NEEDS[op[0]] in modes for op in ops), "an operation of a mode the sequence does not have"
    first = next(i for i, op in enumerate(ops) if _is_step(op))
    assert not any(_reads(op) for op in ops[:first]), "a read precedes every step"
    assert any(a[0] in MUTATIONS and b[0] in MUTATIONS for a, b in zip(ops, ops[1:])), "no two mutations follow each other"
    again = next((i for i, op in enumerate(ops) if op[0] == "readvect"), len(ops))
    late = [op[1] for i, op in enumerate(ops) if op[0] == "enable" and not (op[1] == "buoyancy" and i > again)]
    assert len(set(late)) == len(late) and set(late) <= set(LATE) & set(modes)
    on = _on_at_start(modes, late)                                 # the mixing modes: each call meets the state it needs
    for i, op in enumerate(ops):
        if op[0] == "enable":
            assert all(a in on for a in AFTER.get(op[1], ()) if a in modes and a != "advect"), "%r before what it needs" % (op,)
            on |= _comes_with(op[1], modes)
        assert op[0] != "remix" or "mix" in on, "remix before enable_mixing"
        assert op[0] != "revmix" or "vmix" in on, "revmix before enable_vertical_mixing"
        if op[0] == "implicit":
            assert "mix" in on and isinstance(op[1], bool) and (op[2] is None or op[2] > 0), "%r before enable_mixing, or no switch and bound" % (op,)
            (on.add if op[1] else on.discard)(IMIX)
        assert op[0] != "refused" or (op[1] in REFUSED and ("vmix" in on if op[1] != "vmix" else on & {"diffuse", "kmix"})), "%r would not raise" % (op,)
    last = _last_forced(ops)
    assert any(_is_step(op) for op in ops[last + 1:]), "no step after the last enable"
    if par is not None and "vmix" in modes and par["drag"]:
        at = next((i for i, op in enumerate(ops) if op[0] == "z0m"), None)
        assert at is not None and any(_is_step(op) for op in ops[:at]), "no roughness length behind a step in a sequence of K25 with the drag"
    if "qt" in modes and any(op[0] == "qt_forcings" for op in ops):
        at = next(i for i, op in enumerate(ops) if op[0] == "qt_forcings")
        assert any(_is_step(op) for op in ops[:at]), "no step before the cloud-water forcing is handed over"
    return late


def check_kinds(cases, length=LENGTH):
    """over the (seed, modes) of ``cases`` every kind of operation occurs that the modes of the cases allow"""
    seen = {op[0] for seed, modes in cases for op in generate(seed, modes, length)}
    want = {k for k in KINDS if NEEDS.get(k) is None or any(NEEDS[k] in modes for seed, modes in cases)}
    assert seen == want, (sorted(want - seen), sorted(seen - want))


# -- one operation -----------------------------------------------------------------------------------------------------------
NONE = numpy.zeros(0)                                              # what a getter that returns None is recorded as


def _all_profiles(ens):
    out = {k: numpy.empty_like(numpy.asarray(ens.p[k], dtype=numpy.float64)) for k in PROFILE_KEYS}
    ens.get_profiles_batched(PROFILE_KEYS, out)
    return out


def _row_equals_batched(ens, i, method, got):
    """property (a)"""
    key = ROW_GETTERS[method]
    out = {key: numpy.empty_like(numpy.asarray(ens.p[key], dtype=numpy.float64))}
    ens.get_profiles_batched((key,), out)
    assert_bits("(a) row %d %s against get_profiles_batched((%r,))" % (i, method, key), got, out[key][i])


def _flat(stats):
    return {"stat " + k: v for k, v in lmo.flat(stats).items()}


def _statistics(ens, device, names, pairs):
    """get_statistics as one dict of host arrays; on the device through get_statistics_batched as well: the same bits"""
    host = ens.get_statistics(names, pairs)
    if device:
        dev = ens.get_statistics_batched(names, pairs)
        assert sorted(dev) == ["cov", "mean", "std", "var"] and all(list(dev[kind]) == list(host[kind]) for kind in dev)
        for kind, d in dev.items():
            for key, t in d.items():
                assert_bits("get_statistics_batched %s %s against get_statistics" % (kind, key), numpy.asarray(host_of(t), dtype=numpy.float64), host[kind][key])
    return _flat(host)


def _row_statistics(ens, device, i, names, pairs):
    """a row's get_statistics, the row FIRST; property (a) on the device"""
    if not device:
        return _flat(ens.row_statistics(i, names, pairs))
    got = _flat(ens[i].get_statistics(names, pairs))
    whole = _flat(ens.get_statistics(names, pairs))
    assert list(got) == list(whole)
    for k in got:
        assert_bits("(a) row %d get_statistics %s against row %d of get_statistics" % (i, k, i), got[k], whole[k][i])
    return got


def _optional(t, dtype=None):
    return NONE if t is None else numpy.array(host_of(t), dtype=dtype)


def _lid(ens):
    lid = ens.get_lid_flux_batched()
    return {"lid": NONE} if lid is None else {"lid " + k: numpy.array(host_of(v)) for k, v in lid.items()}


def _number(x):
    return numpy.array([-1.0 if x is None else float(x)])


def _viscosity(ens):
    """K24's capped km (behind a step of K26, enable_mixing(implicit=True), the UNCAPPED km that ``les_hmix`` mixed by: the probe
    ran under ``_hmix_huge``; the bound ``_hmix_kh2`` acts on the faces inside the kernel and shows in the fields alone), the
    viscosity K25 mixed by (under K26 the same km: ``mixing_capped`` is False and there is no second probe), the largest uncapped
    viscosity and whether the cap bound (None: -1)"""
    return {"km": _optional(ens.get_eddy_viscosity_batched()), "kv": _optional(ens.get_vertical_viscosity_batched()),
            "k max": _number(ens.mixing_k_max), "capped": _number(ens.mixing_capped)}


def apply(ens, op, device, modes, on, par=DEFAULT):
    """``op`` on the device ensemble or on the twin; ``on``: the modes enabled now (updated).  Returns None for a mutation, a
    dict name -> host array for an observation"""
    n, kind = ens.n, op[0]
    if kind == "step":
        return ens.evolve_model_batched(ens.model_time + op[1])
    if kind == "step0":
        return ens.evolve_model_batched(ens.model_time)
    if kind == "row_step":
        ens[op[1] % n].evolve_model(ens.model_time + op[2])
        return None
    if kind == "nudge":
        numpy.random.seed(op[2])
        spcpl.variability_nudge_ensemble(ens, 900.0, op[1], write=False)
        return None
    if kind == "forcings":
        rng = numpy.random.default_rng(op[1])
        return ens.set_forcings_batched(THL=rng.normal(0, 2e-4, (n, NL)), QT=rng.normal(0, 2e-7, (n, NL)), U=rng.normal(0, 1e-4, (n, NL)),
                                        V=rng.normal(0, 1e-4, (n, NL)), SP=rng.normal(0, 1e-2, n), WT_surf=ldr.WT * (0.5 + rng.random(n)),
                                        WQ_surf=ldr.WQ * (0.5 + rng.random(n)))
    if kind == "qt_forcings":                                      # the cloud-water forcing and the reference profile of the coupler
        rng = numpy.random.default_rng(op[1])
        return ens.set_forcings_batched(QL=rng.normal(0, 2e-8, (n, NL)), QLp=numpy.asarray(ens.ql_ref) * (0.5 + rng.random((n, NL))))
    if kind == "qt_kind":
        ens.enable_qt_forcing(qf.KINDS[1 - qf.KINDS.index(ens.qt_forcing_kind)])
        return None
    if kind == "readvect":                                         # enable_advection again: the buoyancy is dropped until it is enabled again
        enable(ens, "readvect", modes, par=par)
        on.discard("buoyancy")
        return None
    if kind in ("set_field", "set_wind"):
        cur = numpy.array(host_of(ens.get_fields_batched(op[1])))
        noise = numpy.random.default_rng(op[2]).normal(0, 1e-2 if op[1] in ("QT", "U", "V") else 1e-4, cur.shape)
        return ens.set_fields_batched(op[1], cur * (1.0 + noise))
    if kind == "z0m":                                              # the roughness length of K25's drag
        return ens.set_forcings_batched(Z0M_surf=Z0M * (0.5 + numpy.random.default_rng(op[1]).random(n)))
    if kind == "remix":                                            # enable_mixing again: another cap and Prandtl number, vertical and implicit as they are
        ens.enable_mixing(vertical="kmix" in on, **mixing(dict(par, cap=op[1]), IMIX in on, prandtl=op[2]))
        return None
    if kind == "implicit":                                         # enable_mixing again: K26 switched on or off, another bound, vertical as it is
        ens.enable_mixing(vertical="kmix" in on, implicit=op[1], kh_cap=op[2], **mixing(par))
        (on.add if op[1] else on.discard)(IMIX)
        return None
    if kind == "revmix":
        ens.enable_vertical_mixing(k_bg=op[1], kv_cap=op[2], drag=op[3])
        return None
    if kind == "refused":
        call = {"diffusion": ens.enable_diffusion, "kmix": lambda: ens.enable_mixing(vertical=True), "vmix": ens.enable_vertical_mixing}[op[1]]
        try:
            call()
        except ValueError:
            return None
        raise AssertionError("%r was not refused" % (op,))
    if kind == "presf":
        ens.p["presf"] *= 1.002
        return None
    if kind == "rhobf":
        ens.p["Rhobf"] *= 1.01
        return None
    if kind == "enable":
        enable(ens, op[1], modes, late=True, par=par, implicit=IMIX in on if op[1] == "kmix" else None)
        on.update(_comes_with(op[1], modes))
        return None
    if kind == "profiles":
        out = {k: numpy.empty_like(numpy.asarray(ens.p[k], dtype=numpy.float64)) for k in op[1]}
        ens.get_profiles_batched(op[1], out)
        return out
    if kind == "row":
        i = op[1] % n
        got = numpy.array(getattr(ens[i], op[2])())
        _row_equals_batched(ens, i, op[2], got)
        return {op[2]: got}
    if kind == "field":
        return {op[1]: numpy.array(host_of(ens.get_fields_batched(op[1])))}          # (the device tensor itself: copied at once)
    if kind == "wp":
        return {k: numpy.array(host_of(v)) for k, v in ens.get_water_paths_batched(op[1], cloud_cover=op[2]).items()}
    if kind == "wp_means":
        return {k: numpy.array(v) for k, v in ens.get_water_path_means(op[1]).items()}
    if kind == "row_wp":
        i = op[1] % n
        return {op[2]: numpy.array(ens[i].get_field(op[2]) if device else ens.row_field(i, op[2]))}
    if kind == "cloudfrac":
        idx = numpy.sort(numpy.random.default_rng(op[1]).integers(0, NL + 4, (n, NG)), axis=1).astype(numpy.int32)       # (some beyond ktot)
        idx[0, [3, 11]] = idx[0, [11, 3]]                          # one map that is not monotone, as in slab_ref.hand_case
        out = numpy.empty((n, NG))
        ens.get_cloudfraction_batched(idx, out)
        return {"A": out}
    if kind == "flux":
        return {"flux": numpy.array(host_of(ens.get_radiative_flux_batched()))}
    if kind == "w":
        return {"W": numpy.array(host_of(ens.get_vertical_wind_batched()))}
    if kind == "courant":
        rec = {"substeps": numpy.array([float(ens.advect_substeps)]), "courant": numpy.array([ens.advect_courant])}
        if "vertical" in on:
            rec["courant z"] = _number(ens.advect_courant_z)       # (None in the conservative mode)
        if "buoyancy" in on:
            rec["wind change"] = _number(ens.buoyancy_wind_change)
        return rec
    if kind == "counts":
        return {"counts": _optional(ens.get_qt_forcing_counts_batched(), numpy.float64)}
    if kind == "lid":
        return _lid(ens)
    if kind == "pressure":
        return {"phi": _optional(ens.get_pressure_batched())}
    if kind == "viscosity":
        return _viscosity(ens)
    if kind == "stats":
        return _statistics(ens, device, op[1], op[2])
    if kind == "row_stats":
        return _row_statistics(ens, device, op[1] % n, op[2], op[3])
    assert kind == "record", op
    rec = {"got " + k: v for k, v in _all_profiles(ens).items()}
    rec.update({"p " + k: numpy.array(v) for k, v in ens.p.items()})              # (read above: p is that of the fields as they are)
    names = ("LWP", "TWP") + (("RWP",) if "micro" in modes else ())
    rec.update({"field " + k: numpy.array(host_of(ens.get_fields_batched(k)))
                for k in ("U", "V", "THL", "QT", "QL", "Qsat") + (("QR",) if "micro" in modes else ())})
    rec.update({k: numpy.array(host_of(v)) for k, v in ens.get_water_paths_batched(names, cloud_cover=True).items()})
    rec.update({"mean " + k: numpy.array(v) for k, v in ens.get_water_path_means(names).items()})
    if "micro" in on:
        rec["rain2d"] = numpy.array(host_of(ens.rain2d))
    if "radiate" in on:
        flux = ens.get_radiative_flux_batched()
        rec["flux"] = numpy.zeros((n, ITOT, JTOT, NL)) if flux is None else numpy.array(host_of(flux))
    if "advect" in on:
        rec["substeps"] = numpy.array([-1.0 if ens.advect_substeps is None else float(ens.advect_substeps)])
        rec["courant"] = numpy.array([-1.0 if ens.advect_courant is None else ens.advect_courant])
    if "vertical" in on:
        rec["courant z"] = numpy.array([-1.0 if ens.advect_courant_z is None else ens.advect_courant_z])
        if ens.get_vertical_wind_batched() is not None:
            rec["W"] = numpy.array(host_of(ens.get_vertical_wind_batched()))
    if "qt" in on:
        rec["counts"] = _optional(ens.get_qt_forcing_counts_batched(), numpy.float64)
    if "conservative" in on:
        rec.update(_lid(ens))
    if "buoyancy" in on:
        rec["phi"] = _optional(ens.get_pressure_batched())
        rec["wind change"] = _number(ens.buoyancy_wind_change)
    if "mix" in modes:
        rec.update(_viscosity(ens))
    if "stats" in modes:
        rec.update(_statistics(ens, device, None, None))
    for i in range(n):
        for method in sorted(ROW_GETTERS):
            _row_equals_batched(ens, i, method, numpy.array(getattr(ens[i], method)()))
        if "stats" in modes and device:
            _row_statistics(ens, device, i, None, None)
    return rec


# -- launch counting -----------------------------------------------------------------------------------------------------------
class Counter:
    """wraps the COUNTED methods of an engine (of every engine of a MultiDeviceEngine) on the instances; ``calls`` lists their
    names in the order of the launches; ``restore`` takes the wrappers off again"""

    def __init__(self, engine):
        self.calls, self._wrapped = [], []
        for e in getattr(engine, "engines", [engine]):
            for name in COUNTED:
                inner = getattr(e, name, None)
                if callable(inner):
                    setattr(e, name, lambda *a, _n=name, _f=inner, **kw: (self.calls.append(_n), _f(*a, **kw))[1])
                    self._wrapped.append((e, name))

    def restore(self):
        for e, name in self._wrapped:
            delattr(e, name)
        self._wrapped = []


def check_step(calls, ens, on):
    """the launches of one step of the device ensemble with the mixing: with K25 ``les_mix`` ran twice (the probe again under a cap
    that never binds) exactly where the step's cap bound, else once, per ``les_vmix`` (one per engine that holds rows); with
    K15 enabled as well nothing stands between ``les_mix`` and ``les_diffuse`` but, with vertical=True, one ``slab_means`` (of km) per
    engine.  With K26 (enable_mixing was last called with implicit=True) every engine that holds rows launched exactly ONE ``les_mix``, K25
    or not, one ``les_hmix`` directly behind them and ``mixing_capped`` is False; then the ``les_hmix`` stand between ``les_mix`` and
    ``les_diffuse`` in front of the ``slab_means``.  Without K26 no ``les_hmix`` is launched at all"""
    hmix = []
    if IMIX in on:
        rows = len([t for t in getattr(ens.fields3d["U"], "parts", [ens.fields3d["U"]]) if t.numel()])
        hmix = ["les_hmix"] * rows
        assert rows >= 1 and calls.count("les_mix") == calls.count("les_hmix") == rows, \
            "%d engines hold rows and the implicit step launched %r" % (rows, [c for c in calls if c in ("les_mix", "les_hmix")])
        at = calls.index("les_mix")
        assert calls[at:at + 2 * rows] == ["les_mix"] * rows + hmix, calls
        assert ens.mixing_capped is False, "mixing_capped is %r behind an implicit step" % (ens.mixing_capped,)
    else:
        assert "les_hmix" not in calls, calls
    if "vmix" in on:
        per = 2 if ens.mixing_capped else 1
        assert calls.count("les_vmix") >= 1 and calls.count("les_mix") == per * calls.count("les_vmix"), \
            "mixing_capped is %r and the step launched %r" % (ens.mixing_capped, [c for c in calls if c in ("les_mix", "les_vmix")])
    elif "mix" in on:
        assert "les_mix" in calls and "les_vmix" not in calls, calls
    if "mix" in on and "diffuse" in on:
        between = calls[max(i for i, c in enumerate(calls) if c == "les_mix") + 1:calls.index("les_diffuse")]
        assert between == hmix + (["slab_means"] * calls.count("les_mix") if "kmix" in on else []), calls


def check_launched(calls, modes):
    """every enabled mode launched its method; the conservative transport stands in the place of the split pair"""
    for mode in modes:
        if "conservative" in modes and mode in ("advect", "vertical"):
            assert METHOD[mode] not in calls, "the conservative transport is enabled and %s launched" % METHOD[mode]
        else:
            assert METHOD[mode] in calls, "%s was enabled and %s never launched" % (mode, METHOD[mode])


# -- a whole sequence ----------------------------------------------------------------------------------------------------------
def _compare(key, got, want):
    if key == "W":                                                 # a torch expression: the bound of les_vadvect_ref.check_w
        assert got.shape == want.shape and numpy.isfinite(want).all() and numpy.abs(want).max() > 0
        assert got.dtype == want.dtype, "W: dtype %s, expected %s" % (got.dtype, want.dtype)
        err, bound = numpy.abs(got - want).max(), 4 * numpy.finfo(want.dtype).eps * numpy.abs(want).max()
        assert err <= bound, "W: max abs err %.3e > %.3e" % (err, bound)
    else:
        assert_bits(key, got, want, dtypes=True)


def _holds_w(key):
    """a statistics entry that W enters: "stat mean W", "stat cov W-THL", "stat cov U-W", ... (TKE: where there is a variance of W)"""
    return key.startswith("stat ") and st.FACE in key.split(" ")[-1].split("-")


def _of_the_own_w(ens, got, want, row=None):
    """``want`` (the twin's record) with the moments that hold W replaced by the oracle of K20 on the device's own W and its own
    partner fields, as they are at this operation"""
    keys = [k for k in got if _holds_w(k)]
    if not keys:
        return want
    pairs = [tuple(k.split(" ")[-1].split("-")) for k in keys if k.startswith("stat cov ")]
    names = [k for k in st.FIELDS if k == st.FACE or any(k in p for p in pairs)]
    fields = {k: numpy.asarray(host_of(ens.get_vertical_wind_batched() if k == st.FACE else ens.get_fields_batched(k))) for k in names}
    own = _flat({kind: {k: numpy.asarray(a, dtype=numpy.float64) for k, a in d.items()} for kind, d in lmo.les_moments(fields, pairs, st.FACE).items()})
    want = dict(want)
    for k in keys:
        want[k] = own[k] if row is None else own[k][row]
    if "stat TKE" in got and "stat var W" in got:
        want["stat TKE"] = st.tke({"U": want["stat var U"], "V": want["stat var V"], "W": want["stat var W"]})
    return want


def replay(ops, modes, n, engine_for_twin, engine_for_device, what="", par=DEFAULT):
    """the list ``ops`` on the twin (NumPy fields; its nudge runs on ``engine_for_twin``) and on the device ensemble on
    ``engine_for_device``; every observation compared, properties (a), (b) and (c) checked on the way.  ``par``: the kind of K19,
    the limiter of K23 and the parameters of K24 and K25 (``params``).  An AssertionError names ``what``, the modes, the index of
    the operation and the
    operations up to it.  Returns the launches of the device side."""
    modes = tuple(m for m in MODES if m in modes)
    late = check_sequence(ops, modes, par=par)

    def told(i, side, e):
        return AssertionError("%s modes %s n %d, operation %d %r on the %s: %s\nthe operations up to it (ensemble_sequences.replay(ops, %r, %d, ..., par=%r)):\n%r"
                              % (what, name_of(modes), n, i, ops[i], side, e, modes, n, par, list(ops[:i + 1])))
    twin, on, want = build(engine_for_twin, False, n, modes, late, par), _on_at_start(modes, late), []
    for i, op in enumerate(ops):
        try:
            want.append(apply(twin, op, False, modes, on, par))
        except AssertionError as e:
            raise told(i, "twin", e) from e
    assert len(want) == len(ops)
    counter = Counter(engine_for_device)
    done = 0
    cached = set()                                                 # property (c): the statistics read since the last mutation
    handed = None                                                  # the launches before the first qt_forcings
    try:
        ens, on = build(engine_for_device, True, n, modes, late, par), _on_at_start(modes, late)
        for i, op in enumerate(ops):
            try:
                if op[0] == "qt_forcings" and handed is None:
                    handed = len(counter.calls)
                mark = len(counter.calls)
                got = apply(ens, op, True, modes, on, par)
                assert (got is None) == (want[i] is None) and (got is None or list(got) == list(want[i])), (got and list(got), want[i] and list(want[i]))
                if got is not None:
                    stats = {k for k in got if k.startswith("stat ") and k != "stat TKE"}
                    if stats and stats <= cached:                  # property (c)
                        assert "les_moments" not in counter.calls[mark:], "(c) K20 launched for statistics that were cached: %s" % sorted(stats)
                    cached |= stats
                    ref = _of_the_own_w(ens, got, want[i], row=op[1] % n if op[0] == "row_stats" else None)
                    for k in got:
                        _compare(k, got[k], ref[k])
                    mark = len(counter.calls)                      # property (b)
                    again = apply(ens, op, True, modes, on, par)
                    extra = set(counter.calls[mark:]) - RELAUNCH.get(op[0], set())
                    assert not extra, "(b) the second read launched %s" % sorted(extra)
                    for k in got:
                        assert_bits("(b) the second read of " + k, again[k], got[k])
                elif op[0] == "rhobf":
                    cached = {k for k in cached if not _holds_w(k)}
                else:
                    cached = set()
                if _is_step(op) and "mix" in on and len(counter.calls) > mark:
                    check_step(counter.calls[mark:], ens, on)
            except AssertionError as e:
                raise told(i, "device ensemble", e) from e
            done += 1
    finally:
        counter.restore()
    assert done == len(ops) and ens.model_time == twin.model_time
    assert "les_qt_local" not in counter.calls[:handed], "K19 launched before the cloud-water forcing was handed over"
    check_launched(counter.calls, [m for m in modes if m != "qt" or handed is not None])
    return counter.calls


def mixing_steps(engine_for_twin, seed, modes, n=3, length=LENGTH):
    """what the twin alone shows of every step of ``generate(seed, modes, length)`` that K24 or K26 ran in: a list of dicts with
    ``implicit`` (K26 ran), ``vmix`` (K25 followed), ``capped`` (the twin's mixing_capped), ``k_max`` (its mixing_k_max) and
    ``kh_cap`` (the bound of K26 in force)"""
    modes = tuple(m for m in MODES if m in modes)
    ops, par = generate(seed, modes, length), params(seed, modes)
    late = check_sequence(ops, modes, par=par)
    twin, on, out = build(engine_for_twin, False, n, modes, late, par), _on_at_start(modes, late), []
    for op in ops:
        before = twin.model_time
        apply(twin, op, False, modes, on, par)
        if _is_step(op) and "mix" in on and twin.model_time > before:
            assert twin.mix_par["implicit"] == (IMIX in on)
            out.append({"implicit": IMIX in on, "vmix": "vmix" in on, "capped": bool(twin.mixing_capped), "k_max": twin.mixing_k_max,
                        "kh_cap": twin.mix_par["kh_cap"]})
    return out


def implicit_conditions(cases, engine, length=LENGTH):
    """the conditions on a set of "imix" cases (seed, modes), measured on the twin and on the generated lists; returns the counts:
    switches implicit -> explicit and explicit -> implicit, sequences that hold steps of both paths, late enables of mix with
    implicit and of kmix behind an implicit mix, "vmix" sequences with a step of two ``les_mix`` (the explicit cap bound) and an
    implicit step, and the implicit steps whose largest viscosity lies above and below the ``kh_cap`` in force"""
    count = dict.fromkeys(("to explicit", "to implicit", "both paths", "late mix", "late kmix", "vmix both", "above", "below", "switching"), 0)
    for seed, modes in cases:
        ops, par = generate(seed, modes, length), params(seed, modes)
        assert IMIX in modes and ops == generate(seed, modes, length) and par == params(seed, modes) and par["kh_cap"] in KH_CAPS
        late = check_sequence(ops, modes, par=par)
        on = _on_at_start(modes, late)
        assert (IMIX in on) == ("mix" not in late)
        switched = False
        for op in ops:
            if op[0] == "implicit":
                assert op[2] in KH_CAPS
                count["to explicit"] += IMIX in on and not op[1]
                count["to implicit"] += IMIX not in on and op[1]
                switched = switched or (IMIX in on) != op[1]
                (on.add if op[1] else on.discard)(IMIX)
            elif op[0] == "enable":
                on |= _comes_with(op[1], modes)
                count["late mix"] += op[1] == "mix" and IMIX in on
                count["late kmix"] += op[1] == "kmix" and IMIX in on
        count["switching"] += switched
        steps = mixing_steps(engine, seed, modes, length=length)
        assert any(s["implicit"] for s in steps), "no implicit step in seed %d %s" % (seed, name_of(modes))
        assert all(s["capped"] is False for s in steps if s["implicit"])
        count["both paths"] += len({s["implicit"] for s in steps}) == 2
        count["vmix both"] += any(s["vmix"] and s["implicit"] for s in steps) and any(s["vmix"] and not s["implicit"] and s["capped"] for s in steps)
        bound = lambda s: hmx.KH_CAP if s["kh_cap"] is None else s["kh_cap"]                  # noqa: E731
        count["above"] += sum(s["implicit"] and s["k_max"] > bound(s) for s in steps)
        count["below"] += sum(s["implicit"] and s["k_max"] <= bound(s) for s in steps)
        # the drawn bounds are what ensemble_sequences says of them: one binds nowhere, one in most steps of the 250 m spacing
        assert all(s["k_max"] < KH_NEVER for s in steps)
    fine = [s for seed, modes in cases if params(seed, modes)["dx"] == 250.0 for s in mixing_steps(engine, seed, modes, length=length)]
    assert fine and sum(s["k_max"] > KH_BINDS for s in fine) > len(fine) / 2, [s["k_max"] for s in fine]
    assert all(count[k] >= 1 for k in count), count
    assert count["switching"] > len(cases) / 2, (count, len(cases))                         # most sequences switch at least once
    return count


def run(engine_for_twin, engine_for_device, seed, modes, n, length=LENGTH):
    """``generate(seed, modes)`` through ``replay``"""
    return replay(generate(seed, modes, length), modes, n, engine_for_twin, engine_for_device, what="seed %d" % seed, par=params(seed, modes))


def dtype_conditions(cases, engine, n=3, length=LENGTH):
    """what the twin alone, in the dtype of ``engine`` (les_harness.np_of: the twin's nudge runs on it), reaches over the
    ``cases`` (seed, modes): the counts of advective steps of more than one substep and of one, of steps of K24 whose cap binds
    and whose cap does not, of levels with a positive and with a negative increment ``a`` handed to K19, of implicit steps whose
    largest viscosity lies above and below the ``kh_cap`` in force, and of steps of K14 behind which rain has reached the ground
    in every LES.  Every count is asserted to be 1 or more where a case holds the mode it belongs to, and every field of every
    twin to be of that dtype at the end"""
    from tests import les_qt_local_ref as qlr
    from tests.les_harness import np_of
    T = numpy.dtype(np_of(engine))
    count = dict.fromkeys(("substeps > 1", "substeps 1", "capped", "uncapped", "a > 0", "a < 0", "above kh_cap", "below kh_cap", "rain"), 0)
    inner = qlr.les_qt_local

    def counted(qt, ql, A, QTM):
        assert A.dtype == T
        count["a > 0"] += int((A > 0).sum())
        count["a < 0"] += int((A < 0).sum())
        return inner(qt, ql, A, QTM)
    qlr.les_qt_local = counted
    try:
        for seed, modes in cases:
            modes = tuple(m for m in MODES if m in modes)
            ops, par = generate(seed, modes, length), params(seed, modes)
            late = check_sequence(ops, modes, par=par)
            twin, on = build(engine, False, n, modes, late, par), _on_at_start(modes, late)
            assert twin.dtype == T.type
            for op in ops:
                before = twin.model_time
                apply(twin, op, False, modes, on, par)
                if not (_is_step(op) and twin.model_time > before):
                    continue
                if "advect" in on:
                    count["substeps > 1" if twin.advect_substeps > 1 else "substeps 1"] += 1
                if "mix" in on and IMIX not in on:
                    count["capped" if twin.mixing_capped else "uncapped"] += 1
                if IMIX in on:
                    bound = hmx.KH_CAP if twin.mix_par["kh_cap"] is None else twin.mix_par["kh_cap"]
                    count["above kh_cap" if twin.mixing_k_max > bound else "below kh_cap"] += 1
                if "micro" in on:
                    count["rain"] += bool((twin.p["Rain"] > 0).all() and (twin.rain2d > 0).any())
            assert all(a.dtype == T for a in twin.fields3d.values()), {k: a.dtype for k, a in twin.fields3d.items()}
            assert all(numpy.asarray(v).dtype == numpy.float64 for k, v in twin.p.items()), {k: numpy.asarray(v).dtype for k, v in twin.p.items()}
    finally:
        qlr.les_qt_local = inner
    has = lambda mode: any(mode in modes for seed, modes in cases)                          # noqa: E731
    needs = {"substeps > 1": "advect", "substeps 1": "advect", "capped": "mix", "uncapped": "mix", "a > 0": "qt", "a < 0": "qt",
             "above kh_cap": IMIX, "below kh_cap": IMIX, "rain": "micro"}
    assert all(count[k] >= 1 for k, mode in needs.items() if has(mode)), count
    return count
