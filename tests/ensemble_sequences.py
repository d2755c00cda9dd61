"""Random operation sequences of models.DeviceLESEnsemble (the class lives in sp_coupler_amd/device_les.py; the name in models
is the same object) against its eager NumPy twin (tests/les_radiate_ref.py:
HostRadiateLESEnsemble / HostThermoRadiateLESEnsemble, the top of the chain of twins): the body of
tests/test_ensemble_sequences_cpu.py (on oracle-backed engines) and tests/test_ensemble_sequences_gpu.py (on the card).

The device ensemble is a lazy, cached state machine (_thermo_stale, _means, _wp / _wp_host / _wp_w, _thermo_means, four profile
uploads keyed on their inputs, the ping-pong buffers of K14 / K16 / K17, the fused K11 step); the twin computes everything
eagerly from its fields.  ``generate`` draws a list of operations that are all valid in the state they meet, mutations and
sparse observations mixed; ``replay`` applies the list to both and compares every observation bit for bit
(gpu_util.assert_bits), W alone within the bound of les_vadvect_ref.check_w (a torch expression).

Conditions, asserted here and not left to the callers:
  * every sequence has its full length, runs to its end on both sides and ends with a full record: every profile (batched,
    raw and through every row), every field, the water paths with the cloud cover and their means, rain2d, the flux, W and
    the Courant numbers of what is enabled;
  * every sequence holds a step that no read precedes and two consecutive mutations;
  * every mode a sequence enables launches its engine method at least once on the device side (``check_launched``);
  * over a set of cases every kind of operation occurs (``check_kinds``).
Properties of the device ensemble (and of the twin, where it has the method) that need no twin:
  (a) a row getter of key k returns row i of what get_profiles_batched((k,)) returns at that moment: checked at every ``row``
      operation, the row getter FIRST (so it has to refresh p itself), and for every row and key at the final record;
  (b) reading anything twice in a row gives the same bits and launches nothing the second time: checked at every observation.
      Two readers hold no cache of their own and launch their own reduction every time, and only that: the cloud fraction
      (slab_cloud_fraction) and the water path means (slab_means of the cached paths)."""
import itertools

import numpy

from sp_coupler_amd import diffusion as df
from sp_coupler_amd import models, spcpl
from sp_coupler_amd import radiation as rad
from tests import les_diffuse_ref as ldr
from tests import les_radiate_ref as lrr
from tests import les_vadvect_ref as lvr
from tests.gpu_util import assert_bits
from tests.les_harness import host_of
from tests.test_vnudge import make_les_fields

MODES = ("thermo", "diffuse", "micro", "advect", "vertical", "radiate")
LATE = ("diffuse", "micro", "advect", "radiate")                  # may be enabled mid-sequence (vertical comes with advect)
METHOD = {"thermo": "les_thermo", "diffuse": "les_diffuse", "micro": "les_microphysics", "advect": "les_advect",
          "vertical": "les_vadvect", "radiate": "les_radiate"}
COUNTED = ("slab_means", "slab_cloud_fraction", "variability_nudge", "les_advance", "les_thermo", "les_water_paths", "les_microphysics",
           "les_diffuse", "les_advect", "les_vadvect", "les_radiate")
MUTATIONS = ("step", "step0", "row_step", "nudge", "forcings", "set_field", "presf", "rhobf", "enable")
OBSERVATIONS = ("profiles", "row", "field", "wp", "wp_means", "row_wp", "cloudfrac", "flux", "w", "courant")
KINDS = MUTATIONS + OBSERVATIONS + ("record",)
RELAUNCH = {"cloudfrac": {"slab_cloud_fraction"}, "wp_means": {"slab_means"}, "record": {"slab_means"}}      # property (b)
PROFILE_KEYS = ("U", "V", "THL", "QT", "QL", "T", "QL_ice", "QR", "presf", "Rhobf", "Rain", "PS")
ROW_GETTERS = {"get_profile_U": "U", "get_profile_V": "V", "get_profile_THL": "THL", "get_profile_QT": "QT", "get_profile_QL": "QL",
               "get_profile_QL_ice": "QL_ice", "get_profile_QR": "QR", "get_profile_T": "T", "get_rain": "Rain", "get_presf": "presf"}
DTS = (300.0, 450.0, 900.0, 900.0)
ITOT, JTOT, NL, NG = 4, 5, 20, 19
LENGTH = 14


def combinations():
    """the 48 valid subsets of MODES (vertical needs advect), in a fixed order"""
    out = [c for r in range(len(MODES) + 1) for c in itertools.combinations(MODES, r) if "advect" in c or "vertical" not in c]
    assert len(out) == 48
    return out


def name_of(modes):
    return "+".join(modes) or "plain"


# -- the ensemble ------------------------------------------------------------------------------------------------------------
def enable(ens, mode, modes, late=False):
    """one of the four opt-in modes: with the parameters of les_radiate_ref.ensemble_run, or, ``late``, with others"""
    n = ens.n
    if mode == "diffuse":
        ens.enable_diffusion(**(dict(k_max=0.5 * df.K_MAX, h_mix=1.25 * df.H_MIX, k_bg=2.0 * df.K_BG) if late else {}))
    elif mode == "micro":
        ens.enable_microphysics(**(dict(qc0=8e-5, v_fall=0.04, k_acc=3.0) if late else dict(qc0=1e-4, v_fall=0.05)))
    elif mode == "advect":
        dx = 1.25 * lvr.DX if late else lvr.DX
        ens.enable_advection(dx=dx, dy=1.5 * dx, vertical="vertical" in modes, **(dict(cfl=0.4) if late else {}))
    else:
        assert mode == "radiate", mode
        s = 0.9 if late else 1.0
        ens.enable_radiation(f0=s * rad.F0 * (1.0 + 0.05 * numpy.arange(n)), f1=rad.F1 * (1.0 + 0.1 * (numpy.arange(n) % 3)),
                             kappa=rad.KAPPA * (1.0 + 0.02 * (numpy.arange(n) % 5)))


def build(engine, device, n, modes, late=()):
    """the ensemble of les_radiate_ref.ensemble_run (fields of make_les_fields at 4 x 5 x 20, the thermo variant's THL and QT,
    U raised in lvr.RAISED with the vertical advection, QR with the microphysics, presf, ql_ref, model_time = 900) on
    ``engine``: the device ensemble or the twin (thermo is the twin's class, so it is enabled here), with every mode of
    ``modes`` enabled that is not in ``late``"""
    assert set(modes) <= set(MODES) and ("advect" in modes or "vertical" not in modes) and set(late) <= set(LATE) & set(modes)
    spcpl.set_engine(engine)
    thermo = "thermo" in modes
    cls = models.DeviceLESEnsemble if device else (lrr.HostThermoRadiateLESEnsemble if thermo else lrr.HostRadiateLESEnsemble)
    fs = [make_les_fields(ITOT, JTOT, NL, seed=60 + (i % 7)) for i in range(n)]
    stack = lambda k: numpy.stack([f[k] for f in fs])                                      # noqa: E731
    gcm = models.BatchedSyntheticGCM(n + 4, NG, 21)
    ens = cls.for_gcm(gcm, numpy.arange(1, n + 1), nL=NL, seed=21, itot=ITOT, jtot=JTOT)
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
            enable(ens, mode, modes)
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
    printed list can be pasted into ``replay``.  A row is given as any integer, taken modulo n."""
    modes = tuple(m for m in MODES if m in modes)
    rng = numpy.random.default_rng([int(seed), sum(1 << MODES.index(m) for m in modes)])
    pending = [m for m in LATE if m in modes and rng.random() < 0.5]
    on = set(modes) - set(pending) - ({"vertical"} if "advect" in pending else set())
    stepped = set()                                                # modes that have seen a step since they were enabled
    lag = [False]                                                  # without thermo the QL field follows a new QT at the next step only
    small = lambda: int(rng.integers(0, 1 << 16))                                         # noqa: E731
    wp_names = ("LWP", "TWP") + (("RWP",) if "micro" in modes else ())
    field_names = ("U", "V", "THL", "QT", "QL", "Qsat") + (("QR",) if "micro" in modes else ())

    def subset(names, most):
        k = int(rng.integers(1, min(most, len(names)) + 1))
        return tuple(names[i] for i in sorted(rng.choice(len(names), k, replace=False)))

    def mutation(kind=None, room=True):
        # (a nudge whose ql_av is not that of its QT is refused, "f(a) and f(b) must have different signs": none is drawn there)
        kind = kind or _choose(rng, [("step", 5), ("step0", 1), ("row_step", 1), ("nudge", 0 if lag[0] else 2), ("forcings", 1.5), ("set_field", 1.5), ("presf", 1),
                                     ("rhobf", 1), ("enable", 2.5 if pending and room else 0)])
        if kind == "step":
            op = ("step", DTS[int(rng.integers(len(DTS)))])
        elif kind == "row_step":
            op = ("row_step", small(), DTS[int(rng.integers(len(DTS)))])
        elif kind == "nudge":
            op = ("nudge", bool(rng.integers(2)), 1 + small())
        elif kind in ("forcings", "cloudfrac"):
            op = (kind, small())
        elif kind == "set_field":
            op = ("set_field", ("QT", "THL")[int(rng.integers(2))], small())
        elif kind == "enable":
            mode = pending.pop(int(rng.integers(len(pending))))
            on.update({mode} | ({"vertical"} if mode == "advect" and "vertical" in modes else set()))
            op = ("enable", mode)
        else:
            op = (kind,)
        if _is_step(op):
            stepped.update(on)
            lag[0] = False
        elif op[0] == "nudge" or op[:2] == ("set_field", "QT"):
            lag[0] = "thermo" not in modes
        return op

    def observation():
        kind = _choose(rng, [("profiles", 3), ("row", 3), ("field", 1.5), ("wp", 3), ("wp_means", 1), ("row_wp", 1), ("cloudfrac", 1),
                             ("flux", 3 if "radiate" in stepped else 0), ("w", 3 if "vertical" in stepped else 0),
                             ("courant", 2 if "advect" in stepped else 0)])
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
        return (kind,)

    # the head: a step that no read precedes, and two consecutive mutations
    head = int(rng.integers(3))
    if head == 0:
        ops = [mutation("step"), mutation(room=False)]
    elif head == 1:
        ops = [mutation(("forcings", "set_field", "presf", "rhobf")[int(rng.integers(4))]), mutation("step")]
    else:
        ops = [mutation("enable" if pending else "forcings"), mutation("step")]
    while len(ops) < length - 1:
        room = len(ops) < length - 3
        if pending and length - 1 - len(ops) <= len(pending) + 1:  # a mode that is to be enabled late is, with a step behind it
            ops.append(mutation("enable"))
        elif rng.random() < 0.4:
            ops.append(observation())
        else:
            ops.append(mutation(room=room))
    last = max([i for i, op in enumerate(ops) if op[0] == "enable"], default=-1)
    if not any(_is_step(op) for op in ops[last + 1:]):
        ops[-1] = mutation("step")
        assert last < len(ops) - 1
    ops.append(("record",))
    check_sequence(ops, modes, length)
    return ops


def check_sequence(ops, modes, length=None):
    """the conditions every sequence meets, whoever made it"""
    assert length is None or len(ops) == length, (len(ops), length)
    assert ops[-1] == ("record",) and all(op[0] in KINDS for op in ops)
    first = next(i for i, op in enumerate(ops) if _is_step(op))
    assert not any(_reads(op) for op in ops[:first]), "a read precedes every step"
    assert any(a[0] in MUTATIONS and b[0] in MUTATIONS for a, b in zip(ops, ops[1:])), "no two mutations follow each other"
    late = [op[1] for op in ops if op[0] == "enable"]
    assert len(set(late)) == len(late) and set(late) <= set(LATE) & set(modes)
    last = max([i for i, op in enumerate(ops) if op[0] == "enable"], default=-1)
    assert any(_is_step(op) for op in ops[last + 1:]), "no step after the last enable"
    return late


def check_kinds(cases):
    """over the (seed, modes) of ``cases`` every kind of operation occurs"""
    seen = {op[0] for seed, modes in cases for op in generate(seed, modes)}
    assert seen == set(KINDS), sorted(set(KINDS) - seen)


# -- one operation -----------------------------------------------------------------------------------------------------------
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


def apply(ens, op, device, modes, on):
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
    if kind == "set_field":
        cur = numpy.array(host_of(ens.get_fields_batched(op[1])))
        noise = numpy.random.default_rng(op[2]).normal(0, 1e-2 if op[1] == "QT" else 1e-4, cur.shape)
        return ens.set_fields_batched(op[1], cur * (1.0 + noise))
    if kind == "presf":
        ens.p["presf"] *= 1.002
        return None
    if kind == "rhobf":
        ens.p["Rhobf"] *= 1.01
        return None
    if kind == "enable":
        enable(ens, op[1], modes, late=True)
        on.update({op[1]} | ({"vertical"} if op[1] == "advect" and "vertical" in modes else set()))
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
            rec["courant z"] = numpy.array([ens.advect_courant_z])
        return rec
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
    for i in range(n):
        for method in sorted(ROW_GETTERS):
            _row_equals_batched(ens, i, method, numpy.array(getattr(ens[i], method)()))
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


def check_launched(calls, modes):
    for mode in modes:
        assert METHOD[mode] in calls, "%s was enabled and %s never launched" % (mode, METHOD[mode])


# -- a whole sequence ----------------------------------------------------------------------------------------------------------
def _compare(key, got, want):
    if key == "W":                                                 # a torch expression: the bound of les_vadvect_ref.check_w
        assert got.shape == want.shape and numpy.isfinite(want).all() and numpy.abs(want).max() > 0
        err, bound = numpy.abs(got - want).max(), 4 * numpy.finfo(numpy.float64).eps * numpy.abs(want).max()
        assert err <= bound, "W: max abs err %.3e > %.3e" % (err, bound)
    else:
        assert_bits(key, got, want)


def replay(ops, modes, n, engine_for_twin, engine_for_device, what=""):
    """the list ``ops`` on the twin (NumPy fields; its nudge runs on ``engine_for_twin``) and on the device ensemble on
    ``engine_for_device``; every observation compared, properties (a) and (b) checked on the way.  An AssertionError names
    ``what``, the modes, the index of the operation and the operations up to it.  Returns the launches of the device side."""
    modes = tuple(m for m in MODES if m in modes)
    late = check_sequence(ops, modes)

    def told(i, side, e):
        return AssertionError("%s modes %s n %d, operation %d %r on the %s: %s\nthe operations up to it (ensemble_sequences.replay(ops, %r, %d, ...)):\n%r"
                              % (what, name_of(modes), n, i, ops[i], side, e, modes, n, list(ops[:i + 1])))
    twin, on, want = build(engine_for_twin, False, n, modes, late), set(modes) - set(late) - ({"vertical"} if "advect" in late else set()), []
    for i, op in enumerate(ops):
        try:
            want.append(apply(twin, op, False, modes, on))
        except AssertionError as e:
            raise told(i, "twin", e) from e
    assert len(want) == len(ops)
    counter = Counter(engine_for_device)
    done = 0
    try:
        ens, on = build(engine_for_device, True, n, modes, late), set(modes) - set(late) - ({"vertical"} if "advect" in late else set())
        for i, op in enumerate(ops):
            try:
                got = apply(ens, op, True, modes, on)
                assert (got is None) == (want[i] is None) and (got is None or list(got) == list(want[i])), (got and list(got), want[i] and list(want[i]))
                for k in got or ():
                    _compare(k, got[k], want[i][k])
                if got is not None:                                # property (b)
                    mark = len(counter.calls)
                    again = apply(ens, op, True, modes, on)
                    extra = set(counter.calls[mark:]) - RELAUNCH.get(op[0], set())
                    assert not extra, "(b) the second read launched %s" % sorted(extra)
                    for k in got:
                        assert_bits("(b) the second read of " + k, again[k], got[k])
            except AssertionError as e:
                raise told(i, "device ensemble", e) from e
            done += 1
    finally:
        counter.restore()
    assert done == len(ops) and ens.model_time == twin.model_time
    check_launched(counter.calls, modes)
    return counter.calls


def run(engine_for_twin, engine_for_device, seed, modes, n, length=LENGTH):
    """``generate(seed, modes)`` through ``replay``"""
    return replay(generate(seed, modes, length), modes, n, engine_for_twin, engine_for_device, what="seed %d" % seed)
