"""The host side of the column-tile kernels that have one of their own (K15, K18, K21, K25), without a GPU: every refusal of
spc_les_diffuse_*, spc_les_radiate_*, spc_les_buoyancy_* and spc_les_vmix_* up to "too many workgroups", with its return code and
the complete text of spc_last_error(), in the order the checks are made (blocks that break two rules at once pin the order), and
the no-op of an ensemble without LES after the checks of the scalars.  No pointer is dereferenced before these checks, so none
of the calls needs a device.  (K17, K22 and K23: test_les_transport_host_texts_cpu.py.)"""
import ctypes

import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi

E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
SKEW = {"f32": 2, "f64": 4}                                        # bytes off the element grid
SKEWED = 4096 * 200

# per kernel: the args struct, its pointer members, its pointer arrays with their length, other scalars, the default field
# count, and the smallest ktot of which 16 columns do not fit the LDS
KERNELS = {
    "les_diffuse": dict(cls=_abi.LesDiffuseArgs, ptrs=("a", "m", "cp", "s0"), arrays=("fields", "flux"), maxf=4, n_fields=3, scalars={},
                        levels={"f32": 2560, "f64": 1280}),
    "les_vmix": dict(cls=_abi.LesVmixArgs, ptrs=("km", "kb", "kv2", "s0", "u", "v", "speed"), arrays=("fields", "flux", "dr", "el", "eu"), maxf=6,
                     n_fields=4, scalars={}, levels={"f32": 1280, "f64": 640}),
    "les_radiate": dict(cls=_abi.LesRadiateArgs, ptrs=("ql", "thl", "w", "c", "f0", "f1", "etab", "flux", "fsfc"), arrays=(), maxf=0, n_fields=None,
                        scalars=dict(n_tab=2049, inv_step=128.0), levels={"f32": 1279, "f64": 639}),
    "les_buoyancy": dict(cls=_abi.LesBuoyancyArgs, ptrs=("thl", "qt", "ql", "u", "v", "hx", "hy", "t0", "lex", "s", "phi", "psfc", "amax"), arrays=(),
                         maxf=0, n_fields=None, scalars=dict(c1=0.608, c2=1.0), levels={"f32": 2560, "f64": 1280}),
}


def ptr(name, member, f=None):
    """the default value of pointer ``member`` (entry f of an array): distinct, 16-byte aligned, never dereferenced"""
    k = KERNELS[name]
    if f is None:
        return 4096 * (1 + k["ptrs"].index(member))
    return 4096 * (20 + 10 * k["arrays"].index(member) + f)


def block(name, n=4, itot=8, jtot=8, ktot=20, pitch_prof=None, **kw):
    k = KERNELS[name]
    a = k["cls"]()
    a.n_les, a.itot, a.jtot, a.ktot = n, itot, jtot, ktot
    a.pitch_prof = ktot if pitch_prof is None else pitch_prof
    if k["n_fields"] is not None:
        a.n_fields = kw.pop("n_fields", k["n_fields"])
    for s, v in k["scalars"].items():
        setattr(a, s, kw.pop(s, v))
    for m in k["ptrs"]:
        setattr(a, m, kw.pop(m, ptr(name, m)))
    for m in k["arrays"]:
        over = kw.pop(m, {})
        for f in range(k["maxf"]):
            getattr(a, m)[f] = over.get(f, ptr(name, m, f)) if isinstance(over, dict) else over
    assert not kw, kw
    return a


HUGE = dict(n=1 << 40, ktot=3)     # a block that passes every earlier check ends at "too many workgroups": no call reaches a device
EXTENT = "{name}: itot, jtot and ktot must be >= 1"
PITCH = "{name}: pitch_prof {v} smaller than ktot"
NULL = "required pointer {x} is NULL"
ALIGN = "{name}: a pointer is not aligned to its element type"
KTOT = "{name}: ktot {levels} above the {below} levels of which 16 columns fit the LDS"
MANY = "{name}: too many workgroups"
INPUT = "{name}: {x} is also an input (it is written while they are read)"
SAME = "{name}: {x} is the same array as another output"
COUNT = "{name}: field count {v} outside 1 ... {maxf}"
SAME_FIELD = "{name}: fields[{g}] and fields[{f}] are the same field"
NO_S0 = "{name}: flux[{f}] without s0"

# 2. the extents, the same for the four kernels
EXTENTS = [
    (dict(n=-1), E, "{name}: n_les = -1 < 0"),
    (dict(itot=0), E, EXTENT),
    (dict(jtot=-3), E, EXTENT),
    (dict(ktot=0), E, EXTENT),
    (dict(itot=65536, jtot=65536), U, "{name}: more than 2^31 - 1 points per plane"),
    (dict(n=-1, itot=0), E, "{name}: n_les = -1 < 0"),
    (dict(ktot=0, pitch_prof=-1), E, EXTENT),                                                        # extents before pitch_prof
]


def p15(m, f=None):
    return ptr("les_diffuse", m, f)


K15_ALSO = "les_diffuse: fields[{f}] is also a profile, s0 or its flux (it is written while they are read)"
DIFFUSE = EXTENTS + [
    (dict(ktot=0, n_fields=9), E, EXTENT),                                                           # extents before field count
    # 3. field count
    (dict(n_fields=0), E, COUNT.format(name="{name}", v=0, maxf=4)),
    (dict(n_fields=5), E, COUNT.format(name="{name}", v=5, maxf=4)),
    (dict(n_fields=-1, pitch_prof=19), E, COUNT.format(name="{name}", v=-1, maxf=4)),              # field count before pitch_prof
    # 4. pitch_prof
    (dict(pitch_prof=19), E, PITCH.format(name="{name}", v=19)),
    (dict(pitch_prof=-1, a=None), E, PITCH.format(name="{name}", v=-1)),                             # pitch_prof before NULL a
    # 6. the required arrays, in their order; s0 is needed only by a flux
    (dict(a=None), E, NULL.format(x="a")),
    (dict(m=None), E, NULL.format(x="m")),
    (dict(cp=None), E, NULL.format(x="cp")),
    (dict(m=None, cp=None, a=None), E, NULL.format(x="a")),
    (dict(cp=None, fields={0: None}), E, NULL.format(x="cp")),
    (dict(s0=None, flux=None, **HUGE), U, MANY),
    # 7. per field: NULL, an earlier field, what is read, a flux without s0
    (dict(fields={1: None}), E, NULL.format(x="fields[f]")),
    (dict(fields={3: None}, **HUGE), U, MANY),                                                       # (beyond n_fields = 3: not looked at)
    (dict(fields={2: p15("fields", 0)}), E, SAME_FIELD.format(name="{name}", g=0, f=2)),
    (dict(fields={2: p15("fields", 1), 1: p15("fields", 0)}), E, SAME_FIELD.format(name="{name}", g=0, f=1)),
    (dict(fields={1: p15("a")}), E, K15_ALSO.format(f=1)),
    (dict(fields={0: p15("m")}), E, K15_ALSO.format(f=0)),
    (dict(fields={2: p15("cp")}), E, K15_ALSO.format(f=2)),
    (dict(fields={1: p15("s0")}), E, K15_ALSO.format(f=1)),
    (dict(fields={1: p15("flux", 1)}), E, K15_ALSO.format(f=1)),
    (dict(fields={1: p15("flux", 0)}, **HUGE), U, MANY),                                             # (only its own flux is compared)
    (dict(fields={1: p15("fields", 0)}, flux={1: p15("fields", 0)}), E, SAME_FIELD.format(name="{name}", g=0, f=1)),   # same field before its flux
    (dict(fields={0: p15("a"), 1: None}), E, K15_ALSO.format(f=0)),                                  # field by field
    (dict(s0=None), E, NO_S0.format(name="{name}", f=0)),
    (dict(s0=None, flux={0: None}), E, NO_S0.format(name="{name}", f=1)),
    (dict(s0=None, fields={1: p15("fields", 0)}), E, NO_S0.format(name="{name}", f=0)),             # field 0 whole before field 1
    (dict(s0=None, fields={0: p15("cp")}), E, K15_ALSO.format(f=0)),                                 # what is read before the flux
    (dict(fields={0: "skew", 1: p15("m")}), E, K15_ALSO.format(f=1)),                                # aliases before alignment
    # 8. alignment
    (dict(fields={0: "skew"}), E, ALIGN),
    (dict(flux={2: "skew"}), E, ALIGN),
    (dict(a="skew"), E, ALIGN),
    (dict(s0="skew"), E, ALIGN),
    (dict(flux={3: "skew"}, **HUGE), U, MANY),                                                       # (beyond n_fields = 3)
    (dict(cp="skew", ktot="levels", pitch_prof=4000), E, ALIGN),                                     # before ktot
    # 9. unsupported ktot
    (dict(ktot="levels", pitch_prof=4000), U, KTOT),
    (dict(ktot="levels", pitch_prof=4000, n=1 << 40), U, KTOT),
    (dict(ktot=100000, pitch_prof=100000), U, KTOT.replace("{levels}", "100000")),
    # 10. too many workgroups
    (dict(**HUGE), U, MANY),
    (dict(n_fields=1, **HUGE), U, MANY),
]


def p25(m, f=None):
    return ptr("les_vmix", m, f)


K25_ALSO = "les_vmix: fields[{f}] is also km, speed, a profile, s0, a drag or a flux (it is written while they are read)"
K25_DRAG = "les_vmix: dr[{f}] without u, v and speed"
K25_SPEED = "les_vmix: speed is also an input (it is written while they are read)"
VMIX = EXTENTS + [
    (dict(ktot=0, n_fields=9), E, EXTENT),
    # 3. field count
    (dict(n_fields=0), E, COUNT.format(name="{name}", v=0, maxf=6)),
    (dict(n_fields=7), E, COUNT.format(name="{name}", v=7, maxf=6)),
    (dict(n_fields=7, pitch_prof=19), E, COUNT.format(name="{name}", v=7, maxf=6)),
    # 4. pitch_prof
    (dict(pitch_prof=19), E, PITCH.format(name="{name}", v=19)),
    (dict(pitch_prof=-1, km=None), E, PITCH.format(name="{name}", v=-1)),
    # 6. the required arrays, in their order
    (dict(km=None), E, NULL.format(x="km")),
    (dict(kb=None), E, NULL.format(x="kb")),
    (dict(kv2=None), E, NULL.format(x="kv2")),
    (dict(kv2=None, kb=None), E, NULL.format(x="kb")),
    (dict(kv2=None, fields={0: None}), E, NULL.format(x="kv2")),
    # 7. per field: fields[f], el[f], eu[f]; an earlier field; what is read; a flux without s0; a drag without the winds
    (dict(fields={1: None}), E, NULL.format(x="fields[f]")),
    (dict(el={0: None}), E, NULL.format(x="el[f]")),
    (dict(eu={2: None}), E, NULL.format(x="eu[f]")),
    (dict(fields={1: None}, el={0: None}), E, NULL.format(x="el[f]")),
    (dict(el={1: None}, eu={1: None}), E, NULL.format(x="el[f]")),
    (dict(fields={4: None}, el={5: None}, eu={4: None}, **HUGE), U, MANY),                           # (beyond n_fields = 4: not looked at)
    (dict(fields={3: p25("fields", 0)}), E, SAME_FIELD.format(name="{name}", g=0, f=3)),
    (dict(fields={1: p25("km")}), E, K25_ALSO.format(f=1)),
    (dict(fields={2: p25("speed")}), E, K25_ALSO.format(f=2)),
    (dict(fields={0: p25("kb")}), E, K25_ALSO.format(f=0)),
    (dict(fields={0: p25("kv2")}), E, K25_ALSO.format(f=0)),
    (dict(fields={1: p25("s0")}), E, K25_ALSO.format(f=1)),
    (dict(fields={1: p25("flux", 1)}), E, K25_ALSO.format(f=1)),
    (dict(fields={1: p25("flux", 3)}), E, K25_ALSO.format(f=1)),                                     # any field's flux, drag, el and eu
    (dict(fields={2: p25("dr", 0)}), E, K25_ALSO.format(f=2)),
    (dict(fields={0: p25("el", 3)}), E, K25_ALSO.format(f=0)),
    (dict(fields={3: p25("eu", 0)}), E, K25_ALSO.format(f=3)),
    (dict(fields={0: p25("el", 5)}, **HUGE), U, MANY),                                               # (el[5] is beyond n_fields = 4)
    (dict(fields={0: p25("u"), 1: p25("v")}, **HUGE), U, MANY),                                      # (the winds are mixed in place)
    (dict(fields={1: p25("fields", 0)}, flux={1: p25("fields", 0)}), E, K25_ALSO.format(f=0)),       # field 0 meets flux[1] first
    (dict(fields={1: p25("fields", 0)}, flux={1: p25("fields", 1)}), E, SAME_FIELD.format(name="{name}", g=0, f=1)),
    (dict(s0=None), E, NO_S0.format(name="{name}", f=0)),
    (dict(s0=None, flux={0: None}), E, NO_S0.format(name="{name}", f=1)),
    (dict(s0=None, flux=None, **HUGE), U, MANY),
    (dict(u=None), E, K25_DRAG.format(f=0)),
    (dict(speed=None), E, K25_DRAG.format(f=0)),
    (dict(v=None, dr={0: None}), E, K25_DRAG.format(f=1)),
    (dict(u=None, v=None, speed=None, dr=None, **HUGE), U, MANY),
    (dict(s0=None, u=None), E, NO_S0.format(name="{name}", f=0)),                                    # the flux before the drag
    (dict(u=None, fields={0: p25("kb")}), E, K25_ALSO.format(f=0)),
    (dict(u=None, fields={1: p25("kb")}), E, K25_DRAG.format(f=0)),                                  # field 0 whole before field 1
    # 8. speed, where a field has a drag
    (dict(speed=p25("u")), E, K25_SPEED),
    (dict(speed=p25("v")), E, K25_SPEED),
    (dict(speed=p25("km")), E, K25_SPEED),
    (dict(speed=p25("kb")), E, K25_SPEED),
    (dict(speed=p25("kv2")), E, K25_SPEED),
    (dict(speed=p25("s0")), E, K25_SPEED),
    (dict(speed=p25("el", 1)), E, K25_SPEED),
    (dict(speed=p25("eu", 0)), E, K25_SPEED),
    (dict(speed=p25("flux", 2)), E, K25_SPEED),
    (dict(speed=p25("dr", 3)), E, K25_SPEED),
    (dict(speed=p25("fields", 0)), E, K25_ALSO.format(f=0)),
    (dict(speed=p25("u"), dr=None, **HUGE), U, MANY),                                                # (no drag: speed is not used)
    (dict(speed=p25("u"), km="skew"), E, K25_SPEED),                                                 # aliases before alignment
    # 9. alignment
    (dict(fields={0: "skew"}), E, ALIGN),
    (dict(el={3: "skew"}), E, ALIGN),
    (dict(eu={0: "skew"}), E, ALIGN),
    (dict(dr={1: "skew"}), E, ALIGN),
    (dict(flux={1: "skew"}), E, ALIGN),
    (dict(km="skew"), E, ALIGN),
    (dict(s0="skew"), E, ALIGN),
    (dict(speed="skew"), E, ALIGN),
    (dict(u="skew"), E, ALIGN),
    (dict(u="skew", dr=None, **HUGE), U, MANY),                                                      # (no drag: u is not used)
    (dict(kb="skew", ktot="levels", pitch_prof=4000), E, ALIGN),                                     # before ktot
    # 10. unsupported ktot
    (dict(ktot="levels", pitch_prof=4000), U, KTOT + " twice"),
    (dict(ktot="levels", pitch_prof=4000, n=1 << 40), U, KTOT + " twice"),
    (dict(ktot=100000, pitch_prof=100000), U, KTOT.replace("{levels}", "100000") + " twice"),
    # 11. too many workgroups: of the speed launch where a field has a drag, else of the mixing launch
    (dict(**HUGE), U, MANY),
    (dict(dr=None, **HUGE), U, MANY),
    (dict(n_fields=1, **HUGE), U, MANY),
]


def p18(m):
    return ptr("les_radiate", m)


RADIATE = EXTENTS + [
    (dict(ktot=0, n_tab=1), E, EXTENT),                                                              # extents before the table
    # 3. the table
    (dict(n_tab=1), E, "{name}: n_tab = 1 < 2"),
    (dict(n_tab=-5), E, "{name}: n_tab = -5 < 2"),
    (dict(inv_step=0.0), E, "{name}: inv_step must be > 0"),
    (dict(inv_step=-1.0), E, "{name}: inv_step must be > 0"),
    (dict(inv_step=float("nan")), E, "{name}: inv_step must be > 0"),
    (dict(n_tab=1, inv_step=0.0), E, "{name}: n_tab = 1 < 2"),
    (dict(inv_step=0.0, pitch_prof=19), E, "{name}: inv_step must be > 0"),
    # 4. pitch_prof
    (dict(pitch_prof=19), E, PITCH.format(name="{name}", v=19)),
    (dict(pitch_prof=-1, ql=None), E, PITCH.format(name="{name}", v=-1)),
    # 6. the required arrays, in their order; flux and fsfc are optional
    (dict(ql=None), E, NULL.format(x="ql")),
    (dict(thl=None), E, NULL.format(x="thl")),
    (dict(w=None), E, NULL.format(x="w")),
    (dict(c=None), E, NULL.format(x="c")),
    (dict(f0=None), E, NULL.format(x="f0")),
    (dict(f1=None), E, NULL.format(x="f1")),
    (dict(etab=None), E, NULL.format(x="etab")),
    (dict(etab=None, c=None, f1=None), E, NULL.format(x="c")),
    (dict(flux=None, fsfc=None, **HUGE), U, MANY),
    # 7. thl, flux, fsfc, each against the inputs and then the outputs before it
    (dict(thl=p18("ql")), E, INPUT.format(name="{name}", x="thl")),
    (dict(thl=p18("w")), E, INPUT.format(name="{name}", x="thl")),
    (dict(thl=p18("c")), E, INPUT.format(name="{name}", x="thl")),
    (dict(thl=p18("f0")), E, INPUT.format(name="{name}", x="thl")),
    (dict(thl=p18("f1")), E, INPUT.format(name="{name}", x="thl")),
    (dict(thl=p18("etab")), E, INPUT.format(name="{name}", x="thl")),
    (dict(flux=p18("ql")), E, INPUT.format(name="{name}", x="flux")),
    (dict(flux=p18("etab")), E, INPUT.format(name="{name}", x="flux")),
    (dict(flux=p18("thl")), E, SAME.format(name="{name}", x="flux")),
    (dict(fsfc=p18("f0")), E, INPUT.format(name="{name}", x="fsfc")),
    (dict(fsfc=p18("thl")), E, SAME.format(name="{name}", x="fsfc")),
    (dict(fsfc=p18("flux")), E, SAME.format(name="{name}", x="fsfc")),
    (dict(fsfc=p18("thl"), flux=None), E, SAME.format(name="{name}", x="fsfc")),
    (dict(flux=p18("ql"), fsfc=p18("thl")), E, INPUT.format(name="{name}", x="flux")),               # flux before fsfc
    (dict(thl=p18("w"), flux=p18("w")), E, INPUT.format(name="{name}", x="thl")),                    # thl before flux
    (dict(flux=p18("thl"), fsfc=p18("c")), E, SAME.format(name="{name}", x="flux")),
    (dict(thl=p18("ql"), w="skew"), E, INPUT.format(name="{name}", x="thl")),                        # aliases before alignment
    # 8. alignment
    (dict(ql="skew"), E, ALIGN),
    (dict(thl="skew"), E, ALIGN),
    (dict(etab="skew"), E, ALIGN),
    (dict(f1="skew"), E, ALIGN),
    (dict(flux="skew"), E, ALIGN),
    (dict(fsfc="skew"), E, ALIGN),
    (dict(c="skew", ktot="levels", pitch_prof=4000), E, ALIGN),                                      # before ktot
    # 9. unsupported ktot
    (dict(ktot="levels", pitch_prof=4000), U, KTOT),
    (dict(ktot="levels", pitch_prof=4000, n=1 << 40), U, KTOT),
    (dict(ktot=100000, pitch_prof=100000), U, KTOT.replace("{levels}", "100000")),
    # 10. too many workgroups
    (dict(**HUGE), U, MANY),
    (dict(flux=None, **HUGE), U, MANY),
]


def p21(m):
    return ptr("les_buoyancy", m)


BUOYANCY = EXTENTS + [
    # 3. pitch_prof
    (dict(pitch_prof=19), E, PITCH.format(name="{name}", v=19)),
    (dict(pitch_prof=-1, thl=None), E, PITCH.format(name="{name}", v=-1)),
    # 5. the required arrays, in their order; ql, psfc and amax are optional
    (dict(thl=None), E, NULL.format(x="thl")),
    (dict(qt=None), E, NULL.format(x="qt")),
    (dict(u=None), E, NULL.format(x="u")),
    (dict(v=None), E, NULL.format(x="v")),
    (dict(phi=None), E, NULL.format(x="phi")),
    (dict(hx=None), E, NULL.format(x="hx")),
    (dict(hy=None), E, NULL.format(x="hy")),
    (dict(t0=None), E, NULL.format(x="t0")),
    (dict(lex=None), E, NULL.format(x="lex")),
    (dict(s=None), E, NULL.format(x="s")),
    (dict(phi=None, hx=None), E, NULL.format(x="phi")),
    (dict(u=None, qt=None, s=None), E, NULL.format(x="qt")),
    (dict(ql=None, psfc=None, amax=None, **HUGE), U, MANY),
    # 6. phi, u, v, psfc, amax, each against the inputs and then the outputs before it
    (dict(phi=p21("thl")), E, INPUT.format(name="{name}", x="phi")),
    (dict(phi=p21("qt")), E, INPUT.format(name="{name}", x="phi")),
    (dict(phi=p21("ql")), E, INPUT.format(name="{name}", x="phi")),
    (dict(phi=p21("hx")), E, INPUT.format(name="{name}", x="phi")),
    (dict(phi=p21("hy")), E, INPUT.format(name="{name}", x="phi")),
    (dict(phi=p21("t0")), E, INPUT.format(name="{name}", x="phi")),
    (dict(phi=p21("lex")), E, INPUT.format(name="{name}", x="phi")),
    (dict(phi=p21("s")), E, INPUT.format(name="{name}", x="phi")),
    (dict(u=p21("thl")), E, INPUT.format(name="{name}", x="u")),
    (dict(u=p21("phi")), E, SAME.format(name="{name}", x="u")),
    (dict(v=p21("hx")), E, INPUT.format(name="{name}", x="v")),
    (dict(v=p21("u")), E, SAME.format(name="{name}", x="v")),
    (dict(v=p21("phi")), E, SAME.format(name="{name}", x="v")),
    (dict(psfc=p21("s")), E, INPUT.format(name="{name}", x="psfc")),
    (dict(psfc=p21("phi")), E, SAME.format(name="{name}", x="psfc")),
    (dict(amax=p21("t0")), E, INPUT.format(name="{name}", x="amax")),
    (dict(amax=p21("psfc")), E, SAME.format(name="{name}", x="amax")),
    (dict(amax=p21("v")), E, SAME.format(name="{name}", x="amax")),
    (dict(amax=p21("phi"), psfc=None), E, SAME.format(name="{name}", x="amax")),
    (dict(phi=p21("thl"), u=p21("thl")), E, INPUT.format(name="{name}", x="phi")),                   # phi before u
    (dict(u=p21("phi"), v=p21("thl")), E, SAME.format(name="{name}", x="u")),                        # u before v
    (dict(psfc=p21("u"), amax=p21("qt")), E, SAME.format(name="{name}", x="psfc")),                  # psfc before amax
    (dict(phi=p21("qt"), hx="skew"), E, INPUT.format(name="{name}", x="phi")),                       # aliases before alignment
    # 7. alignment
    (dict(thl="skew"), E, ALIGN),
    (dict(ql="skew"), E, ALIGN),
    (dict(hx="skew"), E, ALIGN),
    (dict(phi="skew"), E, ALIGN),
    (dict(psfc="skew"), E, ALIGN),
    (dict(amax="skew"), E, ALIGN),
    (dict(s="skew", ktot="levels", pitch_prof=4000), E, ALIGN),                                      # before ktot
    # 8. unsupported ktot
    (dict(ktot="levels", pitch_prof=4000), U, KTOT),
    (dict(ktot="levels", pitch_prof=4000, n=1 << 40), U, KTOT),
    (dict(ktot=100000, pitch_prof=100000), U, KTOT.replace("{levels}", "100000")),
    # 9. too many workgroups
    (dict(**HUGE), U, MANY),
    (dict(ql=None, **HUGE), U, MANY),
    (dict(amax=None, **HUGE), U, MANY),
]

# the table, how many entries it has at least, and the scalars that are checked before "n_les == 0": (block, text)
TABLES = {
    "les_diffuse": (DIFFUSE, 45, [(dict(n_fields=0), COUNT.format(name="{name}", v=0, maxf=4))]),
    "les_vmix": (VMIX, 75,[(dict(n_fields=7), COUNT.format(name="{name}", v=7, maxf=6))]),
    "les_radiate": (RADIATE, 50,[(dict(n_tab=1), "{name}: n_tab = 1 < 2"), (dict(inv_step=0.0), "{name}: inv_step must be > 0")]),
    "les_buoyancy": (BUOYANCY, 50,[]),
}


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    return _abi.load_library()


def materialise(kw, name, sfx):
    """the table's placeholders: "skew" is a pointer off the element grid, "levels" the first unsupported ktot"""
    out = {}
    for k, v in kw.items():
        if isinstance(v, dict):
            v = {f: (SKEWED + SKEW[sfx] if x == "skew" else x) for f, x in v.items()}
        elif v == "skew":
            v = SKEWED + SKEW[sfx]
        elif v == "levels":
            v = KERNELS[name]["levels"][sfx]
        out[k] = v
    return out


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("name", list(KERNELS))
def test_every_refusal_has_its_code_and_text_in_order(lib, name, sfx):
    fn = getattr(lib, "spc_%s_%s" % (name, sfx))
    table, at_least, scalars = TABLES[name]
    levels = KERNELS[name]["levels"][sfx]
    assert (fn(None, None), lib.spc_last_error()) == (E, b"args is NULL")                                # 1. NULL args
    made = 0
    for kw, rc, text in table:
        want = text.format(name=name, levels=levels, below=levels - 1).encode()
        assert (fn(ctypes.byref(block(name, **materialise(kw, name, sfx))), None), lib.spc_last_error()) == (rc, want), kw
        made += 1
    assert made >= at_least
    # an empty ensemble is a no-op before any pointer is looked at, after the checks of the scalars
    k = KERNELS[name]
    nulls = dict({m: None for m in k["ptrs"]}, **{m: None for m in k["arrays"]})
    assert fn(ctypes.byref(block(name, n=0, **nulls)), None) == 0
    for kw, text in scalars + [(dict(pitch_prof=19), PITCH.format(name="{name}", v=19))]:
        assert (fn(ctypes.byref(block(name, n=0, **dict(nulls, **kw))), None), lib.spc_last_error()) == (E, text.format(name=name).encode()), kw
