"""The host side of the slab-chain kernels (K10, K11, K12, K14, K20), without a GPU: every refusal of spc_slab_means_*,
spc_les_advance_*, spc_les_thermo_*, spc_les_microphysics_* and spc_les_moments_* up to "too many workgroups", with its return
code and the complete text of spc_last_error(), in the order the checks are made (blocks that break two rules at once pin the
order), and the no-op of an ensemble without LES after the checks of the scalars.  No pointer is dereferenced before these
checks, so none of the calls needs a device.  (The column-tile kernels: test_les_column_host_texts_cpu.py.)"""
import ctypes

import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi

E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
SKEW = {"f32": 2, "f64": 4}                                        # bytes off the element grid
SKEWED = 4096 * 400

# per kernel (the name in its texts; the entry points are spc_<name>_f64 / _f32): the args struct, its pointer members, its
# pointer arrays with their length, its pitches, other scalars and the default field count
KERNELS = {
    "slab_means": dict(cls=_abi.SlabMeansArgs, ptrs=(), arrays=dict(fields=16, out=16), pitches=("pitch_out",), n_fields=3, scalars={}),
    "les_advance": dict(cls=_abi.LesAdvanceArgs, ptrs=("qsat", "ql", "ql_mean"), arrays=dict(fields=8, tend=8, mean=8),
                        pitches=("pitch_tend", "pitch_mean"), n_fields=3, scalars=dict(dt=60.0, sat_field=1)),
    "les_thermo": dict(cls=_abi.LesThermoArgs, ptrs=("thl", "qt", "presf", "ex", "es_tab", "qsat", "ql", "temp", "ql_mean", "t_mean"), arrays={},
                       pitches=("pitch_prof", "pitch_mean"), n_fields=None, scalars=dict(n_iter=6, n_tab=2000, table_mode=0, t_lo=150.0, inv_step=5.0)),
    "les_microphysics": dict(cls=_abi.LesMicroArgs, ptrs=("qt", "ql", "qr", "qr_new", "thl", "temp", "rain", "sed_out", "sed_in", "lcpex", "w",
                                                          "qt_mean", "thl_mean", "qr_mean", "qi_mean"), arrays={},
                             pitches=("pitch_prof", "pitch_mean"), n_fields=None,
                             scalars=dict(dt=60.0, qc0=1e-4, k_auto=1e-3, k_acc=2.0, t_up=268.0, t_dn=253.0)),
    "les_moments": dict(cls=_abi.LesMomentsArgs, ptrs=(), arrays=dict(fields=8, mean=8, var=8, std=8, cov=8), pitches=("pitch_out",), n_fields=3,
                        scalars=dict(face_field=-1)),
}
PAIRS = ((0, 1), (1, 2))                                          # K20's default pairs


def ptr(name, member, f=None):
    """the default value of pointer ``member`` (entry f of an array): distinct, 16-byte aligned, never dereferenced"""
    k = KERNELS[name]
    if f is None:
        return 4096 * (1 + k["ptrs"].index(member))
    return 4096 * (40 + 20 * list(k["arrays"]).index(member) + f)


def block(name, n=4, itot=8, jtot=8, ktot=20, **kw):
    k = KERNELS[name]
    a = k["cls"]()
    a.n_les, a.itot, a.jtot, a.ktot = n, itot, jtot, ktot
    for m in k["pitches"]:
        setattr(a, m, kw.pop(m, ktot))
    if k["n_fields"] is not None:
        a.n_fields = kw.pop("n_fields", k["n_fields"])
    for s, v in k["scalars"].items():
        setattr(a, s, kw.pop(s, v))
    for m in k["ptrs"]:
        setattr(a, m, kw.pop(m, ptr(name, m)))
    for m, length in k["arrays"].items():
        over = kw.pop(m, {})
        for f in range(length):
            getattr(a, m)[f] = over.get(f, ptr(name, m, f)) if isinstance(over, dict) else over
    if name == "les_moments":
        pairs = kw.pop("pairs", PAIRS)
        a.n_pairs = kw.pop("n_pairs", len(pairs))
        for q, (pa, pb) in enumerate(pairs):
            a.pair_a[q], a.pair_b[q] = pa, pb
    assert not kw, kw
    return a


HUGE = dict(n=1 << 40, ktot=3)     # a block that passes every earlier check ends at "too many workgroups": no call reaches a device
EXTENT = "{name}: itot, jtot and ktot must be >= 1"
PLANE = "{name}: more than 2^31 - 1 points per plane"
NULL = "required pointer {x} is NULL"
ALIGN = "{name}: a pointer is not aligned to its element type"
MANY = "{name}: too many workgroups"
COUNT = "{name}: field count {v} outside 1 ... {maxf}"
PITCH2 = "{name}: {a} {va} or {b} {vb} smaller than ktot"

# 2. the extents, the same for K10, K11, K12 and K14 (K20 has a check in front of them)
EXTENTS = [
    (dict(n=-1), E, "{name}: n_les = -1 < 0"),
    (dict(itot=0), E, EXTENT),
    (dict(jtot=-3), E, EXTENT),
    (dict(ktot=0), E, EXTENT),
    (dict(itot=65536, jtot=65536), U, PLANE),
    (dict(n=-1, itot=0), E, "{name}: n_les = -1 < 0"),
    (dict(itot=0, jtot=65536), E, EXTENT),
]


def p10(m, f):
    return ptr("slab_means", m, f)


K10_PITCH = "slab_means: pitch_out {v} smaller than ktot {k}"
MEANS = EXTENTS + [
    (dict(ktot=0, n_fields=17), E, EXTENT),                                                          # extents before field count
    # 3. field count
    (dict(n_fields=0), E, COUNT.format(name="{name}", v=0, maxf=16)),
    (dict(n_fields=17), E, COUNT.format(name="{name}", v=17, maxf=16)),
    (dict(n_fields=-1, pitch_out=19), E, COUNT.format(name="{name}", v=-1, maxf=16)),              # field count before pitch_out
    # 4. pitch_out
    (dict(pitch_out=19), E, K10_PITCH.format(v=19, k=20)),
    (dict(pitch_out=-1, fields=None), E, K10_PITCH.format(v=-1, k=20)),                              # pitch_out before NULL fields
    (dict(pitch_out=2, ktot=3), E, K10_PITCH.format(v=2, k=3)),
    # 6. per field: fields[f], out[f], their alignment
    (dict(fields={0: None}), E, NULL.format(x="fields[f]")),
    (dict(fields={2: None}), E, NULL.format(x="fields[f]")),
    (dict(out={1: None}), E, NULL.format(x="out[f]")),
    (dict(fields={0: None}, out={0: None}), E, NULL.format(x="fields[f]")),
    (dict(fields={1: None}, out={0: None}), E, NULL.format(x="out[f]")),                             # field by field
    (dict(fields={3: None}, out={15: None}, **HUGE), U, MANY),                                       # (beyond n_fields = 3: not looked at)
    (dict(fields={0: "skew"}), E, ALIGN),
    (dict(out={2: "skew"}), E, ALIGN),
    (dict(fields={0: "skew", 1: None}), E, ALIGN),                                                   # field 0 whole before field 1
    (dict(fields={1: "skew"}, out={0: None}), E, NULL.format(x="out[f]")),
    (dict(fields={5: "skew"}, **HUGE), U, MANY),                                                     # (beyond n_fields = 3)
    (dict(fields={1: p10("fields", 0)}, out={1: p10("out", 0), 2: p10("fields", 2)}, **HUGE), U, MANY),   # (no alias is looked for)
    # 7. too many workgroups; ktot == 1 is K10's own (k_slab_means_k1)
    (dict(**HUGE), U, MANY),
    (dict(n_fields=1, **HUGE), U, MANY),
    (dict(n=1 << 40, ktot=1), U, MANY),
    (dict(n=1 << 40, ktot=4), U, MANY),
    (dict(n=1 << 41, ktot=1, n_fields=16), U, MANY),
]


def p11(m, f=None):
    return ptr("les_advance", m, f)


K11_PITCH = PITCH2.format(name="{name}", a="pitch_tend", va="{t}", b="pitch_mean", vb="{m}")
K11_SAT = "les_advance: sat_field {v} outside -1 ... {top}"
K11_QL = "les_advance: ql is also a field or qsat (it is written while they are read)"
K11_QSAT = "les_advance: qsat is also a field (it is read while they are updated)"
K11_SAME = "les_advance: fields[{g}] and fields[{f}] are the same field"
K11_KTOT = "les_advance: ktot == 1 (numpy reduces a one-level plane pairwise: step the field and call slab_means)"
ADVANCE = EXTENTS + [
    (dict(ktot=0, n_fields=9), E, EXTENT),
    # 3. field count
    (dict(n_fields=0), E, COUNT.format(name="{name}", v=0, maxf=8)),
    (dict(n_fields=9), E, COUNT.format(name="{name}", v=9, maxf=8)),
    (dict(n_fields=9, pitch_tend=19), E, COUNT.format(name="{name}", v=9, maxf=8)),
    # 4. the pitches
    (dict(pitch_tend=19), E, K11_PITCH.format(name="{name}", t=19, m=20)),
    (dict(pitch_mean=-1), E, K11_PITCH.format(name="{name}", t=20, m=-1)),
    (dict(pitch_mean=19, sat_field=3), E, K11_PITCH.format(name="{name}", t=20, m=19)),             # pitches before sat_field
    # 5. sat_field
    (dict(sat_field=3), E, K11_SAT.format(v=3, top=2)),
    (dict(sat_field=-2), E, K11_SAT.format(v=-2, top=2)),
    (dict(sat_field=1, n_fields=1), E, K11_SAT.format(v=1, top=0)),
    (dict(sat_field=8, n_fields=8, qsat=None), E, K11_SAT.format(v=8, top=7)),                       # sat_field before NULL qsat
    # 7. qsat, where a field is saturated
    (dict(qsat=None), E, NULL.format(x="qsat")),
    (dict(qsat=None, fields={0: None}), E, NULL.format(x="qsat")),
    (dict(qsat=None, ql="skew", ql_mean="skew", sat_field=-1, **HUGE), U, MANY),                    # (no saturation: none of the three is used)
    # 8. per field: NULL, ql against it and qsat, qsat against it, an earlier field
    (dict(fields={0: None}), E, NULL.format(x="fields[f]")),
    (dict(fields={2: None}), E, NULL.format(x="fields[f]")),
    (dict(fields={3: None}, **HUGE), U, MANY),                                                       # (beyond n_fields = 3: not looked at)
    (dict(tend=None, mean=None, ql=None, ql_mean=None, **HUGE), U, MANY),                           # (all optional)
    (dict(ql=p11("fields", 0)), E, K11_QL),
    (dict(ql=p11("fields", 2)), E, K11_QL),
    (dict(ql=p11("qsat")), E, K11_QL),
    (dict(ql=p11("qsat"), fields={1: None}), E, K11_QL),                                             # ql against qsat with field 0
    (dict(ql=p11("fields", 1), fields={0: None}), E, NULL.format(x="fields[f]")),                    # field by field
    (dict(ql=p11("fields", 3), **HUGE), U, MANY),
    (dict(ql=p11("fields", 0), sat_field=-1, **HUGE), U, MANY),
    (dict(qsat=p11("fields", 1)), E, K11_QSAT),
    (dict(qsat=p11("fields", 1), ql=p11("fields", 2)), E, K11_QSAT),                                 # field 1 whole before field 2
    (dict(qsat=p11("fields", 1), ql=p11("fields", 1)), E, K11_QL),                                   # ql before qsat
    (dict(qsat=p11("fields", 0), sat_field=-1, **HUGE), U, MANY),
    (dict(fields={2: p11("fields", 0)}), E, K11_SAME.format(g=0, f=2)),
    (dict(fields={2: p11("fields", 1), 1: p11("fields", 0)}), E, K11_SAME.format(g=0, f=1)),
    (dict(fields={1: p11("fields", 0)}, qsat=p11("fields", 0)), E, K11_QSAT),                        # qsat before an earlier field
    (dict(fields={1: p11("fields", 0)}, qsat=p11("fields", 2)), E, K11_SAME.format(g=0, f=1)),
    (dict(mean={0: p11("fields", 0)}, tend={1: p11("fields", 2)}, ql_mean=p11("ql"), **HUGE), U, MANY),   # (no other alias is looked for)
    (dict(fields={0: "skew"}, ql=p11("fields", 1)), E, K11_QL),                                      # aliases before alignment
    (dict(tend={0: "skew"}, fields={2: p11("fields", 1)}), E, K11_SAME.format(g=1, f=2)),
    # 9. alignment
    (dict(fields={1: "skew"}), E, ALIGN),
    (dict(tend={0: "skew"}), E, ALIGN),
    (dict(mean={2: "skew"}), E, ALIGN),
    (dict(qsat="skew"), E, ALIGN),
    (dict(ql="skew"), E, ALIGN),
    (dict(ql_mean="skew"), E, ALIGN),
    (dict(mean={3: "skew"}, **HUGE), U, MANY),                                                       # (beyond n_fields = 3)
    (dict(tend={1: "skew"}, ktot=1), E, ALIGN),                                                      # before ktot == 1
    # 10. ktot == 1
    (dict(ktot=1), U, K11_KTOT),
    (dict(ktot=1, n=1 << 40), U, K11_KTOT),
    (dict(ktot=1, sat_field=-1), U, K11_KTOT),
    # 11. too many workgroups
    (dict(**HUGE), U, MANY),
    (dict(n=1 << 40, ktot=4), U, MANY),
    (dict(n_fields=1, sat_field=0, **HUGE), U, MANY),
]


def p12(m):
    return ptr("les_thermo", m)


K12_PITCH = PITCH2.format(name="{name}", a="pitch_prof", va="{p}", b="pitch_mean", vb="{m}")
K12_INPUT = "les_thermo: an output is also an input (thl, qt, presf, ex and es_tab are read while it is written)"
K12_SAME = "les_thermo: two outputs are the same array"
K12_KTOT = "les_thermo: ktot == 1 (numpy reduces a one-level plane pairwise; as in les_advance)"
THERMO = EXTENTS + [
    (dict(ktot=0, pitch_prof=-1), E, EXTENT),                                                        # extents before the pitches
    # 3. the pitches
    (dict(pitch_prof=19), E, K12_PITCH.format(name="{name}", p=19, m=20)),
    (dict(pitch_mean=-1), E, K12_PITCH.format(name="{name}", p=20, m=-1)),
    (dict(pitch_mean=19, n_tab=1), E, K12_PITCH.format(name="{name}", p=20, m=19)),                 # pitches before the table
    # 4. n_tab, n_iter, table_mode, inv_step
    (dict(n_tab=1), E, "{name}: n_tab = 1 < 2"),
    (dict(n_tab=-5), E, "{name}: n_tab = -5 < 2"),
    (dict(n_iter=-1), E, "{name}: n_iter = -1 < 0"),
    (dict(table_mode=-1), E, "{name}: table_mode -1 outside 0 ... 2"),
    (dict(table_mode=3), E, "{name}: table_mode 3 outside 0 ... 2"),
    (dict(inv_step=0.0), E, "{name}: inv_step must be > 0"),
    (dict(inv_step=-1.0), E, "{name}: inv_step must be > 0"),
    (dict(inv_step=float("nan")), E, "{name}: inv_step must be > 0"),
    (dict(n_tab=1, n_iter=-1), E, "{name}: n_tab = 1 < 2"),
    (dict(n_iter=-1, table_mode=3), E, "{name}: n_iter = -1 < 0"),
    (dict(table_mode=3, inv_step=0.0), E, "{name}: table_mode 3 outside 0 ... 2"),
    (dict(inv_step=0.0, thl=None), E, "{name}: inv_step must be > 0"),                               # the scalars before NULL thl
    (dict(n_iter=0, table_mode=1, **HUGE), U, MANY),
    (dict(table_mode=2, **HUGE), U, MANY),
    # 6. the required arrays, in their order; temp and the means are optional
    (dict(thl=None), E, NULL.format(x="thl")),
    (dict(qt=None), E, NULL.format(x="qt")),
    (dict(presf=None), E, NULL.format(x="presf")),
    (dict(ex=None), E, NULL.format(x="ex")),
    (dict(es_tab=None), E, NULL.format(x="es_tab")),
    (dict(qsat=None), E, NULL.format(x="qsat")),
    (dict(ql=None), E, NULL.format(x="ql")),
    (dict(ql=None, ex=None, qsat=None), E, NULL.format(x="ex")),
    (dict(temp=None, ql_mean=None, t_mean=None, **HUGE), U, MANY),
    (dict(ql=None, qsat=p12("thl")), E, NULL.format(x="ql")),                                        # NULL before aliases
    # 7. qsat, ql, temp, ql_mean, t_mean, each against the inputs and then the outputs before it
    (dict(qsat=p12("thl")), E, K12_INPUT),
    (dict(qsat=p12("es_tab")), E, K12_INPUT),
    (dict(ql=p12("qt")), E, K12_INPUT),
    (dict(temp=p12("presf")), E, K12_INPUT),
    (dict(ql_mean=p12("ex")), E, K12_INPUT),
    (dict(t_mean=p12("thl")), E, K12_INPUT),
    (dict(ql=p12("qsat")), E, K12_SAME),
    (dict(temp=p12("ql")), E, K12_SAME),
    (dict(ql_mean=p12("qsat")), E, K12_SAME),
    (dict(t_mean=p12("ql_mean")), E, K12_SAME),
    (dict(t_mean=p12("temp")), E, K12_SAME),
    (dict(t_mean=p12("temp"), temp=None, **HUGE), U, MANY),                                          # (a NULL output is no array)
    (dict(ql=p12("qsat"), temp=p12("thl")), E, K12_SAME),                                            # ql whole before temp
    (dict(ql=p12("qt"), qsat=p12("ql")), E, K12_INPUT),
    (dict(temp=p12("qsat"), ql=p12("ex")), E, K12_INPUT),
    (dict(t_mean=p12("qt"), ql_mean=p12("ql")), E, K12_SAME),                                        # ql_mean before t_mean
    (dict(ql=p12("qsat"), thl="skew"), E, K12_SAME),                                                 # aliases before alignment
    # 8. alignment
    (dict(thl="skew"), E, ALIGN),
    (dict(ex="skew"), E, ALIGN),
    (dict(es_tab="skew"), E, ALIGN),
    (dict(ql="skew"), E, ALIGN),
    (dict(temp="skew"), E, ALIGN),
    (dict(t_mean="skew"), E, ALIGN),
    (dict(presf="skew", ktot=1), E, ALIGN),                                                          # before ktot == 1
    # 9. ktot == 1
    (dict(ktot=1), U, K12_KTOT),
    (dict(ktot=1, n=1 << 40), U, K12_KTOT),
    # 10. too many workgroups
    (dict(**HUGE), U, MANY),
    (dict(n=1 << 40, ktot=4), U, MANY),
    (dict(temp=None, **HUGE), U, MANY),
]


def p14(m):
    return ptr("les_microphysics", m)


K14_INPUT = "les_microphysics: a written array is also an input (qr_new must not be qr: the level below reads the old qr)"
K14_SAME = "les_microphysics: two written arrays are the same array"
K14_KTOT = "les_microphysics: ktot == 1 (numpy reduces a one-level plane pairwise; as in les_advance)"
K14_THL = "les_microphysics: thl_mean without thl"
K14_QI = "les_microphysics: qi_mean without temp (the cloud ice needs the temperature)"
NO_THL = dict(thl=None, thl_mean=None)
NO_TEMP = dict(temp=None, qi_mean=None)
MICRO = EXTENTS + [
    (dict(ktot=0, pitch_prof=-1), E, EXTENT),
    # 3. the pitches
    (dict(pitch_prof=19), E, K12_PITCH.format(name="{name}", p=19, m=20)),
    (dict(pitch_mean=-1), E, K12_PITCH.format(name="{name}", p=20, m=-1)),
    (dict(pitch_mean=19, qt=None), E, K12_PITCH.format(name="{name}", p=20, m=19)),                 # pitches before NULL qt
    # 5. the required arrays, in their order, then what an optional array needs
    (dict(qt=None), E, NULL.format(x="qt")),
    (dict(ql=None), E, NULL.format(x="ql")),
    (dict(qr=None), E, NULL.format(x="qr")),
    (dict(qr_new=None), E, NULL.format(x="qr_new")),
    (dict(sed_out=None), E, NULL.format(x="sed_out")),
    (dict(sed_in=None), E, NULL.format(x="sed_in")),
    (dict(lcpex=None), E, NULL.format(x="lcpex (thl is given)")),
    (dict(w=None), E, NULL.format(x="w (rain is given)")),
    (dict(thl=None), E, K14_THL),
    (dict(temp=None), E, K14_QI),
    (dict(sed_in=None, qr=None, lcpex=None), E, NULL.format(x="qr")),
    (dict(lcpex=None, w=None), E, NULL.format(x="lcpex (thl is given)")),
    (dict(w=None, thl=None), E, NULL.format(x="w (rain is given)")),
    (dict(thl=None, temp=None), E, K14_THL),
    (dict(temp=None, qr_new=p14("qr")), E, K14_QI),                                                  # before the aliases
    (dict(lcpex=None, **NO_THL, **HUGE), U, MANY),
    (dict(w=None, rain=None, **HUGE), U, MANY),
    (dict(qt_mean=None, thl_mean=None, qr_mean=None, qi_mean=None, temp=None, **HUGE), U, MANY),
    # 6. qr_new, qt, thl, rain and the four means, each against the inputs and then the written arrays before it
    (dict(qr_new=p14("qr")), E, K14_INPUT),
    (dict(qr_new=p14("ql")), E, K14_INPUT),
    (dict(qt=p14("temp")), E, K14_INPUT),
    (dict(thl=p14("sed_out")), E, K14_INPUT),
    (dict(rain=p14("sed_in")), E, K14_INPUT),
    (dict(qt_mean=p14("lcpex")), E, K14_INPUT),
    (dict(qi_mean=p14("w")), E, K14_INPUT),
    (dict(qt=p14("lcpex"), **NO_THL, **HUGE), U, MANY),                                              # (without thl, lcpex is not read)
    (dict(qr_mean=p14("w"), rain=None, **HUGE), U, MANY),                                            # (without rain, w is not read)
    (dict(qt=p14("qr_new")), E, K14_SAME),
    (dict(thl=p14("qt")), E, K14_SAME),
    (dict(rain=p14("thl")), E, K14_SAME),
    (dict(qt_mean=p14("rain")), E, K14_SAME),
    (dict(thl_mean=p14("qt_mean")), E, K14_SAME),
    (dict(qr_mean=p14("qr_new")), E, K14_SAME),
    (dict(qi_mean=p14("qr_mean")), E, K14_SAME),
    (dict(qt_mean=p14("rain"), rain=None, **HUGE), U, MANY),                                         # (a NULL array is no array)
    (dict(qt=p14("qr_new"), thl=p14("ql")), E, K14_SAME),                                            # qt whole before thl
    (dict(qt=p14("qr"), qr_new=p14("qt")), E, K14_INPUT),
    (dict(rain=p14("qt"), thl=p14("temp")), E, K14_INPUT),                                           # thl before rain
    (dict(qi_mean=p14("ql"), qr_mean=p14("qt_mean")), E, K14_SAME),                                  # qr_mean before qi_mean
    (dict(qt=p14("qr_new"), ql="skew"), E, K14_SAME),                                                # aliases before alignment
    # 7. alignment
    (dict(qt="skew"), E, ALIGN),
    (dict(qr="skew"), E, ALIGN),
    (dict(temp="skew"), E, ALIGN),
    (dict(sed_in="skew"), E, ALIGN),
    (dict(lcpex="skew"), E, ALIGN),
    (dict(w="skew"), E, ALIGN),
    (dict(rain="skew"), E, ALIGN),
    (dict(qr_new="skew"), E, ALIGN),
    (dict(qi_mean="skew"), E, ALIGN),
    (dict(lcpex="skew", **NO_THL, **HUGE), U, MANY),                                                 # (without thl, lcpex is not looked at)
    (dict(sed_out="skew", ktot=1), E, ALIGN),                                                        # before ktot == 1
    # 8. ktot == 1
    (dict(ktot=1), U, K14_KTOT),
    (dict(ktot=1, n=1 << 40), U, K14_KTOT),
    # 9. too many workgroups
    (dict(**HUGE), U, MANY),
    (dict(n=1 << 40, ktot=4), U, MANY),
    (dict(**NO_THL, **NO_TEMP, rain=None, **HUGE), U, MANY),
]


def p20(m, f):
    return ptr("les_moments", m, f)


K20_PLANE = "les_moments: more than 2^24 points per plane (their number is not exact in float)"
K20_KTOT = "les_moments: ktot == 1 (numpy reduces a plane of one level pairwise, not in this order)"
K20_PAIRS = "les_moments: pair count {v} outside 0 ... 8"
K20_FACE = "les_moments: face_field {v} is neither -1 nor a field index"
K20_PITCH = "les_moments: pitch_out {v} smaller than ktot"
K20_PAIR = "les_moments: pair {q} is not two different field indices"
K20_NONE = "les_moments: no output asked for"
K20_SAME = "les_moments: an output is the same array as a field or as another output"
NO_OUT = dict(mean=None, var=None, std=None, cov=None)
MOMENTS = [
    # 2. the plane of at most 2^24 points, ahead of the extents
    (dict(itot=4097, jtot=4096), E, K20_PLANE),
    (dict(itot=65536, jtot=65536), E, K20_PLANE),                                                    # (not the 2^31 - 1 of the extents)
    (dict(itot=4097, jtot=4096, n=-1), E, K20_PLANE),
    (dict(itot=4097, jtot=4096, ktot=0), E, K20_PLANE),
    (dict(itot=4096, jtot=4096, **HUGE), U, MANY),                                                   # (2^24 itself is carried)
    # 3. the extents
    (dict(n=-1), E, "{name}: n_les = -1 < 0"),
    (dict(itot=0), E, EXTENT),
    (dict(jtot=-3), E, EXTENT),
    (dict(ktot=0), E, EXTENT),
    (dict(itot=0, jtot=1 << 30), E, EXTENT),
    (dict(n=-1, ktot=1), E, "{name}: n_les = -1 < 0"),
    # 4. ktot == 1, before everything of the fields
    (dict(ktot=1), U, K20_KTOT),
    (dict(ktot=1, n_fields=0), U, K20_KTOT),
    (dict(ktot=1, fields={0: "skew"}), U, K20_KTOT),
    (dict(ktot=1, n=0), U, K20_KTOT),
    # 5. the counts, face_field, pitch_out, the pairs
    (dict(n_fields=0), E, COUNT.format(name="{name}", v=0, maxf=8)),
    (dict(n_fields=9), E, COUNT.format(name="{name}", v=9, maxf=8)),
    (dict(n_fields=9, n_pairs=9), E, COUNT.format(name="{name}", v=9, maxf=8)),
    (dict(n_pairs=-1), E, K20_PAIRS.format(v=-1)),
    (dict(n_pairs=9), E, K20_PAIRS.format(v=9)),
    (dict(n_pairs=9, face_field=3), E, K20_PAIRS.format(v=9)),
    (dict(face_field=3), E, K20_FACE.format(v=3)),
    (dict(face_field=-2), E, K20_FACE.format(v=-2)),
    (dict(face_field=3, pitch_out=19), E, K20_FACE.format(v=3)),
    (dict(face_field=2, **HUGE), U, MANY),
    (dict(pitch_out=19), E, K20_PITCH.format(v=19)),
    (dict(pitch_out=-1, pairs=((0, 0),)), E, K20_PITCH.format(v=-1)),
    (dict(pairs=((0, 0),)), E, K20_PAIR.format(q=0)),
    (dict(pairs=((0, 1), (1, 3))), E, K20_PAIR.format(q=1)),
    (dict(pairs=((0, 1), (-1, 2))), E, K20_PAIR.format(q=1)),
    (dict(pairs=((2, 3), (1, 1))), E, K20_PAIR.format(q=0)),
    (dict(pairs=((0, 1), (1, 1)), n_pairs=1, **HUGE), U, MANY),                                      # (beyond n_pairs: not looked at)
    (dict(pairs=((1, 1),), **NO_OUT), E, K20_PAIR.format(q=0)),                                      # the pairs before "no output"
    (dict(pairs=(), **HUGE), U, MANY),
    # 7. no output; the fields; an output against the fields and the outputs before it
    (dict(**NO_OUT), E, K20_NONE),
    (dict(fields=None, **NO_OUT), E, K20_NONE),                                                      # before NULL fields
    (dict(mean={0: None, 1: None, 2: None}, var=None, std=None, cov={0: None, 1: None}), E, K20_NONE),   # (beyond the counts: not looked at)
    (dict(fields={0: None}), E, NULL.format(x="fields[f]")),
    (dict(fields={2: None}), E, NULL.format(x="fields[f]")),
    (dict(fields={3: None}, **HUGE), U, MANY),
    (dict(fields={1: None}, mean={0: p20("fields", 0)}), E, NULL.format(x="fields[f]")),             # NULL before aliases
    (dict(mean={0: p20("fields", 0)}), E, K20_SAME),
    (dict(std={2: p20("fields", 1)}), E, K20_SAME),
    (dict(cov={1: p20("fields", 2)}), E, K20_SAME),
    (dict(var={0: p20("mean", 0)}), E, K20_SAME),
    (dict(std={1: p20("var", 0)}), E, K20_SAME),
    (dict(cov={0: p20("std", 2)}), E, K20_SAME),
    (dict(cov={1: p20("cov", 0)}), E, K20_SAME),
    (dict(fields={1: p20("fields", 0)}, **HUGE), U, MANY),                                           # (a field may be given twice)
    (dict(cov={2: p20("cov", 0)}, mean={3: p20("fields", 0)}, **HUGE), U, MANY),                     # (beyond the counts)
    (dict(mean={0: p20("fields", 0)}, fields={2: "skew"}), E, K20_SAME),                             # aliases before alignment
    # 8. alignment
    (dict(fields={0: "skew"}), E, ALIGN),
    (dict(mean={1: "skew"}), E, ALIGN),
    (dict(var={2: "skew"}), E, ALIGN),
    (dict(std={0: "skew"}), E, ALIGN),
    (dict(cov={1: "skew"}), E, ALIGN),
    (dict(cov={2: "skew"}, std={3: "skew"}, **HUGE), U, MANY),
    # 9. too many workgroups
    (dict(**HUGE), U, MANY),
    (dict(n=1 << 40, ktot=4), U, MANY),
    (dict(mean=None, var=None, std=None, **HUGE), U, MANY),
    (dict(cov=None, n_fields=1, pairs=(), **HUGE), U, MANY),
]

# the table, how many entries it has at least, and the scalars that are checked before "n_les == 0": (block, text)
TABLES = {
    "slab_means": (MEANS, 30, [(dict(n_fields=0), COUNT.format(name="{name}", v=0, maxf=16)), (dict(pitch_out=19), K10_PITCH.format(v=19, k=20))]),
    "les_advance": (ADVANCE, 55, [(dict(n_fields=9), COUNT.format(name="{name}", v=9, maxf=8)),
                                  (dict(pitch_tend=19), K11_PITCH.format(name="{name}", t=19, m=20)), (dict(sat_field=3), K11_SAT.format(v=3, top=2))]),
    "les_thermo": (THERMO, 60, [(dict(pitch_mean=19), K12_PITCH.format(name="{name}", p=20, m=19)), (dict(n_tab=1), "{name}: n_tab = 1 < 2"),
                                (dict(n_iter=-1), "{name}: n_iter = -1 < 0"), (dict(table_mode=3), "{name}: table_mode 3 outside 0 ... 2"),
                                (dict(inv_step=0.0), "{name}: inv_step must be > 0")]),
    "les_microphysics": (MICRO, 65, [(dict(pitch_prof=19), K12_PITCH.format(name="{name}", p=19, m=20))]),
    "les_moments": (MOMENTS, 60, [(dict(itot=4097, jtot=4096), K20_PLANE), (dict(n_fields=0), COUNT.format(name="{name}", v=0, maxf=8)),
                                  (dict(n_pairs=9), K20_PAIRS.format(v=9)), (dict(face_field=3), K20_FACE.format(v=3)),
                                  (dict(pitch_out=19), K20_PITCH.format(v=19)), (dict(pairs=((0, 0),)), K20_PAIR.format(q=0))]),
}


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    return _abi.load_library()


def materialise(kw, sfx):
    """the table's placeholder: "skew" is a pointer off the element grid"""
    out = {}
    for k, v in kw.items():
        if isinstance(v, dict):
            v = {f: (SKEWED + SKEW[sfx] if x == "skew" else x) for f, x in v.items()}
        elif isinstance(v, str) and v == "skew":
            v = SKEWED + SKEW[sfx]
        out[k] = v
    return out


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("name", list(KERNELS))
def test_every_refusal_has_its_code_and_text_in_order(lib, name, sfx):
    fn = getattr(lib, "spc_%s_%s" % (name, sfx))
    table, at_least, scalars = TABLES[name]
    assert (fn(None, None), lib.spc_last_error()) == (E, b"args is NULL")                                # 1. NULL args
    made = 0
    for kw, rc, text in table:
        want = text.format(name=name).encode()
        assert (fn(ctypes.byref(block(name, **materialise(kw, sfx))), None), lib.spc_last_error()) == (rc, want), kw
        made += 1
    assert made >= at_least
    # an empty ensemble is a no-op before any pointer is looked at, after the checks of the scalars
    k = KERNELS[name]
    nulls = dict({m: None for m in k["ptrs"]}, **{m: None for m in k["arrays"]})
    assert fn(ctypes.byref(block(name, n=0, **nulls)), None) == 0
    for kw, text in scalars:
        assert (fn(ctypes.byref(block(name, n=0, **dict(nulls, **kw))), None), lib.spc_last_error()) == (E, text.format(name=name).encode()), kw
