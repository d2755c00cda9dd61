"""The host side that K17, K22 and K23 share, without a GPU: every refusal of spc_les_vadvect_*, spc_les_transport_* and
spc_les_transport2_* up to "too many workgroups", with its return code and the complete text of spc_last_error(), in the order
the checks are made (blocks that break two rules at once pin the order).  No pointer is dereferenced before these checks, so
none of the calls needs a device."""
import ctypes

import pytest

import __graft_entry__ as ge
from sp_coupler_amd import _abi

E, U = _abi.SPC_ERR_INVALID_ARGUMENT, _abi.SPC_ERR_UNSUPPORTED
KERNELS = {"les_vadvect": _abi.LesVadvectArgs, "les_transport": _abi.LesTransportArgs, "les_transport2": _abi.LesTransport2Args}
PTRS = ("u", "v", "hx", "hy", "cmax", "g", "r", "mtop", "ftop")
P = {k: 4096 * (i + 1) for i, k in enumerate(PTRS)}               # distinct, 16-byte aligned, never dereferenced
FIELD0, OUT0 = 4096 * 10, 4096 * 20                                # fields[f] = FIELD0 + 4096 f, out[f] = OUT0 + 4096 f
LEVELS = {"f32": 2560, "f64": 1280}                                # the smallest ktot of which 16 columns do not fit the LDS
SKEW = {"f32": 2, "f64": 4}                                        # bytes off the element grid


@pytest.fixture(scope="module")
def lib():
    ge.build_hip()
    return _abi.load_library()


def block(cls, n=4, itot=8, jtot=8, ktot=20, n_fields=4, pitch_prof=None, limiter=1, fields=None, out=None, **ptrs):
    a = cls()
    a.n_les, a.itot, a.jtot, a.ktot, a.n_fields = n, itot, jtot, ktot, n_fields
    a.pitch_prof = ktot if pitch_prof is None else pitch_prof
    if hasattr(a, "limiter"):
        a.limiter = limiter
    for k in PTRS:
        if hasattr(a, k):
            setattr(a, k, ptrs.get(k, P[k]))
    for f in range(6):
        a.fields[f] = (fields or {}).get(f, FIELD0 + 4096 * f)
        a.out[f] = (out or {}).get(f, OUT0 + 4096 * f)
    return a


NOTHING = "{name}: no field, no cmax and no mtop: nothing to do"
SAME = "{name}: {x} is the same array as another output"
INPUT = "{name}: {x} is also an input (it is written while they are read)"
OUT_INPUT = "{name}: out[{f}] is also an input (every cell reads its neighbours' old values)"
HUGE = dict(n=1 << 40, ktot=3)     # a block that passes every earlier check ends at "too many workgroups": no call reaches a device
LIMITER = "les_transport2: limiter {v} is neither SPC_LIMITER_NONE nor SPC_LIMITER_MC"

# (the argument block, which kernels it is for (None: all three), the return code, the text); {name}: the kernel's, {levels}: LEVELS
TABLE = [
    # 2. extents
    (dict(n=-1), None, E, "{name}: n_les = -1 < 0"),
    (dict(itot=0), None, E, "{name}: itot, jtot and ktot must be >= 1"),
    (dict(jtot=-3), None, E, "{name}: itot, jtot and ktot must be >= 1"),
    (dict(ktot=0), None, E, "{name}: itot, jtot and ktot must be >= 1"),
    (dict(itot=65536, jtot=65536), None, U, "{name}: more than 2^31 - 1 points per plane"),
    (dict(n=-1, itot=0), None, E, "{name}: n_les = -1 < 0"),
    (dict(ktot=0, n_fields=7), None, E, "{name}: itot, jtot and ktot must be >= 1"),                 # extent before field count
    # 3. field count
    (dict(n_fields=7), None, E, "{name}: field count 7 outside 0 ... 6"),
    (dict(n_fields=-1), None, E, "{name}: field count -1 outside 0 ... 6"),
    (dict(n_fields=7, limiter=2), None, E, "{name}: field count 7 outside 0 ... 6"),
    # 4. K23's limiter
    (dict(limiter=2), ("les_transport2",), E, LIMITER.format(v=2)),
    (dict(limiter=-1), ("les_transport2",), E, LIMITER.format(v=-1)),
    (dict(limiter=1 << 20, n_fields=0), ("les_transport2",), E, LIMITER.format(v=1 << 20)),
    (dict(limiter=2, n_fields=0, cmax=None, mtop=None), ("les_transport2",), E, LIMITER.format(v=2)),  # limiter before nothing to do
    (dict(limiter=2, n_fields=0, cmax=None, mtop=None), ("les_vadvect", "les_transport"), E, NOTHING),
    # 5. nothing to do
    (dict(n_fields=0, cmax=None, mtop=None), None, E, NOTHING),
    (dict(n_fields=0, cmax=None, mtop=None, ftop=None), None, E, NOTHING),
    (dict(n_fields=0, cmax=None, mtop=None, pitch_prof=19), None, E, NOTHING),
    # 6. pitch_prof
    (dict(pitch_prof=19), None, E, "{name}: pitch_prof 19 smaller than ktot"),
    (dict(pitch_prof=-1, u=None), None, E, "{name}: pitch_prof -1 smaller than ktot"),                # pitch_prof before NULL u
    # 8. the required arrays, in their order
    (dict(u=None), None, E, "required pointer u is NULL"),
    (dict(v=None), None, E, "required pointer v is NULL"),
    (dict(hx=None), None, E, "required pointer hx is NULL"),
    (dict(hy=None), None, E, "required pointer hy is NULL"),
    (dict(g=None), None, E, "required pointer g is NULL"),
    (dict(r=None), None, E, "required pointer r is NULL"),
    (dict(v=None, r=None, hx=None), None, E, "required pointer v is NULL"),
    (dict(r=None, fields={0: None}), None, E, "required pointer r is NULL"),
    # 9. per field, fields[f] then out[f]
    (dict(fields={1: None}), None, E, "required pointer fields[f] is NULL"),
    (dict(out={3: None}), None, E, "required pointer out[f] is NULL"),
    (dict(fields={1: None}, out={1: None}), None, E, "required pointer fields[f] is NULL"),
    (dict(fields={2: None}, out={1: None}), None, E, "required pointer out[f] is NULL"),
    (dict(fields={5: None}, out={4: None}, **HUGE), None, U, "{name}: too many workgroups"),            # (beyond n_fields = 4: not looked at)
    (dict(out={3: None}, mtop=P["u"]), None, E, "required pointer out[f] is NULL"),
    # 10. out[f] against earlier outputs, then against inputs
    (dict(out={3: OUT0}), None, E, "{name}: out[0] and out[3] are the same array"),
    (dict(out={2: OUT0 + 4096, 3: OUT0}), None, E, "{name}: out[1] and out[2] are the same array"),
    (dict(out={2: P["u"]}), None, E, OUT_INPUT.format(name="{name}", f=2)),
    (dict(out={0: P["r"]}), None, E, OUT_INPUT.format(name="{name}", f=0)),
    (dict(out={1: P["hx"]}), None, E, OUT_INPUT.format(name="{name}", f=1)),
    (dict(out={3: FIELD0 + 4096}), None, E, OUT_INPUT.format(name="{name}", f=3)),
    (dict(out={1: FIELD0, 2: FIELD0}), None, E, OUT_INPUT.format(name="{name}", f=1)),               # an input and another out
    (dict(out={3: OUT0, 1: P["v"]}), None, E, OUT_INPUT.format(name="{name}", f=1)),
    (dict(out={3: OUT0, 2: OUT0}), None, E, "{name}: out[0] and out[2] are the same array"),
    (dict(out={1: FIELD0 + 4096 * 5}, **HUGE), None, U, "{name}: too many workgroups"),               # (fields[5] is beyond n_fields = 4)
    # 11. mtop, cmax, ftop, each against outputs and then inputs
    (dict(mtop=OUT0), None, E, SAME.format(name="{name}", x="mtop")),
    (dict(mtop=P["u"]), None, E, INPUT.format(name="{name}", x="mtop")),
    (dict(mtop=FIELD0 + 4096 * 3), None, E, INPUT.format(name="{name}", x="mtop")),
    (dict(cmax=OUT0 + 4096 * 3), None, E, SAME.format(name="{name}", x="cmax")),
    (dict(cmax=P["mtop"]), None, E, SAME.format(name="{name}", x="cmax")),
    (dict(cmax=P["hy"]), None, E, INPUT.format(name="{name}", x="cmax")),
    (dict(mtop=P["u"], cmax=P["u"]), None, E, INPUT.format(name="{name}", x="mtop")),                 # mtop is cmax and an input
    (dict(mtop=OUT0, cmax=OUT0), None, E, SAME.format(name="{name}", x="mtop")),
    (dict(ftop=OUT0 + 4096), ("les_transport", "les_transport2"), E, SAME.format(name="{name}", x="ftop")),
    (dict(ftop=P["mtop"]), ("les_transport", "les_transport2"), E, SAME.format(name="{name}", x="ftop")),
    (dict(ftop=P["cmax"]), ("les_transport", "les_transport2"), E, SAME.format(name="{name}", x="ftop")),
    (dict(ftop=P["g"]), ("les_transport", "les_transport2"), E, INPUT.format(name="{name}", x="ftop")),
    (dict(ftop=FIELD0), ("les_transport", "les_transport2"), E, INPUT.format(name="{name}", x="ftop")),
    (dict(ftop=P["u"], cmax=P["u"]), ("les_transport", "les_transport2"), E, INPUT.format(name="{name}", x="cmax")),
    (dict(ftop=P["u"], n_fields=0, **HUGE), ("les_transport", "les_transport2"), U, "{name}: too many workgroups"),   # no field: ftop is dropped
    (dict(ftop=P["u"] + 1, n_fields=0, **HUGE), ("les_transport", "les_transport2"), U, "{name}: too many workgroups"),
    (dict(mtop=P["u"], fields={0: 1}), None, E, INPUT.format(name="{name}", x="mtop")),               # aliases before alignment
    # 12. alignment
    (dict(fields={0: "skew"}), None, E, "{name}: a pointer is not aligned to its element type"),
    (dict(out={3: "skew"}), None, E, "{name}: a pointer is not aligned to its element type"),
    (dict(hx="skew"), None, E, "{name}: a pointer is not aligned to its element type"),
    (dict(cmax="skew"), None, E, "{name}: a pointer is not aligned to its element type"),
    (dict(mtop="skew"), None, E, "{name}: a pointer is not aligned to its element type"),
    (dict(ftop="skew"), ("les_transport", "les_transport2"), E, "{name}: a pointer is not aligned to its element type"),
    (dict(r="skew", ktot="levels", pitch_prof=4000), None, E, "{name}: a pointer is not aligned to its element type"),  # before ktot
    # 13. unsupported ktot
    (dict(ktot="levels", pitch_prof=4000), None, U, "{name}: ktot {levels} above the {below} levels of which 16 columns fit the LDS"),
    (dict(ktot="levels", pitch_prof=4000, n=1 << 40), None, U, "{name}: ktot {levels} above the {below} levels of which 16 columns fit the LDS"),
    (dict(ktot=100000, pitch_prof=100000), None, U, "{name}: ktot 100000 above the {below} levels of which 16 columns fit the LDS"),
    # 14. too many workgroups
    (dict(n=1 << 40, ktot=3), None, U, "{name}: too many workgroups"),
    (dict(n=1 << 40, ktot=3, limiter=0), None, U, "{name}: too many workgroups"),
    (dict(n=1 << 40, ktot=3, n_fields=0), None, U, "{name}: too many workgroups"),
    (dict(n=1 << 40, ktot=3, n_fields=0, cmax=None), None, U, "{name}: too many workgroups"),
]


def materialise(kw, sfx):
    """the table's placeholders: "skew" is a pointer off the element grid, "levels" the first unsupported ktot"""
    out = {}
    for k, v in kw.items():
        if isinstance(v, dict):
            v = {f: (FIELD0 + 4096 * 7 + SKEW[sfx] if x == "skew" else x) for f, x in v.items()}
        elif v == "skew":
            v = 4096 * 40 + SKEW[sfx]
        elif v == "levels":
            v = LEVELS[sfx]
        out[k] = v
    return out


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("name", list(KERNELS))
def test_every_refusal_has_its_code_and_text_in_order(lib, name, sfx):
    fn = getattr(lib, "spc_%s_%s" % (name, sfx))
    cls = KERNELS[name]
    assert (fn(None, None), lib.spc_last_error()) == (E, b"args is NULL")                                # 1. NULL args
    made = 0
    for kw, only, rc, text in TABLE:
        if only is not None and name not in only:
            continue
        kw = materialise(kw, sfx)
        want = text.format(name=name, levels=LEVELS[sfx], below=LEVELS[sfx] - 1).encode()
        assert (fn(ctypes.byref(block(cls, **kw)), None), lib.spc_last_error()) == (rc, want), kw
        made += 1
    assert made >= 60
    # 7. an empty ensemble is a no-op before any pointer is looked at, after the checks of the scalars
    nulls = dict(fields={f: None for f in range(6)}, out={f: None for f in range(6)}, **{k: None for k in PTRS})
    assert fn(ctypes.byref(block(cls, n=0, **nulls)), None) == 0
    assert (fn(ctypes.byref(block(cls, n=0, pitch_prof=19, **nulls)), None), lib.spc_last_error()) == (E, ("%s: pitch_prof 19 smaller than ktot" % name).encode())
    assert (fn(ctypes.byref(block(cls, n=0, n_fields=0, **nulls)), None), lib.spc_last_error()) == (E, NOTHING.format(name=name).encode())
