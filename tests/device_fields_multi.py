"""models.DeviceLESEnsemble under a multi.MultiDeviceEngine against its host twin (slab_ref.HostFieldLESEnsemble) on ONE
engine: the bodies of tests/test_device_fields_multi_gpu.py (HIP engines sharing one card) and of
tests/test_device_fields_multi_cpu.py (the oracle-backed engines of tests/fake_engine.py).  Every function takes the single
engine and the multi-device engine; every comparison is numpy.array_equal, the state of numpy's global generator included."""
import numpy
import torch

from sp_coupler_amd import driver, models, spcpl
from sp_coupler_amd.transfer import Sharded
from tests import slab_ref
from tests.test_vnudge import make_les_fields

#: (engines, LES, min_cols_per_device): blocks 3 + 2; 3 + 3 + 1; 1 + 1 + 0 (a device without rows); below the threshold
#: (everything stays on the primary engine as plain tensors)
PARTITIONS = [(2, 5, 1), (3, 7, 1), (3, 2, 1), (2, 5, 8)]
BLOCKS = {(2, 5, 1): [3, 2], (3, 7, 1): [3, 3, 1], (3, 2, 1): [1, 1, 0], (2, 5, 8): None}
FIELDS = ("U", "V", "THL", "QT")


def same_state(a, b):
    assert a[0] == b[0] and numpy.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


def host_of(t):
    return models.DeviceLESEnsemble._host(t)


def parts_of(t):
    return list(t.parts) if isinstance(t, Sharded) else [t]


def check_placement(multi, part, t, trailing):
    """a Sharded whose part d lies on engine d with that engine's rows -- or the primary engine's plain tensor"""
    blocks = BLOCKS[part]
    if blocks is None:
        assert isinstance(t, torch.Tensor) and t.device == multi.primary.device and tuple(t.shape) == (part[1],) + tuple(trailing)
        return
    assert isinstance(t, Sharded) and len(t.parts) == len(multi.engines) == part[0]
    assert list(t.bounds) == list(numpy.concatenate([[0], numpy.cumsum(blocks)])) == multi.bounds_for(part[1])
    for p, e, rows in zip(t.parts, multi.engines, blocks):
        assert isinstance(p, torch.Tensor) and p.device == e.device and p.dtype == e.dtype, (p.device, e.device)
        assert tuple(p.shape) == (rows,) + tuple(trailing) and p.is_contiguous()
    assert tuple(t.shape) == (part[1],) + tuple(trailing)


# -- initial state ---------------------------------------------------------------------------------------------------------
def _initial(engine, cls, n, nG, nL, itot, jtot):
    spcpl.set_engine(engine)
    gcm = models.BatchedSyntheticGCM(n + 7, nG, 1)
    ens = cls.for_gcm(gcm, numpy.arange(1, 2 * n + 1, 2), nL=nL, seed=2, itot=itot, jtot=jtot)
    numpy.random.seed(5)
    numpy.random.normal()                                    # a cached Gaussian: has_gauss must survive
    spcpl.gather_gcm_data(gcm, ens, True)
    spcpl.set_les_state_batched(ens)
    return ens, numpy.random.get_state()


def check_initial_state(one, multi, part, nG=19, nL=40, itot=6, jtot=5):
    n = part[1]
    host, s_host = _initial(one, slab_ref.HostFieldLESEnsemble, n, nG, nL, itot, jtot)
    dev, s_dev = _initial(multi, models.DeviceLESEnsemble, n, nG, nL, itot, jtot)
    same_state(s_dev, s_host)
    for name in FIELDS:
        t = dev.fields3d[name]
        check_placement(multi, part, t, (itot, jtot, nL))
        assert t is dev.get_fields_batched(name)                 # handed out as it is, no copy
        assert numpy.array_equal(host_of(t), host.fields3d[name]), name
    assert not numpy.array_equal(host.fields3d["U"][0], host.fields3d["U"][-1])
    assert numpy.array_equal(dev.p["PS"], host.p["PS"])
    return dev


# -- variability nudge -----------------------------------------------------------------------------------------------------
def _nudge_ensemble(engine, cls, n, itot, jtot, nL):
    spcpl.set_engine(engine)
    fs = [make_les_fields(itot, jtot, nL, seed=60 + i) for i in range(n)]
    stack = lambda k: numpy.stack([f[k] for f in fs])                                      # noqa: E731
    fields = {"Qsat": stack("qsat"), "QT": stack("qt"), "THL": stack("thl"), "QL": stack("ql")}
    gcm = models.BatchedSyntheticGCM(n + 4, 19, 21)
    ens = cls.for_gcm(gcm, numpy.arange(1, n + 1), nL=nL, seed=21, itot=itot, jtot=jtot)
    ens.attach_fields({k: v.copy() for k, v in fields.items()})     # (a CPU test engine's "upload" shares the array's memory)
    ens.p["presf"] = stack("presf")
    ens.ql_ref = stack("ql_ref")
    ens.model_time = 900.0
    return ens, fields


def _nudge(engine, cls, n, constantT, itot, jtot, nL):
    ens, fields = _nudge_ensemble(engine, cls, n, itot, jtot, nL)
    ptr = {k: [p.data_ptr() for p in parts_of(ens.fields3d[k])] for k in ("QT", "THL")} if cls is models.DeviceLESEnsemble else None
    numpy.random.seed(11)
    res = spcpl.variability_nudge_ensemble(ens, 900.0, constantT, write=False)
    return ens, fields, res, numpy.random.get_state(), ptr


def compare_nudges(a, b):
    """(ens, fields, results, generator state, ...) of two runs: equal bits everywhere"""
    same_state(a[3], b[3])
    assert len(a[2]) == len(b[2])
    for x, y in zip(a[2], b[2]):
        for k in ("beta", "a", "qt_std", "status", "alpha"):
            assert numpy.array_equal(x[k], y[k], equal_nan=(k == "alpha")), k
    for k in ("QT", "THL"):
        fa, fb = a[0].fields3d[k], b[0].fields3d[k]
        assert numpy.array_equal(fa if isinstance(fa, numpy.ndarray) else host_of(fa), fb if isinstance(fb, numpy.ndarray) else host_of(fb)), k


def check_variability_nudge(one, multi, part, constantT, itot=8, jtot=6, nL=20):
    n = part[1]
    host = _nudge(one, slab_ref.HostFieldLESEnsemble, n, constantT, itot, jtot, nL)
    dev = _nudge(multi, models.DeviceLESEnsemble, n, constantT, itot, jtot, nL)
    compare_nudges(host, dev)
    ens, fields = dev[0], dev[1]
    for k in ("QT", "THL", "Qsat", "QL"):
        check_placement(multi, part, ens.fields3d[k], (itot, jtot, nL))
    assert {k: [p.data_ptr() for p in parts_of(ens.fields3d[k])] for k in ("QT", "THL")} == dev[4]      # in place, every part
    assert any(r["status"].any() for r in dev[2]) and all(numpy.isfinite(r["beta"]).all() for r in dev[2])
    qt, thl = host_of(ens.fields3d["QT"]), host_of(ens.fields3d["THL"])
    for l in range(n):                                           # every LES of every block was nudged, none twice
        assert not numpy.array_equal(qt[l], fields["QT"][l]), l
        assert numpy.array_equal(thl[l], fields["THL"][l]) != constantT, l


def check_chunked_nudge(monkeypatch, one, multi, n, constantT, itot=8, jtot=6, nL=20):
    """launches of at most VN_MAX_COLS LES: with 2 and 3 per launch the bits of the unsplit run, on one engine and on several"""
    host = _nudge(one, slab_ref.HostFieldLESEnsemble, n, constantT, itot, jtot, nL)
    whole = _nudge(one, models.DeviceLESEnsemble, n, constantT, itot, jtot, nL)
    compare_nudges(host, whole)
    launches = []
    for engine in (one, multi):
        for e in getattr(engine, "engines", [engine]):
            def counted(*a, _inner=e.variability_nudge, **kw):
                launches.append(int(a[0].shape[0]))
                return _inner(*a, **kw)
            monkeypatch.setattr(e, "variability_nudge", counted, raising=False)
    for cols in (2, 3):
        monkeypatch.setattr(spcpl, "VN_MAX_COLS", cols)
        for engine in (one, multi):
            del launches[:]
            got = _nudge(engine, models.DeviceLESEnsemble, n, constantT, itot, jtot, nL)
            compare_nudges(whole, got)
            assert got[4] == {k: [p.data_ptr() for p in parts_of(got[0].fields3d[k])] for k in ("QT", "THL")}
            blocks = [n] if engine is one else [int(b) for b in numpy.diff(engine.bounds_for(n)) if b]
            assert launches == [min(cols, b - c) for b in blocks for c in range(0, b, cols)], (cols, launches)
            assert max(launches) <= cols and (len(launches) > 1 or engine is not one)


# -- closed loop -----------------------------------------------------------------------------------------------------------
def _loop(engine, cls, n, nG, nL, itot, jtot, steps):
    spcpl.set_engine(engine)
    gcm = models.BatchedSyntheticGCM(n + 7, nG, 3)
    ens = cls.for_gcm(gcm, numpy.arange(1, 2 * n + 1, 2), nL=nL, seed=4, itot=itot, jtot=jtot)
    rng = numpy.random.default_rng(8)
    ens.attach_fields({"Qsat": ens.p["QT"][:, None, None, :] * (1.0 + 2e-3 * rng.normal(size=(n, itot, jtot, nL)))})
    # cplsurf=True: init_les_state gathers WITH the surface fields (splib.py:197) and an ensemble's profiles are tied to
    # the transfer buffers of that batch geometry, so the steps that follow must gather the same way
    cpl = driver.Coupler(gcm, ens, cplsurf=True, qt_forcing="variance")
    numpy.random.seed(42)
    cpl.init_les_state()
    log = []

    def record():
        log.append({"tend": {k: numpy.array(v[1]) for k, v in gcm.tendencies.items()},
                    "prof": {k: numpy.array(v) for k, v in ens.p.items()}, "time": ens.model_time})
    cpl.run_spinup(900.0, 1)
    record()
    for _ in range(steps):
        cpl.step()
        record()
    return ens, log, numpy.random.get_state()


def check_closed_loop(one, multi, ndev, n, nG=19, nL=40, itot=6, jtot=5, steps=3):
    host, log_h, s_h = _loop(one, slab_ref.HostFieldLESEnsemble, n, nG, nL, itot, jtot, steps)
    dev, log_d, s_d = _loop(multi, models.DeviceLESEnsemble, n, nG, nL, itot, jtot, steps)
    same_state(s_d, s_h)
    assert len(log_h) == len(log_d) == steps + 1 and log_d[-1]["time"] > log_d[0]["time"] > 0
    for step, (a, b) in enumerate(zip(log_h, log_d)):
        assert a["time"] == b["time"] and set(a["tend"]) == set(b["tend"]) and (step == 0 or len(a["tend"]) >= 6)
        for k in a["tend"]:
            assert numpy.array_equal(a["tend"][k], b["tend"][k], equal_nan=True), (step, "tendency", k)
        assert set(a["prof"]) == set(b["prof"])
        for k in a["prof"]:
            assert numpy.array_equal(a["prof"][k], b["prof"][k], equal_nan=True), (step, "profile", k)
    for k in ("U", "V", "THL", "QT", "QL", "Qsat"):
        t = dev.fields3d[k]
        assert isinstance(t, Sharded) and len(t.parts) == ndev and sum(p.shape[0] for p in t.parts) == n
        assert numpy.array_equal(host_of(t), host.fields3d[k]), k
    assert not numpy.array_equal(log_d[-1]["prof"]["QT"], log_d[0]["prof"]["QT"])          # the state did evolve
    assert (log_d[-1]["prof"]["QL"] > 0).any()                                              # and holds cloud
