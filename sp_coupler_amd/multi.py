"""All GPUs of the node from ONE process: the column batch split into contiguous row blocks, one per device.

The reference's master is a single process that holds every LES object (``splib/splib.py:146-154``) and loops over
the columns (``splib.py:317-332``).  ``MultiDeviceEngine`` keeps that shape: it owns one ``Engine`` per visible GPU,
gives device d rows ``shard_bounds(n, k)[d:d+2]`` of every ``[n x n_lev]`` array (the same partition
``sharding.py`` uses for one-rank-per-GPU runs; the shared LES grid is replicated), and issues each device's copies
and launches on that device's own stream, one device after the other -- everything is asynchronous, so the devices
work concurrently.  Columns are independent (``splib.py:317,330``): no collective, no peer traffic on the hot path.
``spcpl.get_engine()`` returns one when ``SPC_DEVICES`` asks for it (``all`` or a list of ids; opt-in since round 4: the
path has only ever run on engines sharing one card), so ``driver.Coupler.step`` and the reference-named ``spcpl`` calls
use every GPU without any change on the caller's side.

Plans mirror ``engine._Plan`` (``set_scalars`` / ``launch`` / ``outputs``): a ``MultiPlan`` holds the per-device
plans, its ``outputs`` are ``transfer.Sharded`` arrays.  Small batches stay on fewer devices (``MIN_COLS_PER_DEVICE``):
a launch of a few hundred columns is latency-bound and gains nothing from being split.
"""
import os

import torch

from .sharding import shard_bounds
from .transfer import Sharded, ShardedArena

MIN_COLS_PER_DEVICE = 2048


class MultiPlan:
    def __init__(self, plans, outputs):
        self.plans, self.outputs = plans, outputs

    def set_scalars(self, factor, dt):
        for p in self.plans:
            if p is not None:
                p.set_scalars(factor, dt)

    def launch(self, stream=None):
        if stream is not None:
            raise ValueError("a multi-device plan launches on each device's current stream")
        for p in self.plans:
            if p is not None:
                p.launch()
        return self.outputs

    def describe(self):
        return [p.describe() if p is not None else None for p in self.plans]


def _part(x, d):
    """device d's share of an argument: a Sharded's part, or the object itself (scalars, None)"""
    return x.parts[d] if isinstance(x, Sharded) else x


def _parts_of(dct, d):
    return None if dct is None else {k: _part(v, d) for k, v in dct.items()}


class MultiDeviceEngine:
    """``engines``: one ``Engine`` per device (default: every visible GPU, or the ids in ``SPC_DEVICES=0,1,...``).
    Tests pass other engine objects with the same interface (two test engines on the CPU; two engines on one GPU)."""

    def __init__(self, engines=None, dtype=torch.float64, min_cols_per_device=MIN_COLS_PER_DEVICE):
        if engines is None:
            from .engine import Engine
            want = os.environ.get("SPC_DEVICES", "").strip()
            ids = [int(x) for x in want.split(",")] if want and want != "all" else list(range(torch.cuda.device_count()))
            engines = [Engine("cuda:%d" % i, dtype=dtype) for i in ids]
        if not engines:
            raise RuntimeError("MultiDeviceEngine needs at least one engine")
        self.engines = list(engines)
        self.primary = self.engines[0]
        self.device, self.dtype = self.primary.device, self.primary.dtype     # the primary device (slow paths, traces)
        self.lib = getattr(self.primary, "lib", None)
        self.min_cols_per_device = int(min_cols_per_device)

    # -- partition ------------------------------------------------------------------------------------------------
    def devices_for(self, n):
        """how many devices a batch of n columns is split over (>= min_cols_per_device columns each)"""
        return max(1, min(len(self.engines), n // max(1, self.min_cols_per_device)))

    def bounds_for(self, n):
        k = self.devices_for(n)
        b = shard_bounds(n, k)
        return b + [n] * (len(self.engines) - k)          # unused devices get empty blocks

    def arena(self, specs, rows):
        if self.devices_for(rows) == 1:              # everything on the primary engine: its plain single-copy arena
            return self.primary.arena(specs, rows)
        return ShardedArena([e.device for e in self.engines], self.bounds_for(rows), specs, rows,
                            streams=[getattr(e, "stream", None) for e in self.engines])

    def to_devices(self, host_array, rows=None, n_cols=None, dtype=None):
        """a host array on every device: replicated (``rows`` None: the shared LES grid) or row-sharded, in the engines'
        dtype or ``dtype`` (variability_nudge's R: float64 on any engine).  A batch that stays on the primary engine
        (``n_cols`` / ``rows`` below the threshold) gets a plain tensor."""
        if self.devices_for(rows if rows is not None else (n_cols if n_cols is not None else self.min_cols_per_device * 2)) == 1:
            return self.primary.to_devices(host_array, rows, dtype=dtype)
        t = torch.from_numpy(host_array)
        if rows is None:
            out = Sharded([t.to(e.device, dtype or e.dtype) for e in self.engines], None)
        else:
            b = self.bounds_for(rows)
            out = Sharded([t[b[i]:b[i + 1]].to(e.device, dtype or e.dtype) for i, e in enumerate(self.engines)], b)
        self.synchronize()                            # made on the current streams, used on the engines' own
        return out

    # -- plans: one per device that holds rows ----------------------------------------------------------------------
    def _plans(self, make, example):
        """``make(engine, d)`` for every device with a non-empty row block of ``example`` (a Sharded with bounds)"""
        b = example.bounds
        return [make(e, d) if b[d + 1] > b[d] else None for d, e in enumerate(self.engines)]

    @staticmethod
    def _outputs(plans, bounds):
        keys = next(p for p in plans if p is not None).outputs.keys()
        ref = {k: next(p for p in plans if p is not None).outputs[k] for k in keys}
        out = {}
        for k in keys:
            parts = [p.outputs[k] if p is not None else ref[k][:0] for p in plans]
            out[k] = Sharded(parts, bounds)
        return out

    def plan_forward(self, gcm, zf, prof, factor, dt, zh=None, out=None, **kw):
        ex = gcm["T"]
        if not isinstance(ex, Sharded):
            return self.primary.plan_forward(gcm, zf, prof, factor, dt, zh=zh, out=out, **kw)
        plans = self._plans(lambda e, d: e.plan_forward(_parts_of(gcm, d), _part(zf, d), _parts_of(prof, d), factor, dt,
                                                        zh=_part(zh, d), out=_parts_of(out, d), **kw), ex)
        return MultiPlan(plans, self._outputs(plans, ex.bounds))

    def plan_backward(self, gcm, zf, prof, factor, dt, Zf=None, zh=None, Zh=None, out=None, **kw):
        ex = gcm["T"]
        if not isinstance(ex, Sharded):
            return self.primary.plan_backward(gcm, zf, prof, factor, dt, Zf=Zf, zh=zh, Zh=Zh, out=out, **kw)
        plans = self._plans(lambda e, d: e.plan_backward(_parts_of(gcm, d), _part(zf, d), _parts_of(prof, d), factor, dt,
                                                         Zf=_part(Zf, d), zh=_part(zh, d), Zh=_part(Zh, d),
                                                         out=_parts_of(out, d), **kw), ex)
        return MultiPlan(plans, self._outputs(plans, ex.bounds))

    def plan_diagnostics(self, gcm, zf=None, prof=None, out=None, **kw):
        ex = gcm["T"]
        if not isinstance(ex, Sharded):
            return self.primary.plan_diagnostics(gcm, zf, prof, out=out, **kw)
        plans = self._plans(lambda e, d: e.plan_diagnostics(_parts_of(gcm, d), _part(zf, d), _parts_of(prof, d),
                                                            out=_parts_of(out, d), **kw), ex)
        return MultiPlan(plans, self._outputs(plans, ex.bounds))

    def plan_cloud_indices(self, zh, Zh, out=None, **kw):
        if not isinstance(Zh, Sharded):
            return self.primary.plan_cloud_indices(zh, Zh, out=out, **kw)
        plans = self._plans(lambda e, d: e.plan_cloud_indices(_part(zh, d), _part(Zh, d), out=_part(out, d), **kw), Zh)
        return MultiPlan(plans, self._outputs(plans, Zh.bounds))

    def plan_exchange(self, gcm, zf, zh, prof, factor_les, factor_gcm, dt, cols_per_block=0):
        """the lean K1 / K3 pair of ``Engine.plan_exchange`` on every device's rows"""
        lean = {k: v for k, v in prof.items() if k not in ("Rain", "rain_last")}
        fp = self.plan_forward(gcm, zf, lean, factor_les, dt, zh=zh, want_profiles=False, want_heights=False,
                               cols_per_block=cols_per_block)
        bp = self.plan_backward(gcm, zf, prof, factor_gcm, dt, Zf=None, want_start_index=False, cols_per_block=cols_per_block)
        return fp, bp

    # -- convenience forms and slow paths: per device, on that device's rows (round 5; rounds 3-4 gathered the whole batch
    #    onto the primary device first -- 14 GB onto one card at config 4) -----------------------------------------------
    @staticmethod
    def _example(*xs):
        """the first row-sharded argument (a Sharded with bounds), else None: plain tensors run on the primary engine"""
        for x in xs:
            if isinstance(x, dict):
                x = MultiDeviceEngine._example(*x.values())
            if isinstance(x, Sharded) and x.bounds is not None:
                return x
        return None

    def _each(self, name, ex, args, kw):
        """``engine.<name>(*args, **kw)`` on every device that holds rows of ``ex``, with every Sharded argument replaced by
        that device's block; returns the per-device results (None for devices without rows)"""
        res = []
        for d, e in enumerate(self.engines):
            if ex.bounds[d + 1] <= ex.bounds[d]:
                res.append(None)
                continue
            a = [_parts_of(x, d) if isinstance(x, dict) else _part(x, d) for x in args]
            k = {key: (_parts_of(v, d) if isinstance(v, dict) else _part(v, d)) for key, v in kw.items()}
            res.append(getattr(e, name)(*a, **k))
        return res

    @staticmethod
    def _join(results, bounds):
        """per-device results (tensors, tuples or dicts of tensors) -> the same shape of Sharded arrays"""
        ref = next(r for r in results if r is not None)
        pick = lambda r, get: get(r) if r is not None else get(ref)[:0]                       # noqa: E731
        if isinstance(ref, dict):
            return {k: Sharded([pick(r, lambda x, k=k: x[k]) for r in results], bounds) for k in ref}
        if isinstance(ref, (tuple, list)):
            return tuple(Sharded([pick(r, lambda x, i=i: x[i]) for r in results], bounds) for i in range(len(ref)))
        return Sharded([pick(r, lambda x: x) for r in results], bounds)

    def _run(self, name, *args, **kw):
        ex = self._example(*args, *kw.values())
        if ex is None:
            return getattr(self.primary, name)(*args, **kw)
        return self._join(self._each(name, ex, args, kw), ex.bounds)

    def forward(self, gcm, zf, prof, factor, dt, **kw):
        return self._run("forward", gcm, zf, prof, factor, dt, **kw)

    def backward(self, gcm, zf, prof, factor, dt, **kw):
        return self._run("backward", gcm, zf, prof, factor, dt, **kw)

    def diagnostics(self, gcm, zf=None, prof=None, **kw):
        return self._run("diagnostics", gcm, zf, prof, **kw)

    def cloud_indices(self, zh, Zh, **kw):
        return self._run("cloud_indices", zh, Zh, **kw)

    def surface_fluxes(self, *a, **kw):
        return self._run("surface_fluxes", *a, **kw)

    def variability_nudge(self, *a, **kw):
        """K6 on every device's LES (spcpl.py:377-382 nudges one LES at a time; columns are independent): Sharded fields in,
        Sharded results out, ``qt`` / ``thl`` updated in place block by block.  R is float64 on every engine: shard it with
        ``to_devices(R, rows=n, dtype=torch.float64)`` (the fields and profiles in the engines' dtype)"""
        return self._run("variability_nudge", *a, **kw)

    def slab_means(self, fields, out=None, **kw):
        """K10 on every device's LES: dict of Sharded fields [n x itot x jtot x ktot] in, dict of Sharded [n x ktot] out"""
        return self._run("slab_means", fields, out=out, **kw)

    def les_advance(self, fields, tend, dt, qsat=None, sat=None, ql=None, means=None, ql_mean=True, **kw):
        """K11 on every device's LES: dicts of Sharded fields and tendencies in (the fields stepped in place, block by block),
        dict of Sharded [n x ktot] slab means of the stepped fields out; one launch per device that holds rows"""
        return self._run("les_advance", fields, tend, dt, qsat=qsat, sat=sat, ql=ql, means=means, ql_mean=ql_mean, **kw)

    def les_thermo(self, thl, qt, presf, ex, n_iter=None, qsat=None, ql=None, temp=None, means=True, **kw):
        """K12 on every device's LES: Sharded fields and [n x ktot] profiles in (``qsat``, ``ql`` and ``temp`` written block by
        block), dict of Sharded [n x ktot] slab means of QL and T out; one launch per device that holds rows"""
        return self._run("les_thermo", thl, qt, presf, ex, n_iter=n_iter, qsat=qsat, ql=ql, temp=temp, means=means, **kw)

    def les_water_paths(self, fields, w, cloud=None, out=None, top=False, cover=False, **kw):
        """K13 on every device's LES: dict of Sharded fields and the Sharded weight profile [n x ktot] in, dict of Sharded
        [n x itot x jtot] water paths (with ``"top"`` and ``"cover"`` [n] where asked) out; one launch per device that holds rows"""
        return self._run("les_water_paths", fields, w, cloud=cloud, out=out, top=top, cover=cover, **kw)

    def les_microphysics(self, qt, ql, qr, qr_new, sed_out, sed_in, lcpex, w, dt, thl=None, temp=None, rain=None, means=True, **kw):
        """K14 on every device's LES: Sharded fields and [n x ktot] profiles in (``qt``, ``thl``, ``qr_new`` and ``rain`` written
        block by block), dict of Sharded [n x ktot] slab means out; one launch per device that holds rows"""
        return self._run("les_microphysics", qt, ql, qr, qr_new, sed_out, sed_in, lcpex, w, dt, thl=thl, temp=temp, rain=rain,
                         means=means, **kw)

    def les_diffuse(self, fields, a, m, cp, s0=None, flux=None, **kw):
        """K15 on every device's LES: dict of Sharded fields (diffused in place, block by block), Sharded [n x ktot] profiles,
        ``s0`` [n] and dict of Sharded [n] fluxes in; one launch per device that holds rows, none on the others"""
        ex = self._example(fields)
        if ex is None:
            return self.primary.les_diffuse(fields, a, m, cp, s0=s0, flux=flux, **kw)
        self._each("les_diffuse", ex, (fields, a, m, cp), dict(kw, s0=s0, flux=flux))

    def _largest(self, name, key, ex, args, kw):
        """``engine.<name>(*args, **kw)`` for the methods that return the largest value of every LES where ``kw[key]`` asks for
        it (``cmax``, ``amax``): on the primary engine when ``ex`` is no Sharded, else on every device that holds rows of it.
        Returns None for False / None, the caller's own (Sharded) tensor where one was given, the joined results for True"""
        ex = self._example(ex)
        if ex is None:
            return getattr(self.primary, name)(*args, **kw)
        res = self._each(name, ex, args, kw)
        top = kw[key]
        if top is None or top is False:
            return None
        return top if top is not True else self._join(res, ex.bounds)

    def les_advect(self, fields, out, u, v, hx, hy, cmax=True, **kw):
        """K16 on every device's LES: dicts of Sharded fields and outputs (written block by block), Sharded winds and ``hx``,
        ``hy`` [n] in; the Sharded [n] Courant sums out (None without ``cmax``); one launch per device that holds rows"""
        return self._largest("les_advect", "cmax", u, (fields, out, u, v, hx, hy), dict(kw, cmax=cmax))

    def les_vadvect(self, fields, out, u, v, hx, hy, g, r, cmax=True, mtop=None, **kw):
        """K17 on every device's LES: dicts of Sharded fields and outputs (written block by block), Sharded winds, ``hx``, ``hy``
        [n], the profiles ``g`` and ``r`` [n x ktot] and ``mtop`` (or None) in; the Sharded [n] vertical Courant sums out (None
        without ``cmax``); one launch per device that holds rows"""
        return self._largest("les_vadvect", "cmax", u, (fields, out, u, v, hx, hy, g, r), dict(kw, cmax=cmax, mtop=mtop))

    def les_transport(self, fields, out, u, v, hx, hy, g, r, cmax=True, mtop=None, ftop=None, **kw):
        """K22 on every device's LES: dicts of Sharded fields and outputs (written block by block), Sharded winds, ``hx``, ``hy``
        [n], the profiles ``g`` and ``r`` [n x ktot], ``mtop`` (or None) and ``ftop`` (or None: a Sharded whose part on device
        d is [len(fields) x that device's rows x itot x jtot]) in; the Sharded [n] outflow Courant sums out (None without
        ``cmax``); one launch per device that holds rows"""
        return self._largest("les_transport", "cmax", u, (fields, out, u, v, hx, hy, g, r), dict(kw, cmax=cmax, mtop=mtop, ftop=ftop))

    def les_transport2(self, fields, out, u, v, hx, hy, g, r, limiter="mc", cmax=True, mtop=None, ftop=None, **kw):
        """K23 on every device's LES: the arguments and the result of ``les_transport`` with the ``limiter`` of
        ``Engine.les_transport2``; one launch per device that holds rows"""
        return self._largest("les_transport2", "cmax", u, (fields, out, u, v, hx, hy, g, r),
                             dict(kw, limiter=limiter, cmax=cmax, mtop=mtop, ftop=ftop))

    def les_radiate(self, ql, thl, w, c, f0, f1, *, flux=None, fsfc=None, **kw):
        """K18 on every device's LES: the Sharded fields ``ql`` and ``thl`` (updated in place, block by block), the Sharded
        profiles ``w`` and ``c`` [n x ktot], ``f0`` and ``f1`` [n] and ``flux`` / ``fsfc`` (or None) in; one launch per device
        that holds rows, none on the others"""
        ex = self._example(ql)
        if ex is None:
            return self.primary.les_radiate(ql, thl, w, c, f0, f1, flux=flux, fsfc=fsfc, **kw)
        self._each("les_radiate", ex, (ql, thl, w, c, f0, f1), dict(kw, flux=flux, fsfc=fsfc))

    def les_qt_local(self, qt, ql, a, qtm, *, count=None, split=0, **kw):
        """K19 on every device's LES: the Sharded fields ``qt`` (updated in place, block by block) and ``ql``, the Sharded
        profiles ``a`` and ``qtm`` [n x ktot] and ``count`` (or None) in, the Sharded int32 [n x ktot] counts out; one launch per
        device that holds rows, none on the others"""
        return self._run("les_qt_local", qt, ql, a, qtm, count=count, split=split, **kw)

    def les_moments(self, fields, pairs=(), mean=True, var=True, std=False, face=None, out=None, **kw):
        """K20 on every device's LES: the dict of Sharded fields [n x itot x jtot x ktot] in, ``{kind: {name or pair: Sharded
        [n x ktot]}}`` out (``out``: the same structure of Sharded tensors to write into); one launch per device that holds
        rows, none on the others"""
        ex = self._example(fields)
        if ex is None:
            return self.primary.les_moments(fields, pairs, mean=mean, var=var, std=std, face=face, out=out, **kw)
        res = []
        for d, e in enumerate(self.engines):
            if ex.bounds[d + 1] <= ex.bounds[d]:
                res.append(None)
                continue
            o = None if out is None else {kind: _parts_of(v, d) for kind, v in out.items()}
            res.append(e.les_moments(_parts_of(fields, d), pairs, mean=mean, var=var, std=std, face=face, out=o, **kw))
        ref = next(r for r in res if r is not None)
        return {kind: self._join([None if r is None else r[kind] for r in res], ex.bounds) for kind in ref}

    def les_buoyancy(self, thl, qt, ql, u, v, hx, hy, t0, lex, s, phi, psfc=None, amax=True, **kw):
        """K21 on every device's LES: the Sharded fields ``thl``, ``qt``, ``ql`` (or None), ``u`` and ``v`` (updated in place,
        block by block), ``hx``, ``hy`` [n], the Sharded profiles ``t0``, ``lex`` and ``s`` [n x ktot], ``phi`` and ``psfc`` (or
        None) in; the Sharded [n] largest wind changes out (None without ``amax``); two launches per device that holds rows,
        none on the others"""
        return self._largest("les_buoyancy", "amax", thl, (thl, qt, ql, u, v, hx, hy, t0, lex, s, phi), dict(kw, psfc=psfc, amax=amax))

    def les_mix(self, fields, out, u, v, theta, gx, gy, gz, bz, l2, kcap, km, ax, ay, kmax=True, **kw):
        """K24 on every device's LES: dicts of Sharded fields and outputs (written block by block), the Sharded winds, ``theta``
        (or None), ``gx``, ``gy``, ``kcap`` [n], the Sharded profiles ``gz``, ``bz`` (or None) and ``l2`` [n x ktot], ``km`` and the
        dicts ``ax`` and ``ay`` of Sharded [n] in; the Sharded [n] largest uncapped viscosities out (None without ``kmax``); two
        launches per device that holds rows, none on the others"""
        return self._largest("les_mix", "kmax", u, (fields, out, u, v, theta, gx, gy, gz, bz, l2, kcap, km, ax, ay), dict(kw, kmax=kmax))

    def les_vmix(self, fields, km, el, eu, kb, kv2, s0=None, flux=None, drag=None, u=None, v=None, speed=None, **kw):
        """K25 on every device's LES: dict of Sharded fields (mixed in place, block by block), the Sharded ``km``, the dicts ``el``
        and ``eu`` of Sharded [n x ktot], ``kb`` [n x ktot], ``kv2`` and ``s0`` [n], the dicts of Sharded [n] fluxes and drags, the
        Sharded winds and the Sharded plane ``speed`` [n x itot x jtot] in; two launches per device that holds rows, none on the
        others"""
        ex = self._example(fields)
        if ex is None:
            return self.primary.les_vmix(fields, km, el, eu, kb, kv2, s0=s0, flux=flux, drag=drag, u=u, v=v, speed=speed, **kw)
        self._each("les_vmix", ex, (fields, km, el, eu, kb, kv2), dict(kw, s0=s0, flux=flux, drag=drag, u=u, v=v, speed=speed))

    def les_hmix(self, fields, km, ax, ay, kh2, axes=3, **kw):
        """K26 on every device's LES: dict of Sharded fields (mixed in place, block by block), the Sharded ``km``, the dicts ``ax``
        and ``ay`` of Sharded [n] and ``kh2`` [n] in; two launches per device that holds rows, none on the others"""
        ex = self._example(fields)
        if ex is None:
            return self.primary.les_hmix(fields, km, ax, ay, kh2, axes=axes, **kw)
        self._each("les_hmix", ex, (fields, km, ax, ay, kh2), dict(kw, axes=axes))

    def slab_cloud_fraction(self, ql, idx, out=None, **kw):
        """K10's cloud fraction on every device's LES: Sharded QL field and index map in, Sharded [n x nG] out"""
        return self._run("slab_cloud_fraction", ql, idx, out=out, **kw)

    # the helpers of splib/sputils.py (K7) on row-sharded arguments: each device runs the operator on its rows; an argument
    # shared by all rows (a 1-D grid) is a replicated Sharded (``to_devices(host)``) or a plain tensor on the primary device
    def exner(self, p, inverse=False, **kw):
        return self._run("exner", p, inverse=inverse, **kw)

    def interp(self, x, xp, fp, **kw):
        return self._run("interp", x, xp, fp, **kw)

    def searchsorted(self, a, v, side="left", **kw):
        return self._run("searchsorted", a, v, side=side, **kw)

    def interp_c(self, Zh, zh, q, rho=None, mode="interp_c", **kw):
        return self._run("interp_c", Zh, zh, q, rho, mode=mode, **kw)

    def rms(self, a, **kw):
        return self._run("rms", a, **kw)

    # the geometry of sputils.get_mask_indices (K8): once at start-up, on the primary engine
    def point_in_polygon(self, *a, **kw):
        return self.primary.point_in_polygon(*a, **kw)

    def haversine(self, *a, **kw):
        return self.primary.haversine(*a, **kw)

    def on_stream(self):
        """the slow paths run on the primary engine: its stream context (Engine.on_stream)"""
        return self.primary.on_stream()

    def synchronize(self):
        for e in self.engines:
            if e.device.type == "cuda":
                st = getattr(e, "stream", None)
                if st is not None:
                    st.synchronize()
                else:
                    torch.cuda.current_stream(e.device).synchronize()


def describe_partition(engine, n):
    """text for logs / bench output: which rows go where"""
    b = engine.bounds_for(n)
    return ", ".join("%s: rows %d-%d" % (e.device, b[i], b[i + 1]) for i, e in enumerate(engine.engines) if b[i + 1] > b[i])
