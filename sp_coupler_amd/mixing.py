"""The constants, the coefficients and the profiles of K24, the Smagorinsky-Lilly subgrid closure of the device-resident LES fields
(include/spc.h: spc_les_mix_*): an eddy viscosity per cell from the resolved deformation and the stratification,
km = l^2 sqrt(max(D^2 - N^2 / Pr, 0)), capped, and the horizontal mixing of the carried fields by it in flux form.

Everything the kernels multiply by is computed ONCE in float64 NumPy and rounded once to the element type on upload; the kernels
and the NumPy oracle of the tests receive the same arrays, so neither divides and neither takes a cube root.  The winds and the
scalars differ by the Prandtl number in ``ax`` and ``ay`` alone: one pair of vectors per set, so the kernel needs no extra
rounding.  Left out of the rule: the gradients of W (diagnosed from continuity under the hydrostatic closure of K21), the moist
correction of the stability (theta is THL), and substeps where the cap binds: the cap-free way is the implicit step of K26
(horizontal_mixing.py; ``enable_mixing(implicit=True)``), which mixes by the closure's own viscosity in one call."""
import numpy

from . import microphysics, sputils

GRAV = sputils.grav
CS = 0.17             # the Smagorinsky constant
PRANDTL = 1.0 / 3.0   # the turbulent Prandtl number: the scalars mix 1 / PRANDTL times as fast as the winds
KAPPA = 0.4           # von Karman's constant of the wall correction of the mixing length
THETA_REF = 300.0     # K: the reference potential temperature of the stability term
CAP = 0.5             # the largest sum of the four face weights (kw + ke) ax + (ks + kn) ay the cap lets a cell have


def _positive(**kw):
    for name, v in kw.items():
        a = numpy.asarray(v, dtype=numpy.float64)
        if not (numpy.isfinite(a).all() and (a > 0).all()):
            raise ValueError("the mixing (K24) needs a positive and finite %s, got %r" % (name, v))


def coefficients(dt, dx, dy, prandtl=PRANDTL, n=None):
    """float64 ``(gx, gy, (ax, ay) of the winds, (ax, ay) of the scalars)``, [n] each, of LES with the grid spacings ``dx`` and
    ``dy`` (scalars or [n]) for a step of ``dt`` seconds: gx = 0.5 / dx and gy = 0.5 / dy (centred differences);
    ax = 0.5 dt / dx^2 and ay = 0.5 dt / dy^2 for the winds (0.5: a face takes the mean of its two cells' km, which the kernel
    forms as a sum), the same divided by ``prandtl`` for the scalars.  ValueError for a dt, dx, dy or prandtl that is not
    positive and finite"""
    _positive(dt=dt, dx=dx, dy=dy, prandtl=prandtl)
    dx, dy = numpy.asarray(dx, dtype=numpy.float64), numpy.asarray(dy, dtype=numpy.float64)
    shape = (int(n),) if n is not None else numpy.broadcast(dx, dy).shape or (1,)
    full = lambda a: numpy.array(numpy.broadcast_to(a, shape), order="C")                     # noqa: E731
    ax, ay = 0.5 * float(dt) / dx ** 2, 0.5 * float(dt) / dy ** 2
    return full(0.5 / dx), full(0.5 / dy), (full(ax), full(ay)), (full(ax / float(prandtl)), full(ay / float(prandtl)))


def cap(wind, scalar, cap=CAP):
    """float64 kcap [n] = cap / (4 max(ax + ay over both sets)) of ``coefficients``' two pairs: with km <= kcap the four face
    weights of a cell sum to at most ``cap``, so for cap <= 1 a mixed value is a convex combination of the cell and its four
    neighbours.  ValueError for a cap that is not positive and finite"""
    _positive(cap=cap)
    worst = numpy.maximum(numpy.asarray(wind[0]) + numpy.asarray(wind[1]), numpy.asarray(scalar[0]) + numpy.asarray(scalar[1]))
    return float(cap) / (4.0 * worst)


def profiles(zf, zh, dx, dy, cs=CS, prandtl=PRANDTL, theta_ref=THETA_REF, n=None):
    """float64 ``(gz, bz, l2)``, [n x ktot] each, of LES with the full levels ``zf`` and half levels ``zh`` ([ktot] or
    [n x ktot]) and the grid spacings ``dx`` and ``dy`` (scalars or [n]):
    gz[k] = 1 / (zf[kp] - zf[kq]) with kp = min(k + 1, ktot - 1) and kq = max(k - 1, 0) (one-sided at the ground and the lid),
    0 where ktot == 1;
    bz = grav / (prandtl theta_ref) * gz, so that (theta[kp] - theta[kq]) * bz is N^2 / Pr;
    l2 = l^2 from 1 / l^2 = 1 / (cs Delta)^2 + 1 / (KAPPA zf)^2 with Delta = (dx dy dz)^(1/3), dz that of
    ``water_path_weights``.  ValueError for a cs, prandtl, theta_ref, dx or dy that is not positive and finite, for levels that
    do not ascend, or for a zf that is not positive"""
    _positive(cs=cs, prandtl=prandtl, theta_ref=theta_ref, dx=dx, dy=dy)
    zf = numpy.asarray(zf, dtype=numpy.float64)
    rows = int(n) if n is not None else max([zf.shape[0] if zf.ndim == 2 else 1, numpy.size(dx), numpy.size(dy)])
    ktot = zf.shape[-1]
    zf = numpy.broadcast_to(zf, (rows, ktot))
    dz = numpy.broadcast_to(microphysics.layer_thickness(zh, zf), (rows, ktot))
    column = lambda a: numpy.broadcast_to(numpy.asarray(a, dtype=numpy.float64), (rows,))[:, None]          # noqa: E731
    _positive(zf=zf, dz=dz)
    gz = numpy.zeros((rows, ktot))
    if ktot > 1:
        k = numpy.arange(ktot)
        span = zf[:, numpy.minimum(k + 1, ktot - 1)] - zf[:, numpy.maximum(k - 1, 0)]
        _positive(span=span)
        gz = 1.0 / span
    bz = GRAV / (float(prandtl) * float(theta_ref)) * gz
    delta = numpy.cbrt(column(dx) * column(dy) * dz)
    l2 = 1.0 / (1.0 / (float(cs) * delta) ** 2 + 1.0 / (KAPPA * zf) ** 2)
    return numpy.array(gz, order="C"), numpy.array(bz, order="C"), numpy.array(l2, order="C")


def face_diffusivity(m, k_bg):
    """float64 kd [n x ktot] for ``diffusion.profiles(kd=...)`` from the slab means ``m`` [n x ktot] of km: at face k (between
    the levels k - 1 and k) k_bg + 0.5 (m[k-1] + m[k]); the entry of face 0, the ground, is not used and is k_bg + m[0]"""
    m = numpy.asarray(m, dtype=numpy.float64)
    kd = float(k_bg) + m
    kd[:, 1:] = float(k_bg) + 0.5 * (m[:, :-1] + m[:, 1:])
    return kd
