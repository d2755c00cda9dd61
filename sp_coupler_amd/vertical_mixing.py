"""The constants, the coefficients and the profiles of K25, the implicit vertical mixing of the device-resident LES fields by each
column's own eddy viscosity (include/spc.h: spc_les_vmix_*): one backward-Euler step of
d(x)/dt = (1 / (rho dz)) d/dz (rho_h K dx/dz) per column, K at a face the mean of K24's km of its two cells plus a background,
with K15's surface fluxes and a neutral bulk drag on the lowest wind level.

Everything the kernel multiplies by is computed ONCE in float64 NumPy and rounded once to the element type on upload; the kernel
and the NumPy oracle of the tests receive the same arrays.  The winds and the scalars differ by the Prandtl number in ``el`` and
``eu`` alone: one pair of profiles per class, so the kernel needs no extra rounding.  Left out of the rule: a drag that depends
on the stability (Monin-Obukhov), and the gradients of W in the closure (mixing.py)."""
import numpy

from . import diffusion, microphysics, mixing

K_BG = diffusion.K_BG  # m2/s: the background diffusivity, everywhere (K15's)
KV_CAP = 1000.0        # m2/s: the largest face diffusivity; a sanity bound that keeps the matrix finite, no stability cap
KAPPA = mixing.KAPPA   # von Karman's constant of the drag coefficient


def coefficients(zh, zf, rhobf, dt, prandtl=mixing.PRANDTL):
    """float64 ``((el, eu) of the winds, (el, eu) of the scalars, s0)`` of LES with the half levels ``zh`` and full levels ``zf``
    ([ktot] or [n x ktot]) and the base-state density ``rhobf`` [n x ktot] for a step of ``dt`` seconds, [n x ktot] each and s0 [n]:
    with w = rhobf dz and rho_h[k] the mean of rhobf[k - 1] and rhobf[k],
    el[k] = 0.5 dt rho_h[k] / (w[k] (zf[k] - zf[k - 1])) and eu[k] = 0.5 dt rho_h[k + 1] / (w[k] (zf[k + 1] - zf[k])) for the winds
    (0.5: the kernel forms the face mean of km as a sum), the same divided by ``prandtl`` for the scalars; el[0] and eu[ktot - 1],
    which the kernel never reads, are 0; s0 = dt / dz[0].  ValueError for a dt or prandtl that is not positive and finite and for
    levels that do not ascend"""
    mixing._positive(dt=dt, prandtl=prandtl)
    rhobf = numpy.atleast_2d(numpy.asarray(rhobf, dtype=numpy.float64))
    shape = rhobf.shape
    dz = numpy.broadcast_to(microphysics.layer_thickness(zh, zf), shape)
    zf = numpy.broadcast_to(numpy.asarray(zf, dtype=numpy.float64), shape)
    mixing._positive(rhobf=rhobf, dz=dz)
    w = rhobf * dz
    el, eu = numpy.zeros(shape), numpy.zeros(shape)
    if shape[-1] > 1:
        span = zf[..., 1:] - zf[..., :-1]
        mixing._positive(span=span)
        g = 0.5 * float(dt) * (0.5 * (rhobf[..., 1:] + rhobf[..., :-1])) / span          # at the faces 1 ... ktot - 1
        el[..., 1:] = g / w[..., 1:]
        eu[..., :-1] = g / w[..., :-1]
    s0 = numpy.array(float(dt) / dz[..., 0], order="C")
    return (el, eu), (el / float(prandtl), eu / float(prandtl)), s0


def background(n, ktot, k_bg=K_BG, kv_cap=KV_CAP):
    """float64 ``(kb, kv2)``: kb [n x ktot], twice the background diffusivity ``k_bg`` (a scalar, [ktot] or [n x ktot]; not negative)
    at every face, and kv2 [n], twice the largest face diffusivity ``kv_cap`` (a scalar or [n]; positive).  ValueError otherwise"""
    k_bg = numpy.asarray(k_bg, dtype=numpy.float64)
    if not (numpy.isfinite(k_bg).all() and (k_bg >= 0).all()):
        raise ValueError("the vertical mixing (K25) needs a finite k_bg that is not negative, got %r" % (k_bg,))
    mixing._positive(kv_cap=kv_cap)
    kb = numpy.array(numpy.broadcast_to(2.0 * k_bg, (int(n), int(ktot))), order="C")
    kv2 = numpy.array(numpy.broadcast_to(2.0 * numpy.asarray(kv_cap, dtype=numpy.float64), (int(n),)), order="C")
    return kb, kv2


def drag(z0m, zf, dz, dt):
    """float64 dr [n] = dt cd / dz[0] with the neutral drag coefficient cd = (KAPPA / ln(zf[0] / z0m))^2 of the roughness lengths
    ``z0m`` (a scalar or [n]), the lowest full level ``zf`` and the thickness ``dz`` of the lowest layer ([ktot] or [n x ktot]; only
    level 0 is read).  ValueError for a z0m outside (0, zf[0])"""
    mixing._positive(dt=dt)
    z0m = numpy.atleast_1d(numpy.asarray(z0m, dtype=numpy.float64))
    zf0 = numpy.broadcast_to(numpy.asarray(zf, dtype=numpy.float64)[..., 0], z0m.shape)
    dz0 = numpy.broadcast_to(numpy.asarray(dz, dtype=numpy.float64)[..., 0], z0m.shape)
    mixing._positive(dz=dz0)
    if not (numpy.isfinite(z0m).all() and (z0m > 0).all() and (z0m < zf0).all()):
        raise ValueError("the drag (K25) needs a roughness length z0m inside (0, zf[0]), got %r against zf[0] = %r" % (z0m, zf0))
    cd = (KAPPA / numpy.log(zf0 / z0m)) ** 2
    return numpy.array(float(dt) * cd / dz0, order="C")
