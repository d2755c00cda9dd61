"""The constants and the profiles of K15, the implicit vertical diffusion of the device-resident LES fields with the surface
fluxes (include/spc.h: spc_les_diffuse_*).

The matrix of the backward-Euler step depends on the LES and the level only, so the Thomas elimination is done ONCE per LES
here, in float64 NumPy, and rounded once to the element type on upload; the kernel and the NumPy oracle of the tests receive
the same arrays, and neither divides."""
import numpy

from . import microphysics

K_MAX = 50.0          # m2/s: the eddy diffusivity at a third of the mixed layer, on top of K_BG
H_MIX = 1500.0        # m: depth of the mixed layer
K_BG = 0.1            # m2/s: the background diffusivity, everywhere


def diffusivity(zh, k_max=K_MAX, h_mix=H_MIX, k_bg=K_BG):
    """Kd at the faces ``zh``: k_bg + k_max (27/4) s (1 - s)**2 with s = clip(zh / h_mix, 0, 1) (maximum k_bg + k_max at
    s = 1/3); ``h_mix`` may be [n x 1] against ``zh`` [n x nL]"""
    s = numpy.clip(numpy.asarray(zh, dtype=numpy.float64) / h_mix, 0.0, 1.0)
    return k_bg + k_max * (27.0 / 4.0) * s * (1.0 - s) ** 2


def matrix(zh, zf, rhobf, dt, k_max=K_MAX, h_mix=H_MIX, k_bg=K_BG, kd=None):
    """float64 ``(a, b, c, w, dz)``, [n x nL] each: the lower, main and upper diagonal of one backward-Euler step of
    d(x)/dt = (1 / (rho dz)) d/dz (rho_h K dx/dz), K13's weights w = rhobf * dz and dz.  ``kd``: the diffusivity at the faces
    ``zh`` [n x nL] (the value at face 0, the ground, is not used) in place of ``diffusivity``'s profile; None: that profile"""
    rhobf = numpy.atleast_2d(numpy.asarray(rhobf, dtype=numpy.float64))
    shape = rhobf.shape
    dz = numpy.broadcast_to(microphysics.layer_thickness(zh, zf), shape)
    zh = numpy.broadcast_to(numpy.asarray(zh, dtype=numpy.float64), shape)
    zf = numpy.broadcast_to(numpy.asarray(zf, dtype=numpy.float64), shape)
    w = rhobf * dz
    g = numpy.zeros(shape)                                      # face conductance; face k lies at zh[k], g[0] = 0: no face below
    if shape[-1] > 1:
        if kd is None:
            kf = diffusivity(zh[..., 1:], k_max, h_mix, k_bg)
        else:
            kf = numpy.broadcast_to(numpy.asarray(kd, dtype=numpy.float64), shape)[..., 1:]
            if not (numpy.isfinite(kf).all() and (kf >= 0).all()):
                raise ValueError("the face diffusivity kd must be finite and not negative")
        g[..., 1:] = 0.5 * (rhobf[..., 1:] + rhobf[..., :-1]) * kf / (zf[..., 1:] - zf[..., :-1])
    a = -float(dt) * g / w
    c = numpy.zeros(shape)
    c[..., :-1] = -float(dt) * g[..., 1:] / w[..., :-1]
    b = 1.0 - a - c
    return a, b, c, w, dz


def profiles(zh, zf, rhobf, dt, k_max=K_MAX, h_mix=H_MIX, k_bg=K_BG, kd=None):
    """float64 ``(a, m, cp, s0)`` of LES with the half levels ``zh`` and full levels ``zf`` ([nL] or [n x nL]) and the
    base-state density ``rhobf`` [n x nL] for a step of ``dt`` seconds: ``a`` the lower diagonal, ``m`` the reciprocal pivots
    and ``cp`` the eliminated upper diagonal of the Thomas algorithm, [n x nL] each, and s0 = dt / dz[0], [n]:
    m[0] = 1 / b[0], cp[0] = c[0] m[0], m[k] = 1 / (b[k] - a[k] cp[k - 1]), cp[k] = c[k] m[k].  The matrix is an M-matrix:
    m lies in (0, 1] and cp in (-1, 0].  ``kd``: ``matrix``'s (the eddy viscosity of K24 in place of the prescribed profile)."""
    a, b, c, _, dz = matrix(zh, zf, rhobf, dt, k_max, h_mix, k_bg, kd)
    m, cp = numpy.empty_like(a), numpy.empty_like(a)
    m[..., 0] = 1.0 / b[..., 0]
    cp[..., 0] = c[..., 0] * m[..., 0]
    for k in range(1, a.shape[-1]):
        m[..., k] = 1.0 / (b[..., k] - a[..., k] * cp[..., k - 1])
        cp[..., k] = c[..., k] * m[..., k]
    return numpy.array(a, order="C"), m, cp, numpy.array(float(dt) / dz[..., 0], order="C")
