"""The constants and the coefficients of K16, the horizontal upwind advection of the device-resident LES fields on the doubly
periodic plane (include/spc.h: spc_les_advect_*), and the profiles of K17, their vertical advection by the mass
flux of continuity (spc_les_vadvect_*).

The kernel takes hx = 0.5 dt / dx and hy = 0.5 dt / dy per LES: formed ONCE here, in float64 NumPy, and rounded once to the
element type on upload; the kernel and the NumPy oracle of the tests receive the same arrays, and neither divides.  K17 takes
g = rho dz and r = 1 / g per LES and level (``vertical_profiles``), formed the same way; neither depends on dt."""
import math

import numpy

DX = 200.0            # m: the grid spacing along i
DY = 200.0            # m: the grid spacing along j
CFL = 0.5             # the largest Courant sum ((pw + pe) + ps) + pn of a cell a substep may have
MAX_SUBSTEPS = 256    # a step that would need more is refused


def coefficients(dt, dx=DX, dy=DY, n=None):
    """float64 ``(hx, hy)``, [n] each: 0.5 * dt / dx and 0.5 * dt / dy of LES with the grid spacings ``dx`` and ``dy`` (scalars or
    [n]) for a step of ``dt`` seconds"""
    dx, dy = numpy.asarray(dx, dtype=numpy.float64), numpy.asarray(dy, dtype=numpy.float64)
    if not ((dx > 0).all() and (dy > 0).all() and numpy.isfinite(dx).all() and numpy.isfinite(dy).all()):
        raise ValueError("the grid spacings must be positive and finite")
    shape = (int(n),) if n is not None else numpy.broadcast(dx, dy).shape or (1,)
    hx = numpy.broadcast_to(0.5 * float(dt) / dx, shape)
    hy = numpy.broadcast_to(0.5 * float(dt) / dy, shape)
    return numpy.array(hx, order="C"), numpy.array(hy, order="C")


def substeps(c, cfl=CFL, max_substeps=MAX_SUBSTEPS):
    """the substeps of a step whose largest Courant sum with the coefficients of the whole step is ``c``:
    max(1, ceil(c / cfl)); RuntimeError (naming c) where c is not finite or more than ``max_substeps`` would be needed"""
    c = float(c)
    if not math.isfinite(c):
        raise RuntimeError("the advection (K16) found the Courant sum c = %r: the winds are not finite" % c)
    n_sub = max(1, int(math.ceil(c / float(cfl))))
    if n_sub > int(max_substeps):
        raise RuntimeError("the advection (K16) found the Courant sum c = %r: %d substeps at cfl %g, more than max_substeps = %d"
                           % (c, n_sub, float(cfl), int(max_substeps)))
    return n_sub


def vertical_profiles(weights):
    """float64 ``(g, r)``, the shape of ``weights``: g = rho * dz (``DeviceLESEnsemble.water_path_weights()``) and r = 1 / g, the
    profiles of K17; ValueError unless every weight is positive and finite"""
    g = numpy.array(weights, dtype=numpy.float64, order="C")
    if not (numpy.isfinite(g).all() and (g > 0).all()):
        raise ValueError("the weights rho * dz must be positive and finite")
    return g, 1.0 / g


def vertical_wind(mtop, rhobf, dt):
    """W in m/s at the upper faces of the cells from K17's ``mtop`` [n x itot x jtot x nL] (the mass through the upper face in
    a step of ``dt`` seconds, kg / m2, positive upward) and the density profile ``rhobf`` [n x nL] on the same device:
    mtop / (rho_face * dt), rho_face[k] = 0.5 (rhobf[k] + rhobf[min(k + 1, nL - 1)]).  A torch expression, not bit-checked."""
    import torch
    up = torch.cat([rhobf[:, 1:], rhobf[:, -1:]], dim=1)
    face = 0.5 * (rhobf + up)
    return mtop / (face * float(dt))[:, None, None, :]
