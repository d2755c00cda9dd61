"""The constants and the coefficients of K16, the horizontal upwind advection of the device-resident LES fields on the doubly
periodic plane (include/spc.h: spc_les_advect_*).

The kernel takes hx = 0.5 dt / dx and hy = 0.5 dt / dy per LES: formed ONCE here, in float64 NumPy, and rounded once to the
element type on upload; the kernel and the NumPy oracle of the tests receive the same arrays, and neither divides."""
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
