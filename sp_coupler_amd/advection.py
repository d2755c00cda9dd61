"""The constants and the coefficients of K16, the horizontal upwind advection of the device-resident LES fields on the doubly
periodic plane (include/spc.h: spc_les_advect_*), and the profiles of K17, their vertical advection by the mass
flux of continuity (spc_les_vadvect_*), and of K22, their conservative transport along all three axes in one launch
(spc_les_transport_*).

The kernel takes hx = 0.5 dt / dx and hy = 0.5 dt / dy per LES: formed ONCE here, in float64 NumPy, and rounded once to the
element type on upload; the kernel and the NumPy oracle of the tests receive the same arrays, and neither divides.  K17 takes
g = rho dz and r = 1 / g per LES and level (``vertical_profiles``), formed the same way; neither depends on dt.

K22 (``Engine.les_transport``) takes the same hx, hy, g and r.  Its rule, per cell (l, i, j, k) in the element type, one
rounding per operation, no fma, no division (include/spc.h is the definition):
    cw, ce, cs, cn                      K16's face Courant numbers
    d = (ce - cw) + (cn - cs);  e = g * d;  M[0] = +0;  M[k+1] = M[k] - e        K17's chain; mtop = M[k+1]
    pw = cw > 0 ? cw : 0;  qw = cw < 0 ? cw : 0       likewise (pe, qe), (ps, qs), (pn, qn), (pb, qb) of M[k], (pt, qt) of M[k+1]
    Fw = pw * x[im] + qw * x;   Fe = pe * x + qe * x[ip];   Fs = ps * x[jm] + qs * x;   Fn = pn * x + qn * x[jp]
    Fb = pb * x[km] + qb * x;   Ft = pt * x + qt * x[kp]                         km, kp clamped: closed ground, open lid
    x' = (x - ((Fe - Fw) + (Fn - Fs))) - r * (Ft - Fb)
    s  = ((pe - qw) + (pn - qs)) + r * (pt - qb)      the outflow Courant sum: x' is a convex combination where s <= 1
    ftop = Ft at the top level                        what left through the lid, in units of g x
Both cells that share a face form its flux from the same operands, so sum(g x') + sum(ftop) = sum(g x) to rounding
(``lid_budget``); a constant stays constant to rounding, not bit for bit.

K23 (``Engine.les_transport2``) is K22 with a second-order face value: every face adds to its donor flux a correction from
the slope of its upwind cell, 0.5 * (p * (1 - p) * s[upwind of p] - q * (1 + q) * s[upwind of q]), the slope
0.5 * ((x - x[m]) + (x[p] - x)) unlimited or MC-limited (include/spc.h); hx, hy, g, r, cmax, mtop and the budget are K22's."""
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


def lid_budget(g, x_old, x_new, ftop):
    """float64 ``(residual, scale)``, [n] each, of one K22 step (or of several, ``ftop`` their sum) on the host:
    residual = sum_ijk g x_new + sum_ij ftop - sum_ijk g x_old and scale = sum_ijk g |x_old| per LES, every sum formed with
    ``math.fsum`` of float64 products (exact for float32 inputs), so the residual holds the step's own roundings only.
    ``g`` [n x ktot], the fields [n x itot x jtot x ktot], ``ftop`` [n x itot x jtot] or None (a closed lid)"""
    g = numpy.asarray(g, dtype=numpy.float64)
    a, b = numpy.asarray(x_old, dtype=numpy.float64), numpy.asarray(x_new, dtype=numpy.float64)
    n = a.shape[0]
    res, scale = numpy.zeros(n), numpy.zeros(n)
    for l in range(n):
        w = g[l][None, None, :]
        lid = [] if ftop is None else list(numpy.asarray(ftop[l], dtype=numpy.float64).ravel())
        res[l] = math.fsum(list((w * b[l]).ravel()) + lid + list(-(w * a[l]).ravel()))
        scale[l] = math.fsum((w * numpy.abs(a[l])).ravel())
    return res, scale
