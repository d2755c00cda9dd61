"""The constants and the profiles of K21, the hydrostatic pressure force of the device-resident LES fields (include/spc.h:
spc_les_buoyancy_*): the buoyancy of every column against the virtual potential temperature of the slab means is
integrated downward from the lid to a pressure perturbation, and the horizontal gradient of that pressure accelerates U and V.

The profiles are computed ONCE in float64 NumPy and rounded once to the element type on upload; the kernel and the NumPy oracle
of the tests receive the same arrays, so neither a power nor a division of the host has to agree with one of the device."""
import math

import numpy

from . import microphysics, sputils, thermo

GRAV, RLV, CP, RD, RV = sputils.grav, sputils.rlv, sputils.cp, sputils.rd, sputils.rv
C1 = RV / RD - 1.0    # the weight of the vapour in the virtual potential temperature
C2 = RV / RD          # the weight of the liquid water
#: m/s: the fastest internal mode N H / pi of a troposphere of H = 10 km with N = 0.01 / s.  A parameter, not a measurement:
#: the substeps of DeviceLESEnsemble.enable_buoyancy() keep wave_speed * dt / min(dx, dy) below the Courant limit.
WAVE_SPEED = 30.0


def profiles(thl, qt, ql, presf, zh, zf=None):
    """float64 ``(t0, lex, s)``, [n x ktot] each, of LES with the slab means ``thl``, ``qt`` and ``ql`` (``ql`` None: no liquid
    water), the pressure ``presf`` [n x ktot] and the half levels ``zh`` ([ktot] or [n x ktot]; the layer thickness is that of
    ``water_path_weights``: an LES of one level needs its full level ``zf`` as well):
    lex = rlv / (cp * exner(presf)), what a unit of liquid water adds to THL;
    t0 = (thl + lex ql) * ((1 + c1 qt) - c2 ql), the virtual potential temperature of the means;
    s = 0.5 * grav * dz / t0, half a layer's weight per unit of virtual potential temperature.
    ValueError where a dz or t0 is not positive, or where anything is not finite."""
    thl = numpy.asarray(thl, dtype=numpy.float64)
    qt = numpy.asarray(qt, dtype=numpy.float64)
    ql = numpy.zeros_like(thl) if ql is None else numpy.asarray(ql, dtype=numpy.float64)
    zh = numpy.asarray(zh, dtype=numpy.float64)
    if zh.shape[-1] < 2 and zf is None:
        raise ValueError("an LES of one level needs zf for its layer thickness")
    dz = numpy.broadcast_to(microphysics.layer_thickness(zh, zf), thl.shape)
    ex = thermo.exner(presf)
    if not (thl.ndim == 2 and qt.shape == thl.shape and ql.shape == thl.shape and ex.shape == thl.shape):
        raise ValueError("the means and the pressure must be [n x ktot]")
    if not (numpy.isfinite(dz).all() and (dz > 0).all() and numpy.isfinite(ex).all() and (ex > 0).all()):
        raise ValueError("the layer thickness and the pressure must be positive and finite")
    lex = RLV / (CP * ex)
    t0 = (thl + lex * ql) * ((1.0 + C1 * qt) - C2 * ql)
    if not (numpy.isfinite(t0).all() and (t0 > 0).all()):
        raise ValueError("the virtual potential temperature of the means must be positive and finite")
    s = 0.5 * GRAV * dz / t0
    return numpy.array(t0, order="C"), numpy.array(lex, order="C"), numpy.array(s, order="C")


def wave_substeps(dt, dx, dy, cfl, wave_speed=WAVE_SPEED):
    """the substeps that keep the fastest gravity wave below the Courant limit: max(1, ceil(wave_speed * dt / (cfl * min(dx, dy))))"""
    d = min(float(numpy.min(dx)), float(numpy.min(dy)))
    return max(1, int(math.ceil(float(wave_speed) * float(dt) / (float(cfl) * d))))
