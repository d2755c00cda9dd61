"""The constants and the profiles of K14, the warm-rain microphysics of the device-resident LES fields (include/spc.h:
spc_les_microphysics_*).

The profiles are computed ONCE in float64 NumPy and rounded once to the element type on upload; the kernel and the NumPy
oracle of the tests receive the same arrays, so no division of the host has to agree with one of the device."""
import numpy

from . import sputils, thermo

QC0 = 5e-4            # kg/kg: cloud water above it converts to rain
K_AUTO = 1e-3         # 1/s: rate of the autoconversion of the excess
K_ACC = 2.2           # 1/s per kg/kg of rain: rate of the accretion
T_UP = 268.0          # K: at and above it the cloud water holds no ice
T_DN = 253.0          # K: at and below it the cloud water is all ice
V_FALL = 5.0          # m/s: fall speed of the rain


def layer_thickness(zh, zf):
    """dz of ``DeviceLESEnsemble.water_path_weights()``: dz[k] = zh[k + 1] - zh[k] from the half levels (the lower faces), the
    top layer takes the thickness of the layer below it; an LES of one level twice the distance of zf from zh"""
    zh = numpy.asarray(zh, dtype=numpy.float64)
    if zh.shape[-1] > 1:
        dz = numpy.diff(zh, axis=-1)
        return numpy.concatenate([dz, dz[..., -1:]], axis=-1)
    return 2.0 * (numpy.asarray(zf, dtype=numpy.float64) - zh)


def profiles(zh, zf, rhobf, presf, dt, v_fall=V_FALL):
    """float64 ``(sed_out, sed_in, lcpex, w)``, [n x nL] each, of LES with the half levels ``zh`` and full levels ``zf`` ([nL]
    or [n x nL]), the base-state density ``rhobf`` and the pressure ``presf`` [n x nL], for a step of ``dt`` seconds:
    w = rhobf * dz (K13's weights); c = min(v_fall dt / dz, 1), the share of a layer's rain that leaves it (upwind, never more
    than there is); sed_out = c; sed_in[k] = c[k + 1] w[k + 1] / w[k], the mass that leaves layer k + 1 as mixing ratio of
    layer k, 0 at the top; lcpex = (rlv / cp) / exner(presf)."""
    rhobf = numpy.asarray(rhobf, dtype=numpy.float64)
    dz = layer_thickness(zh, zf)
    w = rhobf * dz
    c = numpy.broadcast_to(numpy.minimum(float(v_fall) * float(dt) / dz, 1.0), w.shape)
    sed_in = numpy.zeros_like(w)
    sed_in[..., :-1] = c[..., 1:] * w[..., 1:] / w[..., :-1]
    lcpex = (sputils.rlv / sputils.cp) / thermo.exner(presf)
    return numpy.array(c, order="C"), sed_in, lcpex, w
