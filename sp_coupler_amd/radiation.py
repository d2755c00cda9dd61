"""The constants, the table and the profiles of K18, the longwave cooling and warming that the liquid water of a column of the
device-resident LES fields gives its own air (include/spc.h: spc_les_radiate_*): the first two terms of the
GCSS / DYCOMS-II parametrised flux (Stevens et al. 2005, Mon. Wea. Rev. 133, eq. 3),

    F(z) = F0 exp(-Q(z, inf)) + F1 exp(-Q(0, z)),        Q(a, b) = kappa * integral from a to b of rho ql dz.

The third term, the cooling of the free troposphere above the inversion, needs the inversion height of every column and is
left out.

The profiles and the table of exp(-x) are computed ONCE in float64 NumPy and rounded once to the element type on upload; the
kernel and the NumPy oracle of the tests receive the same arrays, so neither an exp nor a division of the host has to agree
with one of the device."""
import numpy

from . import advection, sputils, thermo

F0 = 70.0             # W/m2: the flux that a thick cloud takes from the air at its top
F1 = 22.0             # W/m2: the flux that it gives the air at its base
KAPPA = 85.0          # m2/kg: the absorptivity of liquid water
STEP = 1.0 / 64       # optical depth between two table nodes
INV_STEP = 64.0       # 1 / STEP, a power of two: s = x * INV_STEP and fr = s - m are exact
N_TAB = 2049          # nodes: x = 0 ... 32, where exp(-x) is 1.3e-14


def exp_table(dtype=numpy.float64):
    """etab[m] = exp(-STEP m), m < N_TAB, computed in float64 and rounded once to ``dtype`` (a NumPy or torch dtype);
    etab[0] is exactly 1"""
    x = STEP * numpy.arange(N_TAB, dtype=numpy.float64)
    return numpy.exp(-x).astype(thermo._np_dtype(dtype))


def x_hi(dtype=numpy.float64, n_tab=N_TAB, inv_step=INV_STEP):
    """the optical depth of the last table node in ``dtype``: where the lookup clamps"""
    return thermo._np_dtype(dtype).type(float(n_tab - 1) / float(inv_step))


def profiles(rhobf, zh, presf, dt, kappa=KAPPA, zf=None):
    """float64 ``(w, c)``, [n x ktot] each, of LES with the base-state density ``rhobf`` and the pressure ``presf`` [n x ktot]
    and the half levels ``zh`` ([ktot] or [n x ktot]; the layer thickness is that of ``water_path_weights``: an LES of one level
    needs its full level ``zf`` as well) for a step of ``dt`` seconds: with g = rhobf * dz (``advection.vertical_profiles``),
    w = kappa * g, the optical depth of a layer per unit of liquid water (``kappa``: a scalar or one per LES), and
    c = dt / (cp * g * exner(presf)), the THL change per W/m2 of flux divergence.  ValueError where a dz or a density is
    not positive, or where anything is not finite."""
    from . import microphysics
    rhobf = numpy.asarray(rhobf, dtype=numpy.float64)
    zh = numpy.asarray(zh, dtype=numpy.float64)
    if zh.shape[-1] < 2 and zf is None:
        raise ValueError("an LES of one level needs zf for its layer thickness")
    dz = numpy.broadcast_to(microphysics.layer_thickness(zh, zf), rhobf.shape)
    kappa = numpy.asarray(kappa, dtype=numpy.float64)
    dt = float(dt)
    if not (numpy.isfinite(dz).all() and (dz > 0).all() and numpy.isfinite(rhobf).all() and (rhobf > 0).all()):
        raise ValueError("the layer thickness and the density must be positive and finite")
    ex = thermo.exner(presf)
    if not (numpy.isfinite(kappa).all() and numpy.isfinite(dt) and numpy.isfinite(ex).all() and ex.shape == rhobf.shape):
        raise ValueError("kappa, dt and the pressure [n x ktot] must be finite")
    if kappa.ndim:
        if kappa.shape != rhobf.shape[:1]:
            raise ValueError("kappa must be a scalar or one value per LES")
        kappa = kappa[:, None]
    g, _ = advection.vertical_profiles(rhobf * dz)
    w = kappa * g
    c = dt / ((sputils.cp * g) * ex)
    if not (numpy.isfinite(w).all() and numpy.isfinite(c).all()):
        raise ValueError("the profiles are not finite")
    return numpy.array(w, order="C"), numpy.array(c, order="C")
