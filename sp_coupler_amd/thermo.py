"""The saturation-pressure table and the constants of K12 (include/spc.h: spc_les_thermo_*).

The table is computed ONCE in float64 NumPy and rounded once to the element type; the kernel and the NumPy oracle of the
tests receive the same array, so exp never has to agree between host and device."""
import numpy

from . import sputils

T_LO = 150.0          # K, temperature of table entry 0
STEP = 0.2            # K between entries
INV_STEP = 5.0        # 1 / STEP, exact: what the kernel multiplies by
N_TAB = 2000          # entries: 150.0 ... 549.8 K
#: Newton iterations per cell.  The smallest count whose cloud water lies within 1e-9 kg/kg (the reference's significance
#: bound for cloud water, splib/spcpl.py:661) of 30 iterations everywhere on Tl 230 ... 310 K, p 5e4 ... 1.05e5 Pa,
#: qt 0 ... 0.03 (float64 oracle; DESIGN.md 7.3 has the measured maximum for 1 ... 6 iterations)
DEFAULT_N_ITER = 6


def _np_dtype(dtype):
    try:
        return numpy.dtype(dtype)
    except TypeError:                                  # a torch dtype
        import torch
        return torch.empty(0, dtype=dtype).numpy().dtype


def saturation_table(dtype=numpy.float64):
    """es[m] = 610.78 exp(17.2694 (t - 273.16) / (t - 35.86)) Pa at t = T_LO + STEP m, m < N_TAB, as a NumPy array of
    ``dtype`` (a NumPy or torch dtype)"""
    t = T_LO + STEP * numpy.arange(N_TAB, dtype=numpy.float64)
    es = 610.78 * numpy.exp(17.2694 * (t - 273.16) / (t - 35.86))
    return es.astype(_np_dtype(dtype))


def t_hi(dtype=numpy.float64, n_tab=N_TAB):
    """the temperature of the last table entry in ``dtype``: where the lookup clamps"""
    return _np_dtype(dtype).type(T_LO + STEP * (n_tab - 1))


def exner(presf):
    """(presf / 1e5) ** (rd / cp) in float64 NumPy: the factor K12 multiplies THL by (the kernel forms no power)"""
    return (numpy.asarray(presf, dtype=numpy.float64) / 1e5) ** (sputils.rd / sputils.cp)
