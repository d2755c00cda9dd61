"""What the second moments of an LES ensemble's fields are taken of (K20, ``Engine.les_moments``): the fields, the
pairs whose covariances are the resolved turbulent fluxes, and the turbulence kinetic energy of the variances.  NumPy only."""
import numpy

# the fields ``DeviceLESEnsemble.get_statistics_batched`` covers where the ensemble holds them (W: the vertical wind of K17, which
# is given at the upper faces of the cells and brought to their centres first)
FIELDS = ("U", "V", "W", "THL", "QT", "QL", "QR")
# the covariances: w'thl', w'qt', u'w', v'w' (the resolved fluxes) and thl'qt'
PAIRS = (("W", "THL"), ("W", "QT"), ("U", "W"), ("V", "W"), ("THL", "QT"))
FACE = "W"


def tke(var):
    """the resolved turbulence kinetic energy per level, ``0.5 * (var U + var V + var W)`` in float64, of a dict of host
    variances; an ensemble without a vertical wind has no W and the term is left out"""
    u, v = numpy.asarray(var["U"], dtype=numpy.float64), numpy.asarray(var["V"], dtype=numpy.float64)
    w = numpy.asarray(var.get("W", 0), dtype=numpy.float64)
    return 0.5 * (u + v + w)
