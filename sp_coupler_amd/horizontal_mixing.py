"""The constants and the coefficients of K26, the implicit horizontal mixing of the device-resident LES fields by each line's own
eddy viscosity (include/spc.h: spc_les_hmix_*): one backward-Euler step of d(x)/dt = d/dx (K dx/dx) per periodic
grid line along i, then one along j, K at a face the mean of K24's UNCAPPED km of its two cells.  The step is unconditionally
stable, so the closure's own viscosity acts where K24's explicit step has to cut it at ``mixing.cap``.

The coefficients are K24's: ``mixing.coefficients`` forms ``ax`` and ``ay`` ONCE in float64 NumPy, one pair for the winds and one
for the scalars (the winds' divided by the Prandtl number), rounded once to the element type on upload; the kernel and the NumPy
oracle of the tests receive the same arrays.  Left out of the rule: a splitting of higher order than Lie's (i, then j), and the
gradients of W in the closure (mixing.py)."""
import numpy

from . import mixing

KH_CAP = 1000.0        # m2/s: the largest face viscosity; a sanity bound that keeps the matrix finite, no stability cap
coefficients = mixing.coefficients


def bound(n, kh_cap=KH_CAP):
    """float64 kh2 [n]: twice the largest face viscosity ``kh_cap`` (a scalar or [n]): the kernel forms the face mean of km as a
    sum.  ValueError for a kh_cap that is not positive and finite"""
    mixing._positive(kh_cap=kh_cap)
    return numpy.array(numpy.broadcast_to(2.0 * numpy.asarray(kh_cap, dtype=numpy.float64), (int(n),)), order="C")
