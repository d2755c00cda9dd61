"""The local cloud-water forcing of the LES moisture (qt_forcing 'local' | 'strong', kernel family K19): what the coupler's
cloud-water hand-over (splib/spcpl.py:346-347: set_tendency_QL "used in experimental local qt nudging", set_ref_profile_QL)
becomes per LES and level before ``Engine.les_qt_local`` moves moisture between the cloudy cells and the rest.  NumPy only,
float64; include/spc.h has the rule of the launch itself, DESIGN.md 7.3 its reasons."""
import numpy

KINDS = ("local", "strong")


def increments(kind, f_ql, ql_ref, ql_mean, dt):
    """A [n x ktot] float64: the wanted change of the slab-mean cloud water in one LES step of ``dt`` seconds.
    ``"local"``:  A = f_ql * dt, the relaxed forcing the coupler computed (f_ql in kg/kg/s);
    ``"strong"``: A = ql_ref - ql_mean, the whole gap to the GCM's cloud water closed in this step."""
    if kind == "local":
        return numpy.asarray(f_ql, dtype=numpy.float64) * float(dt)
    if kind == "strong":
        return numpy.asarray(ql_ref, dtype=numpy.float64) - numpy.asarray(ql_mean, dtype=numpy.float64)
    raise ValueError("qt_forcing kind must be one of %s, got %r" % (KINDS, kind))
