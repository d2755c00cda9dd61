"""TEST INFRASTRUCTURE ONLY -- a units shim under which the reference's unmodified ``splib/spcpl.py`` and ``splib/sputils.py``
import and run without omuse / amuse / netCDF4 / shapely.  Written for this project; it holds none of the
reference's text and none of AMUSE's.

One rule: a ``Quantity`` is a float64 ``number`` (NumPy scalar or ndarray) with ONE dummy unit, and every arithmetic operation
on it is the plain NumPy float64 operation on ``.number``, operands in the order the calling text writes them.  Every unit on
the reference's coupling path is SI-coherent with factor 1, so ``value_in`` returns ``.number`` unchanged.  Nothing here
checks dimensions: the shim exists to let the recorder (tests/golden/make_reference_goldens.py) evaluate the reference's
expressions, not to replace a units library.

``ndarray <op> Quantity`` and ``numpy.float64 <op> Quantity`` reach ``Quantity.__array_ufunc__``: the same ufunc on the numbers, in
the same operand order; a float64 result is a Quantity again, and with ``out=`` (``ndarray[...] += Quantity``) the plain array
that was written into comes back.
"""
import numpy


def _n(x):
    return x.number if isinstance(x, Quantity) else x


class Unit:
    """the one dummy unit: products, quotients and powers of units are the same unit; ``x | unit`` makes a Quantity"""
    __array_ufunc__ = None

    def _same(self, *_):
        return self

    __mul__ = __rmul__ = __truediv__ = __rtruediv__ = __pow__ = _same

    def __ror__(self, x):
        return Quantity(x)

    def new_quantity(self, x):
        return Quantity(x)


UNIT = Unit()


class Quantity:
    unit = UNIT

    def __array_ufunc__(self, ufunc, method, *inputs, out=None, **kw):
        if method != "__call__":
            return NotImplemented
        args = [_n(x) for x in inputs]
        if out is not None:
            return ufunc(*args, out=tuple(_n(o) for o in out), **kw)
        res = ufunc(*args, **kw)
        if isinstance(res, (numpy.ndarray, numpy.generic)) and res.dtype == numpy.float64:
            return Quantity(res)
        return res

    def __init__(self, number):
        if isinstance(number, Quantity):
            number = number.number
        if isinstance(number, numpy.ndarray) and number.ndim:
            if number.dtype != numpy.float64:
                number = number.astype(numpy.float64)
        elif isinstance(number, (list, tuple)):
            number = numpy.asarray(number, dtype=numpy.float64)
        else:
            number = numpy.float64(number)
        self.number = number

    def value_in(self, unit):
        return self.number

    def __array__(self, dtype=None, copy=None):
        return numpy.asarray(self.number, dtype=dtype)

    # arithmetic: NumPy's float64 operation on the numbers, operands in the written order
    def __add__(self, o):
        return Quantity(self.number + _n(o))

    def __radd__(self, o):
        return Quantity(_n(o) + self.number)

    def __sub__(self, o):
        return Quantity(self.number - _n(o))

    def __rsub__(self, o):
        return Quantity(_n(o) - self.number)

    def __mul__(self, o):
        return Quantity(self.number * _n(o))

    def __rmul__(self, o):
        return Quantity(_n(o) * self.number)

    def __truediv__(self, o):
        return Quantity(self.number / _n(o))

    def __rtruediv__(self, o):
        return Quantity(_n(o) / self.number)

    def __pow__(self, o):
        return Quantity(self.number ** _n(o))

    def __rpow__(self, o):
        return Quantity(_n(o) ** self.number)

    def __neg__(self):
        return Quantity(-self.number)

    def __abs__(self):
        return Quantity(abs(self.number))

    def __imul__(self, o):              # on a slice: the view's numbers change in place, then __setitem__ stores them back
        self.number *= _n(o)
        return self

    # containers
    def __getitem__(self, i):
        return Quantity(self.number[i])

    def __setitem__(self, i, v):
        self.number[i] = _n(v)

    def __len__(self):
        return len(self.number)

    def __iter__(self):
        return (Quantity(x) for x in self.number)

    def sum(self, *a, **kw):
        return Quantity(self.number.sum(*a, **kw))

    # comparisons and truth: of the numbers
    def __lt__(self, o):
        return self.number < _n(o)

    def __le__(self, o):
        return self.number <= _n(o)

    def __gt__(self, o):
        return self.number > _n(o)

    def __ge__(self, o):
        return self.number >= _n(o)

    def __eq__(self, o):
        return self.number == _n(o)

    def __ne__(self, o):
        return self.number != _n(o)

    __hash__ = None

    def __bool__(self):
        return bool(self.number)

    def __float__(self):
        return float(self.number)

    def __repr__(self):
        return "Quantity(%r)" % (self.number,)


def to_quantity(x):
    return x if isinstance(x, Quantity) else Quantity(x)


class _Units:
    """``units.m``, ``units.K``, ``units.mfu`` ...: every name is the dummy unit"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return UNIT


units = _Units()


class AsyncRequestsPool:
    """imported by the reference at module level; the recorder runs everything synchronously"""

    def __init__(self, *requests):
        self.requests = list(requests)

    def add_request(self, request, *a, **kw):
        self.requests.append(request)

    def waitall(self):
        pass

    def __len__(self):
        return len(self.requests)


class Point:
    """shapely.geometry.Point as far as sputils.get_mask_indices uses it: ``x`` and ``y``"""

    def __init__(self, *args):
        xy = args[0] if len(args) == 1 else args
        self.x, self.y = float(xy[0]), float(xy[1])
