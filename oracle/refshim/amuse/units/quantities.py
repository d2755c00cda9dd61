"""stand-in package, see oracle/refshim/spc_refshim.py"""
from spc_refshim import Quantity, to_quantity  # noqa: F401
