"""stand-in package, see oracle/refshim/spc_refshim.py"""
from spc_refshim import Point  # noqa: F401
