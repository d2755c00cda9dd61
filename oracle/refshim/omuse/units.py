"""stand-in package, see oracle/refshim/spc_refshim.py"""
from spc_refshim import units  # noqa: F401
