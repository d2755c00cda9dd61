"""stand-in package, see oracle/refshim/spc_refshim.py"""
