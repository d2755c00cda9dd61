"""stand-in for netCDF4: the reference's spio imports it at module level; the recorder opens no file (see spc_refshim.py)"""


class Dataset:
    def __init__(self, *a, **kw):
        raise RuntimeError("oracle/refshim: netCDF4 is a stand-in, no file can be opened")
