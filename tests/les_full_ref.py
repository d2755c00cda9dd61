"""The host twins of models.DeviceLESEnsemble and the oracle-backed engine with every opt-in mode up to K23 and the statistics in
one class.  The twins of K24 (tests/les_mix_ref.py) and, on those, of K25 (tests/les_vmix_ref.py: the top of the chain, what
tests/ensemble_sequences.py runs) stand on these.  Nothing is defined a second time: the mixins of tests/les_qt_local_ref.py (K19),
tests/les_transport2_ref.py (K23, and K22 below it) and tests/les_buoyancy_ref.py (K21, on the twins of K18 and everything
before it) stay the definitions; this module composes them and adds what only a sequence of operations needs:

  * ``enable_advection`` called again forgets the last step of the earlier call (W, the lid flux, the vertical Courant sum) and
    drops the buoyancy until ``enable_buoyancy`` is called again, as DeviceLESEnsemble.enable_advection documents;
  * ``enable_buoyancy`` forgets the pressure and the wind change of an earlier call; ``get_pressure_batched`` answers only while
    the buoyancy is enabled, ``get_lid_flux_batched`` only in the conservative mode;
  * ``get_statistics``, computed eagerly from the twin's own fields by the oracle of K20 (tests/les_moments_ref.py)."""
from tests import les_buoyancy_ref as lbr
from tests import les_moments_ref as lmo
from tests import les_qt_local_ref as qlr
from tests import les_transport2_ref as lt2


class FullOracleEngine(lmo.MomentsOracleEngine, lt2.Transport2OracleEngine):
    """every launch of the device ensemble by a NumPy oracle: K20 and K19 on one branch, K23, K22 and K21 on the other, K18 and
    everything before it below both"""


class _HostFull:
    def enable_advection(self, **kw):
        super().enable_advection(**kw)
        self._mtop = self._mtop_dt = self._lid = self.advect_courant_z = None
        self.buoyancy_wave_speed = self.buoyancy_wind_change = self._phi = None

    def enable_buoyancy(self, wave_speed=None):
        super().enable_buoyancy(wave_speed)
        self.buoyancy_wind_change = self._phi = None

    def get_pressure_batched(self):
        return self._phi if self.buoyancy_wave_speed is not None else None

    def get_lid_flux_batched(self):
        return self._lid if self.advect_conservative else None

    def get_statistics(self, names=None, pairs=None):
        """what DeviceLESEnsemble.get_statistics returns, of the fields as they are now; W is the twin's own"""
        return lmo.twin_statistics(self, self.get_vertical_wind_batched(), names, pairs)

    def row_statistics(self, i, names=None, pairs=None):
        """what row i's get_statistics returns"""
        host = self.get_statistics(names, pairs)
        return {kind: (v[i].copy() if kind == "TKE" else {k: a[i].copy() for k, a in v.items()}) for kind, v in host.items()}


class HostFullLESEnsemble(_HostFull, qlr._HostQtLocal, lt2._HostTransport2, lbr.HostBuoyancyLESEnsemble):
    """without enable_thermo(): QL = max(QT - Qsat, 0)"""


class HostThermoFullLESEnsemble(_HostFull, qlr._HostQtLocal, lt2._HostTransport2, lbr.HostThermoBuoyancyLESEnsemble):
    """after enable_thermo(): K12's oracle wherever QL is read"""
