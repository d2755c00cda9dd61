"""sp_coupler_amd.device_les holds the device ensemble; sp_coupler_amd.models hands out the same objects and does not import
it (nor torch through it) before one of them is asked for."""
import subprocess
import sys

from sp_coupler_amd import device_les, models


def _child(code):
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)


def test_models_hands_out_the_objects_of_device_les():
    assert models.DeviceLESEnsemble is device_les.DeviceLESEnsemble and models._DeviceLESRow is device_les._DeviceLESRow
    assert device_les.DeviceLESEnsemble.__module__ == "sp_coupler_amd.device_les"
    assert issubclass(device_les.DeviceLESEnsemble, models.SyntheticLESEnsemble)
    assert not hasattr(models, "no_such_name")


def test_either_module_can_be_imported_first_and_models_alone_leaves_device_les_out():
    r = _child("import sp_coupler_amd.device_les as d, sp_coupler_amd.models as m; assert m.DeviceLESEnsemble is d.DeviceLESEnsemble")
    assert r.returncode == 0, r.stderr
    r = _child("import sys, sp_coupler_amd.models as m; assert 'sp_coupler_amd.device_les' not in sys.modules; "
               "m._DeviceLESRow; assert 'sp_coupler_amd.device_les' in sys.modules")
    assert r.returncode == 0, r.stderr
