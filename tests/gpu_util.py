"""Helpers shared by the -m gpu parity tests, and the no-device rerun of CPU tests that walk fallbacks."""
import os
import subprocess
import sys

import numpy
import pytest
import torch

EPS = 2.220446049250313e-16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ran_without_a_device(request):
    """For a CPU test of what happens WITHOUT a HIP device (the library's occupancy / CU-count fallbacks, bench.py's live
    PMC pass giving up): False when this process sees no GPU -- the test runs here; True when it does, after the same
    test has passed in a child pytest that sees none (HIP_VISIBLE_DEVICES=-1) -- the test then returns."""
    if not torch.cuda.is_available():
        return False
    if os.environ.get("SPC_TEST_CHILD_WITHOUT_DEVICE"):
        pytest.fail("HIP_VISIBLE_DEVICES=-1 left a device visible to the child process")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", SPC_TEST_CHILD_WITHOUT_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "%s::%s" % (request.node.path, request.node.name)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    return True


def to_dev(d, device, dtype=torch.float64):
    out = {}
    for k, v in d.items():
        t = torch.from_numpy(numpy.ascontiguousarray(v))
        out[k] = t.to(device=device, dtype=dtype if t.is_floating_point() else t.dtype)
    return out


def host(t):
    return t.detach().cpu().numpy()


def assert_bits(name, got, want, dtypes=False):
    """bit-exact including the sign of zero and NaN positions; ``dtypes``: of one dtype as well (where a device tensor is
    compared: a float64 array that happens to hold float32 values is no field of a float32 ensemble)"""
    got, want = numpy.asarray(got), numpy.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert not dtypes or got.dtype == want.dtype, "%s: dtype %s, expected %s" % (name, got.dtype, want.dtype)
    same = (got == want) | (numpy.isnan(got) & numpy.isnan(want))
    assert same.all(), "%s: %d of %d elements differ (max abs %.3e)" % (
        name, (~same).sum(), same.size, numpy.nanmax(numpy.abs(got - want)))
    num = ~numpy.isnan(want)   # the sign bit of a NaN carries no meaning (differs between x86 and gfx950)
    assert numpy.array_equal(numpy.signbit(got)[num], numpy.signbit(want)[num]), name + ": sign of zero differs"


def assert_close_scaled(name, got, want, tol, scale):
    err = numpy.abs(numpy.asarray(got) - numpy.asarray(want))
    assert numpy.isfinite(err).all(), name
    assert err.max() <= tol * scale, "%s: max abs err %.3e > %.3e (tol %.1e x scale %.3e)" % (
        name, err.max(), tol * scale, tol, scale)
