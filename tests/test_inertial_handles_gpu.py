"""The omv_inertial_opt handle's memory (openmavis_amd/csrc/inertial.hip): every buffer goes through omv_host.h's
DeviceArena, so create / destroy returns omv_debug_live_allocations to where it was, a create that fails at any of its
allocations returns OMV_ERR_HIP, leaves *out alone and leaks nothing, and one handle serves growing and shrinking calls.
The counterpart of tests/test_mlpnp_handles_gpu.py for this handle."""
import ctypes

import numpy as np
import pytest

from openmavis_amd import _lib, inertial_init as ii, synth_inertial as si

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEAD0
N_ALLOC = 7   # the upload and read-back blocks (device + pinned), the workspace, the two debug buffers


@pytest.fixture
def lib(torch_cuda):
    lib = _lib.load()
    assert lib.omv_debug_fail_allocation(0) == _lib.OMV_OK
    yield lib
    assert lib.omv_debug_fail_allocation(0) == _lib.OMV_OK


def _live(lib):
    n = ctypes.c_int64(-1)
    assert lib.omv_debug_live_allocations(ctypes.byref(n)) == _lib.OMV_OK
    return n.value


def test_create_destroy_returns_every_allocation(lib):
    base = _live(lib)
    for _ in range(3):
        out = ctypes.c_void_p()
        assert lib.omv_inertial_opt_create(2, 16, 16, ctypes.byref(out)) == _lib.OMV_OK
        assert _live(lib) == base + N_ALLOC
        assert lib.omv_inertial_opt_destroy(out) == _lib.OMV_OK
        assert _live(lib) == base


def test_create_unwinds_a_failure_at_each_allocation(lib):
    base = _live(lib)
    k = 0
    while True:
        k += 1
        assert k <= 100, "create never succeeded"
        assert lib.omv_debug_fail_allocation(k) == _lib.OMV_OK
        out = ctypes.c_void_p(SENTINEL)
        st = lib.omv_inertial_opt_create(2, 16, 16, ctypes.byref(out))
        if st == _lib.OMV_OK:
            break
        assert st == _lib.OMV_ERR_HIP, (k, st)
        assert out.value == SENTINEL, k
        assert _live(lib) == base, k
    assert lib.omv_debug_fail_allocation(0) == _lib.OMV_OK
    assert k - 1 == N_ALLOC
    assert _live(lib) == base + N_ALLOC
    assert lib.omv_inertial_opt_destroy(out) == _lib.OMV_OK
    assert _live(lib) == base
    assert lib.omv_inertial_opt_destroy(None) == _lib.OMV_ERR_ARG


def test_a_reused_handle_serves_growing_and_shrinking_calls(lib):
    """The same jobs give the same bits whatever the handle ran before and whatever else is in the call."""
    base = _live(lib)
    small = si.make_jobs([3, 10], seed=61, modes=(ii.FULL, ii.BIAS), priors=((1e2, 1e5), (1.0, 1e5)))
    large = si.make_jobs([66, 11, 130, 2], seed=71, modes=(ii.FULL, ii.GS, ii.BIAS, ii.FULL), monos=(True, False))
    opt = ii.InertialOptimizer(8, 256, 256)
    fresh = ii.InertialOptimization(small, optimizer=ii.InertialOptimizer(2, 16, 16))
    runs = [ii.InertialOptimization(j, optimizer=opt) for j in (small, large + small, small, [], small[:1])]
    for got in (runs[0], runs[1][4:], runs[2]):
        for a, b in zip(fresh, got):
            for k in ("Rwg", "scale", "bg", "ba", "vel", "vel_f32", "reintegrate"):
                assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert runs[3] == [] and runs[4][0]["bg"].tobytes() == fresh[0]["bg"].tobytes()
    del opt
    assert _live(lib) == base
