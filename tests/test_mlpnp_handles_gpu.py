"""The omv_pnp handle's memory (openmavis_amd/csrc/pnp.hip): every buffer goes through omv_host.h's DeviceArena, so
create / destroy returns omv_debug_live_allocations to where it was, and a create that fails at any of its allocations
(omv_debug_fail_allocation) returns OMV_ERR_HIP, leaves *out alone and leaks nothing.  The counterpart of
tests/test_handles_gpu.py for this handle."""
import ctypes

import pytest

from openmavis_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEAD0
N_ALLOC = 16   # the d_* buffers of struct omv_pnp


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
        assert lib.omv_pnp_create(1, 8, 4, ctypes.byref(out)) == _lib.OMV_OK
        assert _live(lib) == base + N_ALLOC
        assert lib.omv_pnp_destroy(out) == _lib.OMV_OK
        assert _live(lib) == base


def test_create_unwinds_a_failure_at_each_allocation(lib):
    base = _live(lib)
    k = 0
    while True:
        k += 1
        assert k <= 100, "create never succeeded"
        assert lib.omv_debug_fail_allocation(k) == _lib.OMV_OK
        out = ctypes.c_void_p(SENTINEL)
        st = lib.omv_pnp_create(2, 8, 4, ctypes.byref(out))
        if st == _lib.OMV_OK:
            break
        assert st == _lib.OMV_ERR_HIP, (k, st)
        assert out.value == SENTINEL, k
        assert _live(lib) == base, k
    assert lib.omv_debug_fail_allocation(0) == _lib.OMV_OK   # the create made fewer than k allocations: still armed
    assert k - 1 == N_ALLOC   # every buffer of the handle goes through the helper, and nothing else does
    assert _live(lib) == base + N_ALLOC
    assert lib.omv_pnp_destroy(out) == _lib.OMV_OK
    assert _live(lib) == base


def test_create_arguments(lib):
    out = ctypes.c_void_p(SENTINEL)
    for args in ((0, 8, 4), (1, -1, 4), (1, 8, 0)):
        assert lib.omv_pnp_create(*args, ctypes.byref(out)) == _lib.OMV_ERR_ARG and out.value == SENTINEL
    assert lib.omv_pnp_create(1, 8, 4, None) == _lib.OMV_ERR_ARG
    assert lib.omv_pnp_destroy(None) == _lib.OMV_ERR_ARG
