"""Bindings of the library's test hooks for the device linear algebra (omv_selftest_* in include/omv.h): the pose
kernels' pivoted LDL^T solves, pinv15_wave, inertial_info9_wave and the reduced-system solver's inv16, each on a batch
of host arrays (one workgroup per problem on the device).  There is no CPU fallback."""
import ctypes

import numpy as np

from . import _lib

PICK, PIVOT = 0, 1   # ldlt_pick_solve<6 | 9 | 24>, ldlt_pivot_solve_wave<15 | 30>
SW16 = np.array([[16 * r + (c ^ r) for c in range(16)] for r in range(16)])   # the solver's block layout (lba.hip sw16)


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ldlt(routine, H, b, sentinel=-7.5):
    """H [B][n][n], b [B][n] -> (x [B][n], order [B][n], ok [B]).  x is pre-filled with `sentinel` and order with -1:
    what the routine does not write comes back so.  order: the pick order (PICK) or the transpositions (PIVOT)."""
    import torch
    H, b = np.asarray(H, np.float64), np.asarray(b, np.float64)
    B, n = b.shape
    assert H.shape == (B, n, n) and B <= 64
    lib = _lib.load()
    dH, db = _dev(H, np.float64), _dev(b, np.float64)
    x = torch.full((B, n), float(sentinel), dtype=torch.float64, device="cuda")
    order = torch.full((B, n), -1, dtype=torch.int32, device="cuda")
    ok = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.omv_selftest_ldlt(int(routine), n, B, _lib.ptr(dH), _lib.ptr(db), _lib.ptr(x), _lib.ptr(order),
                                     _lib.ptr(ok), _stream()), "omv_selftest_ldlt")
    torch.cuda.synchronize()
    return x.cpu().numpy(), order.cpu().numpy(), ok.cpu().numpy()


def pinv15(A):
    """A [B][15][15] -> (P [B][15][15], path [B]: 1 the LDL^T inverse, 0 the Jacobi eigen-decomposition)."""
    import torch
    A = np.asarray(A, np.float64)
    B = len(A)
    assert A.shape == (B, 15, 15) and B <= 64
    lib = _lib.load()
    dA = _dev(A, np.float64)
    P = torch.full((B, 15, 15), float("nan"), dtype=torch.float64, device="cuda")
    path = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.omv_selftest_pinv15(B, _lib.ptr(dA), _lib.ptr(P), _lib.ptr(path), _stream()), "omv_selftest_pinv15")
    torch.cuda.synchronize()
    return P.cpu().numpy(), path.cpu().numpy()


def inertial_info9(C, par):
    """float C [B][15][15] -> (info [B][9][9], path [B]: 0 the factorisation shortcut, 1 eigen-decomposition with every
    eigenvalue kept, 2 with an eigenvalue zeroed); par: inertial_info9_wave<true> (the pose path) or <false>."""
    import torch
    C = np.asarray(C, np.float32)
    B = len(C)
    assert C.shape == (B, 15, 15) and B <= 64
    lib = _lib.load()
    dC = _dev(C, np.float32)
    info = torch.full((B, 9, 9), float("nan"), dtype=torch.float64, device="cuda")
    path = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.omv_selftest_inertial_info9(int(bool(par)), B, _lib.ptr(dC), _lib.ptr(info), _lib.ptr(path),
                                               _stream()), "omv_selftest_inertial_info9")
    torch.cuda.synchronize()
    return info.cpu().numpy(), path.cpu().numpy()


def inv16(D):
    """D [B][16][16] (plain row-major; only the lower triangle is read) -> (the full inverse [B][16][16], bad [B]).
    The blocks travel in the solver's swizzled layout."""
    import torch
    D = np.asarray(D, np.float64)
    B = len(D)
    assert D.shape == (B, 16, 16) and B <= 64
    lib = _lib.load()
    sw = np.empty((B, 256))
    sw[:, SW16.ravel()] = D.reshape(B, 256)
    dD = _dev(sw, np.float64)
    out = torch.full((B, 256), float("nan"), dtype=torch.float64, device="cuda")
    bad = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.omv_selftest_inv16(B, _lib.ptr(dD), _lib.ptr(out), _lib.ptr(bad), _stream()), "omv_selftest_inv16")
    torch.cuda.synchronize()
    return out.cpu().numpy()[:, SW16.ravel()].reshape(B, 16, 16), bad.cpu().numpy()
