"""Bindings of the library's test hooks (omv_selftest_* in include/omv.h).  The device linear algebra: the pose
kernels' pivoted LDL^T solves, pinv15_wave, inertial_info9_wave and the reduced-system solver's inv16, each on a batch
of host arrays (one workgroup per problem on the device).  The float layer underneath: math(), the functions of
csrc/omv_math.h elementwise.  There is no CPU fallback."""
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


# omv_selftest_math: the OMV_MATH_* codes of include/omv.h
(SINCOSF, ATANF, ATAN2F, TANF, SQRTF, FAST_ATAN2_DEG, ROUND_EVEN, DIVF, MULADD_F32, MULADD_F64, RCP_NR, KB8_PROJECT,
 KB8_UNPROJECT, PINHOLE_PROJECT, PINHOLE_UNPROJECT, PREDICT_SCALE, ROT_BIN, THREE_MAXIMA, PREDICT_SCALE_CLAMPED,
 GRID_CELL_OF, GRID_WINDOW, KP_IN_WINDOW) = range(22)
ROT_HIST_LEN = 30   # omv::kRotHistLen
MATH_NAMES = ("SINCOSF", "ATANF", "ATAN2F", "TANF", "SQRTF", "FAST_ATAN2_DEG", "ROUND_EVEN", "DIVF", "MULADD_F32",
              "MULADD_F64", "RCP_NR", "KB8_PROJECT", "KB8_UNPROJECT", "PINHOLE_PROJECT", "PINHOLE_UNPROJECT",
              "PREDICT_SCALE", "ROT_BIN", "THREE_MAXIMA", "PREDICT_SCALE_CLAMPED", "GRID_CELL_OF", "GRID_WINDOW",
              "KP_IN_WINDOW")
# per fn: input dtype, scalars per element of a, (dtype, scalars per element) of out
MATH_IO = {SINCOSF: (np.float32, 1, np.float32, 2), ATANF: (np.float32, 1, np.float32, 1),
           ATAN2F: (np.float32, 1, np.float32, 1), TANF: (np.float32, 1, np.float32, 1),
           SQRTF: (np.float32, 1, np.float32, 1), FAST_ATAN2_DEG: (np.float32, 1, np.float32, 1),
           ROUND_EVEN: (np.float32, 1, np.int32, 1), DIVF: (np.float32, 1, np.float32, 1),
           MULADD_F32: (np.float32, 1, np.float32, 1), MULADD_F64: (np.float64, 1, np.float64, 1),
           RCP_NR: (np.float64, 1, np.float64, 1), KB8_PROJECT: (np.float32, 3, np.float32, 2),
           KB8_UNPROJECT: (np.float32, 2, np.float32, 3), PINHOLE_PROJECT: (np.float32, 3, np.float32, 2),
           PINHOLE_UNPROJECT: (np.float32, 2, np.float32, 3), PREDICT_SCALE: (np.float32, 1, np.int32, 1),
           ROT_BIN: (np.float32, 1, np.int32, 1), THREE_MAXIMA: (np.int32, ROT_HIST_LEN, np.int32, 3),
           PREDICT_SCALE_CLAMPED: (np.float32, 1, np.int32, 1), GRID_CELL_OF: (np.float32, 2, np.int32, 1),
           GRID_WINDOW: (np.float32, 3, np.int32, 4), KP_IN_WINDOW: (np.float32, 8, np.int32, 1)}
# b shared by every element: fn -> its length (the camera codes: k[8]; the grid codes: min_x, min_y, invW, invH)
MATH_B_SHARED = {KB8_PROJECT: 8, KB8_UNPROJECT: 8, PINHOLE_PROJECT: 8, PINHOLE_UNPROJECT: 8, PREDICT_SCALE: 1,
                 PREDICT_SCALE_CLAMPED: 2, GRID_CELL_OF: 4, GRID_WINDOW: 4}


def math_args(fn, a, b, c):
    """The arrays of one math() / oracle.math_map() call in the hook's layout: (n, a, b, c, an empty out).  b of the
    camera codes is k[8], of PREDICT_SCALE one float, of PREDICT_SCALE_CLAMPED (log scale factor, levels), of the grid
    codes (min_x, min_y, invW, invH); every other
    b / c has one scalar per element."""
    tin, wa, tout, wo = MATH_IO[fn]
    a = np.ascontiguousarray(a, tin)
    n = a.size // wa
    assert a.size == n * wa
    if b is not None:
        b = np.ascontiguousarray(b, tin)
        assert b.size == MATH_B_SHARED.get(fn, n)
    if c is not None:
        c = np.ascontiguousarray(c, tin)
        assert c.size == n
    return n, a, b, c, np.empty((n, wo) if wo > 1 else (n,), tout)


def math(fn, a, b=None, c=None):
    """omv_selftest_math on host arrays -> a numpy array ([n], or [n][2] / [n][3] for the codes with several outputs
    per element; SINCOSF: column 0 sin, column 1 cos).  The output is pre-filled with 0xff bytes."""
    import torch
    n, a, b, c, out = math_args(fn, a, b, c)
    lib = _lib.load()
    da, db, dc = (None if x is None else torch.from_numpy(x).cuda() for x in (a, b, c))
    dout = torch.full((max(out.nbytes, 1),), 0xff, dtype=torch.uint8, device="cuda")
    _lib.check(lib.omv_selftest_math(int(fn), n, _lib.ptr(da), _lib.ptr(db), _lib.ptr(dc), _lib.ptr(dout), _stream()),
               "omv_selftest_math")
    torch.cuda.synchronize()
    return dout[:out.nbytes].cpu().numpy().view(out.dtype).reshape(out.shape)
