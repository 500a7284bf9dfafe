"""The references of tests/test_linalg_gpu.py (oracle/linalg_ref.py), validated without a GPU: the Fraction replay of
Eigen's pivoted LDLT against numpy and against hand-worked pick orders, the exact cases (every intermediate
representable: the replay in float64, in Eigen's left-looking order and in the right-looking order, returns the
Fraction replay's bits), the truncated pseudo-inverse (Penrose identities), the inertial information and the refined
solve of a reduced-system-sized problem.  mpmath is required: without it this module fails to import."""
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import linalg_ref as ref

SIZES = (6, 9, 15, 24, 30)   # every instantiated N of ldlt_pick_solve (6, 9, 24) and ldlt_pivot_solve_wave (15, 30)


def _spd(n, kappa, rng):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    w = np.logspace(0, -np.log10(kappa), n)
    H = (Q * w) @ Q.T
    return (H + H.T) / 2


@pytest.mark.parametrize("n", SIZES)
def test_replay_agrees_with_numpy_on_spd(n):
    rng = np.random.default_rng(100 + n)
    for kappa in (1e2, 1e5):
        H = _spd(n, kappa, rng)
        b = rng.normal(size=n)
        r = ref.ldlt_replay(H.tolist(), b.tolist())
        assert r["ok"] and all(d > 0 for d in r["D"])
        assert r["pick"] == ref.pivot_order(np.diag(H).tolist())[0]
        # the exact replay solves the system: its residual vanishes identically
        for i in range(n):
            assert sum(Fraction(float(H[i, j])) * r["x"][j] for j in range(n)) == Fraction(float(b[i]))
        e = ref.forward_error(np.linalg.solve(H, b), r["x"])
        assert e <= 3 * n * ref.U * ref.mp_cond(H), (n, kappa, e)


def test_pick_order_known_answers():
    # all equal: position k already holds a largest entry at every step
    assert ref.pivot_order([7.0] * 5) == ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4])
    # the first swap parks row 0 behind row 1: the tie of step 1 goes to row 1 (by position), not row 0 (by index)
    assert ref.pivot_order([1.0, 1.0, 2.0]) == ([2, 1, 0], [2, 1, 2])
    # two equal pairs
    assert ref.pivot_order([3.0, 5.0, 3.0, 5.0]) == ([1, 3, 2, 0], [1, 3, 2, 3])
    # equal magnitude, opposite sign: the magnitude decides, the first position wins
    assert ref.pivot_order([2.0, -2.0, 1.0]) == ([0, 1, 2], [0, 1, 2])
    assert ref.pivot_order([1.0, -2.0, 2.0]) == ([1, 2, 0], [1, 2, 2])
    r = ref.ldlt_replay([[2.0, 0.0, 0.0], [0.0, -2.0, 0.0], [0.0, 0.0, 1.0]], [1.0, 1.0, 1.0])
    assert not r["ok"] and r["x"] is None and r["pick"] == [0, 1, 2] and r["D"] == [2, -2, 1]
    # a worked 2 x 2: H = [[1, 2], [2, 8]] pivots on 8: D = (8, 1/2), x = H^-1 b
    r = ref.ldlt_replay([[1.0, 2.0], [2.0, 8.0]], [1.0, 0.0])
    assert r["ok"] and r["pick"] == [1, 0] and r["D"] == [8, Fraction(1, 2)] and r["x"] == [2, Fraction(-1, 2)]
    # a zero first pivot stops with x = 0; a zero pivot later gives that component of D+ y zero
    r = ref.ldlt_replay([[0.0, 1.0], [1.0, 0.0]], [1.0, 2.0])
    assert r["ok"] and r["x"] == [0, 0] and r["tr"] == [0, 1]
    r = ref.ldlt_replay([[4.0, 2.0], [2.0, 1.0]], [4.0, 2.0])   # rank 1: L = (1, 1/2), D = (4, 0), y = (4, 0)
    assert r["ok"] and r["D"] == [4, 0] and r["x"] == [1, 0]
    # D+ is zero at or below DBL_MIN, 1 / D above it
    r = ref.ldlt_replay([[1.0, 0.0], [0.0, ref.DBL_MIN]], [1.0, 1.0])
    assert r["x"] == [1, 0]
    r = ref.ldlt_replay([[1.0, 0.0], [0.0, 2 * ref.DBL_MIN]], [1.0, ref.DBL_MIN])
    assert r["x"] == [1, Fraction(1, 2)]
    assert not ref.ldlt_replay([[1.0, 0.0], [0.0, float("nan")]], [1.0, 1.0])["ok"]


@pytest.mark.parametrize("n", SIZES)
def test_exact_cases_are_exact_and_take_their_paths(n):
    cases = ref.exact_suite(n, seed=7)
    assert cases.keys() == ref.exact_suite(n, seed=7).keys()
    assert {0, 1, n // 2, n - 1} <= set(ref.nan_positions(n)) and len(cases) == 10 + len(ref.nan_positions(n))
    for name, (H, b) in cases.items():
        assert all(H[i][j] == H[j][i] or name.startswith("nan_diagonal") for i in range(n) for j in range(n)), name
        r = ref.ldlt_replay(H, b)
        diag = [abs(H[i][i]) for i in range(n)]
        if name.startswith("nan_diagonal"):
            assert not r["ok"] and sum(H[q][q] != H[q][q] for q in range(n)) == 1
            continue
        assert r["pick"] == ref.pivot_order(diag)[0], name
        for looking in ("left", "right"):   # every intermediate is representable: float64 arithmetic is exact here
            f = ref.ldlt_replay(H, b, num=float, looking=looking)
            assert f["ok"] == r["ok"] and f["pick"] == r["pick"], (name, looking)
            assert [Fraction(d) for d in f["D"]] == r["D"], (name, looking)
            if r["ok"]:
                assert np.array_equal(ref.bits(f["x"]), ref.bits([float(v) for v in r["x"]])), (name, looking)
                assert all(Fraction(float(v)) == v for v in r["x"]), name
        ties = len(set(diag)) < n
        if name == "distinct":
            assert r["ok"] and not ties and all(d > 0 for d in r["D"])
        elif name == "all_equal":
            assert r["ok"] and len(set(diag)) == 1 and r["pick"] == list(range(n))
            assert any(H[i][j] != 0 for i in range(n) for j in range(i)), "a multiple of the identity proves little"
        elif name == "equal_blocks":
            assert r["ok"] and ties and len(set(diag)) > 1
        elif name == "tie_after_swap":
            assert r["ok"] and r["pick"] != sorted(range(n), key=lambda i: (-diag[i], i))
        elif name in ("rank_n_minus_1", "zero_pivot_mid"):
            assert r["ok"] and [d == 0 for d in r["D"]].count(True) == 1 and r["D"][0] != 0
            if name == "zero_pivot_mid":
                assert r["D"].index(0) < n - 1 and r["D"][-1] > 0   # pivots after the zero one are regular again
        elif name == "rank_1":
            assert r["ok"] and r["D"][0] > 0 and all(d == 0 for d in r["D"][1:])
        elif name == "zero_largest_diagonal":
            assert r["ok"] and all(v == 0 for v in r["x"]) and any(v != 0 for v in b)
        elif name == "negative_d":
            assert not r["ok"] and [d < 0 for d in r["D"]].count(True) == 1
        elif name == "indefinite_equal_abs":
            assert not r["ok"] and H[r["pick"][0]][r["pick"][0]] == -H[r["pick"][1]][r["pick"][1]]
        else:
            raise AssertionError(name)


@ref.hp()
def test_truncated_pseudo_inverse_penrose():
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.normal(size=(15, 15)))
    w = np.array([3.0, 1.0, 0.5, 0.2, 1e-1, 5e-2, 1e-2, 5e-3, 1e-3, 5e-4, -2e-4, 1e-4, 1e-9, -1e-9, 0.0])
    A = (Q * w) @ Q.T
    A = (A + A.T) / 2
    P, Pm, kept, allw = ref.mp_pinv_trunc(A)
    assert len(kept) == 12 and min(abs(v) for v in kept) > 9e-5 and sum(1 for v in kept if v < 0) == 1
    Am = ref.mp_matrix(A)
    tiny = mpmath.mpf(10) ** -40
    scale = max(abs(Pm[i, j]) for i in range(15) for j in range(15))

    def nrm(M):
        return max(abs(M[i, j]) for i in range(M.rows) for j in range(M.cols))

    assert nrm(Pm * Am * Pm - Pm) <= tiny * scale        # P A P = P
    assert nrm((Am * Pm).T - Am * Pm) <= tiny * scale     # A P symmetric (the projector on the kept subspace)
    assert nrm(Am * Pm * Am * Pm - Am * Pm) <= tiny * scale
    dropped = max(abs(v) for v in allw if abs(v) <= 1e-6)
    assert nrm(Am * Pm * Am - Am) <= dropped * (1 + mpmath.mpf(10) ** -30)   # A P A = A on the kept subspace
    AP = Am * Pm
    assert abs(sum(AP[i, i] for i in range(15)) - 12) <= tiny   # trace of the projector = the kept rank
    assert np.abs(P - np.linalg.pinv(A, rcond=1e-6 / 3.0, hermitian=True)).max() <= 1e-6 * np.abs(P).max()


@ref.hp()
def test_inertial_info9_reference():
    rng = np.random.default_rng(9)
    Q, _ = np.linalg.qr(rng.normal(size=(9, 9)))
    w = np.logspace(-3, -9, 9)
    C = np.zeros((15, 15), np.float32)
    C[:9, :9] = ((Q * w) @ Q.T).astype(np.float32)
    C[:9, :9] = (C[:9, :9] + C[:9, :9].T) / 2
    info, ev = ref.mp_inertial_info9(C)
    assert min(ev) > 1e-12
    c9 = C[:9, :9].astype(np.float64)
    assert np.abs(info @ c9 - np.eye(9)).max() <= 1e-9
    # a negative direction of C: its inverse eigenvalue is negative and is zeroed
    Cn = C.copy()
    Cn[:9, :9] = ((Q * np.concatenate([w[:8], [-1e-6]])) @ Q.T).astype(np.float32)
    Cn[:9, :9] = (Cn[:9, :9] + Cn[:9, :9].T) / 2
    info_n, ev_n = ref.mp_inertial_info9(Cn)
    assert sum(1 for v in ev_n if v < 1e-12) == 1
    assert np.linalg.matrix_rank(info_n, tol=1e-3) == 8 and np.linalg.eigvalsh(info_n).min() > -1e-6


def test_refined_solve_reproduces_a_known_solution():
    """b = S x0 in exact arithmetic (integer S and x0, every product and sum representable), S of the reduced system's
    size and badly scaled like it: the refinement returns x0 itself."""
    rng = np.random.default_rng(3)
    n = 208
    B = rng.integers(-3, 4, size=(n, n)).astype(np.float64)
    S = B @ B.T + np.diag(2.0 ** rng.integers(0, 20, n))
    assert np.array_equal(S, S.T) and np.abs(S).max() < 2.0 ** 40
    x0 = rng.integers(-1000, 1001, n).astype(np.float64)
    b = S @ x0
    for i in range(0, n, 17):   # the float product was exact
        assert sum(int(S[i, j]) * int(x0[j]) for j in range(n)) == int(b[i])
    terms, steps = ref.refine_solve(S, b)
    x, xf = ref.sum_terms(terms)
    assert np.array_equal(x, x0) and steps <= 6
    assert ref.forward_error(x0, xf) <= 1e-25
    # a right-hand side without a representable solution: the terms still sum to 1e-25 of the solution
    b2 = rng.normal(size=n)
    terms, steps = ref.refine_solve(S, b2)
    x, xf = ref.sum_terms(terms)
    res = max(abs(sum(Fraction(float(S[i, j])) * xf[j] for j in range(n)) - Fraction(float(b2[i]))) for i in range(0, n, 13))
    assert float(res) <= 1e-22 * np.abs(b2).max()
    k = ref.rayleigh_cond_lower_bound(S)
    w = np.linalg.eigvalsh(S)
    assert k <= w[-1] / w[0] * (1 + 1e-9) and k >= 0.999 * w[-1] / w[0]
