"""Plain-Python references for the device linear-algebra routines (test infrastructure, never the product).

Exact replay      Eigen's unblocked LDLT (lower, diagonal pivoting) and LDLT::_solve_impl in fractions.Fraction:
                  the pivot is the first largest |diagonal| of the trailing corner, taken from the not-yet-updated
                  diagonal and applied as a transposition; isPositive() = no negative D; a zero first pivot stops with
                  x = 0; D+ = 0 for |D| <= DBL_MIN.  The same algorithm in float64 (left-looking as Eigen and
                  ldlt_pivot_solve_wave order it, right-looking as ldlt_pick_solve does) shows that a case's
                  intermediates are all representable: then every correct implementation returns the same bits.
High precision    mpmath at 50 digits: solve, inverse, symmetric eigen-decomposition, truncated pseudo-inverse, the
                  inertial information (inverse, symmetrise, clamp); float64 LU with iterative refinement on
                  high-precision residuals for the reduced system of a bundle-adjustment window.
Exact cases       A = L D L^T built in pivoted order with dyadic L, power-of-two (or zero, or negative) D and a
                  non-increasing |diagonal|, scattered to the rows the pivot rule visits in that order.

mpmath is a hard dependency here: a missing module is an ImportError in every test that uses this file.
"""
from fractions import Fraction

import mpmath
import numpy as np

DBL_MIN = 2.2250738585072014e-308
U = 2.0 ** -53
DPS = 50


def hp():
    """Context manager / decorator: mpmath at DPS digits (restored on exit; the process-wide precision stays as it is).
    mpmath values computed here keep their digits outside, but arithmetic on them outside rounds to the precision in
    force there: do it under hp() too."""
    return mpmath.workdps(DPS)


# ---- the pivot rule ---------------------------------------------------------------------------------------------
def pivot_order(diag):
    """Eigen's pivot rule on a diagonal (it is never updated before it is picked): returns (pick, tr) with pick[k] the
    original row at position k and tr[k] the transposition of step k."""
    a = [abs(d) for d in diag]
    n = len(a)
    idx = list(range(n))
    tr = []
    for k in range(n):
        big = k
        for p in range(k + 1, n):
            if a[idx[p]] > a[idx[big]]:
                big = p
        tr.append(big)
        idx[k], idx[big] = idx[big], idx[k]
    return idx, tr


def order_from_transpositions(tr):
    """The pick order (position -> original row) that the transpositions tr[0..n-1] produce."""
    idx = list(range(len(tr)))
    for k, t in enumerate(tr):
        idx[k], idx[t] = idx[t], idx[k]
    return idx


# ---- exact replay -------------------------------------------------------------------------------------------------
def ldlt_replay(H, b, num=Fraction, looking="left"):
    """Eigen::LDLT(H).solve(b).  num = Fraction: exact.  num = float with looking = "left" / "right": the same steps
    in float64, products and sums rounded one by one, in Eigen's order / in the right-looking order.  Returns
    dict(ok, x (None when not ok), pick, tr, D)."""
    n = len(b)
    if any(H[i][i] != H[i][i] for i in range(n)):   # a NaN diagonal: no factorisation (the project's rule)
        return dict(ok=False, x=None, pick=None, tr=None, D=None)
    A = [[num(H[i][j]) for j in range(n)] for i in range(n)]
    zero = num(0)
    tr = []
    neg = False
    stopped = False
    # right-looking updates reach the trailing diagonal early: its order comes from the original one (the same order)
    tr_right = pivot_order([A[i][i] for i in range(n)])[1]
    for k in range(n):
        big = k
        for p in range(k + 1, n):
            if abs(A[p][p]) > abs(A[big][big]):
                big = p
        if looking == "right":
            big = tr_right[k]
        tr.append(big)
        if big != k:
            A[k], A[big] = A[big], A[k]
            for row in A:
                row[k], row[big] = row[big], row[k]
        if looking == "left" and k > 0:
            t = [A[j][j] * A[k][j] for j in range(k)]
            for i in range(k, n):
                s = zero
                for j in range(k):
                    s = s + A[i][j] * t[j]
                A[i][k] = A[i][k] - s
        akk = A[k][k]
        if k == 0 and akk == 0:
            tr = list(range(n))
            stopped = True
            break
        if akk != 0:
            for i in range(k + 1, n):
                A[i][k] = A[i][k] / akk
            if looking == "right":
                for i in range(k + 1, n):
                    for j in range(k + 1, i + 1):
                        A[i][j] = A[j][i] = A[i][j] - A[i][k] * (A[j][k] * akk)   # (the swaps move whole rows)
        neg = neg or akk < 0
    D = [A[i][i] for i in range(n)]
    pick = order_from_transpositions(tr)
    if neg:
        return dict(ok=False, x=None, pick=pick, tr=tr, D=D)
    y = [num(b[pick[i]]) for i in range(n)]
    if stopped:
        y = [zero] * n
    else:
        for j in range(n):
            for i in range(j + 1, n):
                y[i] = y[i] - A[i][j] * y[j]
        y = [y[i] / D[i] if abs(D[i]) > DBL_MIN else zero for i in range(n)]
        for j in range(n - 1, -1, -1):
            for i in range(j):
                y[i] = y[i] - A[j][i] * y[j]
    x = [zero] * n
    for i in range(n):
        x[pick[i]] = y[i]
    return dict(ok=True, x=x, pick=pick, tr=tr, D=D)


def bits(v):
    """float64 bit patterns (so that -0.0 != 0.0 and NaN == NaN compare as the hardware stored them)."""
    return np.asarray(v, np.float64).view(np.uint64)


# ---- exact cases ----------------------------------------------------------------------------------------------
def _pow2(f):
    f = abs(Fraction(f))
    return f != 0 and (f.numerator == 1 or f.denominator == 1) and \
        (f.numerator & (f.numerator - 1)) == 0 and (f.denominator & (f.denominator - 1)) == 0


def exact_case(n, rng, groups, signs=None, zero_at=(), hollow=False, positional=False):
    """One exact system.  groups: sizes of the runs of equal |diagonal| in pivoted order (strictly decreasing from run to
    run); signs[k] = -1 asks for a negative D_k; zero_at: positions whose D is zero (a singular PSD matrix; they must
    not start a run).  hollow: a zero diagonal with integer off-diagonals instead (the ZeroSign stop).  positional: the
    rows are arranged so that the pick order differs from ranking the |diagonal| with ties by original index (a tie
    decided by the positions earlier swaps left).  Returns H (floats, row-major lists), b, x0 and the intended pick
    order."""
    assert sum(groups) == n
    x0 = [int(v) for v in rng.integers(-3, 4, n)]
    if hollow:
        H = [[0.0] * n for _ in range(n)]
        for i in range(n):
            for j in range(i):
                H[i][j] = H[j][i] = float(rng.integers(-2, 3))
        b = [float(sum(Fraction(H[i][j]) * x0[j] for j in range(n))) for i in range(n)]
        return H, b, x0, list(range(n))
    signs = signs or [1] * n
    vals = [Fraction(1, 2), Fraction(-1, 2), Fraction(1, 4), Fraction(-1, 4), Fraction(1), Fraction(-1)]
    L = [[Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    D = [Fraction(0)] * n
    run_size, k0 = {}, 0
    for g in groups:
        run_size[k0] = g
        k0 += g
    level = Fraction(2) ** 8   # |diagonal| of the current run
    for k in range(n):
        found = None
        if k in zero_at:   # a row with sum L^2 D = the run's |diagonal|: the pivot vanishes
            assert k not in run_size
            opts = [((j, v),) for j in range(k) for v in vals if v * v * D[j] == level]
            opts += [((j1, v1), (j2, v2)) for j1 in range(k) for j2 in range(j1 + 1, k) for v1 in vals for v2 in vals
                     if v1 * v1 * D[j1] + v2 * v2 * D[j2] == level]
            assert opts, ("exact_case: no zero pivot reachable", k)
            row = [Fraction(0)] * k
            for j, v in opts[int(rng.integers(0, len(opts)))]:
                row[j] = v
            found = (row, Fraction(0), level)
        for attempt in range(400):
            if found:
                break
            last = attempt == 399
            row = [Fraction(0)] * k
            live = [j for j in range(k) if D[j] != 0]
            if live and not last:
                for j in rng.choice(len(live), size=min(len(live), int(rng.integers(1, 4))), replace=False):
                    row[live[int(j)]] = vals[int(rng.integers(0, len(vals)))]
            s = sum(row[j] * row[j] * D[j] for j in range(k))
            if k in run_size:   # a new run: a power-of-two D that puts |diagonal| below the previous run's; a run of
                                # several needs a power-of-two |diagonal| (its later members may fall back to L = 0)
                top = Fraction(2) ** (level.numerator.bit_length() - level.denominator.bit_length() + 1)
                cand = [signs[k] * top / 2 ** e for e in range(8)]
                cand = [d for d in cand if (k == 0 or 0 < abs(s + d) < level) and (run_size[k] == 1 or _pow2(s + d))]
                if cand:
                    d = cand[int(rng.integers(0, min(2, len(cand))))]
                    found = (row, d, abs(s + d))
            else:
                want = [w for w in (level - s, -level - s) if _pow2(w) and (w > 0) == (signs[k] > 0)]
                if want:
                    found = (row, want[0], level)
        assert found, ("exact_case: no row found", k)
        row, D[k], level = found
        for j in range(k):
            L[k][j] = row[j]
    A = [[sum(L[i][m] * D[m] * L[j][m] for m in range(min(i, j) + 1)) for j in range(n)] for i in range(n)]
    for k in range(1, n):
        assert abs(A[k][k]) <= abs(A[k - 1][k - 1])
    # scatter: a random arrangement of the diagonal over the rows, the pivot rule's visiting order pi, A's row k there
    for _ in range(1000):
        arrangement = [abs(A[int(q)][int(q)]) for q in rng.permutation(n)]
        pi, _ = pivot_order(arrangement)
        if not positional or pi != sorted(range(n), key=lambda i: (-arrangement[i], i)):
            break
    else:
        raise AssertionError("exact_case: no positional tie found")
    H = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            v = A[i][j]
            assert Fraction(float(v)) == v
            H[pi[i]][pi[j]] = float(v)
    b = []
    for i in range(n):
        v = sum(Fraction(H[i][j]) * x0[j] for j in range(n))
        assert Fraction(float(v)) == v
        b.append(float(v))
    return H, b, x0, pi


def exact_suite(n, seed):
    """The named exact cases at size n: name -> (H, b).  Deterministic in (n, seed)."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * n))
    h = n // 2
    cases = {}

    def add(name, **kw):
        H, b, _, _ = exact_case(n, rng, **kw)
        cases[name] = (H, b)

    add("distinct", groups=[1] * n)
    add("all_equal", groups=[n])
    add("equal_blocks", groups=[2, n - 4, 2] if n >= 6 else [n])
    add("tie_after_swap", groups=[1, 2] + [1] * (n - 5) + [2], positional=True)
    add("rank_n_minus_1", groups=[1] * (n - 2) + [2], zero_at=(n - 1,))
    add("zero_pivot_mid", groups=[1] * (h - 1) + [2] + [1] * (n - h - 1), zero_at=(h,))
    add("zero_largest_diagonal", groups=[n], hollow=True)
    add("negative_d", groups=[1] * n, signs=[1] * (n - 2) + [-1, 1])
    add("indefinite_equal_abs", groups=[2] + [1] * (n - 2), signs=[1, -1] + [1] * (n - 2))
    # rank 1: d l l^T with |l| non-increasing dyadic (equal |diagonal| where |l| repeats); pivots 1.. are zero
    l = [Fraction(1)] + [Fraction((-1) ** k, 2 ** min(1 + k // 2, 6)) for k in range(1, n)]
    x0 = [int(v) for v in rng.integers(-3, 4, n)]
    A = [[4 * l[i] * l[j] for j in range(n)] for i in range(n)]
    pi, _ = pivot_order([abs(A[int(q)][int(q)]) for q in rng.permutation(n)])
    H = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            H[pi[i]][pi[j]] = float(A[i][j])
    cases["rank_1"] = (H, [float(sum(Fraction(H[i][j]) * x0[j] for j in range(n))) for i in range(n)])
    # a NaN on the diagonal of an otherwise regular system, at each of NAN_AT's positions
    for q in nan_positions(n):
        H, b = [list(r) for r in cases["distinct"][0]], list(cases["distinct"][1])
        H[q][q] = float("nan")
        cases[f"nan_diagonal_{q}"] = (H, b)
    return cases


def nan_positions(n):
    """Where the NaN cases put it: the first row (the step-0 pivot candidate of lane 0), rows 1, 2 and 4 (lane 0's
    partners in a butterfly reduction over the lanes), a third and a half of the way, and the last row."""
    return sorted({0, 1, 2, 4, n // 3, n // 2, n - 1})


# ---- high precision -------------------------------------------------------------------------------------------
def mp_matrix(A):
    A = np.asarray(A, np.float64)
    return mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in A])


def mp_to_np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


@hp()
def mp_solve(A, b):
    """(x as float64, x as mpmath column) of A x = b at 50 digits."""
    x = mpmath.lu_solve(mp_matrix(A), mpmath.matrix([mpmath.mpf(float(v)) for v in np.asarray(b, np.float64)]))
    return np.array([float(v) for v in x]), x


@hp()
def mp_eigsy(A):
    """Eigenvalues (list of mpf) and eigenvectors (mpmath matrix, columns) of the symmetric A."""
    w, V = mpmath.eigsy(mp_matrix(A))
    return [w[i] for i in range(len(w))], V


@hp()
def mp_cond(A):
    w, _ = mp_eigsy(A)
    a = [abs(v) for v in w]
    return float(max(a) / min(a))


@hp()
def mp_inverse(A):
    """(A^-1 rounded to float64, A^-1 as an mpmath matrix)."""
    M = mpmath.inverse(mp_matrix(A))
    return mp_to_np(M), M


@hp()
def mp_pinv_trunc(A, cut=1e-6):
    """V diag(1 / w over |w| > cut) V^T of the symmetric A.  Returns (P as float64, P as mpmath, kept eigenvalues, all
    eigenvalues)."""
    w, V = mp_eigsy(A)
    n = len(w)
    P = mpmath.zeros(n, n)
    kept = []
    for k in range(n):
        if abs(w[k]) > cut:
            kept.append(w[k])
            v = V[:, k]
            P += (v * v.T) / w[k]
    return mp_to_np(P), P, kept, w


@hp()
def mp_inertial_info9(C15, cut=1e-12):
    """EdgeInertial's information from the float covariance C (15 x 15): inverse of its 9 x 9 corner, symmetrised,
    eigenvalues below `cut` zeroed.  Returns (info as float64, eigenvalues of the symmetrised inverse)."""
    C = np.asarray(C15, np.float32).reshape(15, 15)[:9, :9].astype(np.float64)
    I = mpmath.inverse(mp_matrix(C))
    I = (I + I.T) / 2
    w, V = mpmath.eigsy(I)
    out = mpmath.zeros(9, 9)
    for k in range(9):
        if not w[k] < cut:
            v = V[:, k]
            out += (v * v.T) * w[k]
    return mp_to_np(out), [w[k] for k in range(9)]


def _exact_ints(a):
    """(object array of Python ints m, shift) with a == m 2^-shift exactly."""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)
    ee = np.where(mi != 0, e.astype(np.int64) - 53, 0)
    shift = int(-ee.min()) if ee.size else 0
    out = np.empty(a.shape, dtype=object)
    of, mf, ef = out.ravel(), mi.ravel(), ee.ravel()
    for q in range(of.size):
        of[q] = int(mf[q]) << (int(ef[q]) + shift)
    return out, shift


def refine_solve(S, rhs, tol=1e-25, max_it=80):
    """x of S x = rhs for a system of a few hundred unknowns: float64 LU solves, then iterative refinement with the
    residual rhs - S x formed exactly (integers) until the correction is below `tol` relative.  Returns the float64
    terms whose exact sum is x, and the number of refinement steps."""
    S = np.asarray(S, np.float64)
    rhs = np.asarray(rhs, np.float64)
    n = len(rhs)
    Si, ss = _exact_ints(S)
    terms = [np.linalg.solve(S, rhs)]
    rf = [Fraction(float(v)) for v in rhs]
    x = [Fraction(float(v)) for v in terms[0]]
    for it in range(max_it):
        sx = max(v.denominator.bit_length() - 1 for v in x)
        xi = np.array([v.numerator << (sx - (v.denominator.bit_length() - 1)) for v in x], dtype=object)
        Sx = Si.dot(xi)
        r = np.array([float(rf[i] - Fraction(int(Sx[i]), 1 << (ss + sx))) for i in range(n)])
        d = np.linalg.solve(S, r)
        terms.append(d)
        x = [x[i] + Fraction(float(d[i])) for i in range(n)]
        if np.abs(d).max() <= tol * max(abs(float(v)) for v in x):
            return terms, it + 1
    raise AssertionError("refine_solve did not converge")


def rayleigh_cond_lower_bound(S):
    """A rigorous lower bound of kappa_2 of the symmetric positive definite S, tight when float64 eigenvectors are
    decent: the Rayleigh quotients of eigh's extreme eigenvectors, evaluated exactly (lambda_max >= RQ(v_max),
    lambda_min <= RQ(v_min))."""
    S = np.asarray(S, np.float64)
    _, V = np.linalg.eigh(S)
    Si, ss = _exact_ints(S)
    rq = []
    for v in (V[:, -1], V[:, 0]):
        vi, sv = _exact_ints(v)
        num = Fraction(int(vi.dot(Si.dot(vi))), 1 << (ss + 2 * sv))
        den = Fraction(int(vi.dot(vi)), 1 << (2 * sv))
        rq.append(num / den)
    assert rq[1] > 0
    return float(rq[0] / rq[1])


def sum_terms(terms):
    """The refined solution rounded once to float64, and as Fractions."""
    n = len(terms[0])
    xf = [sum((Fraction(float(t[i])) for t in terms), Fraction(0)) for i in range(n)]
    return np.array([float(v) for v in xf]), xf


@hp()
def forward_error(got, exact):
    """||got - exact||_inf / ||exact||_inf with `exact` a sequence of mpf / Fraction / float (the difference formed in
    high precision)."""
    ex = [mpmath.mpf(v.numerator) / v.denominator if isinstance(v, Fraction) else mpmath.mpf(v) for v in exact]
    g = [mpmath.mpf(float(v)) for v in np.asarray(got, np.float64).ravel()]
    assert len(g) == len(ex)
    num = max(abs(a - b) for a, b in zip(g, ex))
    den = max(abs(b) for b in ex)
    return float(num / den)


def solve_bound(n, kappa, e_ref):
    """The issue's bar for a solve / inverse / pseudo-inverse: max(4 e_ref, 3 n u kappa_2)."""
    return max(4.0 * e_ref, 3.0 * n * U * kappa)
