"""tests/essgraph_ref.py, the float64 restatement the GPU pose-graph tests compare against, checked on its own: g2o::Sim3's
exp and log in all four branches, Edge4DoF's error, ImuCamPose::UpdateW's normalisation, a planted problem, and -- for
every case of tests/essgraph_cases.py -- that the g2o-form run and the near-exact run take the same LM path, the condition
under which tests/test_essgraph_gpu.py may demand identical counts."""
import numpy as np
import pytest

import essgraph_cases
import essgraph_ref as ref
from openmavis_amd.synth_essgraph import make_essgraph_problem

# (|sigma| < eps, theta < eps) for each of the four branches; eps = 1e-5
BRANCHES = [(3e-6, 5e-6), (3e-6, 0.7), (0.2, 5e-6), (-0.3, 1.1)]


def _u(sigma, theta, seed):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(3)
    return np.concatenate([theta * w / np.linalg.norm(w), rng.standard_normal(3), [sigma]])


def _expm(A):
    """Scaling and squaring with a Taylor series to rounding (|A| / 2^10 is tiny)."""
    B = A / 1024.0
    T, term = np.eye(len(A)), np.eye(len(A))
    for k in range(1, 20):
        term = term @ B / k
        T = T + term
    for _ in range(10):
        T = T @ T
    return T


@pytest.mark.parametrize("sigma,theta", BRANCHES)
def test_log_of_exp(sigma, theta):
    """The small-angle forms are first order (R = I + Omega + Omega^2, omega = deltaR / 2): theta^2 = 2.5e-11 there."""
    for seed in range(5):
        u = _u(sigma, theta, seed)
        back = ref.sim3_log(ref.sim3_exp(u))
        assert np.abs(back - u).max() <= (1e-10 if theta < ref.EPS else 1e-12), (sigma, theta, back - u)


@pytest.mark.parametrize("sigma,theta", BRANCHES)
def test_exp_against_the_matrix_exponential(sigma, theta):
    u = _u(sigma, theta, 3)
    A = np.zeros((4, 4))
    A[:3, :3] = ref.hat(u[:3]) + sigma * np.eye(3)
    A[:3, 3] = u[3:6]
    D = np.abs(ref.sim3_matrix(ref.sim3_exp(u)) - _expm(A))
    # the reference's small forms are approximations: below eps the rotation keeps Omega^2 where the series has
    # Omega^2 / 2 (theta^2 / 2 off), and the translation takes C = 1 for (s - 1) / sigma (sigma / 2 of |upsilon| off)
    assert D[:3, :3].max() <= (2e-11 if theta < ref.EPS else 1e-12)
    small = max(abs(sigma) if abs(sigma) < ref.EPS else 0.0, theta if theta < ref.EPS else 0.0)
    assert D[:3, 3].max() <= small * np.abs(u[3:6]).max() + 1e-12


def test_sim3_group():
    rng = np.random.default_rng(0)
    S = np.stack([ref.sim3_exp(_u(0.1 * k, 0.3 + 0.2 * k, k)) for k in range(4)])
    I = ref.s_mul(S, ref.s_inv(S))
    assert np.abs(I - np.array([0, 0, 0, 1, 0, 0, 0, 1.0])).max() < 1e-14
    X = rng.standard_normal((4, 3))
    assert np.abs(ref.s_map(ref.s_mul(S, S[::-1]), X) - ref.s_map(S, ref.s_map(S[::-1], X))).max() < 1e-13
    M = ref.sim3_matrix(S)
    assert np.abs(ref.s_map(S, X) - (np.einsum("nij,nj->ni", M[:, :3, :3], X) + M[:, :3, 3])).max() < 1e-13


def test_edge4dof_error_against_4x4():
    kind, prob = essgraph_cases.make("b_4dof")
    K = ref.make_kind(kind, prob)
    x = K.state0
    e = ref.errors(K, x)

    def T(v):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = v[21:30].reshape(3, 3), v[30:33]
        return M

    for k in (0, 5, len(K.ei) - 1):
        D = np.eye(4)
        D[:3, :3], D[:3, 3] = K.dR[k], K.dt[k]
        Tij = T(x[K.ei[k]]) @ np.linalg.inv(T(x[K.ej[k]]))
        want = np.concatenate([ref.log_so3(Tij[:3, :3] @ D[:3, :3].T), Tij[:3, 3] - D[:3, 3]])
        assert np.abs(e[k] - want).max() < 1e-12
    # the measurement is the relative pose of the table's entries: a graph at its tables has zero error on table-0 edges
    t0 = np.asarray(prob["edge_table"]) == 0
    assert t0.any() and np.abs(e[t0]).max() < 1e-12


def test_updatew_normalises_on_the_fifth_kept_update_only():
    kind, prob = essgraph_cases.make("a_4dof")
    K = ref.make_kind(kind, prob)
    x = K.state0[1:2].copy()
    rwb0 = K.Rwb0[1:2]
    x[:, 0:9] = ref.exp_so3(np.array([[0.02, -0.01, 0.3]])).reshape(1, 9)   # a DR with entries outside the yaw block
    u = np.array([[0.01, 0.1, -0.2, 0.05]])
    zeros = [2, 5, 6, 7]
    for n_acc in range(8):
        y, _ = K.oplus(x, u, n_acc, rwb0)
        DR = y[0, 0:9]
        fired = n_acc % 5 == 4
        assert bool(np.abs(DR[zeros]).max() < 1e-15) == fired, n_acc
        # Rwb comes from the DR before the normalisation and is not recomputed
        unnormalised = ref.exp_so3(np.array([[0, 0, u[0, 0]]])) @ x[:, 0:9].reshape(1, 3, 3)
        assert np.array_equal(y[0, 9:18], (unnormalised @ rwb0).reshape(-1))
        if fired:
            assert not np.allclose((DR.reshape(3, 3) @ rwb0[0]).reshape(-1), y[0, 9:18], atol=1e-6)
    # a rejected trial is popped: the same trial from the same state and count fires again, the count does not move
    a, _ = K.oplus(x, u, 4, rwb0)
    b, _ = K.oplus(x, 2 * u, 4, rwb0)
    assert np.abs(a[0, zeros]).max() < 1e-15 and np.abs(b[0, zeros]).max() < 1e-15
    log = []
    r = ref.optimize(*essgraph_cases.make("d_4dof"), log=log)
    assert r["n_acc"] == sum(l["accepted"] for l in log) >= 6


def test_planted_problem_is_recovered():
    """A consistent graph (no drift: every measurement is the relative pose of the true vertices), the start values
    perturbed: both kinds return to the truth."""
    for kind, name in ((ref.SIM3, "sim3"), (ref.DOF4, "4dof")):
        prob = make_essgraph_problem(name, n_kf=12, seed=2, drift=0.0, n_corrected=2)
        truth = ref.make_kind(kind, prob).caller_vertices(ref.make_kind(kind, prob).state0)
        rng = np.random.default_rng(4)
        K = ref.make_kind(kind, prob)
        opt = np.flatnonzero(~K.fixed)
        start = K.state0.copy()
        u = 0.02 * rng.standard_normal((len(opt), K.V))
        if kind == ref.SIM3:
            start[opt], _ = K.oplus(start[opt], u)
            moved = dict(prob, vertices=start)
        else:
            start[opt], _ = K.oplus(start[opt], u, 0, K.Rwb0[opt])
            # the moved vertices as ImuCamPose's members: Rwb0 := the moved Rwb, DR := I
            moved = dict(prob, vertices=K.caller_vertices(start))
        r = ref.optimize(kind, moved)
        assert r["err"] > 1e-3 and r["err_end"] < 1e-12 * r["err"] + 1e-18, (name, r["err"], r["err_end"])
        assert np.abs(r["vertices"] - truth).max() < 1e-6, name


@pytest.mark.parametrize("name", list(essgraph_cases.CASES))
def test_both_jacobian_forms_take_the_same_lm_path(name):
    kind, prob = essgraph_cases.make(name)
    a = ref.optimize(kind, prob)
    b = ref.optimize(kind, prob, delta=1e-6)
    assert (a["iterations"], a["trials"], a["n_acc"]) == (b["iterations"], b["trials"], b["n_acc"])
    assert a["err_end"] < a["err"] and a["n_acc"] >= 1
    assert np.abs(a["vertices"] - b["vertices"]).max() < 1e-4
    if name == "d_4dof":
        assert a["n_acc"] >= 6
    # the two-run distance is a representative sample of the noise (essgraph_cases' second condition)
    runs = [ref.optimize(kind, prob, delta=d) for d in essgraph_cases.SAMPLE_STEPS]
    assert all((r["iterations"], r["trials"]) == (a["iterations"], a["trials"]) for r in runs)
    dv = np.median([np.abs(r["vertices"] - b["vertices"]).max() for r in runs])
    de = np.median([abs(r["err_end"] - b["err_end"]) for r in runs])
    assert np.abs(a["vertices"] - b["vertices"]).max() >= 0.5 * dv and abs(a["err_end"] - b["err_end"]) >= 0.5 * de


def test_fix_scale_keeps_every_scale():
    kind, prob = essgraph_cases.make("a_sim3_fix_scale")
    r = ref.optimize(kind, prob)
    assert np.array_equal(r["vertices"][:, 7], np.asarray(prob["vertices"])[:, 7])
    K = ref.make_kind(kind, prob)
    Ji, Jj = ref.jacobians(K, K.state0)
    assert not Ji[:, :, 6].any() and not Jj[:, :, 6].any()
