"""Ownership of device memory (openmavis_amd/csrc/omv_host.h): every handle and per-call workspace allocates through one
helper, counted by omv_debug_live_allocations and failed on demand by omv_debug_fail_allocation.  An injected failure
never reaches HIP.  Checked here: create / destroy returns the count to where it was; a create that fails at any of
its allocations returns OMV_ERR_HIP, leaves *out alone and leaks nothing; a failed omv_lba_set_problem, buffer
regrowth or per-call workspace leaves a handle on which the same call then gives the result the feature's own test
expects, bit-exact (LocalInertialBA: the result and the optimised state of a fresh handle, bit for bit)."""
import ctypes

import numpy as np
import pytest

from openmavis_amd import _lib, mapping, synth, synth_ba, synth_fuse, synth_tri
from openmavis_amd import synth_kfmatch as sk
from openmavis_amd.matcher import FrameBatch, ORBmatcher, kf_search_params
from openmavis_amd.optimizer import LocalInertialBA
from openmavis_amd.orb import ORBextractor

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEAD0
ORB_W, ORB_H = 96, 80


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


def _arm(lib, nth):
    assert lib.omv_debug_fail_allocation(nth) == _lib.OMV_OK


def _fails_with_hip(call):
    with pytest.raises(_lib.OmvError, match=r"HIP runtime error \(2\)"):
        call()


# per handle type: create with the smallest parameters that still allocate every buffer, the destroy entry point, and
# the number of allocations the create makes (its device and pinned buffers, counted in the handle's struct)
def _orb(lib, out):   # 96 x 80: the smallest round size whose two levels each hold a FAST cell (a level needs 67 x 67)
    p = _lib.OrbParams(100, 1.2, 2, 20, 7)
    return lib.omv_orb_create(ctypes.byref(p), ORB_W, ORB_H, 1, out)


HANDLES = {
    "orb": (_orb, "omv_orb_destroy", 16),
    "matcher": (lambda lib, out: lib.omv_matcher_create(1, 2, 64, 8, out), "omv_matcher_destroy", 8),
    "lba": (lambda lib, out: lib.omv_lba_create(2, 1, 0, 0, 0, out), "omv_lba_destroy", 3),
    "pose": (lambda lib, out: lib.omv_pose_create(1, 4, out), "omv_pose_destroy", 5),
    "sim3_solver": (lambda lib, out: lib.omv_sim3_solver_create(1, 4, 4, out), "omv_sim3_solver_destroy", 11),
    "optsim3": (lambda lib, out: lib.omv_optimize_sim3_create(1, 4, out), "omv_optimize_sim3_destroy", 7),
    "kfdb": (lambda lib, out: lib.omv_kfdb_create(0, 4, 8, 1, 8, out), "omv_kfdb_destroy", 37),
}


def test_debug_hooks_reject_bad_arguments(lib):
    assert lib.omv_debug_live_allocations(None) == _lib.OMV_ERR_ARG
    assert lib.omv_debug_fail_allocation(-1) == _lib.OMV_ERR_ARG


@pytest.mark.parametrize("name", list(HANDLES))
def test_create_destroy_returns_every_allocation(lib, name):
    create, destroy, n_alloc = HANDLES[name]
    base = _live(lib)
    for _ in range(3):
        out = ctypes.c_void_p()
        assert create(lib, ctypes.byref(out)) == _lib.OMV_OK
        assert _live(lib) == base + n_alloc > base
        assert getattr(lib, destroy)(out) == _lib.OMV_OK
        assert _live(lib) == base


@pytest.mark.parametrize("name", list(HANDLES))
def test_create_unwinds_a_failure_at_each_allocation(lib, name):
    create, destroy, n_alloc = HANDLES[name]
    base = _live(lib)
    k = 0
    while True:
        k += 1
        assert k <= 100, "create never succeeded"
        _arm(lib, k)
        out = ctypes.c_void_p(SENTINEL)
        st = create(lib, ctypes.byref(out))
        if st == _lib.OMV_OK:
            break
        assert st == _lib.OMV_ERR_HIP, (k, st)
        assert out.value == SENTINEL, k
        assert _live(lib) == base, k
    _arm(lib, 0)   # the create made fewer than k allocations: the hook is still armed
    assert k - 1 == n_alloc   # every buffer of the handle goes through the helper, and nothing else does
    assert _live(lib) == base + n_alloc
    assert getattr(lib, destroy)(out) == _lib.OMV_OK
    assert _live(lib) == base


def test_destroy_of_null(lib):
    for name, (_, destroy, _) in HANDLES.items():
        want = _lib.OMV_OK if name == "kfdb" else _lib.OMV_ERR_ARG
        assert getattr(lib, destroy)(None) == want, name


def test_search_for_initialization_requires_the_geometry(lib):
    """A null frame geometry is OMV_ERR_ARG before it is read, with no pairs too (as in every other entry point)."""
    h = ctypes.c_void_p()
    assert HANDLES["matcher"][0](lib, ctypes.byref(h)) == _lib.OMV_OK
    for n_pairs in (0, 1):
        assert lib.omv_matcher_search_for_initialization(h, n_pairs, None, None, None, None, None, None, 10, 0.9, 1,
                                                         None, None, None) == _lib.OMV_ERR_ARG
    assert lib.omv_matcher_destroy(h) == _lib.OMV_OK


# ---- omv_lba_set_problem -------------------------------------------------------------------------------------------
def _lba(prob):
    return LocalInertialBA(max_kf=prob["n_kf"], max_cams=prob["n_cams"], max_pts=len(prob["pts"]),
                           max_mono=len(prob["mono_pt"]), max_imu=max(1, len(prob["imu_kf1"])))


def test_lba_set_problem_failure_leaves_a_usable_handle(lib):
    prob = synth_ba.make_lba_problem(n_kf=12, n_opt=4, n_pts=800, seed=3, n_cams=3)

    def copy():   # optimize() writes the state back into the problem's arrays
        return {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in prob.items()}

    kw = dict(opt_it=4, lambda_init=1e-2, max_trials=10, large=True)
    base = _live(lib)
    fresh = _lba(prob)
    before = _live(lib)
    fresh.set_problem(copy())
    n_prob = _live(lib) - before   # the allocations of this problem
    assert n_prob > 50
    want, want_state = fresh.optimize(**kw)
    fresh.__del__()
    assert _live(lib) == base

    ba = _lba(prob)
    for k in (1, n_prob):   # the first state block; the pinned staging block, allocated last
        _arm(lib, k)
        _fails_with_hip(lambda: ba.set_problem(copy()))
        _arm(lib, 0)
        assert _live(lib) < before + n_prob
    ba.set_problem(copy())
    assert _live(lib) == before + n_prob
    got, got_state = ba.optimize(**kw)
    # every device reduction is a fixed-order sum: bit-identical, as tests/test_lba_gpu.py asserts run to run
    for key in ("err", "err_end", "lambda_", "iterations", "trials", "status"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert np.array_equal(got["mono_chi2"].view(np.uint64), want["mono_chi2"].view(np.uint64))
    for key in ("Rwb", "twb", "Rcw", "tcw", "vel", "bg", "ba", "pts"):
        assert np.array_equal(np.asarray(got_state[key]).view(np.uint64),
                              np.asarray(want_state[key]).view(np.uint64)), key
    ba.__del__()
    assert _live(lib) == base


def _same_bits(got, got_state, want, want_state):
    for key in ("err", "err_end", "lambda_", "iterations", "trials", "status"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert np.array_equal(got["mono_chi2"].view(np.uint64), want["mono_chi2"].view(np.uint64))
    for key in ("Rwb", "twb", "Rcw", "tcw", "vel", "bg", "ba", "pts"):
        assert np.array_equal(np.asarray(got_state[key]).view(np.uint64),
                              np.asarray(want_state[key]).view(np.uint64)), key


def test_lba_rejected_problem_leaves_the_previous_one(lib):
    """OMV_ERR_ARG from omv_lba_set_problem: planned and rejected on the host before the handle is touched, so the
    previous problem, its device memory and its captured steps stay valid."""
    prob = synth_ba.make_lba_problem(n_kf=12, n_opt=4, n_pts=800, seed=3, n_cams=3)
    kw = dict(opt_it=4, lambda_init=1e-2, max_trials=10, large=True)
    ba = _lba(prob).set_problem(prob)
    want, want_state = ba.optimize(**kw)
    held = _live(lib)
    bad = dict(prob, mono_kf=np.array(prob["mono_kf"], copy=True))
    bad["mono_kf"][7] = prob["n_kf"]
    s, keep = synth_ba.as_struct(bad, _lib.LbaProblem)
    assert lib.omv_lba_set_problem(ba._h, ctypes.byref(s)) == _lib.OMV_ERR_ARG
    assert _live(lib) == held
    got, got_state = ba.reset().optimize(**kw)
    _same_bits(got, got_state, want, want_state)


def test_lba_failed_upload_leaves_no_problem(lib):
    """OMV_ERR_HIP from omv_lba_set_problem: the handle ends without a problem, and every call that needs one says
    OMV_ERR_ARG before it launches anything; a later set_problem makes the handle whole again."""
    prob = synth_ba.make_lba_problem(n_kf=12, n_opt=4, n_pts=800, seed=3, n_cams=3)
    kw = dict(opt_it=4, lambda_init=1e-2, max_trials=10, large=True)
    base = _live(lib)
    ba = _lba(prob)
    own = _live(lib)
    assert own == base + HANDLES["lba"][2]
    want, want_state = ba.set_problem(prob).optimize(**kw)
    _arm(lib, 1)   # the first state block
    _fails_with_hip(lambda: ba.set_problem(prob))
    _arm(lib, 0)
    assert _live(lib) == own
    s, keep = synth_ba.as_struct(prob, _lib.LbaProblem)
    E, n = s.n_mono, 16 * s.n_opt
    o, r = _lib.LbaOpts(4, 1e-2, 10, 1), _lib.LbaResult()
    buf = np.zeros(max(18 * E, n * n))
    fail, plan = ctypes.c_int(-1), np.zeros(4 + s.n_opt, np.int32)
    assert lib.omv_lba_optimize(ba._h, ctypes.byref(o), ctypes.byref(s), ctypes.byref(r)) == _lib.OMV_ERR_ARG
    assert lib.omv_lba_evaluate(ba._h, _lib.ptr(buf), None, None, None) == _lib.OMV_ERR_ARG
    assert lib.omv_lba_evaluate_stereo(ba._h, _lib.ptr(buf), None, None) == _lib.OMV_ERR_ARG
    assert lib.omv_lba_reset(ba._h) == _lib.OMV_ERR_ARG
    assert lib.omv_lba_debug_solve(ba._h, ctypes.byref(o), ctypes.c_double(1.0), _lib.ptr(buf), _lib.ptr(buf[:n].copy()),
                                   _lib.ptr(buf[:n].copy()), ctypes.byref(fail), _lib.ptr(plan), len(plan)) == _lib.OMV_ERR_ARG
    assert _live(lib) == own
    got, got_state = ba.set_problem(prob).optimize(**kw)
    _same_bits(got, got_state, want, want_state)
    ba.__del__()
    assert _live(lib) == base


# ---- buffers that grow on demand -------------------------------------------------------------------------------------
W, H, C, NF = 720, 540, 5, 1200
LAP = np.array([[0, 720], [0, 720], [0, 0], [0, 0], [0, 0]], np.int32)


def test_search_last_frame_regrowth_failure(lib, oracle, torch_cuda):
    """d_push and d_npush are replaced together; a failure at either must leave neither to be freed twice."""
    torch = torch_cuda
    F = 3
    ex = ORBextractor(NF, 1.2, 8, 15, 7, width=W, height=H, max_images=F * C)
    cap = ex.max_keypoints()
    imgs = np.concatenate([synth.hilti_frame(f) for f in range(F)])
    fb = FrameBatch(torch, F, C, cap, W, H, ex.GetScaleFactors())
    ex.extract_batch(torch.from_numpy(imgs).cuda(), np.tile(LAP, (F, 1)), fb.kps.view(-1, cap, 6),
                     fb.desc.view(-1, cap, 32), fb.n_kp.view(-1), fb.mono.view(-1))
    torch.cuda.synchronize()
    assert ex.last_error() == 0
    ex.close()
    kps = fb.kps.cpu().numpy().view(oracle.KP_DTYPE).reshape(F, C, cap)
    desc, n_kp = fb.desc.cpu().numpy(), fb.n_kp.cpu().numpy()
    cams, R_cl, t_cl = synth.hilti_rig(C)
    rng = np.random.default_rng(1)
    Tcw = np.stack([synth.random_se3(rng) for _ in range(F)])
    Tlw = Tcw.copy()
    lasts = [synth.make_last_frame(kps[f], desc[f], n_kp[f], 90 + f, cams, Tcw[f]) for f in range(F)]
    Trl = np.concatenate([synth.quat_from_R(R_cl[1].astype(np.float64)), t_cl[1]]).astype(np.float32)
    mb = 0.11
    last = {k: torch.from_numpy(np.stack([l[k] for l in lasts])).cuda() for k in ("pos", "desc", "valid", "has_obs")}
    last["kps"] = torch.from_numpy(np.stack([l["kps"].view(np.int32).reshape(-1, 6) for l in lasts])).cuda()
    occ = (rng.random((F, C * cap)) < 0.03).astype(np.uint8)
    fb.occ_init = torch.from_numpy(occ).cuda()
    fb.kp_to_mp.fill_(-1)
    base = _live(lib)
    m = ORBmatcher(0.9, checkOri=True)
    m._handle(fb, last["pos"].shape[1])
    held = _live(lib)

    def search():
        m.SearchByProjectionLastFrame(fb, last, torch.from_numpy(Tcw).cuda(), torch.from_numpy(Tlw).cuda(), cams, Trl,
                                      th=7.0, bMono=False, mb=mb)
        torch.cuda.synchronize()

    for k in (1, 2):   # d_push, d_npush
        _arm(lib, k)
        _fails_with_hip(search)
        assert _live(lib) == held + k - 1
    search()
    assert _live(lib) == held + 2
    got, got_n = fb.kp_to_mp.cpu().numpy(), fb.n_matches.cpu().numpy()
    g = oracle.frame_geom(C, W, H, [fb.geom.scale_factors[i] for i in range(8)], [0] * C)
    for f in range(F):
        exp = np.full(C * cap, -1, np.int32)
        n = oracle.search_last_frame(g, kps[f], desc[f], n_kp[f], cams, Tcw[f], Tlw[f], Trl, lasts[f]["pos"],
                                     lasts[f]["desc"], lasts[f]["valid"], lasts[f]["has_obs"], lasts[f]["kps"], 7.0,
                                     False, mb, True, occ[f], exp)
        assert n == got_n[f] and np.array_equal(exp, got[f]), f
        assert n > 200
    m.close()
    assert _live(lib) == base


def test_search_kf_regrowth_failure(lib, oracle, torch_cuda):
    torch = torch_cuda
    b = sk.make_kf_search(2, seed=1)   # SearchByProjection(KF, Sim3): a claim mode, so d_jobs and d_geo both grow
    th, md = sk.MODE_PARAMS[2]
    K, Cb, cap = b["n_kf"], b["n_cams"], b["kp_cap"]
    scale = [1.0]
    for _ in range(1, b["nlevels"]):
        scale.append(float(np.float32(scale[-1] * np.float32(1.2))))
    kfs = FrameBatch(torch, K, Cb, cap, b["width"], b["height"], scale, cam_model=b.get("cam_model"))
    kfs.kps.copy_(torch.from_numpy(np.ascontiguousarray(b["kps"]).view(np.int32).reshape(K, Cb, cap, 6)))
    kfs.desc.copy_(torch.from_numpy(b["desc"]))
    kfs.n_kp.copy_(torch.from_numpy(b["n_kp"]))
    kfs.kp_to_mp.copy_(torch.from_numpy(b["kp_match"]))
    mps = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b["mps"].items()}
    mp_list = torch.from_numpy(b["mp_list"]).cuda()
    p = kf_search_params(th, md, b["cams"], bf=float(b["bf"]), nlevels=b["nlevels"],
                         uright=torch.from_numpy(b["uright"]).cuda(), mp_angle=torch.from_numpy(b["mp_angle"]).cuda())
    base = _live(lib)
    m = ORBmatcher(0.8, checkOri=True)
    m._handle(kfs, max(1, -(-len(mp_list) // (K * Cb))))
    held = _live(lib)

    def search():
        r = m.SearchByProjectionSim3(kfs, b["jobs"], mp_list, mps, kfs.kp_to_mp, p)
        torch.cuda.synchronize()
        return r

    for k in (1, 2):   # d_jobs, d_geo
        _arm(lib, k)
        _fails_with_hip(search)
        assert _live(lib) == held + k - 1
    r = search()
    assert m.last_error() == 0 and _live(lib) == held + 2
    g = tuple(t.cpu().numpy() for t in r) + (kfs.kp_to_mp.cpu().numpy(),)
    o = oracle.search_kf(b, th, md)
    for x, y in zip(g, o):
        assert np.array_equal(x, y)
    assert o[2].sum() > 100
    m.close()
    assert _live(lib) == base


def test_extract_host_staging_failure(lib, oracle):
    """The synchronous path's staging buffers appear on first use, four together: a failure at any of them is made
    good by the next call."""
    img = synth.synth_image(5, ORB_W, ORB_H)
    want = oracle.orb_extract(img, 100, 1.2, 2, 20, 7, (0, 0))
    base = _live(lib)
    ex = ORBextractor(100, 1.2, 2, 20, 7, width=ORB_W, height=ORB_H)
    held = _live(lib)
    for k in (1, 2, 3, 4):
        _arm(lib, k)
        _fails_with_hip(lambda: ex(img, None, (0, 0)))
        assert _live(lib) == held + k - 1
    got = ex(img, None, (0, 0))
    assert _live(lib) == held + 4
    assert got[0] == want[0]
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and np.array_equal(got[2], want[2])
    ex.close()
    assert _live(lib) == base


# ---- per-call stream-ordered workspaces --------------------------------------------------------------------------------
def _dev_view(kf, level_sigma2=None):
    import torch
    d = {f: kf[f] for f in ("n", "n_left", "n_right", "n_sideleft")}
    d["kps"] = torch.from_numpy(kf["kps"].view(np.float32).reshape(-1, 6).copy()).cuda()
    for f in ("desc", "has_mp", "node_start", "node_idx"):
        d[f] = torch.from_numpy(np.ascontiguousarray(kf[f])).cuda()
    d["node_id"] = torch.from_numpy(kf["node_id"].view(np.int32).copy()).cuda()
    if level_sigma2 is not None:
        d["level_sigma2"] = level_sigma2
    return d


def test_search_by_bow_workspace_failure(lib, oracle, torch_cuda):
    torch = torch_cuda
    p = synth_tri.make_tri_pair(seed=1, n_pts=360, mp_frac=0.8, n_nodes=70)
    job = dict(kf=_dev_view(p["kf1"]), other=_dev_view(p["kf2"]),
               match=torch.full((p["kf2"]["n"],), -9, dtype=torch.int32, device="cuda"))
    m = ORBmatcher(0.75, True)
    m._scratch_handle()
    held = _live(lib)
    _arm(lib, 1)
    _fails_with_hip(lambda: m.SearchByBoW([job]))
    assert _live(lib) == held
    n = m.SearchByBoW([job]).cpu().numpy()
    assert _live(lib) == held
    n_o, m_o = oracle.search_by_bow(dict(kf=p["kf1"], other=p["kf2"]), kf_kf=False, nnratio=0.75, check_ori=True)
    assert n[0] == n_o and np.array_equal(job["match"].cpu().numpy(), m_o)
    assert n_o > 20


def test_search_for_triangulation_workspace_failure(lib, oracle, torch_cuda):
    torch = torch_cuda
    p = synth_tri.make_tri_pair(seed=1, n_pts=450)
    pair = dict(T=p["T"], kf1=_dev_view(p["kf1"], p["level_sigma2"]), kf2=_dev_view(p["kf2"], p["level_sigma2"]),
                match12=torch.full((p["kf1"]["n"],), -9, dtype=torch.int32, device="cuda"))
    m = ORBmatcher(0.6, False)
    m._scratch_handle()
    held = _live(lib)
    _arm(lib, 1)
    _fails_with_hip(lambda: m.SearchForTriangulation([pair], p["cams"]))
    assert _live(lib) == held
    n = m.SearchForTriangulation([pair], p["cams"]).cpu().numpy()
    assert _live(lib) == held
    n_o, m_o = oracle.search_for_triangulation(p, coarse=False, check_ori=False)
    assert n[0] == n_o and np.array_equal(pair["match12"].cpu().numpy(), m_o)


def test_fuse_workspace_failure(lib, oracle):
    ref = oracle.search_in_neighbors_fuse(synth_fuse.make_fuse_scene(seed=3, n_targets=4))
    base = _live(lib)
    m = ORBmatcher(0.6)
    n_matcher = HANDLES["matcher"][2]
    _arm(lib, n_matcher + 1)   # the call creates the matcher's handle, then takes its first workspace
    _fails_with_hip(lambda: mapping.SearchInNeighborsFuse(synth_fuse.make_fuse_scene(seed=3, n_targets=4), m))
    assert _live(lib) == base + n_matcher   # the handle, no workspace
    held = _live(lib)
    got = mapping.SearchInNeighborsFuse(synth_fuse.make_fuse_scene(seed=3, n_targets=4), m)
    assert _live(lib) == held + 1   # the handle's grown d_jobs stays, the workspace is gone
    for k in ("n_fused", "log", "kf_mps", "bad", "replaced", "n_obs", "obs_start", "obs_kf", "obs_idx", "desc"):
        np.testing.assert_array_equal(np.asarray(got[k]).ravel(), np.asarray(ref[k]).ravel(), err_msg=k)
    m.close()
    assert _live(lib) == base
