"""GPU parity of the keyframe-side projection searches (omv_matcher_search_kf in
openmavis_amd/csrc/match.hip) against the CPU oracle (oracle/match_oracle.cpp): ORBmatcher::Fuse (both
overloads), SearchByProjection(KF, Sim3, ...) and SearchByProjection(Frame&, KF, ...)
(src/ORBmatcher.cc:668-893, 1458-1769, 2415-2535).  Integer / index work: bit-exact — per entry the chosen
keypoint and distance, the per-job return values and the claim arrays."""
import numpy as np
import pytest

from openmavis_amd import synth_kfmatch as sk
from openmavis_amd.matcher import FrameBatch, ORBmatcher, kf_search_params

pytestmark = pytest.mark.gpu


def _run_gpu(b, th, max_dist, check_ori=True):
    import torch
    dev = "cuda:0"
    K, C, cap = b["n_kf"], b["n_cams"], b["kp_cap"]
    scale = [1.0]
    for _ in range(1, b["nlevels"]):
        scale.append(float(np.float32(scale[-1] * np.float32(1.2))))
    kfs = FrameBatch(torch, K, C, cap, b["width"], b["height"], scale, device=dev, cam_model=b.get("cam_model"))
    kfs.kps.copy_(torch.from_numpy(np.ascontiguousarray(b["kps"]).view(np.int32).reshape(K, C, cap, 6)))
    kfs.desc.copy_(torch.from_numpy(b["desc"]))
    kfs.n_kp.copy_(torch.from_numpy(b["n_kp"]))
    kfs.kp_to_mp.copy_(torch.from_numpy(b["kp_match"]))
    mps = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in b["mps"].items()}
    mp_list = torch.from_numpy(b["mp_list"]).to(dev)
    uright = torch.from_numpy(b["uright"]).to(dev)
    angle = torch.from_numpy(b["mp_angle"]).to(dev)
    p = kf_search_params(th, max_dist, b["cams"], bf=float(b["bf"]), nlevels=b["nlevels"], uright=uright,
                         mp_angle=angle)
    m = ORBmatcher(0.8, checkOri=check_ori)
    mode = b["mode"]
    if mode == 0:
        r = m.Fuse(kfs, b["jobs"], mp_list, mps, p)
    elif mode == 1:
        r = m.FuseSim3(kfs, b["jobs"], mp_list, mps, p)
    elif mode == 2:
        r = m.SearchByProjectionSim3(kfs, b["jobs"], mp_list, mps, kfs.kp_to_mp, p)
    else:
        r = m.SearchByProjectionKF(kfs, b["jobs"], mp_list, mps, p)
    torch.cuda.synchronize()
    assert m.last_error() == 0
    return tuple(t.cpu().numpy() for t in r) + (kfs.kp_to_mp.cpu().numpy(),)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("seed", [1, 2])
def test_kf_search_matches_oracle(oracle, mode, seed):
    b = sk.make_kf_search(mode, seed=seed)
    th, md = sk.MODE_PARAMS[mode]
    g = _run_gpu(b, th, md)
    o = oracle.search_kf(b, th, md)
    assert np.array_equal(g[0], o[0]), (g[0] != o[0]).sum()
    assert np.array_equal(g[1], o[1])
    assert np.array_equal(g[2], o[2]), (g[2], o[2])
    if mode >= 2:
        assert np.array_equal(g[3], o[3])
    assert o[2].sum() > 100


def test_sbp_frame_without_orientation_check(oracle):
    b = sk.make_kf_search(3, seed=3)
    g = _run_gpu(b, 10.0, 100.0, check_ori=False)
    o = oracle.search_kf(b, 10.0, 100.0, check_ori=False)
    for x, y in zip(g, o):
        assert np.array_equal(x, y)


def test_sbp_frame_orientation_check_removes_a_match(oracle):
    """A SearchByProjection(Frame&, KF) batch on which the rotation histogram un-claims a match (seed chosen with the
    oracle: 683 matches without the check, 682 with it); the other cases of this file lose none to it."""
    b = sk.make_kf_search(3, seed=31)
    th, md = sk.MODE_PARAMS[3]
    o = oracle.search_kf(b, th, md)
    assert o[2].sum() < oracle.search_kf(b, th, md, check_ori=False)[2].sum()
    for x, y in zip(_run_gpu(b, th, md), o):
        assert np.array_equal(x, y)


def test_sbp_sim3_crowded_claims_rescan(oracle):
    """Dense windows (radius 40 px) so that all 16 stored candidates of many points are claimed and the
    resolve must rescan the window."""
    b = sk.make_kf_search(2, seed=4, pts_per_job=500, kp_cap=400)
    g = _run_gpu(b, 40.0, 200.0)
    o = oracle.search_kf(b, 40.0, 200.0)
    for x, y in zip(g, o):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("model", ["pinhole", ["pinhole", "kb8", "pinhole", "kb8", "kb8"]])
def test_kf_search_pinhole_rig(oracle, mode, model):
    """Fuse / Fuse(Sim3) / SearchByProjection(KF, Sim3) / SearchByProjection(F, KF) on Pinhole (and mixed) rigs:
    pCamera / GetCamera(camId) / CurrentFrame.mpCamera->project by the block's type (ORBmatcher.cc:1536, :1710,
    :710, :2443).  Bit-exact."""
    b = sk.make_kf_search(mode, seed=7, model=model)
    th, md = sk.MODE_PARAMS[mode]
    g = _run_gpu(b, th, md)
    o = oracle.search_kf(b, th, md)
    for x, y in zip(g, o):
        assert np.array_equal(x, y)
    assert o[2].sum() > 100
    # the camera type matters: the same data read as KB8 gives other answers
    okb = oracle.search_kf(dict(b, cam_model=np.zeros_like(b["cam_model"])), th, md)
    assert not np.array_equal(okb[0], o[0])
