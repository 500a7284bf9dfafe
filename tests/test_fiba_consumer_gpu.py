"""The C++ adapter omv_adapt::FullInertialBA (include/omv_adapters.hpp), through the plain g++ consumer
tests/cpp/fiba_consumer.cpp, returns the Python call's bits: the bInit form with bFixLocal and points that only the fixed
keyframe sees, and the per-keyframe form on a Pinhole rig with stereo edges."""
import os
import subprocess

import numpy as np
import pytest

import fiba_cases
from openmavis_amd import build as omv_build
from openmavis_amd.optimizer import FullInertialBA

pytestmark = pytest.mark.gpu


def _write_map(path, p, its):
    E, S, NI = len(p["mono_pt"]), int(p.get("n_stereo", 0)), len(p["imu_kf1"])
    C, K = p["n_cams"], p["n_kf"]
    with open(path, "wb") as f:
        np.array([C, K, len(p["pts"]), E, S, NI, its, int(p["n_opt"] < K), int(p["shared_bias"])], np.int32).tofile(f)
        np.array([p.get("bf", 0.0), p["prior_g"], p["prior_a"]], np.float32).tofile(f)
        np.concatenate([p["bg0"], p["ba0"]]).astype(np.float64).tofile(f)
        empty = dict(cam_model=np.zeros(C, np.int32), stereo_pt=[], stereo_kf=[], stereo_obs=[], stereo_inv_sigma2=[])
        for key, dt in (("cam", np.float32), ("cam_model", np.int32), ("Rcb", np.float64), ("tcb", np.float64),
                        ("Rbc", np.float64), ("tbc", np.float64), ("kf_imu", np.uint8), ("Rwb", np.float64),
                        ("twb", np.float64), ("Rcw", np.float64), ("tcw", np.float64), ("vel", np.float64),
                        ("bg", np.float64), ("ba", np.float64), ("pts", np.float64), ("mono_pt", np.int32),
                        ("mono_kf", np.int32), ("mono_cam", np.int32), ("mono_obs", np.float64),
                        ("mono_inv_sigma2", np.float32), ("stereo_pt", np.int32), ("stereo_kf", np.int32),
                        ("stereo_obs", np.float64), ("stereo_inv_sigma2", np.float32), ("imu_kf1", np.int32),
                        ("imu_kf2", np.int32), ("preint", np.float32)):
            np.ascontiguousarray(p[key] if key in p else empty[key], dt).tofile(f)


@pytest.mark.parametrize("name,over", [("fixed_only_pts", {}), ("pinhole_stereo", dict(shared_bias=0))])
def test_cpp_adapter_returns_the_python_bits(tmp_path, name, over):
    exe = omv_build.build_consumer(False, omv_build.FIBA_CONSUMER_SRC, omv_build.FIBA_CONSUMER_BIN)
    assert os.path.exists(exe)
    p = dict(fiba_cases.problem(name), **over)
    its = 6
    ba = FullInertialBA(p["n_kf"], p["n_cams"], len(p["pts"]), len(p["mono_pt"]) + int(p.get("n_stereo", 0)),
                        len(p["imu_kf1"])).set_problem(p)
    g, s = ba.optimize(iterations=its)
    path = str(tmp_path / "map.bin")
    _write_map(path, p, its)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    free = np.zeros(len(p["pts"]), bool)
    free[np.asarray(p["mono_pt"])[np.asarray(p["mono_kf"]) < p["n_opt"]]] = True
    if p.get("n_stereo", 0):
        free[np.asarray(p["stereo_pt"])[np.asarray(p["stereo_kf"]) < p["n_opt"]]] = True
    want = ["ran", "1", "it", str(g["iterations"]), "tr", str(g["trials"]), "err", "%.17g" % g["err"], "%.17g" % g["err_end"],
            "not_included", str(int((~free).sum()))]
    for k in ("Rwb", "twb", "vel", "bg", "ba", "pts"):
        want += [k] + ["%.17g" % v for v in np.asarray(s[k]).reshape(-1)]
    tok = r.stdout.split()
    assert len(tok) == len(want) and tok == want, name
    assert name != "fixed_only_pts" or int((~free).sum()) == 5
