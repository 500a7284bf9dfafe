"""The C++ adapter omv_adapt::LocalBundleAdjustment (include/omv_adapters.hpp), through the plain g++ consumer
tests/cpp/vba_consumer.cpp, returns the Python call's bits on the `small` window (and on `mixed`, which has stereo
edges and edges to erase in all five groups' order)."""
import os
import subprocess

import numpy as np
import pytest

import vba_cases
from openmavis_amd import build as omv_build
from openmavis_amd.optimizer import LocalBundleAdjustment

pytestmark = pytest.mark.gpu


def _write_window(path, p, inertial_map):
    E, S = len(p["mono_pt"]), len(p["stereo_pt"])
    with open(path, "wb") as f:
        np.array([p["n_cams"], p["n_kf"], p["n_opt"], len(p["pts"]), E, S, int(inertial_map)], np.int32).tofile(f)
        np.array([p[k] for k in ("fx", "fy", "cx", "cy", "bf")], np.float64).tofile(f)
        for key, dt in (("cam", np.float32), ("cam_model", np.int32), ("q_c0", np.float64), ("t_c0", np.float64),
                        ("q_cw", np.float64), ("t_cw", np.float64), ("pts", np.float64), ("mono_pt", np.int32),
                        ("mono_kf", np.int32), ("mono_cam", np.int32), ("mono_obs", np.float64),
                        ("mono_inv_sigma2", np.float32), ("stereo_pt", np.int32), ("stereo_kf", np.int32),
                        ("stereo_obs", np.float64), ("stereo_inv_sigma2", np.float32)):
            np.ascontiguousarray(p[key], dt).tofile(f)


@pytest.mark.parametrize("name,inertial_map", [("small", False), ("mixed", True)])
def test_cpp_adapter_returns_the_python_bits(oracle, tmp_path, name, inertial_map):
    exe = omv_build.build_consumer(False, omv_build.VBA_CONSUMER_SRC, omv_build.VBA_CONSUMER_BIN)
    assert os.path.exists(exe)
    p = vba_cases.problem(name)
    E, S = len(p["mono_pt"]), len(p["stereo_pt"])
    ba = LocalBundleAdjustment(p["n_kf"], p["n_cams"], len(p["pts"]), E + S).set_problem(p)
    g, s = ba.optimize(10, lambda_init=100.0 if inertial_map else 0.0)
    erase = []
    for c in (0, 1):
        erase += [(int(p["mono_kf"][e]), int(p["mono_pt"][e])) for e in np.nonzero((p["mono_cam"] == c) & (g["mono_outlier"] != 0))[0]]
    erase += [(int(p["stereo_kf"][e]), int(p["stereo_pt"][e])) for e in np.nonzero(g["stereo_outlier"])[0]]
    for c in (2, 3):
        erase += [(int(p["mono_kf"][e]), int(p["mono_pt"][e])) for e in np.nonzero((p["mono_cam"] == c) & (g["mono_outlier"] != 0))[0]]
    path = str(tmp_path / "window.bin")
    _write_window(path, p, inertial_map)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    want = (["fixed", str(p["n_kf"] - p["n_opt"]), "opt", str(p["n_opt"]), "mps", str(len(p["pts"])), "edges", str(E + S),
             "it", str(g["iterations"]), "tr", str(g["trials"]), "err", "%.17g" % g["err"], "%.17g" % g["err_end"], "q"]
            + ["%.17g" % v for v in s["q_cw"].reshape(-1)] + ["t"] + ["%.17g" % v for v in s["t_cw"].reshape(-1)]
            + ["pts"] + ["%.17g" % v for v in s["pts"].reshape(-1)] + ["erase"] + [str(v) for kp in erase for v in kp])
    tok = r.stdout.split()
    assert len(tok) == len(want) and tok == want, name
    assert name == "small" or len(erase) > 10
