"""The C++ adapters omv_adapt::OptimizeEssentialGraph / OptimizeEssentialGraph4DoF (include/omv_adapters.hpp), through the
plain g++ consumer tests/cpp/essgraph_consumer.cpp, return the Python call's bits on case (a) in both kinds."""
import os
import subprocess

import numpy as np
import pytest

import essgraph_cases
from openmavis_amd import build as omv_build
from openmavis_amd.optimizer import OptimizeEssentialGraph, OptimizeEssentialGraph4DoF

pytestmark = pytest.mark.gpu


def _write_graph(path, kind, p):
    n, E, m = len(p["vertices"]), len(p["edge_i"]), len(p["point_ref"])
    with open(path, "wb") as f:
        np.array([kind, n, E, m, int(p.get("fix_scale", 0))], np.int32).tofile(f)
        for key, dt in (("S_a", np.float64), ("S_b", np.float64), ("fixed", np.uint8), ("edge_i", np.int32),
                        ("edge_j", np.int32), ("edge_table", np.int32)):
            np.ascontiguousarray(p[key], dt).tofile(f)
        if kind == essgraph_cases.DOF4:
            for key in ("vertices", "Rcb", "tcb"):
                np.ascontiguousarray(p[key], np.float64).tofile(f)
        np.ascontiguousarray(p["points"], np.float32).tofile(f)
        np.ascontiguousarray(p["point_ref"], np.int32).tofile(f)


@pytest.mark.parametrize("name", ["a_sim3", "a_sim3_fix_scale", "a_4dof"])
def test_cpp_adapter_returns_the_python_bits(tmp_path, name):
    exe = omv_build.build_consumer(False, omv_build.ESSGRAPH_CONSUMER_SRC, omv_build.ESSGRAPH_CONSUMER_BIN)
    assert os.path.exists(exe)
    kind, p = essgraph_cases.make(name)
    g = OptimizeEssentialGraph(p) if kind == essgraph_cases.SIM3 else OptimizeEssentialGraph4DoF(p)
    path = str(tmp_path / "graph.bin")
    _write_graph(path, kind, p)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    want = ["it", str(g["iterations"]), "tr", str(g["trials"]), "fail", str(g["solver_failed"]), "err", "%.17g" % g["err"],
            "%.17g" % g["err_end"]]
    want += ["vertices"] + ["%.17g" % v for v in g["vertices"].reshape(-1)]
    want += ["poses"] + ["%.9g" % v for v in g["poses"].reshape(-1)]
    want += ["points"] + ["%.9g" % v for v in g["points"].reshape(-1)]
    tok = r.stdout.split()
    assert len(tok) == len(want) and tok == want, name
    assert g["err_end"] < g["err"]
