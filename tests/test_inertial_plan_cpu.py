"""The host planner of the device InertialOptimization (openmavis_amd/csrc/inertial_plan.h): the keyframes ordered along
their mPrevKF paths.  Through the library's host-only hook omv_inertial_opt_plan (no device is touched), and once more
as a stand-alone program built with -fsanitize=address,undefined (tests/cpp/inertial_plan_host.cpp)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from openmavis_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan():
    assert os.path.exists(_lib.LIB_PATH), "libomv_hip.so not built"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fn = lib.omv_inertial_opt_plan
    fn.restype = ctypes.c_int

    def run(K, kf1, kf2):
        a, b = np.asarray(kf1, np.int32), np.asarray(kf2, np.int32)
        o = [np.full(max(K, 1), -7, np.int32) for _ in range(4)]
        n = ctypes.c_int32(-1)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        st = fn(ctypes.c_int(K), ctypes.c_int(len(a)), p(a), p(b), *[p(x) for x in o], ctypes.byref(n))
        if st != _lib.OMV_OK:
            assert st == _lib.OMV_ERR_ARG
            return None
        return dict(order=o[0][:K].tolist(), pos_of=o[1][:K].tolist(), edge_in=o[2][:K].tolist(),
                    edge_out=o[3][:K].tolist(), n_paths=n.value)

    return run


def _check(P, K, kf1, kf2):
    """The plan's invariants: a permutation; along a path positions are consecutive; the edge arrays agree."""
    assert sorted(P["order"]) == list(range(K))
    assert all(P["pos_of"][P["order"][p]] == p for p in range(K))
    seen = set()
    for p in range(K):
        e = P["edge_out"][p]
        if e >= 0:
            assert kf1[e] == P["order"][p] and kf2[e] == P["order"][p + 1] and P["edge_in"][p + 1] == e
            seen.add(e)
        elif p + 1 < K:
            assert P["edge_in"][p + 1] == -1
    assert P["edge_in"][0] == -1 if K else True
    assert seen == set(range(len(kf1)))
    assert P["n_paths"] == K - len(kf1)


def test_chain(plan):
    P = plan(4, [0, 1, 2], [1, 2, 3])
    assert P["order"] == [0, 1, 2, 3] and P["edge_in"] == [-1, 0, 1, 2] and P["edge_out"] == [0, 1, 2, -1]
    assert P["n_paths"] == 1


def test_chain_split_by_a_bad_keyframe(plan):
    kf1, kf2 = [0, 1, 3, 4], [1, 2, 4, 5]   # no edge into keyframe 3
    P = plan(6, kf1, kf2)
    assert P["order"] == [0, 1, 2, 3, 4, 5] and P["edge_out"] == [0, 1, -1, 2, 3, -1] and P["n_paths"] == 2
    _check(P, 6, kf1, kf2)


def test_isolated_keyframes(plan):
    P = plan(5, [0, 3], [1, 4])
    assert P["order"] == [0, 1, 2, 3, 4] and P["edge_in"] == [-1, 0, -1, -1, 1] and P["n_paths"] == 3
    assert plan(1, [], [])["order"] == [0] and plan(0, [], [])["order"] == []
    P = plan(3, [], [])
    assert P["order"] == [0, 1, 2] and P["edge_out"] == [-1, -1, -1] and P["n_paths"] == 3


def test_shuffled_input_order(plan):
    kf1, kf2 = [3, 0, 2, 4], [0, 2, 4, 1]   # 3 -> 0 -> 2 -> 4 -> 1, edges in any order
    P = plan(5, kf1, kf2)
    assert P["order"] == [3, 0, 2, 4, 1] and P["edge_out"] == [0, 1, 2, 3, -1]
    rng = np.random.default_rng(5)
    for K in (2, 3, 10, 64, 65, 66, 129, 130, 300):
        perm = rng.permutation(K)
        keep = rng.uniform(size=K - 1) > 0.1
        a, b = perm[:-1][keep], perm[1:][keep]
        eo = rng.permutation(len(a))
        _check(plan(K, a[eo], b[eo]), K, a[eo].tolist(), b[eo].tolist())


def test_rejects_what_is_not_a_forest_of_paths(plan):
    assert plan(3, [0, 0], [1, 2]) is None       # two successors
    assert plan(3, [0, 1], [2, 2]) is None       # two predecessors
    assert plan(3, [0, 1, 2], [1, 2, 0]) is None   # a cycle
    assert plan(4, [0, 1, 2], [1, 2, 1]) is None   # a tail that runs into a cycle
    assert plan(3, [0], [3]) is None and plan(3, [-1], [1]) is None   # out of range
    assert plan(3, [1], [1]) is None             # an edge to itself
    assert plan(-1, [], []) is None


def test_planner_under_the_host_sanitizers(tmp_path):
    """The header with a stand-alone main, -fsanitize=address,undefined, run once; the program's lines against the
    plans expected above."""
    assert shutil.which("g++") is not None
    exe = str(tmp_path / "inertial_plan_host")
    src = os.path.join(ROOT, "tests", "cpp", "inertial_plan_host.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "ok 0 | | |" and lines[1] == "ok 1 | 0 | -1 | -1"
    assert lines[2] == "ok 1 | 0 1 2 3 | -1 0 1 2 | 0 1 2 -1"
    assert lines[3] == "ok 2 | 0 1 2 3 4 5 | -1 0 1 -1 2 3 | 0 1 -1 2 3 -1"
    assert lines[4] == "ok 3 | 0 1 2 3 4 | -1 0 -1 -1 1 | 0 -1 -1 1 -1"
    assert lines[5] == "ok 1 | 3 0 2 4 1 | -1 0 1 2 3 | 0 1 2 3 -1"
    assert lines[6:11] == ["reject"] * 5
    assert lines[11] == "long ok 9"
