"""The host part of the batched RANSAC frame (openmavis_amd/csrc/ransac_plan.h) without a GPU: the real C++ as a
stand-alone program built with -fsanitize=address,undefined (tests/cpp/ransac_plan_host.cpp), run once on the
cases below.  mRansacMaxIts against the tables of the two reference tests and tests/ransac_ref.py, the layout of a
ragged batch against numpy cumsums, and the order of the argument checks of omv_sim3_solver_set / omv_pnp_set."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mlpnp_ref
import ransac_ref
import sim3_ref
from openmavis_amd import _lib
from test_mlpnp_ref_cpu import test_ransac_parameter_tables as _pnp_table_test
from test_sim3solver_ref_cpu import MAX_ITS_TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNP_TABLE = [m for m in _pnp_table_test.pytestmark if m.name == "parametrize"][0].args[1]
ARG, CAPACITY = _lib.OMV_ERR_ARG, _lib.OMV_ERR_CAPACITY

N_RAGGED, MN_RAGGED = [0, 63, 64, 65, 1], [0, 70, 64, 200, 1]


def _layout(n, mn, index=None, max_jobs=None, max_corr=None, words_cap=-1, bad_job=-1, nulls=0, corr_start=None):
    """One `layout` line; by default a handle that just fits and index = 0 .. n-1 per job."""
    cs = corr_start if corr_start is not None else np.cumsum([0] + n).tolist() if n else []
    if index is None:
        index = [i for k in n for i in range(k)]
    max_jobs = len(n) if max_jobs is None else max_jobs
    max_corr = (cs[-1] if cs else 0) if max_corr is None else max_corr
    return " ".join(str(v) for v in ["layout", max_jobs, max_corr, words_cap, bad_job, nulls, len(n), *cs, *mn, *index])


# (name, line, expected status): one rejection per rule of the order both `set` functions keep --
#   1 null pointers -> ARG, 2 n_jobs > max_jobs -> CAPACITY, 3 corr_start[0] != 0 -> ARG, 4 per job a non-monotone
#   corr_start / mN < 0 / the camera model -> ARG, 5 n_corr > max_corr -> CAPACITY, 6 null data arrays -> ARG,
#   7 index outside [0, mN) -> ARG, 8 words > words_cap -> CAPACITY -- then three double faults that pin the precedence
REJECTIONS = [
    ("null corr_start", _layout([4], [4], nulls=1), ARG),
    ("null mN", _layout([4], [4], nulls=2), ARG),
    ("negative n_jobs", "layout 1 0 -1 -1 0 -1", ARG),
    ("too many jobs", _layout([4, 4], [4, 4], max_jobs=1), CAPACITY),
    ("corr_start[0] != 0", _layout([4], [9], corr_start=[1, 5], index=[0] * 5), ARG),
    ("corr_start decreases", _layout([4, 0], [4, 4], corr_start=[0, 4, 3]), ARG),
    ("negative mN", _layout([0, 4], [-1, 4]), ARG),
    ("camera model", _layout([4, 4], [4, 4], bad_job=1), ARG),
    ("too many correspondences", _layout([4, 4], [4, 4], max_corr=7), CAPACITY),
    ("null data arrays", _layout([4], [4], nulls=4), ARG),
    ("index == mN", _layout([4], [4], index=[0, 1, 2, 4]), ARG),
    ("negative index", _layout([4], [4], index=[0, -1, 2, 3]), ARG),
    ("too many words", _layout([1, 1, 1], [1, 1, 1], words_cap=2), CAPACITY),
    ("too many jobs and corr_start[0] != 0", _layout([4, 4], [9, 9], corr_start=[1, 5, 9], max_jobs=1), CAPACITY),
    ("too many correspondences and a negative mN", _layout([4, 4], [4, -1], max_corr=7), ARG),
    ("index out of range and too many words", _layout([1, 1, 1], [1, 1, 1], index=[0, 0, 1], words_cap=2), ARG),
]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    """The program's output lines, keyed by the kind of case, from its one run."""
    assert shutil.which("g++") is not None
    exe = str(tmp_path_factory.mktemp("ransac_plan") / "ransac_plan_host")
    src = os.path.join(ROOT, "tests", "cpp", "ransac_plan_host.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    cases = [f"its {p!r} {mi} {n} {mx}" for p, mi, n, mx, _ in MAX_ITS_TABLE]
    cases += [f"pnp {n} {p[0]!r} {p[1]} {p[2]} {p[3]} {p[4]!r}" for n, p, _ in PNP_TABLE]
    cases += [_layout(N_RAGGED, MN_RAGGED), _layout([], [], max_jobs=1)]
    cases += [line for _, line, _ in REJECTIONS]
    r = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = r.stdout.strip().split("\n")
    assert len(out) == len(cases)
    a, b = len(MAX_ITS_TABLE), len(MAX_ITS_TABLE) + len(PNP_TABLE)
    return dict(its=out[:a], pnp=out[a:b], ragged=out[b], empty=out[b + 1], rejections=out[b + 2:])


def test_sim3_max_its_equals_the_table_and_the_reference(lines):
    for (prob, mi, n, mx, expect), line in zip(MAX_ITS_TABLE, lines["its"]):
        eps = np.float32(mi) / np.float32(n)
        assert line == f"its {expect}" == f"its {sim3_ref.ransac_max_its(prob, mi, n, mx)}" \
            == f"its {ransac_ref.ransac_its(prob, eps, mi == n, mx)}", (prob, mi, n, mx)


def test_mlpnp_parameters_equal_the_table_and_the_reference(lines):
    for (n, params, expected), line in zip(PNP_TABLE, lines["pnp"]):
        got = tuple(int(v) for v in line.split()[1:])
        assert got == mlpnp_ref.ransac_parameters(n, *params[:5]), (n, params)
        if n != 20:   # that row's expectation is evaluated by test_ransac_parameter_tables itself
            assert got == expected, (n, params)


def test_layout_of_a_ragged_batch(lines):
    status, inl, word, total, corr_job = (f.split() for f in lines["ragged"].split("|"))
    n, mn = np.array(N_RAGGED), np.array(MN_RAGGED)
    assert status == ["status", "0"]
    assert [int(v) for v in inl] == (np.cumsum(mn) - mn).tolist()
    words = (n + 63) // 64
    assert [int(v) for v in word] == (np.cumsum(words) - words).tolist()
    assert int(total[0]) == words.sum() == 5
    assert [int(v) for v in corr_job] == np.repeat(np.arange(len(n)), n).tolist()
    assert lines["empty"] == "status 0 | | | 0 |"


def test_argument_checks_keep_their_order(lines):
    assert len(lines["rejections"]) == len(REJECTIONS)
    for (name, _, expect), line in zip(REJECTIONS, lines["rejections"]):
        assert line == f"status {expect}", name
