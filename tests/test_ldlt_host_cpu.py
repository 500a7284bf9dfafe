"""The host read-back of the block LDL^T solver (openmavis_amd/csrc/omv_ldlt_host.h, expand_solved: what every
debug_solve returns as S and plan[]), through the stand-alone program tests/cpp/ldlt_host.cpp (its own main): every stored
block lands where its keyframes say, mirrored, a diagonal block's upper triangle is never read, blocks that are not stored
stay exactly zero, and the same program is clean under -fsanitize=address,undefined (host code only, run directly)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -1.0
# a 6-vertex Sim3 graph (one fixed vertex, one loop edge): 5 optimisable vertices in 3 blocks -- three blocks are too few
# for fill; a 10-vertex loop: a cycle of 5 blocks, which no elimination order factors without fill; 4 keyframes in a band
CASES = {"sim3_6": ("sim3", 6, 2, 5, 0), "sim3_10": ("sim3", 10, 0, 9, 1), "band_4": ("band", 4, 2)}


def _build(tmp, sanitize):
    assert shutil.which("g++") is not None
    exe = str(tmp / ("ldlt_host" + ("_san" if sanitize else "")))
    src = os.path.join(ROOT, "tests", "cpp", "ldlt_host.cpp")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        return r.stdout

    return run


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("ldlt_host"), False)


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("ldlt_host_san"), True)


def _parse(text):
    out = {}
    for ln in text.strip().split("\n"):
        k, *v = ln.split()
        out[k] = [int(x) for x in v]
    out["nb"], out["n_slots"], out["n_lds"], out["n_lev"], out["use_lds"] = out["scalars"]
    n = 16 * out["nb"]
    out["S"] = np.array(out["S"], np.float64).reshape(n, n)
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_expansion(host, case):
    p = _parse(host(*CASES[case]))
    nb, S = p["nb"], p["S"]
    slots = list(zip(p["slot_kr"], p["slot_kc"]))
    assert len(slots) == p["n_slots"] == len(set(slots)) and all((k, k) in slots for k in range(nb))
    assert np.array_equal(S, S.T)
    assert not np.any(S == POISON)   # the upper triangle of a diagonal block is not read
    r, c = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    stored = np.zeros((nb, nb), bool)
    for t, (kr, kc) in enumerate(slots):
        want = 1.0 + 256 * t + 16 * r + c
        got = S[16 * kr:16 * kr + 16, 16 * kc:16 * kc + 16]
        if kr == kc:   # the lower triangle as stored, the upper one its mirror
            assert np.array_equal(np.tril(got), np.tril(want)) and np.array_equal(np.triu(got), np.tril(want).T)
        else:
            assert np.array_equal(got, want) and np.array_equal(S[16 * kc:16 * kc + 16, 16 * kr:16 * kr + 16], want.T)
        stored[kr, kc] = stored[kc, kr] = True
    for i in range(nb):
        for j in range(nb):
            if not stored[i, j]:
                assert not np.any(S[16 * i:16 * i + 16, 16 * j:16 * j + 16])   # exactly zero
    assert p["plan"][:4] == [p["use_lds"], p["n_slots"], p["n_lds"], p["n_lev"]]
    assert len(p["plan"]) == 4 + p["n_lev"] and sum(p["plan"][4:]) == nb and min(p["plan"][4:]) >= 1
    # a stored off-diagonal block that no edge joins is fill
    eb = p["edge_blocks"]
    joined = {frozenset(eb[q:q + 2]) for q in range(0, len(eb), 2)}
    fill = [s for s in slots if s[0] != s[1] and frozenset(s) not in joined]
    assert all(frozenset(s) in {frozenset(x) for x in slots} for s in joined if len(s) == 2 and -1 not in s)
    assert fill or case != "sim3_10"   # the case that is there for its fill has some


def test_clean_under_the_sanitizers(host_san, host):
    for args in CASES.values():
        assert host_san(*args) == host(*args)
