"""The KeyFrameDatabase reference (tests/kfdb_ref.py) pinned on the CPU: the dense (first shared word, add sequence)
formulation the device code uses equals the literal inverted-file walk, the score is the L1 score, the order of the
sum matters in the scene built for it, and every designed scene's output depends on the behaviour it is named after
(so the bit-exact GPU comparison on those scenes in tests/test_kfdb_gpu.py means something).

Two of the behaviours the reference has on paper cannot change an output as literally stated, because within one call a keyframe's
map, flags and the room in the lists never change back: marking a first occurrence that was rejected
(spAlreadyAddedKF.insert after a failed push), and the order of the relocalisation map filter and the dedup.  Their
scenes probe the observable consequence instead: a same-map keyframe that finds the loop list full is not offered to
the merge list, and the relocalisation threshold is taken over the keyframes of every map before the map filter."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import kfdb_ref
from openmavis_amd import synth_kfdb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Dense:
    """The array formulation: a table of BowVectors by slot with an occupancy flag, a sequence number and the stored
    query id; lKFsSharingWords = the occupied, sharing, unconnected slots whose stored id differs, ascending in
    (smallest shared word, sequence); the word count = the size of the intersection."""

    def __init__(self, max_kf):
        self.words = [None] * max_kf
        self.occ = np.zeros(max_kf, bool)
        self.seq = np.zeros(max_kf, np.int64)
        self.map = np.zeros(max_kf, np.int64)
        self.stored = {"nbest": np.zeros(max_kf, np.int64), "reloc": np.zeros(max_kf, np.int64)}
        self.next_seq = 0

    def add(self, slot, map_id, bow):
        self.words[slot], self.occ[slot], self.seq[slot], self.map[slot] = set(bow), True, self.next_seq, map_id
        self.stored["nbest"][slot] = self.stored["reloc"][slot] = 0
        self.next_seq += 1

    def listing(self, mode, qid, bow, connected):
        q = set(bow)
        rows = []
        for s in np.nonzero(self.occ)[0]:
            shared = q & self.words[s]
            if not shared or (mode == "nbest" and s in connected) or self.stored[mode][s] == qid:
                continue
            self.stored[mode][s] = qid
            rows.append((min(shared), self.seq[s], int(s), len(shared)))
        rows.sort()
        return [r[2] for r in rows], [r[3] for r in rows]


def run_dense(scene):
    d = Dense(scene["max_kf"])
    out = []
    for op in scene["ops"]:
        if op[0] == "add":
            for s, m, b in zip(op[1], op[2], op[3]):
                d.add(int(s), int(m), kfdb_ref.to_dict(b))
        elif op[0] == "erase":
            d.occ[np.asarray(op[1], np.int64)] = False
        elif op[0] == "clear":
            d.occ[:] = False
        elif op[0] == "clearMap":
            d.occ[d.map == op[1]] = False
        elif op[0] in ("nbest", "reloc"):
            out.append([d.listing(op[0], q["id"], kfdb_ref.to_dict(q["bow"]),
                                  set(int(s) for s in q.get("connected", ()))) for q in op[1]])
    return out


SCENES = [dict(n_kf=120, n_words=400, lengths=[5, 20, 40], seed=11, n_q=3, rounds=3),
          dict(n_kf=65, n_words=50, lengths=[0, 1, 10, 30], seed=12, n_q=3, rounds=3),
          dict(n_kf=64, n_words=5000, lengths=[63, 64, 65, 257], seed=13, n_q=2, rounds=3, mode="reloc")]


@pytest.mark.parametrize("kw", SCENES, ids=lambda kw: f"{kw['n_kf']}kf_{kw['n_words']}w")
def test_dense_formulation_equals_inverted_file_walk(kw):
    scene = synth_kfdb.random_scene(**kw)
    assert any(op[0] == "erase" for op in scene["ops"]) and any(op[0] == "clearMap" for op in scene["ops"])
    ref = kfdb_ref.run_scene(scene)
    dense = run_dense(scene)
    n_listed = 0
    for call_r, call_d in zip(ref, dense):
        for r, (slots, words) in zip(call_r, call_d):
            assert list(r["debug"]["list_slot"]) == slots
            assert list(r["debug"]["list_words"]) == words
            n_listed += len(slots)
    assert n_listed > 20


def test_erase_and_readd_moves_a_keyframe_to_the_back():
    U = synth_kfdb.uniform_bow
    ops = [("add", [0, 1, 2], [0, 0, 0], [U([1, 2]), U([1, 3]), U([1, 4])]),
           ("nbest", [dict(id=1, map=0, bow=U([1]), connected=[])], 3),
           ("erase", [0]), ("add", [0], [0], [U([1, 2])]),
           ("nbest", [dict(id=2, map=0, bow=U([1]), connected=[])], 3)]
    r = kfdb_ref.run_scene(dict(n_words=10, max_kf=4, ops=ops))
    assert list(r[0][0]["debug"]["list_slot"]) == [0, 1, 2] and list(r[1][0]["debug"]["list_slot"]) == [1, 2, 0]


def _l1(v, w):
    keys = set(v) | set(w)
    return sum(abs(v.get(k, 0.0) - w.get(k, 0.0)) for k in keys)


def test_score_is_the_l1_score():
    """1 - 0.5 ||v - w||_1 holds for vectors whose L1 norm is 1; a normalised vector's norm is 1 only to rounding, a
    few 2^-53 per element, so the 1e-15 comparison uses short vectors (<= 24 words), and `exactly 1 for identical
    vectors` uses dyadic weights, whose sums are exact."""
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(300):
        v = kfdb_ref.to_dict(synth_kfdb.random_bow(rng, 40, int(rng.integers(1, 25))))
        w = kfdb_ref.to_dict(synth_kfdb.random_bow(rng, 40, int(rng.integers(1, 25))))
        assert abs(kfdb_ref.l1_score(v, w) - (1.0 - 0.5 * _l1(v, w))) <= 1e-15
        assert abs(kfdb_ref.l1_score(v, v) - 1.0) <= 1e-15
    for n in (1, 7, 64, 100):
        k = rng.integers(1, 9, n)
        k[0] += 1024 - k.sum()   # integers that sum to 1024
        u = {int(i): float(x) / 1024.0 for i, x in enumerate(k)}
        assert kfdb_ref.l1_score(u, u) == 1.0


def _tree_sum(t):
    t = list(t)
    if not t:
        return 0.0
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


def test_order_sensitive_scene_tells_a_tree_sum_from_the_sequential_sum():
    scene = synth_kfdb.order_sensitive()
    bows = {}
    n_diff = n_scored = 0
    for op in scene["ops"]:
        if op[0] == "add":
            bows.update({int(s): kfdb_ref.to_dict(b) for s, b in zip(op[1], op[3])})
    ref = kfdb_ref.run_scene(scene)
    queries = [q for op in scene["ops"] if op[0] == "nbest" for q in op[1]]
    for q, r in zip(queries, [r for call in ref for r in call]):
        for s, d in zip(r["debug"]["scored_slot"], r["debug"]["score"]):
            tree = -_tree_sum(kfdb_ref.l1_terms(kfdb_ref.to_dict(q["bow"]), bows[int(s)])) / 2.0
            n_scored += 1
            n_diff += np.float64(tree).tobytes() != np.float64(d).tobytes()
    assert n_diff >= 10, (n_diff, n_scored)


@pytest.mark.parametrize("name", sorted(synth_kfdb.designed()))
def test_designed_scene_depends_on_its_behaviour(name):
    scene = synth_kfdb.designed()[name]
    quirk = synth_kfdb.quirk_of(name)
    assert quirk in kfdb_ref.QUIRKS
    with_it = kfdb_ref.outputs(kfdb_ref.run_scene(scene))
    without = kfdb_ref.outputs(kfdb_ref.run_scene(scene, quirk))
    assert with_it != without, (name, with_it)


def test_designed_scene_expectations():
    """The outputs the scenes were designed for (slots)."""
    out = {n: kfdb_ref.outputs(kfdb_ref.run_scene(s)) for n, s in synth_kfdb.designed().items()}
    assert out["stale_score"][1] == [dict(loop=[1], merge=[])]
    assert out["connected"] == [[dict(loop=[1], merge=[])]]
    assert out["id_check"] == [[dict(loop=[], merge=[])]]
    assert out["id_check_repeat"] == [[dict(loop=[2], merge=[])], [dict(loop=[], merge=[])]]
    assert out["strict_min"] == [[dict(loop=[0], merge=[])]]
    assert out["stable_sort"] == [[dict(loop=[3], merge=[])]]
    assert out["skip_bad"] == [[dict(loop=[1], merge=[])]]
    assert out["loop_overflow"] == [[dict(loop=[0], merge=[])]]
    assert out["reloc_filter_late"] == [[dict(cand=[])]]


def test_header_adds_no_struct():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_abi_check
    with open(gen_abi_check.OUT) as f:
        assert f.read() == gen_abi_check.generate()
    hdr = open(os.path.join(ROOT, "include", "omv.h")).read()
    assert "typedef struct omv_kfdb omv_kfdb;" in hdr and "omv_kfdb_detect_n_best" in hdr


def test_adapter_and_kfdb_consumer_compile():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("g++") is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("g++ or HIP headers absent")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I",
                        os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"), "-fsyntax-only",
                        os.path.join(ROOT, "tests", "cpp", "kfdb_consumer.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
