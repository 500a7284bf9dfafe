"""The device KeyFrameDatabase (openmavis_amd/kfdb.py, csrc/kfdb.hip) against the literal Python restatement
tests/kfdb_ref.py: everything is compared as exact integers / raw bits, there is no tolerance.  A scene
(openmavis_amd/synth_kfdb.py) is a script of database operations applied to both."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kfdb_ref
from openmavis_amd import _lib, synth_bow, synth_kfdb
from openmavis_amd import build as omv_build

pytestmark = pytest.mark.gpu


def _bow_tensors(torch, bows, stride):
    bw, bv, bn = synth_kfdb.pack_bows(bows, stride)
    return [torch.from_numpy(a).cuda() for a in (bw, bv, bn)]


def run_device(torch, scene, split=False, max_queries=None, extra_stride=0):
    """Applies the scene to a fresh KeyFrameDatabase; returns results shaped like kfdb_ref.run_scene's.  split: every
    query in a call of its own."""
    from openmavis_amd.kfdb import KeyFrameDatabase
    adds = [b for op in scene["ops"] if op[0] == "add" for b in op[3]]
    qs = [q for op in scene["ops"] if op[0] in ("nbest", "reloc") for q in op[1]]
    max_bow = max([len(w) for w, _ in adds] + [1])
    max_qbow = max([len(q["bow"][0]) for q in qs] + [1])
    n_q_max = max([len(op[1]) for op in scene["ops"] if op[0] in ("nbest", "reloc")] + [1])
    db = KeyFrameDatabase(0, scene["max_kf"], max_bow, max_queries or n_q_max, max_qbow)
    out = []
    for op in scene["ops"]:
        kind = op[0]
        if kind == "add":
            db.add(op[1], op[2], *_bow_tensors(torch, op[3], max_bow + extra_stride))
        elif kind == "erase":
            db.erase(op[1])
        elif kind == "clear":
            db.clear()
        elif kind == "clearMap":
            db.clearMap(op[1])
        elif kind == "neigh":
            db.set_neighbours(op[1], op[2])
        elif kind == "flags":
            db.set_flags(op[1], op[2])
        else:
            res = []
            groups = [[q] for q in op[1]] if split else [list(op[1])]
            for g in groups:
                t = _bow_tensors(torch, [q["bow"] for q in g], max_qbow + extra_stride)
                ids, maps = [q["id"] for q in g], [q["map"] for q in g]
                if kind == "nbest":
                    lo, nl, me, nm = db.DetectNBestCandidates(ids, maps, [q["connected"] for q in g], *t, op[2])
                    lo, nl, me, nm = (x.cpu().numpy() for x in (lo, nl, me, nm))
                    for j in range(len(g)):
                        assert 0 <= nl[j] <= op[2] and 0 <= nm[j] <= op[2]
                        assert (lo[j, nl[j]:] == -1).all() and (me[j, nm[j]:] == -1).all()
                        res.append(dict(loop=lo[j, :nl[j]].tolist(), merge=me[j, :nm[j]].tolist(), debug=db.debug(j)))
                else:
                    ca, nc = (x.cpu().numpy() for x in db.DetectRelocalizationCandidates(ids, maps, *t))
                    for j in range(len(g)):
                        assert (ca[j, nc[j]:] == -1).all()
                        res.append(dict(cand=ca[j, :nc[j]].tolist(), debug=db.debug(j)))
            out.append(res)
    return out


def assert_same(ref, dev):
    assert len(ref) == len(dev)
    for c, (call_r, call_d) in enumerate(zip(ref, dev)):
        assert len(call_r) == len(call_d)
        for j, (r, d) in enumerate(zip(call_r, call_d)):
            at = f"call {c} query {j}"
            rd, dd = r["debug"], d["debug"]
            assert (dd["max_common_words"], dd["min_common_words"]) == (rd["max_common_words"],
                                                                         rd["min_common_words"]), at
            for k in ("list_slot", "list_words", "scored_slot", "acc_best"):
                assert np.array_equal(rd[k], dd[k]), (at, k, rd[k], dd[k])
            assert np.array_equal(rd["score"].view(np.uint64), dd["score"].view(np.uint64)), (at, "score bits")
            assert np.array_equal(rd["si"].view(np.uint32), dd["si"].view(np.uint32)), (at, "si bits")
            assert np.array_equal(rd["acc_bits"], dd["acc_bits"]), (at, "accScore bits")
            for k in ("loop", "merge", "cand"):
                assert r.get(k) == d.get(k), (at, k, r.get(k), d.get(k))


LENGTHS = [64, 0, 1, 63, 65, 257]
Q_LENGTHS = [257, 0, 65, 64, 1, 63]
SHAPES = [(n_kf, n_words, (1, 3)[i % 2], (3, 1)[(i // 2) % 2])
          for i, (n_kf, n_words) in enumerate([(k, w) for k in (1, 63, 64, 65, 300) for w in (50, 5000)])]


@pytest.mark.parametrize("n_kf,n_words,n_q,n_cand", SHAPES)
def test_n_best_exact(torch_cuda, n_kf, n_words, n_q, n_cand):
    scene = synth_kfdb.random_scene(n_kf, n_words, LENGTHS, seed=100 + n_kf + n_words, n_q=n_q, n_candidates=n_cand,
                                    q_lengths=Q_LENGTHS, rounds=3 if n_q == 1 else 2)
    ref = kfdb_ref.run_scene(scene)
    assert_same(ref, run_device(torch_cuda, scene))
    if n_kf >= 63:
        assert sum(len(r["debug"]["scored_slot"]) for call in ref for r in call) > 0


@pytest.mark.parametrize("n_kf,n_words,n_q", [(1, 50, 1), (64, 50, 3), (65, 5000, 3), (300, 5000, 1), (300, 50, 3)])
def test_relocalization_exact(torch_cuda, n_kf, n_words, n_q):
    scene = synth_kfdb.random_scene(n_kf, n_words, LENGTHS, seed=200 + n_kf + n_words, n_q=n_q, q_lengths=Q_LENGTHS,
                                    rounds=3 if n_q == 1 else 2, mode="reloc")
    assert_same(kfdb_ref.run_scene(scene), run_device(torch_cuda, scene))


def test_both_modes_keep_separate_state(torch_cuda):
    """The same ids through DetectNBestCandidates and DetectRelocalizationCandidates on one database: two independent
    (query id, score) pairs per keyframe."""
    a = synth_kfdb.random_scene(65, 50, [10, 30], seed=31, n_q=2, rounds=2, churn=False)
    b = synth_kfdb.random_scene(65, 50, [10, 30], seed=31, n_q=2, rounds=2, churn=False, mode="reloc")
    det_a = [op for op in a["ops"] if op[0] == "nbest"]
    det_b = [op for op in b["ops"] if op[0] == "reloc"]
    scene = dict(a, ops=[op for op in a["ops"] if op[0] != "nbest"] + [det_a[0], det_b[0], det_a[1], det_b[1]])
    assert_same(kfdb_ref.run_scene(scene), run_device(torch_cuda, scene))


def test_order_sensitive_scores(torch_cuda):
    """The scene in which a tree sum gives other double bits for most pairs (tests/test_kfdb_ref_cpu.py)."""
    scene = synth_kfdb.order_sensitive()
    assert_same(kfdb_ref.run_scene(scene), run_device(torch_cuda, scene))


@pytest.mark.parametrize("name", sorted(synth_kfdb.designed()))
def test_designed_scene(torch_cuda, name):
    scene = synth_kfdb.designed()[name]
    assert_same(kfdb_ref.run_scene(scene), run_device(torch_cuda, scene))


def test_one_call_equals_one_call_per_query(torch_cuda):
    """Three queries in one call (ids that repeat, so a query depends on the one before it) equal three calls; a row
    stride longer than the vectors and a handle with room for more queries change nothing."""
    scene = synth_kfdb.random_scene(65, 50, [5, 20, 40], seed=41, n_q=3, rounds=3)
    ids = [q["id"] for op in scene["ops"] if op[0] == "nbest" for q in op[1]]
    assert len(set(ids)) < len(ids)
    ref = kfdb_ref.run_scene(scene)
    assert_same(ref, run_device(torch_cuda, scene))
    assert_same(ref, run_device(torch_cuda, scene, split=True, max_queries=5, extra_stride=7))


@pytest.mark.parametrize("max_kf", [5000, 8300])
def test_high_slots_take_the_other_sort_paths(torch_cuda, max_kf):
    """The select stage sorts in LDS up to 8192 slots (more than 48 KB of it above 4096) and in device memory beyond:
    65 keyframes scattered over a slot range that reaches each path."""
    scene = synth_kfdb.random_scene(65, 50, [5, 20, 40], seed=61, n_q=2, max_kf=max_kf, rounds=2)
    top = max(int(s) for op in scene["ops"] if op[0] == "add" for s in op[1])
    assert top >= (8192 if max_kf > 8192 else 4096)
    ref = kfdb_ref.run_scene(scene)
    assert sum(len(r["debug"]["scored_slot"]) for call in ref for r in call) > 50
    assert_same(ref, run_device(torch_cuda, scene))


def test_erase_readd_clear(torch_cuda):
    U = synth_kfdb.uniform_bow
    q = lambda i: dict(id=i, map=0, bow=U([1, 5]), connected=[])   # noqa: E731
    ops = [("add", [0, 1, 2], [0, 1, 0], [U([1, 2]), U([1, 3]), U([1, 4, 5])]),
           ("nbest", [q(1)], 3),
           ("erase", [0]), ("add", [0], [0], [U([1, 2])]),      # slot 0 goes to the back of word 1's list
           ("nbest", [q(2)], 3),
           ("clearMap", 1), ("nbest", [q(3)], 3),
           ("erase", [2]), ("erase", [2]), ("nbest", [q(4)], 3),   # erasing twice is a no-op
           ("clear",), ("nbest", [q(5)], 3),
           ("add", [1], [0], [U([5, 6])]), ("nbest", [q(6)], 3)]
    scene = dict(n_words=10, max_kf=4, ops=ops)
    ref = kfdb_ref.run_scene(scene)
    assert list(ref[1][0]["debug"]["list_slot"]) == [1, 2, 0] and ref[4][0]["loop"] == [] and ref[5][0]["loop"] == [1]
    assert_same(ref, run_device(torch_cuda, scene))


def test_run_to_run_bitwise(torch_cuda):
    scene = synth_kfdb.random_scene(300, 50, [20, 40, 50], seed=51, n_q=3, rounds=2)
    a, b = run_device(torch_cuda, scene), run_device(torch_cuda, scene)
    assert_same(a, b)


def test_end_to_end_from_transform(torch_cuda):
    """Descriptor sets -> device transform -> add straight from its output tensors -> DetectNBestCandidates: the planted
    revisit (a noisy copy of set 5's descriptors) is the first loop candidate, and the lists equal the reference's on
    the BowVectors the transform produced."""
    torch = torch_cuda
    from openmavis_amd import synth
    from openmavis_amd.bow import ORBVocabulary
    from openmavis_amd.kfdb import KeyFrameDatabase
    host = synth_bow.make_vocab(k=6, L=3, seed=3)
    voc = ORBVocabulary(host)
    n_sets, cap = 12, 300
    desc, n_desc = synth_bow.make_sets(host, n_sets=n_sets + 1, cap=cap, seed=4)
    rng = np.random.Generator(np.random.PCG64(9))
    desc[n_sets] = synth.flip_bits(desc[5], rng, 3)
    n_desc[n_sets] = n_desc[5]
    out = voc.transform(torch.from_numpy(desc).cuda(), torch.from_numpy(n_desc).cuda())
    db = KeyFrameDatabase(voc, max_kf=16, max_bow=cap)
    slots = np.arange(n_sets, dtype=np.int32) + 2
    db.add(slots, np.zeros(n_sets, np.int32), out["bow_word"], out["bow_value"], out["bow_n"])
    q = {k: out[k][n_sets:] for k in ("bow_word", "bow_value", "bow_n")}
    loop, n_loop, merge, n_merge = db.DetectNBestCandidates([77], [0], [[2, 3]], q["bow_word"], q["bow_value"],
                                                            q["bow_n"], 3)
    bn = out["bow_n"].cpu().numpy()
    bw, bv = out["bow_word"].cpu().numpy(), out["bow_value"].cpu().numpy()
    m = kfdb_ref.SlotMirror(host["n_words"], 16)
    for i in range(n_sets):
        m.add(int(slots[i]), 0, dict(zip(bw[i, :bn[i]].tolist(), bv[i, :bn[i]].tolist())))
    lo, me = m.DetectNBestCandidates(77, 0, dict(zip(bw[n_sets, :bn[n_sets]].tolist(), bv[n_sets, :bn[n_sets]].tolist())),
                                     [2, 3], 3)
    assert int(n_loop[0]) == 3 and int(n_merge[0]) == 0
    assert loop[0].tolist() == lo and lo[0] == 7 and me == []
    d, r = db.debug(0), m.debug()
    assert np.array_equal(d["score"].view(np.uint64), r["score"].view(np.uint64))
    assert np.array_equal(d["list_slot"], r["list_slot"])


def test_argument_errors(torch_cuda):
    torch = torch_cuda
    from openmavis_amd.kfdb import KeyFrameDatabase
    lib = _lib.load()
    h = ctypes.c_void_p()
    for scoring in (1, 2, 5, -1):   # L1 only
        assert lib.omv_kfdb_create(scoring, 8, 8, 1, 8, ctypes.byref(h)) == _lib.OMV_ERR_ARG
    for a in ((0, 0, 8, 1, 8), (0, 8, 0, 1, 8), (0, 8, 8, 0, 8), (0, 8, 8, 1, 0), (0, -1, 8, 1, 8)):
        assert lib.omv_kfdb_create(*a, ctypes.byref(h)) == _lib.OMV_ERR_ARG
    assert lib.omv_kfdb_create(0, 8, 8, 1, 8, None) == _lib.OMV_ERR_ARG
    db = KeyFrameDatabase(0, max_kf=8, max_bow=4, max_queries=2, max_query_bow=4)
    U = synth_kfdb.uniform_bow
    t = _bow_tensors(torch, [U([1, 2]), U([2, 3])], 6)
    P, st = _lib.ptr, db._stream()
    i32 = lambda *x: np.array(x, np.int32)   # noqa: E731
    add = lambda n, slot, maps, stride=6, tt=t: lib.omv_kfdb_add(   # noqa: E731
        db._h, n, P(slot), P(maps), P(tt[0]), P(tt[1]), P(tt[2]), stride, st)
    assert add(0, None, None) == _lib.OMV_OK
    assert add(-1, i32(0), i32(0)) == _lib.OMV_ERR_ARG
    assert add(1, None, i32(0)) == _lib.OMV_ERR_ARG
    assert add(1, i32(8), i32(0)) == _lib.OMV_ERR_ARG and add(1, i32(-1), i32(0)) == _lib.OMV_ERR_ARG
    assert add(2, i32(3, 3), i32(0, 0)) == _lib.OMV_ERR_ARG          # named twice
    assert add(2, i32(0, 1), i32(0, 0)) == _lib.OMV_OK
    assert add(1, i32(1), i32(0)) == _lib.OMV_ERR_ARG                # occupied
    long = _bow_tensors(torch, [U([1, 2, 3, 4, 5])], 6)
    assert add(1, i32(2), i32(0), tt=long) == _lib.OMV_ERR_CAPACITY  # bow_n > max_bow
    assert lib.omv_kfdb_erase(db._h, 1, P(i32(8)), st) == _lib.OMV_ERR_ARG
    assert lib.omv_kfdb_erase(db._h, 1, None, st) == _lib.OMV_ERR_ARG
    assert lib.omv_kfdb_erase(db._h, 0, None, st) == _lib.OMV_OK
    nb = np.full((1, 10), -1, np.int32)
    assert lib.omv_kfdb_set_neighbours(db._h, 1, P(i32(0)), P(nb), st) == _lib.OMV_OK
    nb[0, 3] = 8
    assert lib.omv_kfdb_set_neighbours(db._h, 1, P(i32(0)), P(nb), st) == _lib.OMV_ERR_ARG
    assert lib.omv_kfdb_set_neighbours(db._h, 1, P(i32(0)), None, st) == _lib.OMV_ERR_ARG
    assert lib.omv_kfdb_set_flags(db._h, 1, P(i32(9)), P(np.zeros(1, np.uint8)), st) == _lib.OMV_ERR_ARG
    assert lib.omv_kfdb_set_flags(db._h, 1, P(i32(0)), None, st) == _lib.OMV_ERR_ARG
    q = _bow_tensors(torch, [U([2]), U([3]), U([1])], 6)
    out = [torch.full((3, 2), -7, dtype=torch.int32, device="cuda"), torch.full((3,), -7, dtype=torch.int32, device="cuda"),
           torch.full((3, 2), -7, dtype=torch.int32, device="cuda"), torch.full((3,), -7, dtype=torch.int32, device="cuda")]
    ids, maps = np.array([1, 2, 3], np.int64), i32(0, 0, 0)

    def nbest(n_q, cstart, cslot, ids=ids, maps=maps, qq=q, n_cand=2, o=out):
        return lib.omv_kfdb_detect_n_best(db._h, n_q, P(ids), P(maps), P(cstart), P(cslot), P(qq[0]), P(qq[1]), P(qq[2]),
                                          6, n_cand, P(o[0]), P(o[1]), P(o[2]), P(o[3]), st)

    assert nbest(0, None, None) == _lib.OMV_OK
    assert nbest(-1, i32(0, 0), None) == _lib.OMV_ERR_ARG
    assert nbest(3, i32(0, 0, 0, 0), None) == _lib.OMV_ERR_ARG       # n_q > max_queries
    assert nbest(2, i32(0, 1, 0), i32(0)) == _lib.OMV_ERR_ARG        # descending conn_start
    assert nbest(2, i32(0, 1, 2), i32(0, 8)) == _lib.OMV_ERR_ARG     # connected slot out of range
    assert nbest(2, i32(0, 1, 2), None) == _lib.OMV_ERR_ARG
    assert nbest(2, None, None) == _lib.OMV_ERR_ARG
    assert nbest(2, i32(0, 0, 0), None, ids=None) == _lib.OMV_ERR_ARG
    assert nbest(2, i32(0, 0, 0), None, n_cand=-1) == _lib.OMV_ERR_ARG
    assert nbest(2, i32(0, 0, 0), None, o=[None] + out[1:]) == _lib.OMV_ERR_ARG
    torch.cuda.synchronize()
    assert all((x == -7).all() for x in out), "an argument error wrote to the outputs"
    assert nbest(2, i32(0, 0, 0), None) == _lib.OMV_OK
    torch.cuda.synchronize()
    assert out[1][:2].tolist() == [2, 1] and out[0][0].tolist() == [0, 1] and out[0][1].tolist() == [1, -1]
    assert lib.omv_kfdb_detect_reloc(db._h, 3, P(ids), P(maps), P(q[0]), P(q[1]), P(q[2]), 6, P(out[0]), P(out[1]),
                                     st) == _lib.OMV_ERR_ARG
    assert lib.omv_kfdb_detect_reloc(db._h, 1, P(ids), None, P(q[0]), P(q[1]), P(q[2]), 6, P(out[0]), P(out[1]),
                                     st) == _lib.OMV_ERR_ARG
    assert lib.omv_kfdb_debug(db._h, 2, *([None] * 11), st) == _lib.OMV_ERR_ARG
    assert lib.omv_kfdb_debug(db._h, 1, *([None] * 11), st) == _lib.OMV_OK
    # a query longer than max_query_bow is flagged by the counts, not truncated
    assert nbest(1, i32(0, 0), None, qq=_bow_tensors(torch, [U([1, 2, 3, 4, 5])], 6)) == _lib.OMV_OK
    torch.cuda.synchronize()
    assert int(out[1][0]) == -1 and int(out[3][0]) == -1


def test_cpp_adapter_consumer(torch_cuda):
    """tests/cpp/kfdb_consumer.cpp (omv_adapt::KeyFrameDatabase, the call shapes of LoopClosing.cc:562 and
    Tracking.cc:3551) as a child process."""
    if not os.path.exists(omv_build.KFDB_CONSUMER_BIN):
        pytest.fail(f"{omv_build.KFDB_CONSUMER_BIN} not built (python -m openmavis_amd.build)")
    r = subprocess.run([omv_build.KFDB_CONSUMER_BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
