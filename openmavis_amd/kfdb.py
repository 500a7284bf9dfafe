"""KeyFrameDatabase (src/KeyFrameDatabase.cc) on the device, batched: add / erase / clear / clearMap,
DetectNBestCandidates (:581-713, the loop / merge candidates of LoopClosing::NewDetectCommonRegions, src/LoopClosing.cc:562)
and DetectRelocalizationCandidates (:715-828, src/Tracking.cc:3551) on one omv_kfdb handle (openmavis_amd/csrc/kfdb.hip).
Bit-exact; there is no CPU fallback.

A keyframe lives in a slot in [0, max_kf) that the caller chooses (its KeyFrame* <-> slot map).  BowVectors are taken
as ORBVocabulary.transform leaves them on the device, rows of (bow_word, bow_value) with bow_n entries each:

    out = voc.transform(desc, n_desc)
    db = KeyFrameDatabase(voc, max_kf=4096, max_bow=desc.shape[1])
    db.add(slots, map_ids, out["bow_word"], out["bow_value"], out["bow_n"])
    db.set_neighbours(slots, neigh)      # GetBestCovisibilityKeyFrames(10) as slots, -1 padded
    db.set_flags(slots, flags)           # bit 0 isBad(), bit 1 GetMap()->IsBad()
    loop, n_loop, merge, n_merge = db.DetectNBestCandidates(ids, maps, connected, q["bow_word"], q["bow_value"],
                                                            q["bow_n"], 3)

What the graph owns arrives as arrays: the connected keyframes of each query, the ten best covisibility neighbours, the
bad flags and the map ids.  The reference's persistent per-keyframe state (mnPlaceRecognitionQuery /
mPlaceRecognitionScore, mnRelocQuery / mRelocScore) is kept per slot by the handle, with every consequence: a query id
of 0 lists no fresh keyframe, a repeated id lists nothing again, and a neighbour contributes its stored score, which is
stale when this query did not score it.  add() makes the slot a fresh KeyFrame: state (0, 0), no neighbours, flags 0.
The queries of one call behave as the same queries made one per call in that order.  Only L1 scoring."""
import ctypes

import numpy as np

from . import _lib


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))


class KeyFrameDatabase:
    def __init__(self, voc, max_kf, max_bow, max_queries=16, max_query_bow=None, device="cuda:0", stream=None):
        """voc: an ORBVocabulary (its scoring is used) or the scoring id itself (bow.SCORING)."""
        import torch
        self._torch, self._lib, self.device, self.stream = torch, _lib.load(), device, stream
        scoring = voc if isinstance(voc, int) else voc.host["scoring"]
        self.max_kf, self.max_bow, self.max_queries = int(max_kf), int(max_bow), int(max_queries)
        self.max_query_bow = int(max_query_bow if max_query_bow is not None else max_bow)
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.omv_kfdb_create(int(scoring), self.max_kf, self.max_bow, self.max_queries,
                                             self.max_query_bow, ctypes.byref(self._h)), "omv_kfdb_create")

    def __del__(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.omv_kfdb_destroy(self._h)
            self._h = ctypes.c_void_p()

    def _stream(self):
        s = self.stream if self.stream is not None else self._torch.cuda.current_stream()
        return ctypes.c_void_p(s.cuda_stream)

    def _bow(self, word, value, n, rows):
        torch = self._torch
        assert word.dtype == torch.int32 and value.dtype == torch.float64 and n.dtype == torch.int32, \
            "BowVectors as ORBVocabulary.transform leaves them: int32 words, float64 values, int32 counts"
        assert word.is_cuda and value.is_cuda and n.is_cuda, "BowVectors stay on the device"
        assert word.dim() == 2 and word.shape == value.shape and word.stride() == value.stride() and \
            word.stride(1) == 1 and n.is_contiguous(), "bow_word / bow_value: [n][stride] rows, bow_n: [n]"
        assert word.shape[0] >= rows and n.numel() >= rows, "fewer BowVectors than keyframes / queries"
        return int(word.stride(0)) if word.shape[0] > 1 else int(word.shape[1])

    # ---- the database ----
    def add(self, slots, map_ids, bow_word, bow_value, bow_n):
        """KeyFrameDatabase::add for len(slots) keyframes; row i of the BowVector tensors goes to slots[i]."""
        slots, map_ids = _i32(slots), _i32(map_ids)
        assert len(slots) == len(map_ids)
        stride = self._bow(bow_word, bow_value, bow_n, len(slots)) if len(slots) else 1
        _lib.check(self._lib.omv_kfdb_add(self._h, len(slots), _lib.ptr(slots), _lib.ptr(map_ids), _lib.ptr(bow_word),
                                          _lib.ptr(bow_value), _lib.ptr(bow_n), stride, self._stream()), "omv_kfdb_add")

    def erase(self, slots):
        slots = _i32(slots)
        _lib.check(self._lib.omv_kfdb_erase(self._h, len(slots), _lib.ptr(slots), self._stream()), "omv_kfdb_erase")

    def clear(self):
        _lib.check(self._lib.omv_kfdb_clear(self._h, self._stream()), "omv_kfdb_clear")

    def clearMap(self, map_id):
        _lib.check(self._lib.omv_kfdb_clear_map(self._h, int(map_id), self._stream()), "omv_kfdb_clear_map")

    def set_neighbours(self, slots, neigh):
        """neigh [n][<= 10]: GetBestCovisibilityKeyFrames(10) of each slot as slots, in its order (-1: not in the
        database's slot map)."""
        slots = _i32(slots)
        nb = np.full((len(slots), 10), -1, np.int32)
        for i, row in enumerate(neigh):
            row = np.asarray(row, np.int32).reshape(-1)[:10]
            nb[i, :len(row)] = row
        _lib.check(self._lib.omv_kfdb_set_neighbours(self._h, len(slots), _lib.ptr(slots), _lib.ptr(nb),
                                                     self._stream()), "omv_kfdb_set_neighbours")

    def set_flags(self, slots, flags):
        slots = _i32(slots)
        fl = np.ascontiguousarray(np.asarray(flags, np.uint8).reshape(-1))
        assert len(fl) == len(slots)
        _lib.check(self._lib.omv_kfdb_set_flags(self._h, len(slots), _lib.ptr(slots), _lib.ptr(fl), self._stream()),
                   "omv_kfdb_set_flags")

    # ---- the queries ----
    def DetectNBestCandidates(self, query_ids, query_maps, connected, bow_word, bow_value, bow_n, nNumCandidates):
        """One query per row of the BowVector tensors.  query_ids: pKF->mnId; query_maps: the map ids; connected: per
        query the slots of pKF->GetConnectedKeyFrames().  Returns device tensors (vpLoopCand [Q][nNumCandidates] slots,
        -1 beyond the count; n_loop [Q]; vpMergeCand; n_merge); nothing is synchronised."""
        torch = self._torch
        ids = np.ascontiguousarray(np.asarray(query_ids, np.int64).reshape(-1))
        maps = _i32(query_maps)
        Q = len(ids)
        assert len(maps) == Q and len(connected) == Q
        cstart = np.concatenate([[0], np.cumsum([len(c) for c in connected])]).astype(np.int32)
        cslot = _i32(np.concatenate([np.asarray(c, np.int32).reshape(-1) for c in connected])) if Q else _i32([])
        n = int(nNumCandidates)
        z = lambda *s: torch.empty(s, dtype=torch.int32, device=self.device)   # noqa: E731
        loop, n_loop, merge, n_merge = z(max(Q, 1), max(n, 1)), z(max(Q, 1)), z(max(Q, 1), max(n, 1)), z(max(Q, 1))
        stride = self._bow(bow_word, bow_value, bow_n, Q) if Q else 1
        _lib.check(self._lib.omv_kfdb_detect_n_best(
            self._h, Q, _lib.ptr(ids), _lib.ptr(maps), _lib.ptr(cstart), _lib.ptr(cslot), _lib.ptr(bow_word),
            _lib.ptr(bow_value), _lib.ptr(bow_n), stride, n, _lib.ptr(loop), _lib.ptr(n_loop), _lib.ptr(merge),
            _lib.ptr(n_merge), self._stream()), "omv_kfdb_detect_n_best")
        return loop.view(-1)[:Q * n].view(Q, n), n_loop[:Q], merge.view(-1)[:Q * n].view(Q, n), n_merge[:Q]

    def DetectRelocalizationCandidates(self, frame_ids, map_ids, bow_word, bow_value, bow_n):
        """frame_ids: F->mnId; map_ids: pMap.  Returns device tensors (vpRelocCandidates [Q][max_kf] slots in the
        reference's order, -1 beyond the count; n_cand [Q]); nothing is synchronised."""
        torch = self._torch
        ids = np.ascontiguousarray(np.asarray(frame_ids, np.int64).reshape(-1))
        maps = _i32(map_ids)
        Q = len(ids)
        assert len(maps) == Q
        cand = torch.empty((max(Q, 1), self.max_kf), dtype=torch.int32, device=self.device)
        n_cand = torch.empty(max(Q, 1), dtype=torch.int32, device=self.device)
        stride = self._bow(bow_word, bow_value, bow_n, Q) if Q else 1
        _lib.check(self._lib.omv_kfdb_detect_reloc(self._h, Q, _lib.ptr(ids), _lib.ptr(maps), _lib.ptr(bow_word),
                                                   _lib.ptr(bow_value), _lib.ptr(bow_n), stride, _lib.ptr(cand),
                                                   _lib.ptr(n_cand), self._stream()), "omv_kfdb_detect_reloc")
        return cand[:Q], n_cand[:Q]

    def debug(self, query=0):
        """The intermediate lists of query `query` of the last Detect call (the library's test hook), host arrays:
        max_common_words, min_common_words, list_slot / list_words (lKFsSharingWords), scored_slot / score (double) /
        si (lScoreAndMatch), acc_bits / acc_best (lAccScoreAndMatch in its final order)."""
        K = self.max_kf
        mx, mn, nl, ns = (ctypes.c_int32() for _ in range(4))
        o = dict(list_slot=np.zeros(K, np.int32), list_words=np.zeros(K, np.int32), scored_slot=np.zeros(K, np.int32),
                 score=np.zeros(K, np.float64), si=np.zeros(K, np.float32), acc_bits=np.zeros(K, np.uint32),
                 acc_best=np.zeros(K, np.int32))
        _lib.check(self._lib.omv_kfdb_debug(self._h, int(query), ctypes.byref(mx), ctypes.byref(mn), ctypes.byref(nl),
                                            _lib.ptr(o["list_slot"]), _lib.ptr(o["list_words"]), ctypes.byref(ns),
                                            _lib.ptr(o["scored_slot"]), _lib.ptr(o["score"]), _lib.ptr(o["si"]),
                                            _lib.ptr(o["acc_bits"]), _lib.ptr(o["acc_best"]), self._stream()),
                   "omv_kfdb_debug")
        out = {k: v[:nl.value if k.startswith("list") else ns.value] for k, v in o.items()}
        out.update(max_common_words=mx.value, min_common_words=mn.value)
        return out
