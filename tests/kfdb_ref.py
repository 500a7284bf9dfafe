"""A literal Python restatement of KeyFrameDatabase (src/KeyFrameDatabase.cc): add / erase / clear / clearMap,
DetectNBestCandidates (:581-713) and DetectRelocalizationCandidates (:715-828), with L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  Test infrastructure: real per-word lists (the inverted file), KF
objects that carry the reference's fields, dict BowVectors walked in ascending word order (std::map), list.sort for the
stable std::list::sort, numpy.float32 where the reference is float and Python floats where it is double.  It does not
use the (first shared word, add sequence) formulation of the device code, so the two are independent.

`quirk` arguments switch one of the reference's behaviours off (None: the reference).  They exist so a test can show
that a designed scene's output depends on the behaviour; see QUIRKS."""
import numpy as np

f32 = np.float32

# The behaviours the designed scenes probe, and what replaces each when it is switched off.
QUIRKS = {
    "stale_score": "the neighbour loop adds only scores written by this query (a neighbour at or under "
                   "minCommonWords adds 0 and cannot be the best)",
    "connected": "connected keyframes are listed like any other",
    "id_check": "every sharing keyframe is listed whatever its stored query id (id 0 and a repeated id list again)",
    "strict_min": "words >= minCommonWords is scored (the reference: >)",
    "stable_sort": "ties in accScore are put in reverse list order",
    "skip_bad": "bad keyframes are not skipped",
    "loop_overflow": "a same-map keyframe that finds the loop list full goes to the merge list (the reference drops it: "
                     "the merge branch tests the maps, and the keyframe is marked as added either way)",
    "reloc_filter_late": "the map filter is applied before bestAccScore is taken (the reference filters after the "
                         "threshold, so a keyframe of another map raises it)",
}


class KF:
    """The fields of KeyFrame these functions touch."""

    def __init__(self, mnId, bow, map_id):
        self.mnId = mnId
        self.mBowVec = dict(bow)   # word -> value
        self.map = map_id
        self.bad = False
        self.map_bad = False
        self.neighbours = []       # GetBestCovisibilityKeyFrames(10)
        self.mnPlaceRecognitionQuery = 0
        self.mnPlaceRecognitionWords = 0
        self.mPlaceRecognitionScore = f32(0)
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = f32(0)   # uninitialised in the reference; 0 here and on the device


def l1_terms(v1, v2):
    """The terms L1Scoring::score adds, in its order (the shared words ascending)."""
    out = []
    for w in sorted(v1):
        if w in v2:
            vi, wi = v1[w], v2[w]
            out.append(abs(vi - wi) - abs(vi) - abs(wi))
    return out


def l1_score(v1, v2):
    score = 0.0
    for t in l1_terms(v1, v2):
        score += t
    return -score / 2.0


class KeyFrameDatabase:
    def __init__(self, n_words):
        self.mvInvertedFile = [[] for _ in range(n_words)]
        self.debug = None

    def add(self, pKF):
        for w in sorted(pKF.mBowVec):
            self.mvInvertedFile[w].append(pKF)

    def erase(self, pKF):
        for w in sorted(pKF.mBowVec):
            lKFs = self.mvInvertedFile[w]
            for i, k in enumerate(lKFs):
                if k is pKF:
                    del lKFs[i]
                    break

    def clear(self):
        self.mvInvertedFile = [[] for _ in self.mvInvertedFile]

    def clearMap(self, map_id):
        for lKFs in self.mvInvertedFile:
            lKFs[:] = [k for k in lKFs if k.map != map_id]

    def _accumulate(self, qid, lScoreAndMatch, query_attr, score_attr, quirk, fresh):
        lAcc = []
        bestAccScore = f32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.neighbours[:10]:
                if pKF2 is None or getattr(pKF2, query_attr) != qid:
                    continue
                if quirk == "stale_score" and id(pKF2) not in fresh:
                    continue
                sc = getattr(pKF2, score_attr)
                accScore = f32(accScore + sc)
                if sc > bestScore:
                    pBestKF = pKF2
                    bestScore = sc
            lAcc.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return lAcc, bestAccScore

    def DetectNBestCandidates(self, pKF, nNumCandidates, quirk=None):
        """Returns (vpLoopCand, vpMergeCand); self.debug holds the intermediate lists."""
        self.debug = dict(maxCommonWords=0, minCommonWords=0, list=[], scored=[], acc=[])
        lKFsSharingWords = []
        spConnectedKF = pKF.connected
        for w in sorted(pKF.mBowVec):
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnPlaceRecognitionQuery != pKF.mnId or (quirk == "id_check" and
                                                                all(pKFi is not k for k in lKFsSharingWords)):
                    pKFi.mnPlaceRecognitionWords = 0
                    if pKFi not in spConnectedKF or quirk == "connected":
                        pKFi.mnPlaceRecognitionQuery = pKF.mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnPlaceRecognitionWords += 1
        if not lKFsSharingWords:
            return [], []
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnPlaceRecognitionWords > maxCommonWords:
                maxCommonWords = k.mnPlaceRecognitionWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.2))
        self.debug.update(maxCommonWords=maxCommonWords, minCommonWords=minCommonWords,
                          list=[(k, k.mnPlaceRecognitionWords) for k in lKFsSharingWords])
        lScoreAndMatch = []
        fresh = set()
        for pKFi in lKFsSharingWords:
            if pKFi.mnPlaceRecognitionWords > minCommonWords or (quirk == "strict_min" and
                                                                 pKFi.mnPlaceRecognitionWords >= minCommonWords):
                d = l1_score(pKF.mBowVec, pKFi.mBowVec)
                si = f32(d)
                pKFi.mPlaceRecognitionScore = si
                fresh.add(id(pKFi))
                lScoreAndMatch.append((si, pKFi))
                self.debug["scored"].append((pKFi, d, si))
        if not lScoreAndMatch:
            return [], []
        lAcc, _ = self._accumulate(pKF.mnId, lScoreAndMatch, "mnPlaceRecognitionQuery", "mPlaceRecognitionScore",
                                   quirk, fresh)
        if quirk == "stable_sort":
            lAcc.reverse()
        lAcc.sort(key=lambda p: -float(p[0]))   # list::sort(compFirst): stable, descending (-0 and +0 equal)
        self.debug["acc"] = list(lAcc)
        vpLoopCand, vpMergeCand = [], []
        spAlreadyAddedKF = []
        i = 0
        while i < len(lAcc) and (len(vpLoopCand) < nNumCandidates or len(vpMergeCand) < nNumCandidates):
            pKFi = lAcc[i][1]
            i += 1
            if pKFi.bad and quirk != "skip_bad":
                continue
            if all(pKFi is not k for k in spAlreadyAddedKF):
                if pKF.map == pKFi.map and len(vpLoopCand) < nNumCandidates:
                    vpLoopCand.append(pKFi)
                elif (pKF.map != pKFi.map or quirk == "loop_overflow") and len(vpMergeCand) < nNumCandidates and \
                        not pKFi.map_bad:
                    vpMergeCand.append(pKFi)
                spAlreadyAddedKF.append(pKFi)
        return vpLoopCand, vpMergeCand

    def DetectRelocalizationCandidates(self, F, map_id, quirk=None):
        """F: anything with mnId and mBowVec.  Returns vpRelocCandidates."""
        self.debug = dict(maxCommonWords=0, minCommonWords=0, list=[], scored=[], acc=[])
        lKFsSharingWords = []
        for w in sorted(F.mBowVec):
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery != F.mnId or (quirk == "id_check" and
                                                   all(pKFi is not k for k in lKFsSharingWords)):
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        self.debug.update(maxCommonWords=maxCommonWords, minCommonWords=minCommonWords,
                          list=[(k, k.mnRelocWords) for k in lKFsSharingWords])
        lScoreAndMatch = []
        fresh = set()
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords or (quirk == "strict_min" and pKFi.mnRelocWords >= minCommonWords):
                d = l1_score(F.mBowVec, pKFi.mBowVec)
                si = f32(d)
                pKFi.mRelocScore = si
                fresh.add(id(pKFi))
                lScoreAndMatch.append((si, pKFi))
                self.debug["scored"].append((pKFi, d, si))
        if not lScoreAndMatch:
            return []
        lAcc, bestAccScore = self._accumulate(F.mnId, lScoreAndMatch, "mnRelocQuery", "mRelocScore", quirk, fresh)
        if quirk == "reloc_filter_late":
            lAcc = [p for p in lAcc if p[1].map == map_id]
            bestAccScore = f32(0)
            for acc, _ in lAcc:
                if acc > bestAccScore:
                    bestAccScore = acc
        self.debug["acc"] = list(lAcc)
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        spAlreadyAddedKF = []
        vpRelocCandidates = []
        for si, pKFi in lAcc:
            if si > minScoreToRetain:
                if pKFi.map != map_id:
                    continue
                if all(pKFi is not k for k in spAlreadyAddedKF):
                    vpRelocCandidates.append(pKFi)
                    spAlreadyAddedKF.append(pKFi)
        return vpRelocCandidates


class Query:
    """pKF / F of a query: mnId, mBowVec, map and the connected keyframes."""

    def __init__(self, mnId, bow, map_id, connected=()):
        self.mnId, self.mBowVec, self.map, self.connected = mnId, dict(bow), map_id, set(connected)


class SlotMirror:
    """The device handle's interface (slots, arrays) on top of the restatement above: what a caller that keeps a
    KeyFrame* <-> slot map does.  A slot's KF object survives erase (it stays a neighbour with its stored score); add
    puts a fresh KF into the slot, as the handle resets the slot's state."""

    def __init__(self, n_words, max_kf):
        self.db = KeyFrameDatabase(n_words)
        self.kf = [None] * max_kf
        self.inside = [False] * max_kf
        self.neigh = [[-1] * 10 for _ in range(max_kf)]

    def add(self, slot, map_id, bow):
        assert not self.inside[slot]
        self.kf[slot] = KF(-1, bow, map_id)
        self.kf[slot].slot = slot
        self.neigh[slot] = [-1] * 10
        self.inside[slot] = True
        self.db.add(self.kf[slot])

    def erase(self, slot):
        if self.inside[slot]:
            self.db.erase(self.kf[slot])
            self.inside[slot] = False

    def clear(self):
        self.db.clear()
        self.inside = [False] * len(self.inside)

    def clearMap(self, map_id):
        self.db.clearMap(map_id)
        for s, k in enumerate(self.kf):
            if k is not None and k.map == map_id:
                self.inside[s] = False

    def set_neighbours(self, slot, neigh):
        self.neigh[slot] = (list(neigh) + [-1] * 10)[:10]

    def set_flags(self, slot, flags):
        self.kf[slot].bad, self.kf[slot].map_bad = bool(flags & 1), bool(flags & 2)

    def _resolve(self):
        for s, k in enumerate(self.kf):
            if k is not None:
                k.neighbours = [self.kf[n] if n >= 0 else None for n in self.neigh[s]]

    def slots(self, kfs):
        return [k.slot for k in kfs]

    def DetectNBestCandidates(self, qid, qmap, bow, connected_slots, n, quirk=None):
        self._resolve()
        q = Query(qid, bow, qmap, [self.kf[s] for s in connected_slots if self.kf[s] is not None])
        lo, me = self.db.DetectNBestCandidates(q, n, quirk)
        return self.slots(lo), self.slots(me)

    def DetectRelocalizationCandidates(self, fid, map_id, bow, quirk=None):
        self._resolve()
        return self.slots(self.db.DetectRelocalizationCandidates(Query(fid, bow, map_id), map_id, quirk))

    def debug(self):
        """The intermediate lists of the last query in the shape of omv_kfdb_debug."""
        d = self.db.debug
        return dict(max_common_words=d["maxCommonWords"], min_common_words=d["minCommonWords"],
                    list_slot=np.array([k.slot for k, _ in d["list"]], np.int32),
                    list_words=np.array([w for _, w in d["list"]], np.int32),
                    scored_slot=np.array([k.slot for k, _, _ in d["scored"]], np.int32),
                    score=np.array([s for _, s, _ in d["scored"]], np.float64),
                    si=np.array([s for _, _, s in d["scored"]], np.float32),
                    acc_bits=np.array([a for a, _ in d["acc"]], np.float32).view(np.uint32),
                    acc_best=np.array([k.slot for _, k in d["acc"]], np.int32))


def to_dict(bow):
    w, v = bow
    return {int(a): float(b) for a, b in zip(w, v)}


def run_scene(scene, quirk=None):
    """Applies a scene of openmavis_amd.synth_kfdb to a SlotMirror.  Returns one entry per Detect op: a list with one
    dict per query: loop / merge (n_best) or cand (reloc) as slot lists, and `debug` (SlotMirror.debug())."""
    m = SlotMirror(scene["n_words"], scene["max_kf"])
    out = []
    for op in scene["ops"]:
        kind = op[0]
        if kind == "add":
            for s, mp, b in zip(op[1], op[2], op[3]):
                m.add(int(s), int(mp), to_dict(b))
        elif kind == "erase":
            for s in op[1]:
                m.erase(int(s))
        elif kind == "clear":
            m.clear()
        elif kind == "clearMap":
            m.clearMap(op[1])
        elif kind == "neigh":
            for s, row in zip(op[1], op[2]):
                m.set_neighbours(int(s), [int(x) for x in row])
        elif kind == "flags":
            for s, f in zip(op[1], op[2]):
                m.set_flags(int(s), int(f))
        elif kind == "nbest":
            res = []
            for q in op[1]:
                lo, me = m.DetectNBestCandidates(q["id"], q["map"], to_dict(q["bow"]),
                                                 [int(s) for s in q["connected"]], op[2], quirk)
                res.append(dict(loop=lo, merge=me, debug=m.debug()))
            out.append(res)
        elif kind == "reloc":
            res = []
            for q in op[1]:
                c = m.DetectRelocalizationCandidates(q["id"], q["map"], to_dict(q["bow"]), quirk)
                res.append(dict(cand=c, debug=m.debug()))
            out.append(res)
        else:
            raise ValueError(kind)
    return out


def outputs(results):
    """The candidate lists alone."""
    return [[{k: v for k, v in r.items() if k != "debug"} for r in call] for call in results]
