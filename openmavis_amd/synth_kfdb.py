"""Seeded synthetic scenes for the KeyFrameDatabase: BowVectors as (ascending word ids, L1-normalised double values),
and scripts of database operations that a test applies to the device class and to its reference alike.

A scene is a dict: n_words, max_kf, and ops, a list of tuples
    ("add", slots, map_ids, bows)            bows: one (words, values) per slot
    ("erase", slots) / ("clear",) / ("clearMap", map_id)
    ("neigh", slots, rows)                   rows: per slot up to ten neighbour slots (-1: none)
    ("flags", slots, flags)                  bit 0 isBad, bit 1 the map IsBad
    ("nbest", queries, n_candidates)         queries: dicts id, map, bow, connected (slots)
    ("reloc", queries)                       queries: dicts id, map, bow
The designed scenes (designed()) each make one behaviour of the reference decide the output; every one is named after
the behaviour it probes."""
import numpy as np


def uniform_bow(words):
    """Equal weights, L1-normalised."""
    w = np.array(sorted(set(int(x) for x in words)), np.int32)
    return w, np.full(len(w), 1.0 / max(len(w), 1), np.float64)


def random_bow(rng, n_words, length):
    length = min(int(length), n_words)
    w = np.sort(rng.choice(n_words, length, replace=False)).astype(np.int32)
    v = rng.uniform(0.5, 5.0, length) * rng.integers(1, 4, length)   # idf weight x term count
    s = 0.0
    for x in v:   # BowVector::normalize: the norm in ascending word order
        s += abs(x)
    return w, (v / s if length else v)


def pack_bows(bows, stride=None):
    """(bow_word [n][stride] int32, bow_value [n][stride] float64, bow_n [n] int32) host arrays, padded with -1 / 0."""
    n = len(bows)
    stride = int(stride if stride is not None else max([len(w) for w, _ in bows] + [1]))
    bw, bv = np.full((n, stride), -1, np.int32), np.zeros((n, stride), np.float64)
    bn = np.zeros(n, np.int32)
    for i, (w, v) in enumerate(bows):
        bw[i, :len(w)], bv[i, :len(w)], bn[i] = w, v, len(w)
    return bw, bv, bn


def random_scene(n_kf, n_words, lengths, seed, n_q=1, n_candidates=3, q_lengths=None, n_maps=2, mode="nbest",
                 max_kf=None, rounds=2, churn=True):
    """n_kf keyframes in scattered slots with BowVector lengths cycling through `lengths`, random neighbours, flags and
    connected sets; `rounds` Detect calls of n_q queries each (revisits of database keyframes with some words replaced,
    ids that partly repeat), with an erase + re-add and a clearMap between the rounds when `churn`."""
    rng = np.random.Generator(np.random.PCG64(seed))
    max_kf = int(max_kf if max_kf is not None else n_kf + 3)
    slots = rng.permutation(max_kf)[:n_kf].astype(np.int32)
    maps = rng.integers(0, n_maps, n_kf).astype(np.int32)
    bows = [random_bow(rng, n_words, lengths[i % len(lengths)]) for i in range(n_kf)]
    ops = []
    half = max(1, n_kf // 2)
    ops.append(("add", slots[:half], maps[:half], bows[:half]))
    if n_kf > half:
        ops.append(("add", slots[half:], maps[half:], bows[half:]))

    def neigh_rows(which):
        rows = []
        for _ in which:
            k = int(rng.integers(0, 11))
            row = rng.choice(slots, min(k, n_kf), replace=False).astype(np.int32) if n_kf else np.zeros(0, np.int32)
            row = np.where(rng.random(len(row)) < 0.1, -1, row)
            rows.append(row)
        return rows

    ops.append(("neigh", slots, neigh_rows(slots)))
    map_bad = rng.random(n_maps) < 0.3
    flags = ((rng.random(n_kf) < 0.1).astype(np.uint8) | (map_bad[maps].astype(np.uint8) << 1)).astype(np.uint8)
    ops.append(("flags", slots, flags))
    q_lengths = list(q_lengths if q_lengths is not None else lengths)
    next_id = 1
    for r in range(rounds):
        queries = []
        for j in range(n_q):
            src = int(rng.integers(0, n_kf))
            w, _ = bows[src]
            L = q_lengths[(r * n_q + j) % len(q_lengths)]
            keep = w[rng.random(len(w)) < 0.7]
            extra = rng.choice(n_words, min(n_words, L), replace=False)
            words = np.unique(np.concatenate([keep, extra]))
            words = np.sort(rng.permutation(words)[:L]).astype(np.int32)   # L words, or all there are
            v = rng.uniform(0.5, 5.0, len(words))
            s = 0.0
            for x in v:
                s += abs(x)
            bow = (words, v / s if len(words) else v)
            qid = next_id if rng.random() < 0.8 else max(1, next_id - 1)   # some ids repeat
            next_id += 1
            q = dict(id=int(qid), map=int(rng.integers(0, n_maps)), bow=bow)
            if mode == "nbest":
                q["connected"] = rng.choice(slots, min(n_kf, int(rng.integers(0, 6))), replace=False).astype(np.int32)
            queries.append(q)
        ops.append(("nbest", queries, n_candidates) if mode == "nbest" else ("reloc", queries))
        if churn and r + 1 < rounds and n_kf >= 4:
            back = slots[:2]
            ops.append(("erase", back))
            ops.append(("add", back[::-1].copy(), maps[:2][::-1].copy(), [bows[1], bows[0]]))   # to the back of every list
            ops.append(("neigh", back, neigh_rows(back)))
            ops.append(("clearMap", int(n_maps - 1)))
    return dict(n_words=n_words, max_kf=max_kf, ops=ops)


def _scene(ops, n_words=50, max_kf=8):
    return dict(n_words=n_words, max_kf=max_kf, ops=ops)


def designed():
    """name -> scene; the name is the behaviour of the reference that decides the scene's output."""
    U = uniform_bow
    R = range
    out = {}
    # A scores slot 1 (identical vector: 1.0).  B lists both; slot 1 shares one word of eleven (<= minCommonWords 2),
    # keeps A's score, and as slot 0's neighbour beats slot 0's own 0.909: the loop candidate is slot 1.
    out["stale_score"] = _scene([
        ("add", [0, 1], [0, 0], [U(R(0, 10)), U(list(R(10, 20)) + [20])]),
        ("neigh", [0], [[1]]),
        ("nbest", [dict(id=5, map=0, bow=U(list(R(10, 20)) + [20]), connected=[])], 1),
        ("nbest", [dict(id=6, map=0, bow=U(list(R(0, 10)) + [20]), connected=[])], 1)])
    # slot 0 is the better match but connected to the query
    out["connected"] = _scene([
        ("add", [0, 1], [0, 0], [U(R(0, 10)), U(R(5, 15))]),
        ("nbest", [dict(id=3, map=0, bow=U(R(0, 10)), connected=[0])], 1)])
    # mnPlaceRecognitionQuery of a fresh keyframe is 0: query id 0 finds nothing
    out["id_check"] = _scene([
        ("add", [2], [0], [U(R(0, 10))]),
        ("nbest", [dict(id=0, map=0, bow=U(R(0, 10)), connected=[])], 1)])
    # the same id twice: the second query lists nothing
    out["id_check_repeat"] = _scene([
        ("add", [2], [0], [U(R(0, 10))]),
        ("nbest", [dict(id=7, map=0, bow=U(R(0, 10)), connected=[])], 1),
        ("nbest", [dict(id=7, map=0, bow=U(R(0, 10)), connected=[])], 1)])
    # maxCommonWords 10 -> minCommonWords 2; slot 1 (the other map) shares exactly 2: not scored, no merge candidate
    out["strict_min"] = _scene([
        ("add", [0, 1], [0, 1], [U(R(0, 10)), U([20, 21, 30, 31])]),
        ("nbest", [dict(id=4, map=0, bow=U(list(R(0, 10)) + [20, 21]), connected=[])], 1)])
    # identical vectors, equal accScore: the one added first (slot 3) stays first
    out["stable_sort"] = _scene([
        ("add", [3], [0], [U(R(0, 10))]),
        ("add", [1], [0], [U(R(0, 10))]),
        ("nbest", [dict(id=2, map=0, bow=U(R(0, 12)), connected=[])], 1)])
    # the best keyframe isBad
    out["skip_bad"] = _scene([
        ("add", [0, 1], [0, 0], [U(R(0, 10)), U(R(3, 13))]),
        ("flags", [0], [1]),
        ("nbest", [dict(id=2, map=0, bow=U(R(0, 10)), connected=[])], 1)])
    # one candidate per list, two keyframes of the query's map: the second finds the loop list full and is dropped
    out["loop_overflow"] = _scene([
        ("add", [0, 1], [0, 0], [U(R(0, 10)), U(R(3, 13))]),
        ("nbest", [dict(id=2, map=0, bow=U(R(0, 10)), connected=[])], 1)])
    # slot 0 (map 1) scores 1.0 and sets the threshold 0.75; slot 1 (map 0, 0.31) fails it although slot 0 is filtered
    out["reloc_filter_late"] = _scene([
        ("add", [0, 1], [1, 0], [U(R(0, 10)), U(list(R(0, 9)) + list(R(20, 40)))]),
        ("reloc", [dict(id=9, map=0, bow=U(R(0, 10)))])])
    return out


def quirk_of(name):
    """The behaviour (tests/kfdb_ref.QUIRKS) a designed scene probes."""
    return "id_check" if name.startswith("id_check") else name


def order_sensitive():
    """Dense sharing (120 keyframes of 60-150 words out of 400, random weights): the scores of most pairs differ in
    their double bits between the reference's sequential sum and a pairwise tree sum of the same terms."""
    return random_scene(120, 400, [60, 90, 120, 150], seed=21, n_q=2, rounds=1, churn=False)
