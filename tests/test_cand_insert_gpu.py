"""The LDS-staged SearchByProjection candidate kernel with position keys on every window (omv::topk_insert, one
v_med3_u32 per list slot) and the level / blocked test folded into one compare on the staged octave field.

Bar: bit-exact.  On one camera whose keypoints sit in chosen cells of two grid columns, the staged kernel's records
(OMV_CAND=lds, every window on one lane at a huge OMV_CAND_SPLIT, and dealt to several lanes at 4) equal the
global-memory kernel's and a numpy restatement of the window order word for word.  The windows are built so that the
list and the tests meet their edge cases, and each case is shown to be present from the restatement."""
import numpy as np
import pytest

import math_inputs as mi
from openmavis_amd._lib import KP_DTYPE
from openmavis_amd.matcher import FrameBatch, MapPointBatch
from test_cand_balance_gpu import _records, _set_knobs

pytestmark = pytest.mark.gpu

W, H = 720, 540
CW = W / mi.GRID_COLS            # 11.25 px cells, both ways; cell (c, r) is centred on (c CW, r CW)
COL = 5
HUGE = 10 ** 9
CAP = 1100
SCALE = [np.float32(1.2) ** k for k in range(8)]
REC_VALID, REC_OVER = np.uint32(1 << 31), np.uint32(1 << 30)


def _flip(desc, d):
    """desc with its first d bits flipped: Hamming distance d from desc."""
    bits = np.unpackbits(desc)
    bits[:d] ^= 1
    return np.packbits(bits)


class _Scene:
    """Windows centred on (COL CW + cx, R CW), R = 1, 3, 5, ...: at levels 0 and 1 (r = 4, 4.8) a window visits rows
    R - 1 .. R + 1, at level 7 (r = 14.3) rows R - 2 .. R + 2, and keypoints sit in rows R only, so a window sees its own
    keypoints alone.  A keypoint is (dx, dy, octave, distance to the window's descriptor or a descriptor, blocked), in
    ascending keypoint index as listed."""

    def __init__(self, rng):
        self.rng = rng
        self.win, self.kp = {}, []   # name -> (row, cx, level, descriptor); (window, dx, dy, octave, desc, blocked)

    def window(self, name, lvl, kps, cx=0.0, row=None):
        row = 1 + 2 * len(self.win) if row is None else row
        d = self.rng.integers(0, 256, 32, dtype=np.uint8)
        self.win[name] = (row, cx, lvl, d)
        for dx, dy, octave, dist, blocked in kps:
            desc = _flip(d, dist) if np.isscalar(dist) else dist
            self.kp.append((name, dx, dy, octave, desc, blocked))


def _build(rng):
    s = _Scene(rng)
    inr = lambda n: list(zip(rng.uniform(-3.5, 3.5, n), rng.uniform(-3.5, 3.5, n)))   # inside r = 4
    # strictly descending distances in window order, more than 16 of them; three outside the radius, two off level
    s.window("descending", 0, [(dx, dy, 0, 120 - 3 * i, 0) for i, (dx, dy) in enumerate(inr(24))] +
             [(0.0, 5.0, 0, 1, 0), (0.0, -5.0, 0, 2, 0), (5.0, 0.0, 0, 3, 0), (1.0, 1.0, 2, 4, 0), (2.0, 1.0, 3, 5, 0)])
    # 15 distinct small distances, then three entries at distance 40 and two at 60.  The window's centre lies 5 px left
    # of column COL's centre, so dx < -0.7 is column COL - 1, which the window walks first: the tie entry listed last
    # (highest keypoint index) is the first of the three in window order, and the one that stays as the 16th
    small = rng.permutation(15) + 1
    s.window("tie", 0, [(dx, dy, 0, int(d), 0) for d, (dx, dy) in zip(small, inr(15))] +
             [(1.0, 2.0, 0, 60, 0), (2.0, -2.0, 0, 40, 0), (3.0, 1.0, 0, 40, 0), (-2.0, 0.5, 0, 60, 0), (-3.0, -1.0, 0, 40, 0)],
             cx=-5.0)
    # exactly 16 pass; two off level, two outside the radius, two blocked
    s.window("sixteen", 1, [(dx, dy, i & 1, int(d), 0) for i, (d, (dx, dy)) in enumerate(zip(rng.integers(0, 200, 16), inr(16)))] +
             [(0.5, 0.5, 2, 0, 0), (1.5, 0.5, 3, 1, 0), (0.0, 5.2, 0, 2, 0), (-5.2, 0.0, 1, 3, 0), (1.0, -1.0, 0, 4, 1), (-1.0, 1.0, 1, 5, 1)])
    # entries, none of which passes
    s.window("none", 0, [(dx, dy, 1 + i % 3, 10 + i, 0) for i, (dx, dy) in enumerate(inr(8))] + [(0.0, 5.0, 0, 0, 0), (1.0, 1.0, 0, 1, 1)])
    s.window("empty", 0, [])
    # octaves lvl - 2 .. lvl + 1, four keypoints each (no octave below 0)
    for lvl in (0, 1):
        s.window(f"octaves{lvl}", lvl, [(dx, dy, o, int(d), 0) for o in range(max(lvl - 2, 0), lvl + 2)
                                        for d, (dx, dy) in zip(rng.integers(0, 200, 4), inr(4))])
    # blocked keypoints at octaves that would pass, among unblocked ones
    s.window("blocked", 1, [(dx, dy, i & 1, int(d), int(i % 3 == 0)) for i, (d, (dx, dy)) in enumerate(zip(rng.integers(0, 200, 12), inr(12)))])
    # the blocked keypoint would be the best
    s.window("blocked_best", 0, [(1.0, 1.0, 0, 30, 0), (2.0, -1.0, 0, 0, 1), (-1.0, 2.0, 0, 20, 0), (-2.0, -2.0, 0, 25, 0)])
    # more than 32 entries in a column's run (a second pass of the scan), up to many times the split: anywhere in the
    # cell, octaves 0 .. 2, descriptors from a set of 8 (ties of distance), an eighth blocked
    base = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    fill = lambda n: [(dx, dy, int(o), base[b], int(bl)) for dx, dy, o, b, bl in
                      zip(rng.uniform(-5.5, 5.5, n), rng.uniform(-5.5, 5.5, n), rng.choice([0, 0, 0, 1, 2], n),
                          rng.integers(0, 8, n), rng.random(n) < 0.125)]
    for n in (33, 65, 129, 257):
        s.window(f"random{n}", n & 1, fill(n))
    s.window("octaves7", 7, [(dx, dy, o, int(d), 0) for o in range(5, 9) for d, (dx, dy) in zip(rng.integers(0, 200, 4), inr(4))],
             row=45)
    s.window("random_rest", 0, fill(CAP - len(s.kp)))
    assert len(s.kp) == CAP and max(r for r, _, _, _ in s.win.values() if r != 45) <= 41
    # keypoint indices: a random subset per window, ascending in listed order
    order = rng.permutation(CAP)
    kp, desc, occ = np.zeros(CAP, KP_DTYPE), np.zeros((CAP, 32), np.uint8), np.zeros(CAP, np.uint8)
    at = 0
    for name, (row, cx, _, _) in s.win.items():
        mine = [k for k in s.kp if k[0] == name]
        for i, (_, dx, dy, octave, d, blocked) in zip(sorted(order[at:at + len(mine)]), mine):
            kp["x"][i], kp["y"][i] = np.float32(COL * CW + cx + dx), np.float32(row * CW + dy)
            kp["octave"][i], desc[i], occ[i] = octave, d, blocked
        at += len(mine)
    # map points: per window its own descriptor, then two from the set of 8 with a few bits changed; then two points with
    # a predicted level outside [0, 8) on a window that holds entries
    names, mdesc, lvl = [], [], []
    for name, (_, _, level, d) in s.win.items():
        for k in range(3):
            names.append(name)
            mdesc.append(d if k == 0 else base[rng.integers(0, 8)] ^ rng.integers(0, 2, 32, dtype=np.uint8))
            lvl.append(level)
    for level in (8, -1):
        names.append("random65"), mdesc.append(base[0]), lvl.append(level)
    mp = dict(desc=np.stack(mdesc), proj_x=np.array([COL * CW + s.win[n][1] for n in names], np.float32).reshape(-1, 1),
              proj_y=np.array([s.win[n][0] * CW for n in names], np.float32).reshape(-1, 1),
              view_cos=np.full((len(names), 1), 0.99, np.float32), level=np.array(lvl, np.int32).reshape(-1, 1),
              in_view=np.ones((len(names), 1), np.uint8), track_depth=np.ones(len(names), np.float32),
              is_bad=np.zeros(len(names), np.uint8), has_obs=np.ones(len(names), np.uint8))
    return kp, desc, occ, mp, names


def _restate(kp, desc, occ, mp_desc, x, y, r, lvl):
    """One window restated: the visited cells' keypoints in GetFeaturesInArea's order (column, row, index), the level /
    radius tests, the blocked ones dropped, then the 16 smallest by (distance, window order).  Returns the record, the
    visited keypoints, which of them pass the level / radius tests, and their distances."""
    g = mi.grid_floats(W, H)
    xy = np.stack([kp["x"], kp["y"]], 1).astype(np.float32)
    cell = mi.grid_cell_of_ref(xy, g)
    (x0, x1, y0, y1), = mi.grid_window_ref(np.array([[x, y, r]], np.float32), g)[0]
    assert x0 >= 0
    px, py = cell // mi.GRID_ROWS, cell % mi.GRID_ROWS
    inside = np.flatnonzero((cell >= 0) & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1))
    inside = inside[np.lexsort((inside, cell[inside]))]
    e = np.empty((len(inside), 8), np.float32)
    e[:, 0], e[:, 1], e[:, 2] = xy[inside, 0], xy[inside, 1], kp["octave"][inside]
    e[:, 3:] = (x, y, r, lvl - 1, lvl)
    geo = mi.kp_in_window_ref(e) == 1
    dist = (np.unpackbits(desc[inside], axis=1) != np.unpackbits(mp_desc)[None]).sum(1)
    cand, cdist = inside[geo & (occ[inside] == 0)], dist[geo & (occ[inside] == 0)]
    top = np.argsort(cdist, kind="stable")[:16]
    rec = np.zeros(16, np.uint32)
    rec[:len(top)] = (cand[top].astype(np.uint32) | (cdist[top].astype(np.uint32) << np.uint32(16)) |
                      (kp["octave"][cand[top]].astype(np.uint32) << np.uint32(25)) | REC_VALID)
    if len(cand) > 16:
        rec[0] |= REC_OVER
    return rec, inside, geo, dist


@pytest.fixture(scope="module")
def scene(torch_cuda):
    """The input on the device, the restatement of every window and the global-memory kernel's records, made once."""
    torch = torch_cuda
    kp, desc, occ, mp, names = _build(np.random.default_rng(23))
    fb = FrameBatch(torch, 1, 1, CAP, W, H, SCALE)
    fb.kps.copy_(torch.from_numpy(kp.view(np.int32).reshape(1, 1, CAP, 6)))
    fb.desc.copy_(torch.from_numpy(desc.reshape(1, 1, CAP, 32)))
    fb.n_kp.fill_(CAP)
    fb.occ_init = torch.from_numpy(occ.reshape(1, CAP)).cuda()
    mpb = MapPointBatch(**{k: torch.from_numpy(v[None]).cuda() for k, v in mp.items()})
    active = (mp["level"][:, 0] >= 0) & (mp["level"][:, 0] < 8)
    win = []
    for i in range(len(names)):
        lvl = int(np.clip(mp["level"][i, 0], 0, 7))
        win.append(_restate(kp, desc, occ, mp["desc"][i], mp["proj_x"][i, 0], mp["proj_y"][i, 0], np.float32(4.0) * SCALE[lvl], lvl))
    env = pytest.MonkeyPatch()
    try:
        _set_knobs(env, "global", None, 64)
        glob = _records(fb, mpb, 1.0, 1, len(names))[0, :, 0]
    finally:
        env.undo()
    return dict(fb=fb, mpb=mpb, kp=kp, occ=occ, mp=mp, names=names, active=active, win=win,
                exp=np.stack([w[0] for w in win]), glob=glob)


def test_every_case_is_in_the_input(scene):
    """From the restatement (and the records it gives), not from what the kernels return."""
    kp, occ, names, win, exp = scene["kp"], scene["occ"], scene["names"], scene["win"], scene["exp"]
    first = {n: names.index(n) for n in dict.fromkeys(names)}   # the map point with the window's own descriptor

    def passing(name):
        _, inside, geo, dist = win[first[name]]
        ok = geo & (occ[inside] == 0)
        return inside[ok], dist[ok], inside, geo, dist

    cand, d, inside, _, _ = passing("descending")
    assert len(cand) > 16 and (np.diff(d) < 0).all() and len(inside) > len(cand)
    assert exp[first["descending"], 0] & REC_OVER
    cand, d, _, _, _ = passing("tie")
    by = np.argsort(d, kind="stable")
    assert len(cand) > 16 and d[by[15]] == d[by[16]] and d[by[14]] < d[by[15]]
    assert cand[by[15]] > cand[by[16]]          # window order, not keypoint index, decides
    assert exp[first["tie"], 0] & REC_OVER and (exp[first["tie"], 15] & np.uint32(0xffff)) == cand[by[15]]
    cand, _, inside, geo, _ = passing("sixteen")
    assert len(cand) == 16 and len(inside) > geo.sum() > 16
    assert (exp[first["sixteen"]] & REC_VALID).all() and not exp[first["sixteen"], 0] & REC_OVER
    cand, _, inside, _, _ = passing("none")
    assert len(cand) == 0 and len(inside) > 0 and (exp[first["none"]] == 0).all()
    assert len(passing("empty")[2]) == 0
    for lvl in (0, 1, 7):
        cand, _, inside, _, _ = passing(f"octaves{lvl}")
        assert set(kp["octave"][inside]) == set(range(max(lvl - 2, 0), lvl + 2))
        assert set(kp["octave"][cand]) == set(range(max(lvl - 1, 0), lvl + 1)) and len(cand) == len(inside) - 4 * (1 + (lvl > 1))
        assert scene["mp"]["level"][first[f"octaves{lvl}"], 0] == lvl
    _, _, inside, geo, _ = passing("blocked")
    assert (geo & (occ[inside] == 1)).sum() >= 3 and (geo & (occ[inside] == 0)).sum() >= 3
    cand, d, inside, geo, dist = passing("blocked_best")
    best = inside[geo][np.argmin(dist[geo])]
    assert occ[best] == 1 and dist[geo].min() < d.min() and len(cand) > 0
    lv = scene["mp"]["level"][:, 0]
    assert (lv == 8).any() and (lv == -1).any() and (scene["mp"]["in_view"][(lv < 0) | (lv > 7)] == 1).all()
    for i in np.flatnonzero(~scene["active"]):
        assert len(win[i][1]) > 0               # their window holds entries
    # between them the windows give short, full and over-full records, and runs of more than 32 entries
    n = ((exp & REC_VALID) != 0).sum(1)
    assert ((n > 0) & (n < 16)).any() and (n == 16).any() and max(len(w[1]) for w in win) > 256


def test_the_global_kernel_equals_the_restatement(scene):
    act = scene["active"]
    bad = np.flatnonzero((scene["glob"] != scene["exp"]).any(1) & act)
    assert len(bad) == 0, f"windows {[scene['names'][b] for b in bad[:6]]} differ"


@pytest.mark.parametrize("split", (HUGE, 4))
def test_staged_records_word_for_word(scene, monkeypatch, split):
    """OMV_CAND=lds with every window on one lane (huge split) and with windows of more than 4 entries dealt to lanes."""
    _set_knobs(monkeypatch, "lds", split, 64)
    got = _records(scene["fb"], scene["mpb"], 1.0, 1, len(scene["names"]))[0, :, 0]
    act = scene["active"]
    for ref in ("exp", "glob"):
        bad = np.flatnonzero((got != scene[ref]).any(1) & act)
        assert len(bad) == 0, f"split {split} against {ref}: windows {[scene['names'][b] for b in bad[:6]]} differ"
