"""The LDS-staged SearchByProjection candidate kernel with windows split over lanes by entry count (OMV_CAND_SPLIT).

Bar: bit-exact.  The records of the staged kernel equal the global-memory kernel's word for word at every split
setting, the assignments equal the oracle's, and windows whose entry counts sit on either side of every split class
boundary give the records of a numpy restatement of the window order.
"""
import numpy as np
import pytest

import math_inputs as mi
from openmavis_amd import synth
from openmavis_amd._lib import KP_DTYPE
from openmavis_amd.matcher import FrameBatch, MapPointBatch, ORBmatcher
from openmavis_amd.orb import ORBextractor
from test_match_gpu import _sbp_case

pytestmark = pytest.mark.gpu

W, H, C, NF = 720, 540, 5, 1200
LAP = np.array([[0, 720], [0, 720], [0, 0], [0, 0], [0, 0]], np.int32)
M = 2100            # three chunks of 1,024 points at OMV_CAND_PW=128, the last partial; five at 64
SPLIT_DEFAULT = 64  # kStageSplit
HUGE = 10 ** 9
SPLITS = (1, 4, 16, None, HUGE)
PWS = (64, 128)
REC_VALID, REC_OVER = np.uint32(1 << 31), np.uint32(1 << 30)


@pytest.fixture(scope="module")
def frames(torch_cuda):
    torch = torch_cuda
    n_frames = 3
    ex = ORBextractor(NF, 1.2, 8, 15, 7, width=W, height=H, max_images=n_frames * C)
    cap = ex.max_keypoints()
    imgs = np.concatenate([synth.hilti_frame(f) for f in range(n_frames)])
    fb = FrameBatch(torch, n_frames, C, cap, W, H, ex.GetScaleFactors())
    ex.extract_batch(torch.from_numpy(imgs).cuda(), np.tile(LAP, (n_frames, 1)), fb.kps.view(-1, cap, 6),
                     fb.desc.view(-1, cap, 32), fb.n_kp.view(-1), fb.mono.view(-1))
    torch.cuda.synchronize()
    assert ex.last_error() == 0
    return fb


def _set_knobs(monkeypatch, mode, split=None, pw=None):
    monkeypatch.setenv("OMV_CAND", mode)
    for k, v in (("OMV_CAND_SPLIT", split), ("OMV_CAND_PW", pw)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _records(fb, mpb, th, n_frames, n_points):
    """Records of one SearchByProjection call under the knobs of the environment (read when the handle is made)."""
    m = ORBmatcher(0.8)
    fb.kp_to_mp.fill_(-1)
    m.SearchByProjection(fb, mpb, th, False, 50.0)
    rec = m.records(n_frames, n_points)
    assert m.last_error() == 0
    fb.kp_to_mp.fill_(-1)
    m.close()
    return rec


def _radius(mp, th, scale):
    """[M][C] window radius: RadiusByViewingCos, th on block 0 only (unless th == 1), the level's scale; float32."""
    r = np.where(mp["view_cos"].astype(np.float64) > 0.998, np.float32(2.5), np.float32(4.0)).astype(np.float32)
    if th != 1.0:
        r[:, 0] = r[:, 0] * np.float32(th)
    return (r * np.asarray(scale, np.float32)[np.clip(mp["level"], 0, 7)]).astype(np.float32)


def _window_entries(cs, x, y, r):
    """Entries of the cells each window (x, y, r) visits, from a camera's cell starts [64 * 48 + 1]; 0 off the grid."""
    rng4, ret, _ = mi.grid_window_ref(np.stack([x, y, r], 1).astype(np.float32), mi.grid_floats(W, H))
    n = np.zeros(len(x), np.int64)
    hit = ret == 0
    x0, x1, y0, y1 = (rng4[:, k].astype(np.int64) for k in range(4))
    for ix in range(mi.GRID_COLS):
        col = hit & (x0 <= ix) & (ix <= x1)
        n[col] += cs[ix * mi.GRID_ROWS + y1[col] + 1] - cs[ix * mi.GRID_ROWS + y0[col]]
    return n


CASES = {(1.0, 0.0): None, (6.0, 0.0): None, (15.0, 0.0): None, (6.0, 0.25): None}


@pytest.fixture(scope="module")
def global_records(frames, torch_cuda):
    """Per (th, occupied fraction): the inputs and the global-memory kernel's records, computed once."""
    torch = torch_cuda
    kps = frames.kps.cpu().numpy().view(KP_DTYPE).reshape(frames.n_frames, C, frames.kp_cap)
    desc, n_kp = frames.desc.cpu().numpy(), frames.n_kp.cpu().numpy()
    scale = [frames.geom.scale_factors[i] for i in range(8)]
    mp_env = pytest.MonkeyPatch()
    out = {}
    try:
        _set_knobs(mp_env, "global")
        grid = ORBmatcher(0.8)
        grid.AssignFeaturesToGrid(frames)
        cs = [[grid.grid(f, c)[0] for c in range(C)] for f in range(frames.n_frames)]
        grid.close()
        for th, occ_frac in CASES:
            per = [synth.make_map_points(kps[f], desc[f], n_kp[f], M, 40 + int(th) + f, W, H)
                   for f in range(frames.n_frames)]
            for f, p in enumerate(per):   # half of the points outside block 0 are seen there too, anywhere, at any level
                rng = np.random.default_rng(90 + f)
                add = (p["in_view"][:, 0] == 0) & (rng.random(M) < 0.5)
                p["proj_x"][add, 0] = rng.uniform(0, W, add.sum()).astype(np.float32)
                p["proj_y"][add, 0] = rng.uniform(0, H, add.sum()).astype(np.float32)
                p["level"][add, 0] = rng.integers(0, 8, add.sum())
                p["in_view"][add, 0] = 1
            mpb = MapPointBatch(**{k: torch.from_numpy(np.stack([p[k] for p in per])).cuda() for k in per[0]})
            occ = (np.random.default_rng(3).random((frames.n_frames, C * frames.kp_cap)) < occ_frac).astype(np.uint8)
            d_occ = torch.from_numpy(occ).cuda() if occ_frac else None
            frames.occ_init = d_occ
            rec = _records(frames, mpb, th, frames.n_frames, M)
            frames.occ_init = None
            active = np.stack([(p["in_view"] != 0) & (p["level"] >= 0) & (p["level"] < 8) for p in per])
            entries = np.zeros(active.shape, np.int64)
            for f, p in enumerate(per):
                r = _radius(p, th, scale)
                for c in range(C):
                    entries[f, :, c] = _window_entries(cs[f][c], p["proj_x"][:, c], p["proj_y"][:, c], r[:, c])
            out[(th, occ_frac)] = dict(mpb=mpb, occ=d_occ, rec=rec, active=active, entries=np.where(active, entries, 0))
    finally:
        mp_env.undo()
    return out


@pytest.mark.parametrize("th,occ_frac", list(CASES))
def test_records_equal_the_global_kernels(frames, global_records, monkeypatch, th, occ_frac):
    """OMV_CAND=lds against OMV_CAND=global on the same inputs, every (point, camera) slot that has a record, for
    OMV_CAND_SPLIT in {1, 4, 16, default, huge} x OMV_CAND_PW in {64, 128}."""
    case = global_records[(th, occ_frac)]
    act = case["active"]
    assert (act[:, :1024, 0].sum(1) > 512).all()   # more active slots than lanes in block 0's first chunk at pw = 128
    frames.occ_init = case["occ"]
    try:
        for split in SPLITS:
            for pw in PWS:
                _set_knobs(monkeypatch, "lds", split, pw)
                rec = _records(frames, case["mpb"], th, frames.n_frames, M)
                bad = np.argwhere((rec != case["rec"]).any(-1) & act)
                assert len(bad) == 0, f"split {split} pw {pw}: {len(bad)} records differ, first (frame, point, cam) {bad[:4].tolist()}"
    finally:
        frames.occ_init = None


def test_cases_reach_every_kind_of_record(global_records):
    """What the cases above contain between them, from the global kernel's records and the windows' entry counts:
    at OMV_CAND_SPLIT=4 every split class at th = 6 and, at th = 15, windows of G = 64 whose lanes walk more than the
    split; no window split at th = 1 under the default; an over-full record, an empty window and, among the windows
    that OMV_CAND_SPLIT=16 splits, a short record and a tie of distance between neighbours of a record (window order
    decides it)."""
    n_at = {}
    over = short = empty = tie = 0
    for (th, occ_frac), case in global_records.items():
        rec, act, ent = case["rec"], case["active"], case["entries"]
        n = ((rec & REC_VALID) != 0).sum(-1)
        dist = (rec >> np.uint32(16)) & np.uint32(0x1ff)
        split = act & (ent > 16)
        over += int((((rec[..., 0] & REC_OVER) != 0) & act).sum())
        short += int(((n > 0) & (n < 16) & split).sum())
        empty += int(((ent == 0) & (n == 0) & act).sum())
        same = (dist[..., 1:] == dist[..., :-1]) & ((rec[..., 1:] & REC_VALID) != 0)
        tie += int((same.any(-1) & split).sum())
        n_at[(th, occ_frac)] = int(ent.max())
        assert ((n == 0) | ~act | (ent > 0)).all()
    print("largest window per case:", n_at, "over", over, "short", short, "empty", empty, "tie", tie)
    assert n_at[(1.0, 0.0)] <= SPLIT_DEFAULT            # th = 1: every window on one lane under the default
    assert n_at[(15.0, 0.0)] > 8 * SPLIT_DEFAULT        # th = 15: G = 16 under the default
    assert n_at[(15.0, 0.0)] > 64 * 4                   # and G = 64 with lanes that walk more than the split at 4
    ent6 = global_records[(6.0, 0.0)]["entries"]
    for k in range(1, 6):                               # th = 6 at OMV_CAND_SPLIT=4: the classes G = 2 .. 32
        assert ((ent6 > 4 << (k - 1)) & (ent6 <= 4 << k)).any(), k
    assert over > 0 and short > 0 and empty > 0 and tie > 0


@pytest.mark.parametrize("pw", PWS)
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", [(6.0, False, 0.8, 0.25, 0.5, True), (15.0, False, 0.9, 0.02, 1.0, False)])
def test_assignments_equal_the_oracles(frames, oracle, torch_cuda, monkeypatch, case, split, pw):
    """SearchByProjection end to end (kp_to_mp, n_matches) against the oracle on two of test_match_gpu.py's cases."""
    _set_knobs(monkeypatch, "lds", split, pw)
    _sbp_case(frames, oracle, torch_cuda, *case)


# ---- windows of a chosen entry count ---------------------------------------------------------------------
COL = 5                                   # every keypoint sits in grid column 5
CW = W / mi.GRID_COLS                     # 11.25 px cells, both ways
COUNTS = (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257)   # E - 1, E, E + 1, 2E, 2E + 1, ... 64E + 1


def _column_camera(rng):
    """One camera whose keypoints fill cells (COL, 2 j), COUNTS[j] of them in row 2 j (odd rows stay empty), at random
    places of the cell, octaves 0 .. 2, descriptors from a set of 8 (ties of distance), in shuffled index order."""
    rows = np.repeat(2 * np.arange(len(COUNTS)), COUNTS)
    n = len(rows)
    order = rng.permutation(n)
    kp = np.zeros(n, KP_DTYPE)
    kp["x"][order] = (COL * CW + rng.uniform(-0.49, 0.49, n) * CW).astype(np.float32)
    kp["y"][order] = (rows * CW + rng.uniform(-0.1, 0.49, n) * CW).astype(np.float32)
    kp["octave"] = rng.choice([0, 0, 0, 1, 2], n)
    base = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    return kp, base[rng.integers(0, 8, n)], base


def _expected_record(kp, desc, occ, mp_desc, x, y, r, lvl):
    """The record of one window, restated: the cells' keypoints in GetFeaturesInArea's order (column, row, index), the
    level / radius / blocked tests, then the 16 smallest by (distance, window order)."""
    g = mi.grid_floats(W, H)
    xy = np.stack([kp["x"], kp["y"]], 1).astype(np.float32)
    cell = mi.grid_cell_of_ref(xy, g)
    (x0, x1, y0, y1), = mi.grid_window_ref(np.array([[x, y, r]], np.float32), g)[0]
    rec = np.zeros(16, np.uint32)
    if x0 < 0:
        return rec, 0
    px, py = cell // mi.GRID_ROWS, cell % mi.GRID_ROWS
    inside = np.flatnonzero((cell >= 0) & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1))
    inside = inside[np.lexsort((inside, cell[inside]))]
    e = np.empty((len(inside), 8), np.float32)
    e[:, 0], e[:, 1], e[:, 2] = xy[inside, 0], xy[inside, 1], kp["octave"][inside]
    e[:, 3:] = (x, y, r, lvl - 1, lvl)
    cand = inside[(mi.kp_in_window_ref(e) == 1) & (occ[inside] == 0)]
    dist = (np.unpackbits(desc[cand], axis=1) != np.unpackbits(mp_desc)[None]).sum(1)
    top = np.argsort(dist, kind="stable")[:16]
    rec[:len(top)] = (cand[top].astype(np.uint32) | (dist[top].astype(np.uint32) << np.uint32(16)) |
                      (kp["octave"][cand[top]].astype(np.uint32) << np.uint32(25)) | REC_VALID)
    if len(cand) > 16:
        rec[0] |= REC_OVER
    return rec, len(inside)


@pytest.mark.parametrize("split", (1, 4))
def test_the_boundary_of_each_class(torch_cuda, monkeypatch, split):
    """Map points whose windows hold exactly E - 1, E, E + 1, 2E, 2E + 1, ... 64E, 64E + 1 entries (E = the split; the
    last is more than 64 lanes x E), three points per window with different descriptors and one with an eighth of the
    keypoints blocked; plus the global kernel on the same input."""
    torch = torch_cuda
    rng = np.random.default_rng(17)
    kp, desc, base = _column_camera(rng)
    n, cap = len(kp), 1100
    scale = [np.float32(1.2) ** k for k in range(8)]
    fb = FrameBatch(torch, 1, 1, cap, W, H, scale)
    kh = np.zeros(cap, KP_DTYPE)
    kh[:n] = kp
    dh = np.zeros((cap, 32), np.uint8)
    dh[:n] = desc
    fb.kps.copy_(torch.from_numpy(kh.view(np.int32).reshape(1, 1, cap, 6)))
    fb.desc.copy_(torch.from_numpy(dh.reshape(1, 1, cap, 32)))
    fb.n_kp.fill_(n)
    occ = np.zeros(cap, np.uint8)
    occ[:n] = rng.random(n) < 0.125
    fb.occ_init = torch.from_numpy(occ.reshape(1, cap)).cuda()
    # window j: centre in row 2 j's upper half, r = 4 (level 0, view_cos below 0.998, th = 1): rows 2 j and 2 j + 1
    J = len(COUNTS)
    Mb = 3 * J
    j = np.arange(Mb) % J
    mp = dict(desc=base[rng.integers(0, 8, Mb)] ^ rng.integers(0, 2, (Mb, 32), dtype=np.uint8),
              proj_x=np.full((Mb, 1), COL * CW, np.float32), proj_y=(2 * j * CW + 5.6).astype(np.float32).reshape(Mb, 1),
              view_cos=np.full((Mb, 1), 0.99, np.float32), level=np.zeros((Mb, 1), np.int32),
              in_view=np.ones((Mb, 1), np.uint8), track_depth=np.ones(Mb, np.float32), is_bad=np.zeros(Mb, np.uint8),
              has_obs=np.ones(Mb, np.uint8))
    mpb = MapPointBatch(**{k: torch.from_numpy(v[None]).cuda() for k, v in mp.items()})
    exp = np.zeros((Mb, 16), np.uint32)
    for i in range(Mb):
        exp[i], entries = _expected_record(kp, desc, occ[:n], mp["desc"][i], mp["proj_x"][i, 0], mp["proj_y"][i, 0],
                                           np.float32(4.0), 0)
        assert entries == COUNTS[j[i]]
    for E in (1, 4):   # the list holds every boundary of either split
        assert {E - 1, E, E + 1, 64 * E, 64 * E + 1} <= set(COUNTS) and all(E << k in COUNTS and (E << k) + 1 in COUNTS for k in range(7))
    assert (exp[:, 0] & REC_OVER).any() and (exp == 0).all(1).any()
    for mode, sp in (("lds", split), ("global", None)):
        _set_knobs(monkeypatch, mode, sp, 64)
        got = _records(fb, mpb, 1.0, 1, Mb)[0, :, 0]
        bad = np.flatnonzero((got != exp).any(1))
        assert len(bad) == 0, f"{mode} split {sp}: windows of {[COUNTS[j[b]] for b in bad[:6]]} entries differ"
