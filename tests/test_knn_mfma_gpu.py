"""The matrix-core knnMatch(k=2) kernel (OMV_KNN=mfma) and the lane kernel (OMV_KNN=lanes) against a numpy brute
force: both must return the two smallest (distance, train index) pairs, bit for bit -- integer work, no tolerance.
Shapes are the smallest that cross the kernel's edges: 16-row MFMA tiles, 64-row LDS tiles, 64-query waves,
256-query blocks, partial last tiles, empty sets.
"""
import numpy as np
import pytest

from openmavis_amd import _lib
from openmavis_amd.matcher import FrameBatch, ORBmatcher, bf_knn2_path

pytestmark = pytest.mark.gpu

INT_MAX = np.iinfo(np.int32).max
UNWRITTEN = -7


def np_knn2(q, t):
    """(idx2, dist2) int32 [nq, 2]: stable sort on (distance, index); (-1, INT_MAX) where no neighbour."""
    nq, nt = len(q), len(t)
    idx2 = np.full((nq, 2), -1, np.int32)
    dist2 = np.full((nq, 2), INT_MAX, np.int32)
    if nq == 0 or nt == 0:
        return idx2, dist2
    qb = np.unpackbits(q, axis=1).astype(np.int32)
    tb = np.unpackbits(t, axis=1).astype(np.int32)
    d = qb @ (1 - tb).T + (1 - qb) @ tb.T
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    k = order.shape[1]
    idx2[:, :k] = order
    dist2[:, :k] = np.take_along_axis(d, order, axis=1)
    return idx2, dist2


def run_knn(torch, q, nq, t, nt):
    """omv_bf_knn2 on host arrays q [P, Q, 32], t [P, T, 32]; outputs prefilled, so unwritten rows show."""
    P, Q, T = q.shape[0], q.shape[1], t.shape[1]
    dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    dnq, dnt = torch.from_numpy(nq.astype(np.int32)).cuda(), torch.from_numpy(nt.astype(np.int32)).cuda()
    idx2 = torch.full((P, Q, 2), UNWRITTEN, dtype=torch.int32, device="cuda")
    dist2 = torch.full((P, Q, 2), UNWRITTEN, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().omv_bf_knn2(P, _lib.ptr(dq), Q, _lib.ptr(dnq), _lib.ptr(dt), T, _lib.ptr(dnt),
                                       _lib.ptr(idx2), _lib.ptr(dist2), None), "omv_bf_knn2")
    torch.cuda.synchronize()
    return idx2.cpu().numpy(), dist2.cpu().numpy()


def check_pairs(torch, monkeypatch, q, nq, t, nt, modes):
    got = {}
    for mode in modes:
        monkeypatch.setenv("OMV_KNN", mode)
        assert bf_knn2_path(q.shape[0], q.shape[1], t.shape[1]) == mode
        i2, d2 = got[mode] = run_knn(torch, q, nq, t, nt)
        for p in range(len(nq)):
            ei, ed = np_knn2(q[p, :nq[p]], t[p, :nt[p]])
            assert np.array_equal(i2[p, :nq[p]], ei), f"{mode}: pair {p} (nq {nq[p]}, nt {nt[p]}) indices"
            assert np.array_equal(d2[p, :nq[p]], ed), f"{mode}: pair {p} (nq {nq[p]}, nt {nt[p]}) distances"
            assert (i2[p, nq[p]:] == UNWRITTEN).all() and (d2[p, nq[p]:] == UNWRITTEN).all(), \
                f"{mode}: pair {p} wrote past nq"
    if len(modes) == 2:
        a, b = got[modes[0]], got[modes[1]]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    return got


def test_ties_and_tile_edges(torch_cuda, monkeypatch):
    """Descriptors drawn from 8 distinct rows, so nearly every distance ties; per-pair counts that differ inside one
    launch; equal rows on both sides of the 16-row and 64-row train tile boundaries (the lower index must win)."""
    shapes = [(1, 0), (1, 1), (1, 2), (16, 16), (17, 15), (33, 65), (130, 257)]
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    Q, T = 136, 264   # one capacity for all pairs
    P = len(shapes)
    q = rows[rng.integers(0, 8, (P, Q))]
    t = rows[rng.integers(0, 8, (P, T))]
    nq = np.array([s[0] for s in shapes], np.int32)
    nt = np.array([s[1] for s in shapes], np.int32)
    # rows[0] only where placed: a pair astride the 16-row tile edge (33 x 65) and the 64-row tile edge (130 x 257)
    for p in (5, 6):
        t[p] = rows[rng.integers(1, 8, T)]
    t[5, 15] = t[5, 16] = rows[0]
    t[6, 63] = t[6, 64] = rows[0]
    t[6, 255] = t[6, 256] = rows[1]
    q[5, 7] = q[6, 5] = q[6, 129] = rows[0]
    got = check_pairs(torch_cuda, monkeypatch, q, nq, t, nt, ["mfma", "lanes"])
    i2, d2 = got["mfma"]
    assert i2[5, 7].tolist() == [15, 16] and d2[5, 7].tolist() == [0, 0]
    assert i2[6, 5].tolist() == [63, 64] and i2[6, 129].tolist() == [63, 64] and d2[6, 129].tolist() == [0, 0]
    assert i2[0, 0].tolist() == [-1, -1] and d2[0, 0].tolist() == [INT_MAX, INT_MAX]
    assert i2[1, 0].tolist() == [0, -1] and d2[1, 0, 1] == INT_MAX


def test_bit_placement(torch_cuda, monkeypatch):
    """The 256 one-hot rows against themselves: query j finds (j, 0) and then the lowest other index at distance 2;
    all zeros against all ones is 256.  A dropped or duplicated bit of the i8 expansion shows here."""
    onehot = np.packbits(np.eye(256, dtype=np.uint8), axis=1)
    zeros, ones = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
    q = np.zeros((3, 256, 32), np.uint8)
    t = np.zeros((3, 256, 32), np.uint8)
    q[0], t[0] = onehot, onehot
    q[1, 0], t[1, 0] = zeros, ones
    q[2, 0], t[2, 0], t[2, 1] = ones, zeros, ones
    nq, nt = np.array([256, 1, 1], np.int32), np.array([256, 1, 2], np.int32)
    got = check_pairs(torch_cuda, monkeypatch, q, nq, t, nt, ["mfma", "lanes"])
    i2, d2 = got["mfma"]
    j = np.arange(256)
    assert np.array_equal(i2[0, :, 0], j) and (d2[0, :, 0] == 0).all()
    assert np.array_equal(i2[0, :, 1], np.where(j == 0, 1, 0)) and (d2[0, :, 1] == 2).all()
    assert i2[1, 0].tolist() == [0, -1] and d2[1, 0].tolist() == [256, INT_MAX]
    assert i2[2, 0].tolist() == [1, 0] and d2[2, 0].tolist() == [0, 256]


@pytest.mark.parametrize("mode", ["mfma", "lanes"])
def test_stereo_lapping_offsets(torch_cuda, monkeypatch, mode):
    """StereoLapping on 3 frames x 2 cameras, kp_cap 96: mono > 0 on both cameras (the q_off / t_off rows), counts
    that differ per frame, frame 1 with an empty lapping set on the left.  l2r / r2l equal those derived from the
    numpy knn by stereo_pairs_kernel's rule (ratio in double, the later left index wins a right keypoint)."""
    torch = torch_cuda
    monkeypatch.setenv("OMV_KNN", mode)
    F, C, cap = 3, 2, 96
    rng = np.random.default_rng(17)
    n_kp = np.array([[90, 75], [20, 60], [55, 96]], np.int32)
    mono = np.array([[10, 5], [20, 7], [3, 30]], np.int32)
    desc = rng.integers(0, 256, (F, C, cap, 32), dtype=np.uint8)
    for f in range(F):   # left lapping rows: right lapping rows with a few bits flipped (some twice: r2l contention)
        nq, ntr = n_kp[f, 0] - mono[f, 0], n_kp[f, 1] - mono[f, 1]
        src = rng.integers(0, ntr, nq)
        rows = desc[f, 1, mono[f, 1] + src].copy()
        for i in range(nq):
            for b in rng.integers(0, 256, rng.integers(0, 12)):
                rows[i, b >> 3] ^= np.uint8(1 << (b & 7))
        desc[f, 0, mono[f, 0]:n_kp[f, 0]] = rows
    fb = FrameBatch(torch, F, C, cap, 720, 540, [1.2 ** i for i in range(8)])
    fb.desc.copy_(torch.from_numpy(desc))
    fb.n_kp.copy_(torch.from_numpy(n_kp))
    fb.mono.copy_(torch.from_numpy(mono))
    m = ORBmatcher(0.8)   # a new handle: the knob is read when it is created
    m.StereoLapping(fb, 0.8)
    torch.cuda.synchronize()
    l2r, r2l = fb.l2r.cpu().numpy(), fb.r2l.cpu().numpy()
    kept = 0
    for f in range(F):
        m0, m1 = mono[f]
        i2, d2 = np_knn2(desc[f, 0, m0:n_kp[f, 0]], desc[f, 1, m1:n_kp[f, 1]])
        el2r = np.full(cap, -1, np.int32)
        er2l = np.full(cap, -1, np.int32)
        for qi in range(len(i2)):
            if i2[qi, 1] >= 0 and float(d2[qi, 0]) < float(d2[qi, 1]) * 0.8:
                el2r[m0 + qi] = m1 + i2[qi, 0]
                er2l[m1 + i2[qi, 0]] = m0 + qi
        assert np.array_equal(el2r, l2r[f]) and np.array_equal(er2l, r2l[f]), f"{mode}: frame {f}"
        kept += int((el2r >= 0).sum())
    assert kept > 50 and (l2r[1] == -1).all()


def test_fallback_past_index_limit(torch_cuda, monkeypatch):
    """A train capacity the packed key (distance << 16 | index) cannot index takes the lane kernel even when the knob
    asks for the matrix cores: checked on the dispatch decision, at the real limit (nt < 2^16) and at a surrogate of 64 rows, and
    the result at the surrogate is still the numpy one."""
    monkeypatch.delenv("OMV_KNN", raising=False)
    monkeypatch.delenv("OMV_KNN_IDX_LIMIT", raising=False)
    assert bf_knn2_path(1, 1500, 1500) == "lanes"       # the B = 1 chain
    assert bf_knn2_path(128, 1500, 1500) == "mfma"      # the batch
    assert bf_knn2_path(128, 1500, 65535) == "mfma"
    assert bf_knn2_path(128, 1500, 65536) == "lanes"
    monkeypatch.setenv("OMV_KNN", "mfma")
    assert bf_knn2_path(1, 8, 65535) == "mfma"
    assert bf_knn2_path(1, 8, 65536) == "lanes"
    monkeypatch.setenv("OMV_KNN_IDX_LIMIT", "64")
    assert bf_knn2_path(2, 40, 63) == "mfma"
    assert bf_knn2_path(2, 40, 64) == "lanes"
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (2, 40, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (2, 65, 32), dtype=np.uint8)
    nq, nt = np.array([40, 33], np.int32), np.array([65, 64], np.int32)
    assert bf_knn2_path(2, 40, 65) == "lanes"
    i2, d2 = run_knn(torch_cuda, q, nq, t, nt)
    for p in range(2):
        ei, ed = np_knn2(q[p, :nq[p]], t[p, :nt[p]])
        assert np.array_equal(i2[p, :nq[p]], ei) and np.array_equal(d2[p, :nq[p]], ed)
    monkeypatch.setenv("OMV_KNN", "lanes")
    assert bf_knn2_path(128, 1500, 1500) == "lanes"
