"""FAST prefilter and describe read their bookkeeping from host tables (csrc/fast_plan.h): the prefilter's slots (LDS
address, entry base, column mask) and describe's Toeplitz operands per patch byte offset.

Each case compares ORBextractor with the CPU oracle bit for bit (keypoint fields as raw bits, order, monoIndex,
descriptors) on an image built to reach what changed, and first asserts from the oracle or numpy alone that it does:
- lattice: single 255 pixels on 0 at a pitch of 9 px (sheared, see _lattice).  Each is a corner and none lies on
  another's ring; corners fall on every bit of a slot and on the first and last window column and row of some cell,
  and their patches start at every byte offset po and reach the level's left and right edges;
- octants: wedges in 8 orientations, so that describe's steering sees every sign combination of (cos, sin);
- faint: every cell retries at minTh, which runs the second inlined copy of the prefilter.
Sizes: 320x240, 333x250 (odd pitch: byte staging), 248x250 (level 5 is one 68-px cell column: per-cell stride).
"""
import numpy as np
import pytest

from openmavis_amd.orb import ORBextractor
from test_fast_corner_list_gpu import INI, MIN, SIZES, _blocks, _compare

pytestmark = pytest.mark.gpu


def _check(oracle, img, nf, tag):
    o_mono, o_kps, o_desc = oracle.orb_extract(img, nf, 1.2, 8, INI, MIN, (0, 0))
    g_mono, g_kps, g_desc = ORBextractor(nf, 1.2, 8, INI, MIN)(img, None, (0, 0))
    _compare(o_mono, o_kps, o_desc, g_mono, g_kps, g_desc, tag)


def _cell_windows(n, skip):
    """Detection windows [first, last] of the level-0 cells along an axis of n pixels (ORBextractor.cc:718-742; a cell
    that starts within `skip` pixels of the far border is dropped: 6 along x, 3 along y)."""
    span = n - 32
    cells = span // 35
    size = -(-span // cells)
    out = []
    for i in range(cells):
        ini = 16 + i * size
        if ini >= n - 16 - skip:
            continue
        out.append((ini + 3, min(ini + size + 6, n - 16) - 4))
    return out


def _lattice(w, h):
    """Single 255 pixels at a pitch of 9 px, sheared: lattice row j starts j % 9 columns further right and every fourth
    lattice column one row further down (fewer than 36 columns: the row shift never wraps), so the points still keep 8 px or more from each other along an axis while
    their columns (and rows) run through all residues of 9.  Unsheared, the 36-px cells of the 320-px shape would see one
    phase of the lattice in every cell and no cell edge opposite the one the lattice starts on."""
    assert w < 19 + 9 * 36
    img = np.zeros((h, w), np.uint8)
    for j in range((h + 8) // 9):
        for i in range((w + 8) // 9):
            x, y = 19 + 9 * i + j % 9, 19 + 9 * j + i // 4
            if x < w and y < h:
                img[y, x] = 255
    return img


@pytest.mark.parametrize("w,h,nf", SIZES)
def test_lattice_reaches_every_slot_bit_and_edge(oracle, w, h, nf):
    img = _lattice(w, h)
    xs, ys, _ = oracle.level_candidates(img, INI, MIN)   # level 0, relative to the FAST border (16)
    x, y = xs.astype(np.int64) + 16, ys.astype(np.int64) + 16
    # every lattice point of the detection area is a keypoint of its cell, and nothing else is
    py, px = np.nonzero(img[19:h - 19, 19:w - 19])
    want = set(zip((px + 19).tolist(), (py + 19).tolist()))
    assert set(zip(x.tolist(), y.tolist())) == want
    assert set((x % 8).tolist()) == set(range(8))
    cols, rows = set(x.tolist()), set(y.tolist())
    assert any(a in cols and b in cols for a, b in _cell_windows(w, 6)), "no cell has corners on both edge columns"
    assert any(a in rows and b in rows for a, b in _cell_windows(h, 3)), "no cell has corners on both edge rows"
    # describe: the keypoints of level 0 start their patches at every byte offset and reach both level edges (a patch
    # spans columns cx - 21 .. cx + 21 and is loaded as 48 bytes from the dword at or below cx - 21)
    nf = 4 * nf   # most of the lattice survives the octree
    _, kps, _ = oracle.orb_extract(img, nf, 1.2, 8, INI, MIN, (0, 0))
    cx = kps["x"][kps["octave"] == 0].astype(np.int64)
    po = (cx - 21) & 3
    assert set(po.tolist()) == {0, 1, 2, 3}
    assert (cx - 21 - po < 0).any() and (cx - 21 - po + 48 > w).any()
    _check(oracle, img, nf, f"lattice {w}x{h}")


def _wedges(w, h):
    """Bright wedges (opening 50 degrees, 13 px long) on a dark ground, their axes at 22.5 + 45 k degrees."""
    img = np.full((h, w), 40, np.uint8)
    yy, xx = np.mgrid[-16:17, -16:17]
    rad, ang = np.hypot(xx, yy), np.degrees(np.arctan2(yy, xx))
    k = 0
    for cy in range(36, h - 36, 40):
        for cx in range(36, w - 36, 40):
            axis = 22.5 + 45 * (k % 8)
            k += 1
            d = (ang - axis + 180) % 360 - 180
            m = (rad <= 13) & (np.abs(d) <= 25)
            img[cy - 16:cy + 17, cx - 16:cx + 17][m] = 210
    return img


@pytest.mark.parametrize("w,h,nf", SIZES)
def test_octants_reach_every_steering_sign(oracle, w, h, nf):
    img = _wedges(w, h)
    _, kps, _ = oracle.orb_extract(img, nf, 1.2, 8, INI, MIN, (0, 0))
    octants = set((kps["angle"] // 45).astype(np.int64).tolist())
    assert octants == set(range(8)), octants
    _check(oracle, img, nf, f"octants {w}x{h}")


@pytest.mark.parametrize("w,h,nf", SIZES)
def test_faint_cells_retry_with_the_slot_table(oracle, w, h, nf):
    img = _blocks(102, w, h, 120, 130)
    assert len(oracle.level_candidates(img, INI, INI)[0]) == 0   # no cell has an iniTh keypoint ...
    assert len(oracle.level_candidates(img, INI, 7)[0]) > 0      # ... and the retry finds some
    _check(oracle, img, nf, f"faint {w}x{h}")
