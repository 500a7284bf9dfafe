"""The pyramid's strip kernels (pyr_strip in orb_extract.hip): a thread walks one output quad column down a strip of
rows, keeps the horizontal sums of the last two source rows, and forms a pixel from two v_mul_hi_u32_u24.

GPU cases: every level bit-identical to the oracle's cv::resize restatement in both launch modes (OMV_PYR_MODE), at
the smallest shapes that reach each way the strip code can go wrong: a partial last quad (width = 1, 2, 3 mod 4), a
short last strip / row block, an odd pitch, scale factors whose source rows are never / alternately reused, and the
image index of a batch.  CPU case: the multiply-high identity and the u16 range of the scaled x coefficients,
exhaustively over the operand ranges the kernel relies on.
"""
import os
import re

import numpy as np
import pytest

from openmavis_amd import synth
from openmavis_amd.orb import ORBextractor

MODES = ["levels", "chain"]
SIZES = [(322, 246, 41), (333, 250, 9)]   # (w, h, seed); 333 is the odd pitch (byte staging)


def _strip_rows():
    """(kPyrStrip, kPyrBlock) of the kernels as built: read from the source, so that another strip length or row block
    is held to the short-strip case below without anyone editing this file."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openmavis_amd", "csrc", "orb_extract.hip")
    text = open(src).read()
    return tuple(int(re.search(rf"constexpr int {k} = (\d+);", text).group(1)) for k in ("kPyrStrip", "kPyrBlock"))


def _levels(ex, oracle, img, index, nlevels, scale=1.2, tag=""):
    shapes = []
    for lvl in range(1, nlevels):
        ref = oracle.pyramid_level(img, lvl, 1200, scale, nlevels)
        got = ex.debug_level(index, lvl)
        assert got.shape == ref.shape, f"{tag} level {lvl}: shape {got.shape} != {ref.shape}"
        assert np.array_equal(got, ref), f"{tag} level {lvl}: {np.count_nonzero(got != ref)} px differ"
        shapes.append(got.shape)
    return shapes


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_partial_quads_and_short_strips(oracle, monkeypatch, mode):
    monkeypatch.setenv("OMV_PYR_MODE", mode)
    shapes = []
    for w, h, seed in SIZES:
        img = synth.synth_image(seed, w, h)
        ex = ORBextractor(1200, 1.2, 8, 15, 7)
        ex(img, None, (0, 0))
        shapes += _levels(ex, oracle, img, 0, 8, tag=f"{w}x{h} {mode}")
    # the cases this test exists for, read back from the levels so that another size list or strip length cannot
    # drop them quietly
    assert {lw % 4 for _, lw in shapes} >= {1, 2, 3}, "no level with a partial last quad of 1, 2 and 3 pixels"
    for r in _strip_rows():
        assert any(lh % r for lh, _ in shapes), f"every level height is a multiple of {r}: no short last strip / block"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scale,nlevels", [(1.5, 5), (2.0, 3)])
def test_other_scale_factors(oracle, monkeypatch, mode, scale, nlevels):
    """2.0: no source row is shared by two output rows; 1.5: reuse alternates (2 of 3 output rows step one row)."""
    monkeypatch.setenv("OMV_PYR_MODE", mode)
    img = synth.synth_image(31, 640, 480)
    ex = ORBextractor(1000, scale, nlevels, 20, 7)
    ex(img, None, (0, 0))
    _levels(ex, oracle, img, 0, nlevels, scale, tag=f"scale {scale} {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_batch_image_index(oracle, torch_cuda, monkeypatch, mode):
    torch = torch_cuda
    monkeypatch.setenv("OMV_PYR_MODE", mode)
    w, h, n = 322, 246, 3
    imgs = np.stack([synth.synth_image(50 + i, w, h) for i in range(n)])
    ex = ORBextractor(300, 1.2, 8, 20, 7, width=w, height=h, max_images=n)
    cap = ex.max_keypoints()
    kps = torch.zeros((n, cap, 6), dtype=torch.int32, device="cuda")
    desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda")
    n_out = torch.zeros(n, dtype=torch.int32, device="cuda")
    mono = torch.zeros(n, dtype=torch.int32, device="cuda")
    ex.extract_batch(torch.from_numpy(imgs).cuda(), np.zeros((n, 2), np.int32), kps, desc, n_out, mono)
    torch.cuda.synchronize()
    assert ex.last_error() == 0
    for i in range(n):
        _levels(ex, oracle, imgs[i], i, 8, tag=f"image {i} {mode}")


def test_mulhi_identity_and_coefficient_range():
    """((b << 8) * (hs << 8)) >> 32 == (b * hs) >> 16 for every vertical coefficient b in [0, 2048] and every
    hs = h >> 4 in [0, 2^15), with both operands inside v_mul_hi_u32_u24's 24 bits; 16 a fits v_dot2_u32_u16's u16
    operand for every horizontal coefficient a in [0, 2048]."""
    s8, s16, s32 = np.uint64(8), np.uint64(16), np.uint64(32)
    hs = np.arange(0, 1 << 15, dtype=np.uint64)[None, :]
    assert 2048 << 8 < 1 << 24 and int((hs << s8).max()) < 1 << 24
    for b0 in range(0, 2049, 128):   # in slabs: the whole table at once is several GB
        b = np.arange(b0, min(b0 + 128, 2049), dtype=np.uint64)[:, None]
        assert np.array_equal(((b << s8) * (hs << s8)) >> s32, (b * hs) >> s16)
    a = np.arange(0, 2049, dtype=np.int64)
    assert (16 * a).max() <= np.iinfo(np.uint16).max
    # the horizontal sum of two bytes under 16 a0 + 16 a1 <= 16 * 2049 stays inside 24 bits, and masking its low
    # byte is (h >> 4) << 8 for h = sum / 16
    H = 255 * 16 * 2049
    assert H < 1 << 24
    h = np.arange(0, 255 * 2049 + 1, dtype=np.int64)
    assert np.array_equal((16 * h) & ~np.int64(0xff), (h >> 4) << 8)
