"""Output-row placement and FAST cell geometry of the HIP ORB extractor against the CPU oracle, bit-exact.

describe_kernel places every keypoint's row from the image's per-level counts (total, monoIndex part, lapping part),
which it reads once per wave and sums in registers; fast_cells_kernel reads its per-cell constants from a host-built
table.  The images here make those sums matter: a dominant lapping part, empty top levels, levels of one to four
keypoints, a batch whose images need different counts, and the two cell geometries off the common path (a 68-px cell
column with the per-cell LDS stride; an odd pitch, which takes the byte path and its run-time constants).

Bar: keypoints (x, y, size, angle, response, octave), their order, monoIndex and all 32 descriptor bytes identical to
oracle.orb_extract.  8 levels, scale 1.2, iniTh 20, minTh 7; the shapes are the smallest at which the reference runs
with 8 levels.
"""
import numpy as np
import pytest

from openmavis_amd import synth
from openmavis_amd.orb import ORBextractor

pytestmark = pytest.mark.gpu

NLEVELS, SCALE, INI, MIN = 8, 1.2, 20, 7


def _compare(o_mono, o_kps, o_desc, g_mono, g_kps, g_desc, tag=""):
    assert g_mono == o_mono, f"{tag} monoIndex {g_mono} != {o_mono}"
    assert len(g_kps) == len(o_kps), f"{tag} count {len(g_kps)} != {len(o_kps)}"
    for f in ("x", "y", "size", "angle", "response", "octave"):
        bad = np.nonzero(g_kps[f].view(np.uint32) != o_kps[f].view(np.uint32))[0]
        assert bad.size == 0, f"{tag} field {f} differs at rows {bad[:10]}: gpu {g_kps[bad[:3]]} oracle {o_kps[bad[:3]]}"
    bad = np.nonzero((g_desc != o_desc).any(1))[0]
    assert bad.size == 0, f"{tag} descriptors differ at rows {bad[:10]}"


def _textured(w, h, seed):
    return synth.synth_image(seed, w, h)


def _right_flat(w, h, seed):
    img = synth.synth_image(seed, w, h)
    img[:, w // 2:] = 90
    return img


def _bottom_flat(w, h, seed):
    img = synth.synth_image(seed, w, h)
    img[h // 3:, :] = 60
    return img


def _left_flat(w, h, seed):
    img = synth.synth_image(seed, w, h)
    img[:, :w // 3] = 50
    return img


def _low_contrast(w, h, seed):
    return (synth.synth_image(seed, w, h) // 16 + 100).astype(np.uint8)


def _level_counts(kps):
    return np.bincount(kps["octave"], minlength=NLEVELS).tolist()


# (name, image, w, h, nfeatures, lapping, seed, what the oracle gives: keypoints, monoIndex or None, per-level
#  counts of all keypoints or None, per-level counts of the lapping keypoints or None)
ROW_CASES = [
    ("textured", _textured, 200, 150, 300, (60, 120), 6, 151, 113, [65, 27, 22, 20, 17, 0, 0, 0], None),
    ("lapping dominates", _right_flat, 200, 150, 300, (60, 120), 6, 107, 35, None, [54, 5, 5, 4, 4, 0, 0, 0]),
    ("top levels empty", _bottom_flat, 240, 180, 300, (0, 90), 7, 132, None, None, None),
    ("every level lapping", _left_flat, 320, 240, 300, (100, 180), 7, 305, None, None, None),
    ("low contrast", _low_contrast, 240, 180, 120, (80, 160), 11, 16, None, [1, 3, 3, 3, 4, 2, 0, 0], None),
]


@pytest.mark.parametrize("name,make,w,h,nf,lap,seed,n_exp,mono_exp,lv_exp,lap_lv_exp", ROW_CASES,
                         ids=[c[0].replace(" ", "_") for c in ROW_CASES])
def test_row_placement_matches_oracle(oracle, name, make, w, h, nf, lap, seed, n_exp, mono_exp, lv_exp, lap_lv_exp):
    img = make(w, h, seed)
    o_mono, o_kps, o_desc = oracle.orb_extract(img, nf, SCALE, NLEVELS, INI, MIN, lap)
    # the case is what it is meant to be (the oracle's own figures, before anything of the GPU is looked at)
    lv, lap_lv = _level_counts(o_kps), _level_counts(o_kps[o_mono:])
    print(f"{name}: oracle keypoints {len(o_kps)} monoIndex {o_mono} per level {lv} lapping per level {lap_lv}")
    assert len(o_kps) == n_exp
    if mono_exp is not None:
        assert o_mono == mono_exp
    if lv_exp is not None:
        assert lv == lv_exp
    if lap_lv_exp is not None:
        assert lap_lv == lap_lv_exp
    if name == "textured":
        assert sum(1 for c in lap_lv if c) == 5
    if name == "top levels empty":
        assert lv[6] == 0 and lv[7] == 0 and all(lv[:6])
    if name == "every level lapping":
        assert all(lv) and all(lap_lv)
    ex = ORBextractor(nf, SCALE, NLEVELS, INI, MIN)
    g_mono, g_kps, g_desc = ex(img, None, lap)
    _compare(o_mono, o_kps, o_desc, g_mono, g_kps, g_desc, f"{name} {w}x{h} seed {seed}")


def test_batch_rows_use_each_images_counts(oracle, torch_cuda):
    """Four different images in one extract_batch, each with its own lapping range: a count table indexed by the wrong
    image, or a prefix that leaks across images, moves rows here."""
    torch = torch_cuda
    w, h, nf = 240, 180, 300
    imgs = np.stack([_textured(w, h, 7), _bottom_flat(w, h, 7), _low_contrast(w, h, 11), np.full((h, w), 77, np.uint8)])
    lap = np.array([[40, 200], [0, 90], [80, 160], [100, 140]], np.int32)
    ex = ORBextractor(nf, SCALE, NLEVELS, INI, MIN, width=w, height=h, max_images=4)
    cap = ex.max_keypoints()
    kps = torch.zeros((4, cap, 6), dtype=torch.int32, device="cuda")
    desc = torch.zeros((4, cap, 32), dtype=torch.uint8, device="cuda")
    n_out = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    mono = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    ex.extract_batch(torch.from_numpy(imgs).cuda(), lap, kps, desc, n_out, mono)
    torch.cuda.synchronize()
    assert ex.last_error() == 0
    kps_h = kps.cpu().numpy().view(oracle.KP_DTYPE).reshape(4, cap)
    desc_h, n_h, m_h = desc.cpu().numpy(), n_out.cpu().numpy(), mono.cpu().numpy()
    counts = []
    for c in range(4):
        o_mono, o_kps, o_desc = oracle.orb_extract(imgs[c], nf, SCALE, NLEVELS, INI, MIN, tuple(int(v) for v in lap[c]))
        counts.append(len(o_kps))
        assert int(n_h[c]) == len(o_kps), f"image {c}: count {int(n_h[c])} != {len(o_kps)}"
        n = int(n_h[c])
        _compare(o_mono, o_kps, o_desc, int(m_h[c]), kps_h[c, :n], desc_h[c, :n], f"image {c}")
    assert counts[3] == 0 and all(counts[:3]) and len(set(counts)) == 4, counts


@pytest.mark.parametrize("w,h,nf,seed", [(248, 250, 150, 12), (333, 250, 300, 9)])
def test_fast_cell_geometry_matches_oracle(oracle, w, h, nf, seed):
    """248x250: level 5 is one 68-px cell column (per-cell LDS row stride); 333x250: odd pitch, so level 0 takes the byte
    path, whose constants the kernel still derives at run time.  Host table and fallback agree with the oracle."""
    img = synth.synth_image(seed, w, h)
    o_mono, o_kps, o_desc = oracle.orb_extract(img, nf, SCALE, NLEVELS, INI, MIN, (0, 0))
    assert len(o_kps) > 0
    ex = ORBextractor(nf, SCALE, NLEVELS, INI, MIN)
    g_mono, g_kps, g_desc = ex(img, None, (0, 0))
    _compare(o_mono, o_kps, o_desc, g_mono, g_kps, g_desc, f"{w}x{h} seed {seed}")


def test_oversized_pitch_is_rejected(torch_cuda):
    """fast_cells_kernel stages its region with 32-bit row offsets (24-bit multiplies by the pitch): a level-0 pitch of
    2^24 bytes or more is a bad argument, returned before any launch."""
    import ctypes
    from openmavis_amd import _lib
    torch = torch_cuda
    w, h = 240, 180
    ex = ORBextractor(300, SCALE, NLEVELS, INI, MIN, width=w, height=h, max_images=1)
    cap = ex.max_keypoints()
    img = torch.zeros((h, w), dtype=torch.uint8, device="cuda")   # never read: the call returns on its arguments
    lap = np.zeros((1, 2), np.int32)
    kps = torch.zeros((1, cap, 6), dtype=torch.int32, device="cuda")
    desc = torch.zeros((1, cap, 32), dtype=torch.uint8, device="cuda")
    n_out = torch.zeros(1, dtype=torch.int32, device="cuda")
    mono = torch.zeros(1, dtype=torch.int32, device="cuda")
    for pitch, want in ((1 << 24, _lib.OMV_ERR_ARG), ((1 << 24) + 16, _lib.OMV_ERR_ARG)):
        st = ex._lib.omv_orb_extract_batch(ex._h, 1, _lib.ptr(img), ctypes.c_size_t(pitch * h), ctypes.c_size_t(pitch),
                                           _lib.ptr(lap), _lib.ptr(kps), _lib.ptr(desc), _lib.ptr(n_out),
                                           _lib.ptr(mono), None)
        assert st == want, (pitch, st)
