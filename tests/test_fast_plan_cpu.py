"""The host plan of the extraction kernels' bookkeeping (openmavis_amd/csrc/fast_plan.h) without a GPU: the real C++ as a
stand-alone program built with -fsanitize=address,undefined (tests/cpp/fast_plan_host.cpp), run once on the pyramids
below.  For every cell and every prefilter slot the table equals a numpy restatement of the closed forms the kernel
evaluated per round before the table (r, jq, q0, klo, khi, j); over a cell's slots the kept columns cover the detection
window exactly once; describe's Toeplitz operands equal the shift expression they replace."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the smallest shapes of tests/test_orb_gpu.py for the dword path, the byte path and the per-cell stride, and the two
# camera shapes of the benchmarks
SHAPES = [(320, 240), (333, 250), (248, 250), (720, 540), (752, 480)]
# the LDS row stride the shapes reach: the 17-dword one, the per-cell one (248x250: a 68-px cell column at level 5), and
# the 13-dword one of the camera shapes
FAST_RS = {(320, 240): 68, (333, 250): 68, (248, 250): 0, (720, 540): 52, (752, 480): 52}
NLEVELS, SCALE = 8, 1.2
CELL_FIELDS = ["level", "y0", "y1", "x0", "x1", "o", "nd", "rpi", "mnd", "ndet", "mdw", "jq0", "npr", "np", "slot_off", "nband"]


def _levels(w, h):
    """Level sizes as the ORBextractor constructor rounds them (mvScaleFactor in float from a double product)."""
    s, out = np.float32(1), []
    for _ in range(NLEVELS):
        inv = np.float32(1) / s
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
        s = np.float32(float(s) * SCALE)
    return out


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """Per shape (fast_rs, table entries, [(cell dict, slots (n, 2) uint32)]), and the Toeplitz words, from one run."""
    assert shutil.which("g++") is not None
    exe = str(tmp_path_factory.mktemp("fast_plan") / "fast_plan_host")
    src = os.path.join(ROOT, "tests", "cpp", "fast_plan_host.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    text = "\n".join(" ".join(f"{w} {h}" for w, h in _levels(*s)) for s in SHAPES) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out, geoms, bop = r.stdout.strip().split("\n"), [], None
    i = 0
    while i < len(out):
        tok = out[i].split()
        if tok[0] == "bop":
            bop = np.array([int(t, 16) for t in tok[1:]], np.uint64)
            i += 1
            continue
        assert tok[0] == "geom"
        n_cells, fast_rs, n_table = int(tok[1]), int(tok[2]), int(tok[3])
        cells = []
        for k in range(n_cells):
            c = out[i + 1 + 2 * k].split()
            s = out[i + 2 + 2 * k].split()
            assert c[0] == "cell" and s[0] == "slots"
            sl = np.array(s[2:], np.int64).astype(np.uint32).reshape(-1, 2)
            assert len(sl) == int(s[1])
            cells.append((dict(zip(CELL_FIELDS, map(int, c[1:]))), sl))
        geoms.append((fast_rs, n_table, cells))
        i += 1 + 2 * n_cells
    assert len(geoms) == len(SHAPES) and bop is not None and len(bop) == 256
    return dict(zip(SHAPES, geoms)), bop


def _closed_forms(c, fast_rs):
    """What the kernel derived per round from the rectangle: per slot tp the row r, the first dword jq of the pair, its
    column q0, the kept columns [klo, khi) and the LDS dword j; plus the cell constants they start from."""
    rw, rh = c["x1"] - c["x0"], c["y1"] - c["y0"]
    o = c["x0"] & 3
    nd = (rw + o + 3) >> 2
    rsw = fast_rs >> 2 if fast_rs else nd
    jq0, jq1 = (o + 3) >> 2, (o + rw - 4) >> 2
    npr = (jq1 - jq0 + 2) >> 1
    dw, dh = rw - 6, rh - 6
    np_ = npr * dh if dw > 0 and dh > 0 else 0
    tp = np.arange(np_)
    rr = tp // npr
    r = 3 + rr
    jq = jq0 + 2 * (tp - rr * npr)
    q0 = 4 * jq - o
    klo = np.minimum(np.maximum(3 - q0, 0), 8)
    khi = np.minimum(np.maximum(rw - 3 - q0, 0), 8)
    j = r * rsw + jq
    return dict(rw=rw, rh=rh, o=o, nd=nd, rsw=rsw, jq0=jq0, npr=npr, np=np_, r=r, jq=jq, q0=q0, klo=klo, khi=khi, j=j)


@pytest.mark.parametrize("shape", SHAPES)
def test_slot_table_equals_the_closed_forms(plans, shape):
    fast_rs, n_table, cells = plans[0][shape]
    assert len(cells) > 0
    max_rw = max(c["x1"] - c["x0"] for c, _ in cells)
    assert fast_rs == (52 if max_rw + 3 <= 52 else 68 if max_rw + 3 <= 68 else 0) == FAST_RS[shape]
    shared = {}
    for c, sl in cells:
        f = _closed_forms(c, fast_rs)
        for k in ("o", "nd", "jq0", "npr", "np"):
            assert c[k] == f[k], (c, k)
        n = f["np"]
        if n == 0:
            assert len(sl) == 0 and c["slot_off"] == 0
            continue
        assert len(sl) == (n + 63) // 64 * 64 + 64   # whole rounds and the spare one
        assert c["slot_off"] + len(sl) <= n_table
        lo, hi = sl[:n, 0].astype(np.int64), sl[:n, 1].astype(np.int64)
        mask = ((1 << f["khi"]) - 1) & ~((1 << f["klo"]) - 1)
        assert np.array_equal(lo & 0xffff, (f["r"] << 7) + f["q0"])
        assert np.array_equal(lo >> 16, mask)
        assert np.array_equal(hi, 4 * (f["j"] - 3 * f["rsw"]))
        # the padding keeps no column and reads what slot 0 reads
        assert (sl[n:, 0] == 0).all() and (sl[n:, 1] == sl[0, 1]).all()
        # the dwords a slot reads: the pair and its left / right neighbours in row r, the pair in rows r - 3 and r + 3.
        # They lie in the cell's staged rows, but for the second dword of a row's last pair, which may be the first
        # dword after the row (all its columns are masked): after the last row that is the dword behind the region
        idx = f["j"][:, None] + np.array([-1, 0, 1, 2, -3 * f["rsw"], -3 * f["rsw"] + 1, 3 * f["rsw"], 3 * f["rsw"] + 1])
        assert idx.min() >= 0 and idx.max() <= f["rh"] * f["rsw"]
        first = f["j"][:, None] + np.array([0, -3 * f["rsw"], 3 * f["rsw"]])
        assert first.max() < f["rh"] * f["rsw"]
        # cells of one shape share a run, and only those
        key = (f["rw"], f["rh"], f["o"])
        assert shared.setdefault(c["slot_off"], key) == key


@pytest.mark.parametrize("shape", SHAPES)
def test_kept_columns_cover_the_window_once(plans, shape):
    fast_rs, _, cells = plans[0][shape]
    for c, sl in cells:
        rw, rh = c["x1"] - c["x0"], c["y1"] - c["y0"]
        hits = np.zeros((rh, rw + 8), np.int32)
        for lo in sl[:, 0].astype(np.int64):
            e, m = lo & 0xffff, lo >> 16
            for k in range(8):
                if m >> k & 1:
                    hits[e >> 7, (e & 127) + k] += 1
        want = np.zeros_like(hits)
        if rw > 6 and rh > 6:
            want[3:rh - 3, 3:rw - 3] = 1
        assert np.array_equal(hits, want), c


def test_bop_table_equals_the_shift_expression(plans):
    bop = plans[1]
    g7 = 0x0012223038302212   # g[0..6] = 18, 34, 48, 56, 48, 34, 18 (byte i = g[i])
    for po in range(4):
        for lane in range(64):
            sb = 8 * (lane >> 4) - (lane & 15) - po
            want = 0 if abs(sb) >= 8 else g7 >> (8 * sb) if sb >= 0 else (g7 << (-8 * sb)) & (2 ** 64 - 1)
            assert int(bop[po * 64 + lane]) == want, (po, lane)
