"""The host plan of a pose graph (openmavis_amd/csrc/essgraph_plan.h over lba_plan.h), through the stand-alone program
tests/cpp/essgraph_plan_host.cpp (its own main): every contribution lands in exactly one stored block, the level
schedule respects the elimination tree, the planner's rejections, the planning time of a 1,000-vertex graph, and the same
program clean under -fsanitize=address,undefined (host code only, run directly)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OMV_OK, OMV_ERR_ARG = 0, 1
SIM3, DOF4 = 0, 1
# planning a 1,000-vertex Sim3 graph (500 blocks, 2,981 stored blocks, 32 cuts) measured 16 ms on the build machine
# (DESIGN 6); the bar is ten times that, for machine noise
PLAN_MS_1000 = 16.0


def _build(tmp, sanitize):
    assert shutil.which("g++") is not None
    exe = str(tmp / ("essgraph_plan_host" + ("_san" if sanitize else "")))
    src = os.path.join(ROOT, "tests", "cpp", "essgraph_plan_host.cpp")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        out = {}
        for ln in r.stdout.strip().split("\n"):
            k, *v = ln.split()
            out[k] = [float(x) if "." in x else int(x) for x in v]
        return out

    return run


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("essgraph_plan"), False)


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("essgraph_plan_san"), True)


def _plan(run, kind, n, lds_ok=1, n_fixed=1, offs=()):
    p = run("plan", kind, n, lds_ok, n_fixed, *offs)
    assert p["status"] == [OMV_OK]
    for k, v in zip(("dim", "per_blk", "n_opt", "nb", "n_red", "n_slots", "n_lev", "use_lds", "n_lds", "blob_ints"), p["scalars"]):
        p[k] = v
    p["cb"] = [tuple(p["cb"][4 * i:4 * i + 4]) for i in range(len(p["cb"]) // 4)]
    p["cv"] = [tuple(p["cv"][4 * i:4 * i + 4]) for i in range(len(p["cv"]) // 4)]
    return p


def _check(p):
    dim, per, nb = p["dim"], p["per_blk"], p["nb"]
    assert (dim, per) in ((7, 2), (4, 4))
    opt = [v for v, f in enumerate(p["fixed"]) if not f]
    assert p["opt_v"] == opt and p["n_opt"] == len(opt) and nb == (len(opt) + per - 1) // per and p["n_red"] == 16 * nb
    # optimisable vertices packed in caller order; pad rows flagged
    for o, v in enumerate(opt):
        assert p["row_of"][v] == 16 * (o // per) + dim * (o % per)
    assert all(p["row_of"][v] == -1 for v, f in enumerate(p["fixed"]) if f)
    real = [0] * (16 * nb)
    for v in opt:
        for r in range(dim):
            real[p["row_of"][v] + r] = 1
    assert p["real_row"] == real
    # stored blocks: lower in positions, every diagonal one present, no duplicates
    ipos = {k: q for q, k in enumerate(p["perm"])}
    assert sorted(p["perm"]) == list(range(nb))
    slots = list(zip(p["slot_kr"], p["slot_kc"]))
    assert len(set(slots)) == len(slots) == p["n_slots"] and all(ipos[r] >= ipos[c] for r, c in slots)
    assert all((k, k) in slots for k in range(nb))
    # every contribution in exactly one stored block, the right one, in edge order
    want = []
    for e, (i, j) in enumerate(zip(p["edge_i"], p["edge_j"])):
        rows = (p["row_of"][i], p["row_of"][j])
        for sr in range(2):
            for sc in range(2):
                if rows[sr] < 0 or rows[sc] < 0:
                    continue
                br, bc = rows[sr] // 16, rows[sc] // 16
                if ipos[br] < ipos[bc]:
                    continue
                want.append((slots.index((br, bc)), e, sr, sc, 16 * (rows[sr] % 16) + rows[sc] % 16))
    got = [(t, *p["cb"][q]) for t in range(p["n_slots"]) for q in range(p["cb_start"][t], p["cb_start"][t + 1])]
    assert sorted(got) == sorted(want) and len(set(got)) == len(got) and p["cb_start"][-1] == len(p["cb"])
    for t in range(p["n_slots"]):
        es = [p["cb"][q] for q in range(p["cb_start"][t], p["cb_start"][t + 1])]
        assert es == sorted(es)   # the sums' fixed order
    # both triangles of a pair sharing a diagonal block are fed, an off-diagonal pair once
    by_pair = {}
    for t, e, sr, sc, _ in got:
        by_pair.setdefault(e, []).append((sr, sc))
    for e, (i, j) in enumerate(zip(p["edge_i"], p["edge_j"])):
        ri, rj = p["row_of"][i], p["row_of"][j]
        n_want = 0 if (ri < 0 and rj < 0) else 1 if (ri < 0 or rj < 0) else 4 if ri // 16 == rj // 16 else 3
        assert len(by_pair.get(e, [])) == n_want, e
    wantv = sorted((r // 16, e, sd, r % 16, 0) for e, (i, j) in enumerate(zip(p["edge_i"], p["edge_j"]))
                   for sd, r in ((0, p["row_of"][i]), (1, p["row_of"][j])) if r >= 0)
    gotv = sorted((k, *p["cv"][q]) for k in range(nb) for q in range(p["cv_start"][k], p["cv_start"][k + 1]))
    assert gotv == wantv
    # the level schedule: every column once; a stored block (i, k) below the diagonal puts i on a higher level than k
    level = {}
    for l in range(p["n_lev"]):
        for c in p["lev_col"][p["lev_start"][l]:p["lev_start"][l + 1]]:
            assert c not in level
            level[c] = l
    assert sorted(level) == list(range(nb))
    assert all(level[ipos[r]] > level[ipos[c]] for r, c in slots if r != c)
    # the adjacency of the graph is stored (fill comes on top)
    for i, j in zip(p["edge_i"], p["edge_j"]):
        ri, rj = p["row_of"][i], p["row_of"][j]
        if ri >= 0 and rj >= 0:
            a, b = ri // 16, rj // 16
            assert (a, b) in slots or (b, a) in slots


@pytest.mark.parametrize("kind,n,n_fixed,offs", [(SIM3, 6, 1, ()), (DOF4, 6, 1, ()), (SIM3, 40, 1, (2, 3)), (DOF4, 41, 1, (2, 3)),
                                                 (SIM3, 24, 3, (2, 5)), (SIM3, 200, 1, (2, 3, 7)), (DOF4, 7, 2, (3,))])
def test_contributions_and_schedule(host, kind, n, n_fixed, offs):
    _check(_plan(host, kind, n, 1, n_fixed, offs))


def test_storage_modes(host):
    small, big = _plan(host, SIM3, 40, 1, 1, (2, 3)), _plan(host, SIM3, 200, 1, 1, (2, 3, 7))
    assert small["use_lds"] == 1 and small["n_lds"] == small["n_slots"] and small["n_lev"] < small["nb"]   # dissected
    assert big["use_lds"] == 2 and 0 < big["n_lds"] < big["n_slots"]                                       # hybrid
    g = _plan(host, SIM3, 40, 0, 1, (2, 3))
    assert g["use_lds"] == 0 and g["blob_ints"] == 0
    for k in ("perm", "slot_kr", "slot_kc", "lev_start", "lev_col", "cb", "cb_start"):
        assert g[k] == small[k] or k == "perm" and sorted(g[k]) == sorted(small[k])
    # the last Sim3 block of five optimisable vertices is half padding
    a = _plan(host, SIM3, 6)
    assert a["nb"] == 3 and a["real_row"][32:48] == [1] * 7 + [0] * 9 and a["real_row"][:16] == [1] * 14 + [0, 0]
    d = _plan(host, DOF4, 6)
    assert d["nb"] == 2 and d["real_row"] == [1] * 16 + [1] * 4 + [0] * 12


def test_rejected_problems(host):
    r = host("reject")
    assert r["ok"] == [OMV_OK] and r["no_edges"] == [OMV_OK]
    for k in ("vertex_out_of_range", "negative_vertex", "self_edge", "bad_table", "all_fixed", "over_max_vertices",
              "over_max_edges", "bad_kind", "null_fixed"):
        assert r[k] == [OMV_ERR_ARG], k


def test_a_thousand_vertices_plan_in_time(host):
    best = min(host("time", SIM3, 1000)["plan_ms"][0] for _ in range(3))
    t = host("time", SIM3, 1000)
    assert t["status"] == [OMV_OK] and t["scalars"][0] == 500 and t["scalars"][3] == 2
    print(f"1,000-vertex Sim3 graph planned in {best:.1f} ms")
    assert best <= 10 * PLAN_MS_1000


def test_clean_under_the_sanitizers(host_san, host):
    for args in (("plan", SIM3, 40, 1, 1, 2, 3), ("plan", DOF4, 41, 1, 2, 2, 3), ("plan", SIM3, 200, 1, 1, 2, 3, 7),
                 ("plan", SIM3, 6, 0, 1), ("reject",), ("time", DOF4, 300)):
        a = host_san(*args)
        if args[0] == "plan":
            assert a == host(*args)
