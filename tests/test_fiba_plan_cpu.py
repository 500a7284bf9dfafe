"""The host plan of a FullInertialBA problem (openmavis_amd/csrc/lba_plan.h: plan_fiba), through a stand-alone program
built with -fsanitize=address,undefined (tests/cpp/fiba_plan_host.cpp, its own main): the shared bias pair as the last
block of the reduced system, the three-sided inertial work lists, and the problems the planner rejects."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OMV_OK, OMV_ERR_ARG = 0, 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++") is not None
    exe = str(tmp_path_factory.mktemp("fiba_plan") / "fiba_plan_host")
    src = os.path.join(ROOT, "tests", "cpp", "fiba_plan_host.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        out = {}
        for ln in r.stdout.strip().split("\n"):
            k, *v = ln.split()
            out[k] = [float(x) if "." in x else int(x) for x in v if x.lstrip("-").replace(".", "").isdigit()]
        return out

    return run


def _plan(host, K, fix_last=0, shared=1, no_imu_first=0, break_at=-1, lds_ok=1):
    p = host("plan", K, fix_last, shared, no_imu_first, break_at, lds_ok)
    assert p["status"] == [OMV_OK]
    nb, shared_blk, shared_kf, n_red, n_slots, n_lev, use_lds = p["scalars"]
    p.update(nb=nb, shared_blk=shared_blk, shared_kf=shared_kf, n_red=n_red, n_slots=n_slots, n_lev=n_lev, use_lds=use_lds)
    p["imu_blk"] = [tuple(p["imu_blk"][3 * i:3 * i + 3]) for i in range(len(p["imu_blk"]) // 3)]
    p["imu_vec"] = [tuple(p["imu_vec"][2 * i:2 * i + 2]) for i in range(len(p["imu_vec"]) // 2)]
    return p


@pytest.mark.parametrize("K,fix_last,no_imu_first,break_at", [(6, 0, 0, -1), (6, 1, 1, 3), (12, 1, 0, 6), (12, 0, 1, -1),
                                                              (40, 0, 0, 17), (3, 1, 0, -1)])
def test_shared_block(host, K, fix_last, no_imu_first, break_at):
    p = _plan(host, K, fix_last, 1, no_imu_first, break_at)
    n_opt = K - fix_last
    S = n_opt
    assert p["nb"] == n_opt + 1 and p["shared_blk"] == S and p["n_red"] == 16 * (n_opt + 1)
    assert p["shared_kf"] == (1 if no_imu_first else 0)
    # last in the elimination order, after a permutation of the keyframes
    assert p["perm"][-1] == S and sorted(p["perm"][:-1]) == list(range(n_opt))
    # adjacent to exactly the keyframes with inertial edges (the optimisable ones: a fixed keyframe has no block)
    with_edge = {k for k in p["imu_kf1"] + p["imu_kf2"] if k < n_opt}
    blocks = set(zip(p["slot_kr"], p["slot_kc"]))
    ipos = {k: q for q, k in enumerate(p["perm"])}
    assert all(ipos[r] >= ipos[c] for r, c in blocks)          # lower blocks in positions
    assert (S, S) in blocks
    # (its stored row may hold fill besides: a keyframe eliminated after a covisible one that has an inertial edge; the
    # adjacency itself is the blocks of its row that an inertial edge contributes to)
    row = {c for r, c in blocks if r == S and c != S}
    slots_ = list(zip(p["slot_kr"], p["slot_kc"]))
    fed = {slots_[t][1] for t in range(p["n_slots"]) if slots_[t][0] == S and slots_[t][1] != S
           and p["ib_start"][t + 1] > p["ib_start"][t]}
    assert fed == with_edge and with_edge <= row
    assert not any(c == S and r != S for r, c in blocks)
    # every bImu keyframe's bias rows are the pair's; its velocity rows its own; no random-walk information
    bimu = [0 if (no_imu_first and k == 0) else 1 for k in range(K)]
    assert p["offG"] == [16 * S + 9 if b else -1 for b in bimu] and p["offA"] == [16 * S + 12 if b else -1 for b in bimu]
    assert p["offV"] == [16 * k + 6 if (bimu[k] and k < n_opt) else -1 for k in range(K)]
    assert p["rw_info_zero"] == [1]
    # every inertial edge once per (block, side pair) it touches: sides 0 = kf1, 1 = kf2, 2 = the pair
    slots = list(zip(p["slot_kr"], p["slot_kc"]))
    want = []
    for e, (a, b) in enumerate(zip(p["imu_kf1"], p["imu_kf2"])):
        blk = {0: a if a < n_opt else None, 1: b if b < n_opt else None, 2: S}
        for sr in range(3):
            for sc in range(3):
                if blk[sr] is None or blk[sc] is None or ipos[blk[sr]] < ipos[blk[sc]]:
                    continue
                want.append((slots.index((blk[sr], blk[sc])), e, sr, sc))
    got = [(t, *p["imu_blk"][q]) for t in range(p["n_slots"]) for q in range(p["ib_start"][t], p["ib_start"][t + 1])]
    assert sorted(got) == sorted(want) and len(set(got)) == len(got)
    assert p["ib_start"][-1] == len(p["imu_blk"])
    for t in range(p["n_slots"]):   # in edge order within a block: the sums' fixed order
        es = [p["imu_blk"][q] for q in range(p["ib_start"][t], p["ib_start"][t + 1])]
        assert es == sorted(es)
    wantv = sorted((blk, e, sd) for e, (a, b) in enumerate(zip(p["imu_kf1"], p["imu_kf2"]))
                   for sd, blk in ((0, a), (1, b), (2, S)) if sd == 2 or blk < n_opt)
    gotv = sorted((k, *p["imu_vec"][q]) for k in range(p["nb"]) for q in range(p["iv_start"][k], p["iv_start"][k + 1]))
    assert gotv == wantv
    assert len(p["rhs_start"]) == p["nb"] + 1 and p["rhs_start"][-1] == p["rhs_start"][-2]   # no landmark record of the pair


def test_per_keyframe_form_is_the_local_plan(host):
    """shared_bias == 0: no extra block, two-sided work lists, random-walk informations present."""
    p = _plan(host, 8, 1, 0)
    assert p["nb"] == 7 and p["shared_blk"] == -1 and p["shared_kf"] == -1 and sorted(p["perm"]) == list(range(7))
    assert all(sr < 2 and sc < 2 for _, sr, sc in p["imu_blk"]) and p["rw_info_zero"] == [0]
    assert p["offG"] == [16 * k + 9 for k in range(7)] + [-1]


def test_dissection_without_the_pair(host):
    """A chain of 40 keyframes: the keyframes are cut in two although the pair borders them all (levels well under 41)."""
    p = _plan(host, 40)
    assert p["n_lev"] <= 24, p["n_lev"]


@pytest.mark.parametrize("shared", [1, 0])
def test_whole_map_orders_past_the_lds_budget(host, shared):
    """100 keyframes do not fit the solver's LDS (hybrid storage): the budget then does not choose among the orders, and the
    keyframes are still cut in two, in either bias form."""
    p = _plan(host, 100, 0, shared)
    assert p["use_lds"] == 2 and p["n_lev"] <= 54, (p["use_lds"], p["n_lev"])


@pytest.mark.parametrize("K", [6, 12, 40])
def test_global_scratch_storage_with_the_pair(host, K):
    """Without the solver's LDS attribute (use_lds == 0, every block in global scratch) the pattern, the order and the
    level schedule with the pair's block are those of the LDS modes: the solver runs one schedule in three storages."""
    a, b = _plan(host, K, 1, 1, 0, -1, 1), _plan(host, K, 1, 1, 0, -1, 0)
    assert b["use_lds"] == 0 and b["storage"] == [b["n_slots"], 0, 0]   # n_lds = all (unused), no staged schedule, no LDS
    assert a["use_lds"] in (1, 2)
    for k in ("perm", "slot_kr", "slot_kc", "lev_start", "imu_blk", "imu_vec", "ib_start", "iv_start", "nb", "n_lev", "n_slots"):
        assert a[k] == b[k], k
    assert b["perm"][-1] == b["shared_blk"]


def test_a_landmark_past_32_keyframes_is_a_group_of_its_own(host):
    """kGrpW = 32 optimisable keyframes per build group: a landmark on 40 keyframes goes to the one-landmark path
    (build_big_kernel), one on 30 does not."""
    assert host("big", 40)["n_big"] == [1] and host("big", 40)["kGrpW"] == [32]
    assert host("big", 30)["n_big"] == [0]


def test_rejected_problems(host):
    r = host("reject")
    assert r["no_imu_kf"] == [OMV_ERR_ARG] and r["no_imu_kf_per_kf_form"] == [OMV_OK]
    assert r["no_imu_edge"] == [OMV_ERR_ARG] and r["edge_on_non_imu"] == [OMV_ERR_ARG]
    assert r["negative_prior_g"] == [OMV_ERR_ARG] and r["negative_prior_a"] == [OMV_ERR_ARG] and r["nan_prior"] == [OMV_ERR_ARG]
    assert r["negative_prior_unread"] == [OMV_OK]
    assert r["over_capacity"] == [OMV_ERR_ARG]
    assert r["many_imu_edges"] == [OMV_OK] and r["over_max_imu"] == [OMV_ERR_ARG]   # 299 edges: the capacity decides


def test_bounded_cuts_plan_within_a_few_levels(host):
    """The whole-map entry tries at most 32 evenly spaced cuts: on a chain of 200 keyframes it finds a dissection within
    five levels of the best of all 199 cuts, which is about half the chain."""
    t = host("time", 200)
    assert t["every_cut"][0] == OMV_OK and t["bounded"][0] == OMV_OK
    n_lev_all, n_lev_bounded = t["every_cut"][3], t["bounded"][3]
    assert n_lev_all <= 104 and n_lev_all <= n_lev_bounded <= n_lev_all + 5, (n_lev_all, n_lev_bounded)
