"""The sorted insertion of the candidate lists (openmavis_amd/csrc/omv_topk.h) without a GPU: the real C++ as a
stand-alone program built with -fsanitize=address,undefined (tests/cpp/topk_host.cpp), run once on the sequences below.
After every insert the 16-slot list equals the 16 smallest keys seen so far, ascending, padded with ~0u."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 16
EMPTY = 0xFFFFFFFF


def _unique(rng, n):
    """n different keys below ~0u, in random order."""
    keys = np.unique(rng.integers(0, EMPTY, 2 * n, dtype=np.uint64))
    assert len(keys) >= n
    return rng.permutation(keys)[:n].tolist()


def _sequences():
    rng = np.random.default_rng(5)
    seq = {}
    seq["random"] = _unique(rng, 200)
    seq["ascending"] = sorted(_unique(rng, 40))
    seq["descending"] = sorted(_unique(rng, 40), reverse=True)   # every insert shifts the whole list
    seq["equal_distance_ascending_p"] = [(57 << 16) | p for p in range(3, 3 + 40)]
    seq["fewer_than_16"] = _unique(rng, 9)
    seq["exactly_16"] = _unique(rng, 16)
    seq["seventeen"] = _unique(rng, 17)
    seq["thousand"] = _unique(rng, 1000)
    # the keys the kernel builds: distance << 16 | position, few distances, so that most keys tie on the distance
    seq["kernel_keys"] = [(int(d) << 16) | int(p) for d, p in zip(rng.integers(0, 257, 300), rng.permutation(65536)[:300])]
    seq["extremes"] = [EMPTY - 1, 0, 1, EMPTY - 2]
    seq["empty"] = []
    return seq


@pytest.fixture(scope="module")
def lists(tmp_path_factory):
    """Per sequence (the keys, the list after every insert [n][16]), from one run of the program."""
    assert shutil.which("g++") is not None
    exe = str(tmp_path_factory.mktemp("topk") / "topk_host")
    src = os.path.join(ROOT, "tests", "cpp", "topk_host.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    seq = _sequences()
    text = "".join(" ".join(map(str, s)) + "\n" for s in seq.values())
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out, blocks, cur = r.stdout.strip().split("\n"), [], []
    for line in out:
        if line == "end":
            blocks.append(cur)
            cur = []
        else:
            cur.append([int(t, 16) for t in line.split()])
    assert cur == [] and len(blocks) == len(seq)
    return {name: (s, b) for (name, s), b in zip(seq.items(), blocks)}


@pytest.mark.parametrize("name", list(_sequences()))
def test_list_after_every_insert(lists, name):
    keys, got = lists[name]
    assert len(got) == len(keys)
    assert len(set(keys)) == len(keys) and EMPTY not in keys   # the header's precondition
    seen = []
    for i, k in enumerate(keys):
        seen.append(k)
        want = sorted(seen)[:K]
        want += [EMPTY] * (K - len(want))
        assert got[i] == want, (name, i)


def test_sequences_are_what_they_claim(lists):
    s = {n: v[0] for n, v in lists.items()}
    assert s["ascending"] == sorted(s["ascending"]) and s["descending"] == sorted(s["descending"], reverse=True)
    assert len({k >> 16 for k in s["equal_distance_ascending_p"]}) == 1
    assert [k & 0xFFFF for k in s["equal_distance_ascending_p"]] == sorted(k & 0xFFFF for k in s["equal_distance_ascending_p"])
    assert len(s["fewer_than_16"]) < K and len(s["exactly_16"]) == K and len(s["seventeen"]) == K + 1
    assert len(s["thousand"]) == 1000 and len(s["ascending"]) > K and len(s["descending"]) > K
    assert s["random"] != sorted(s["random"]) and s["random"] != sorted(s["random"], reverse=True)
