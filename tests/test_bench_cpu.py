"""bench.py's accounting on the CPU: the matching kernels' algorithmic bytes split SURVEY §8(d)'s 968,000 B per
multi-camera frame exactly (no design-internal candidate records counted), and the extraction formula gives §8(d)'s
2,085,018 B per Hilti camera-frame.  Also the plain / --full switch and the --dump-outputs writer on host tensors."""
import bench


def test_matching_bytes_split_survey_8d():
    B, n_kp = 10, 10 * 5 * 1200   # the nominal 1200 keypoints per camera of §8(d)
    P = [a * b for a, b in bench.level_sizes(bench.W, bench.H)]
    b = bench.per_step_algorithmic_bytes(B, P, n_kp, 0)
    matching = sum(b[k] for k in ("grid", "stereo_knn", "proj_candidates", "proj_resolve"))
    assert matching == B * 968_000
    assert set(b) == set(bench.BYTES_FORMULA)


def test_extraction_bytes_survey_8d():
    assert bench.cam_bytes(720, 540, 1200) == 2_085_018
    assert bench.cam_bytes(1920, 1080, 2000) == 10_877_042


def test_plain_run_switches_every_secondary_leg_off():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)
    assert a.no_cpu_baseline
    legs = ("parity_check", "iso_reps", "latency_frames", "p1080_frames", "shard_frames", "lba_steps", "pose_frames",
            "tri_pairs", "aux")
    assert all(getattr(a, k) == 0 for k in legs)
    f = bench.parse_args(["--full", "--steps", "7", "--lba-steps", "3"])
    assert f.full and f.steps == 7 and not f.no_cpu_baseline and f.lba_steps == 3
    assert all(getattr(f, k) > 0 for k in legs)


def test_dump_outputs_sample_and_padding(tmp_path):
    """Two groups of 6 frames, 2 cameras, capacity 4: the seeded 8-frame sample, float32 files, per-frame counts for
    every frame, padding slots past n_kp stored as 0 / -1 and the octave stored as a number."""
    import types

    import numpy as np
    import torch
    Bg, C, cap, M, G = 6, 2, 4, 3, 2
    rng = np.random.default_rng(1)
    groups = []
    for g in range(G):
        fb = types.SimpleNamespace(
            kps=torch.from_numpy(rng.standard_normal((Bg, C, cap, 6)).astype(np.float32).view(np.int32)),
            desc=torch.from_numpy(rng.integers(1, 256, (Bg, C, cap, 32), dtype=np.uint8)),
            n_kp=torch.from_numpy(rng.integers(0, cap + 1, (Bg, C), dtype=np.int32)),
            mono=torch.zeros((Bg, C), dtype=torch.int32),
            l2r=torch.from_numpy(rng.integers(0, cap, (Bg, cap), dtype=np.int32)),
            r2l=torch.from_numpy(rng.integers(0, cap, (Bg, cap), dtype=np.int32)),
            kp_to_mp=torch.from_numpy(rng.integers(-1, M, (Bg, C * cap), dtype=np.int32)),
            n_matches=torch.full((Bg,), g, dtype=torch.int32))
        fb.kps[..., 5] = 3   # octave: an int32 in the record's last word
        mps = types.SimpleNamespace(**{k: torch.from_numpy(rng.standard_normal((Bg, M, C)).astype(np.float32))
                                       for k in ("proj_x", "proj_y", "view_cos", "level", "in_view", "track_depth")})
        groups.append(dict(fb=fb, mps=mps, uright=torch.from_numpy(rng.random((Bg, C, cap)).astype(np.float32))))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), groups, Bg)
    out = {f.name[:-4]: np.load(f) for f in (tmp_path / "a").iterdir()}
    assert all(v.dtype == np.float32 for v in out.values())
    assert all(np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy"))) for k, v in out.items())
    sel = out["frames"].astype(int)
    assert len(sel) == bench.DUMP_FRAMES and len(set(sel)) == len(sel) and (np.diff(sel) > 0).all() and sel.max() < G * Bg
    assert out["n_kp"].shape == (G * Bg, C) and np.array_equal(out["n_matches"], np.repeat([0.0, 1.0], Bg))
    for i, f in enumerate(sel):
        fb = groups[f // Bg]["fb"]
        for c in range(C):
            n = int(fb.n_kp[f % Bg, c])
            want = fb.kps[f % Bg, c, :n].numpy().view(np.float32).copy()
            want[:, 5] = 3.0
            assert np.array_equal(out["kps"][i, c, :n], want) and not out["kps"][i, c, n:].any()
            assert np.array_equal(out["desc"][i, c, :n], fb.desc[f % Bg, c, :n].numpy()) and not out["desc"][i, c, n:].any()
            assert np.array_equal(out["uright"][i, c, :n], groups[f // Bg]["uright"][f % Bg, c, :n].numpy())
            assert (out["uright"][i, c, n:] == -1).all()
        n0, n1 = int(fb.n_kp[f % Bg, 0]), int(fb.n_kp[f % Bg, 1])
        assert np.array_equal(out["l2r"][i, :n0], fb.l2r[f % Bg, :n0].numpy()) and (out["l2r"][i, n0:] == -1).all()
        assert np.array_equal(out["r2l"][i, :n1], fb.r2l[f % Bg, :n1].numpy()) and (out["r2l"][i, n1:] == -1).all()
        assert np.array_equal(out["kp_to_mp"][i], fb.kp_to_mp[f % Bg].numpy())
        assert np.array_equal(out["proj_x"][i], groups[f // Bg]["mps"].proj_x[f % Bg].numpy())
