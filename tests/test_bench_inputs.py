"""bench.py's inputs and --dump-outputs on the CPU: the generators are seeded (same calls, same data) and keep SynthWorld's geometry;
the dump holds one float64 array per output of the step."""
import os

import numpy as np
import torch

import bench


def test_crops_are_seeded_and_shaped():
    ids = [3, 7, 3]
    a = bench.Crops("dinov2_vitb14", 21).variants(ids, np.random.default_rng(5), "cpu")
    b = bench.Crops("dinov2_vitb14", 21).variants(ids, np.random.default_rng(5), "cpu")
    assert a.shape == (3, 224, 224, 3) and a.dtype == torch.uint8 and a.is_contiguous() and torch.equal(a, b)
    assert not torch.equal(a[0], a[2])                         # two noisy views of one instance
    assert (a[0].float() - a[2].float()).abs().mean() < 12      # ... of the same pattern (noise sigma 0.03 * 255)
    rgb, dep = bench.Crops("dator", 21).variants(ids, np.random.default_rng(5), "cpu")
    assert rgb.shape == (3, 256, 128, 3) and dep.shape == (3, 64, 32) and dep.dtype == torch.float32
    assert 0.2 < float(dep.min()) and float(dep.max()) < 8.1


def test_device_world_is_seeded_and_keeps_synthworld_geometry():
    w = bench.DeviceWorld(20, "cpu", pts_per_object=500, E=2, D=16, seed=3)
    w2 = bench.DeviceWorld(20, "cpu", pts_per_object=500, E=2, D=16, seed=3)
    assert len(w.points) == 20 and all(p.shape == (500, 3) for p in w.points) and w.embeddings.shape == (20, 2, 16)
    assert all(np.array_equal(p, q) for p, q in zip(w.points, w2.points))
    for p, c, o in zip(w.points, w.colors, w.centers):
        assert np.linalg.norm(p - o, axis=1).max() < 0.16 * 3 ** 0.5 + 0.3 * 3 ** 0.5 + 0.02     # primitive centre + half extent
        assert c.min() >= 0.0 and c.max() <= 1.0
    f = w.frame(np.random.default_rng(1), q=7)
    assert f["ids"] == bench.SynthWorld.neighbours(w, f["ids"][0], 7) and f["pose"].shape == (4, 4)
    assert np.allclose(f["pose"][:3, :3] @ f["pose"][:3, :3].T, np.eye(3)) and np.all((0.6 <= f["frac"]) & (f["frac"] <= 0.9))


def test_dump_outputs_writes_every_field_as_float64(tmp_path):
    from ibloc_amd.engine import FrameResult
    rec = dict(assn=[(0, 4)], T=np.eye(4), rmse=0.01, fitness=0.9, full_rmse=0.02, full_fitness=0.8, T_global=np.eye(4),
               detected_mean=np.zeros(3), memory_mean=np.ones(3), ransac_stats=np.array([5, 6, 7]))
    res = [FrameResult(np.arange(7.0), np.arange(7.0) + 1, [[(0, 4)], [(0, 4), (1, 5)]], [rec, rec], 1, 4900),
           FrameResult(np.zeros(7), np.zeros(7))]
    bench.dump_outputs(str(tmp_path), res)
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["pose"].shape == (2, 7) and got["best"].tolist() == [1, -1] and got["n_clean"].tolist() == [4900, 0]
    assert got["assignments"].shape == (2, 2, 2, 2) and got["assignments"][0, 1].tolist() == [[0, 4], [1, 5]]
    assert (got["assignments"][1] == -1).all() and np.isnan(got["record_rmse"][1]).all()
    assert got["record_T"].shape == (2, 2, 4, 4) and got["record_ransac_stats"][0, 0].tolist() == [5, 6, 7]
