"""What the three live-memory GPU test files (tests/test_gpu_live_memory*.py) share: builders of device inputs and the comparisons of a
live object with one built fresh -- grids by their exported arrays and by the bytes every query sees, feature sets and results bit for
bit.  The worlds and edit sets are in tests/live_remove_cases.py and tests/live_replace_cases.py."""
import copy

import numpy as np
import torch

from tests.live_remove_cases import THR


def pts4_of(clouds, colors):
    from ibloc_amd.engine import intensity_from_colors
    from ibloc_amd.registration import CloudBatch
    return CloudBatch.from_numpy(clouds, [intensity_from_colors(c) for c in colors]).pts4


def pick(xs, idx):
    return [xs[i] for i in idx]


def queries(pts):
    """~4 000 query points: 3 600 around the points of `pts` (2 mm-1 cm off them) and 400 far from everything"""
    rng = np.random.default_rng(73)
    allp = np.concatenate(pts).astype(np.float32)
    near = allp[rng.choice(len(allp), 3600)] + rng.normal(0, 0.004, size=(3600, 3)).astype(np.float32)
    far = allp[rng.choice(len(allp), 400)] + np.array([0, 0, 25.0], dtype=np.float32)
    return np.concatenate([near, far]).astype(np.float32)


def point_distances(ctx, grid, q, thr=THR):
    from ibloc_amd.registration import evaluate_points
    q4 = torch.from_numpy(np.concatenate([q, np.zeros((len(q), 1), np.float32)], axis=1)).cuda().contiguous()
    d2, rmse, fit = evaluate_points(ctx, grid, q4, [0], [len(q)], np.eye(4)[None], thr)
    return d2.cpu().numpy(), float(rmse[0]), float(fit[0])


def exported(grid):
    return {k: v.cpu().numpy() for k, v in grid.export().items()}


def grid_state(ctx, grid, q, thr=THR):
    """everything a refused call must leave alone"""
    return grid.info(), {k: v.tobytes() for k, v in exported(grid).items()}, point_distances(ctx, grid, q, thr)[0].tobytes()


def assert_same_grid(ctx, live, fresh, q, thr=THR):
    a, b = live.info(), fresh.info()
    assert (a["n"], a["n_cells"], a["table_slots"]) == (b["n"], b["n_cells"], b["table_slots"]), (a, b)
    assert a["ustart_end"] == a["n"] == b["ustart_end"]
    ea, eb = exported(live), exported(fresh)
    for name in ("sorted", "ukeys", "ustart"):
        assert ea[name].shape == eb[name].shape and ea[name].tobytes() == eb[name].tobytes(), name
    assert ea["sorted"].shape == (a["n"], 4) and ea["ukeys"].shape == (a["n_cells"],) and ea["ustart"][-1] == a["n"]
    da, rmse_a, fit_a = point_distances(ctx, live, q, thr)
    db, rmse_b, fit_b = point_distances(ctx, fresh, q, thr)
    assert np.array_equal(np.isinf(da), np.isinf(db))
    assert da.tobytes() == db.tobytes()
    assert (rmse_a, fit_a) == (rmse_b, fit_b)
    return da


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_features(fa, fb, n, n_seg, compact):
    assert (fa.fpfh_split is None) == compact == (fb.fpfh_split is None)
    assert (fa.n, fa.n_seg) == (fb.n, fb.n_seg) == (n, n_seg)
    for name in ("normals", "fpfh", "fpfh_split", "fpfh_norm", "grad"):
        a, b = getattr(fa, name), getattr(fb, name)
        assert same_bits(None if a is None else a[:n], None if b is None else b[:n]), name
        assert a is None or a.shape[0] == n, name
    assert fa.grad is not None
    assert same_bits(fa.bbox[:n_seg], fb.bbox[:n_seg])
    assert (fa.voxel_size, fa.grad_radius) == (fb.voxel_size, fb.grad_radius)


def frame_of(w, rng, ids):
    """a query frame that sees exactly the objects `ids` (SynthWorld.make_frame picks an anchor's neighbours: here they are given)"""
    seen = copy.copy(w)
    seen.neighbours = lambda anchor, q: list(ids)
    return seen.make_frame(rng, q=len(ids), pts_per_object=800, anchor=ids[0])


def run_frames(eng, frames):
    from ibloc_amd.engine import intensity_from_colors
    from ibloc_amd.registration import CloudBatch
    det = CloudBatch.from_numpy([c[0] for f in frames for c in f["clouds"]], [intensity_from_colors(c[1]) for f in frames for c in f["clouds"]])
    return eng.localise_batch(det, [len(f["ids"]) for f in frames], det_emb=np.concatenate([f["det_emb"] for f in frames]),
                              fpfh_voxel_size=0.05, fpfh_global_dist_factor=1.5, fpfh_local_dist_factor=1.5, seed=7)


def assert_same_results(ra, rb):
    assert len(ra) == len(rb)
    for a, b in zip(ra, rb):
        assert a.assignments == b.assignments and a.best == b.best and a.n_clean == b.n_clean
        assert a.pose.tobytes() == b.pose.tobytes() and a.pose_corrected.tobytes() == b.pose_corrected.tobytes()
        assert len(a.records) == len(b.records)
        for x, y in zip(a.records, b.records):
            assert x["fitness"] == y["fitness"] and x["rmse"] == y["rmse"]
            assert x["full_fitness"] == y["full_fitness"] and x["full_rmse"] == y["full_rmse"]
            assert x["T"].tobytes() == y["T"].tobytes() and x["T_global"].tobytes() == y["T_global"].tobytes()
