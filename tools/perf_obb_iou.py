"""Cost of the oriented-box IoU matrix of memory consolidation (ObjectMemory._recluster_IoU, iou_backend="device") on a synthetic
memory of N fragments (ibloc_amd.synth.fragment_scene), against the host pair loop it replaces.

    python tools/perf_obb_iou.py N [--seed S] [--threads T] [--host-pairs P] [--no-e2e]

Prints one JSON line: boxes_s (N oriented boxes on host threads), matrix_s (ibl_obb_iou_matrix, median of 3 after a warm-up),
d2h_s (the n x n float64 matrix to the host), sklearn_s (the AgglomerativeClustering call of _recluster_IoU), overlapping_pairs (pairs
past the separating-axis test), host_pair_ms (1 - calculate_obj_aligned_3d_IoU per pair over a sample: half uniform pairs, half
fragments of one object), host_loop_extrapolated_s (the uniform cost for the separated pairs + the same-object cost for the overlapping
ones, over all N (N - 1) / 2 pairs), host_sample_max_abs_diff (device against host on the sample) and e2e_recluster_s: one whole
ObjectMemory._recluster_IoU(0.3) with the device backend (boxes, matrix, copy, clustering, merge).  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threads", type=int, default=None, help="box threads (default: the pool's 16)")
    ap.add_argument("--host-pairs", type=int, default=2000, help="host-loop sample (0 = skip)")
    ap.add_argument("--no-e2e", dest="e2e", action="store_false", help="skip the whole _recluster_IoU call")
    a = ap.parse_args()

    import torch
    from sklearn.cluster import AgglomerativeClustering
    from ibloc_amd.build import obb_iou_matrix
    from ibloc_amd.registration import RegContext
    from ibloc_amd.synth import fragment_scene
    from ibloc_amd.utils.IoU_ops import calculate_obj_aligned_3d_IoU, oriented_bounding_boxes
    if not torch.cuda.is_available():
        raise SystemExit("perf_obb_iou.py measures the device matrix: no GPU here")

    clouds, owner = fragment_scene(a.n, seed=a.seed)
    out = {"n": a.n, "points_mean": float(np.mean([len(c) for c in clouds])), "objects": int(owner.max() + 1)}
    t = time.perf_counter()
    boxes, valid = oriented_bounding_boxes(clouds, threads=a.threads)
    out["boxes_s"] = time.perf_counter() - t
    out["box_threads"] = a.threads or 16
    ctx = RegContext(64 << 20)
    B = torch.from_numpy(boxes).cuda()
    V = torch.from_numpy(valid).cuda()
    D, n_ov = obb_iou_matrix(ctx, B, V, return_overlapping=True)        # warm-up (code object load)
    del D
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        D = obb_iou_matrix(ctx, B, V)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    out["matrix_s"] = float(np.median(times))
    out["matrix_s_all"] = times
    out["overlapping_pairs"] = n_ov
    t = time.perf_counter()
    Dh = D.cpu().numpy()
    out["d2h_s"] = time.perf_counter() - t
    out["matrix_bytes"] = Dh.nbytes
    del D
    t = time.perf_counter()
    labels = AgglomerativeClustering(n_clusters=None, distance_threshold=1 - 0.3, metric='precomputed', linkage='average').fit(Dh).labels_
    out["sklearn_s"] = time.perf_counter() - t
    out["clusters"] = int(labels.max() + 1)

    if a.host_pairs:
        # uniform pairs stand for the (nearly all separated) pairs of a large memory, pairs of fragments of one object for the overlapping
        rng = np.random.default_rng(a.seed + 1)
        n_same = a.host_pairs // 2
        same = np.flatnonzero(owner[:-1] == owner[1:])
        samples = {"uniform": [tuple(rng.choice(a.n, 2, replace=False)) for _ in range(a.host_pairs - n_same)],
                   "same_object": [(i, i + 1) for i in rng.choice(same, n_same, replace=len(same) < n_same)]}
        worst, per = 0.0, {}
        for kind, pairs in samples.items():
            t = time.perf_counter()
            for i, j in pairs:
                worst = max(worst, abs(1 - calculate_obj_aligned_3d_IoU(clouds[i], clouds[j]) - Dh[i, j]))
            per[kind] = (time.perf_counter() - t) / len(pairs)
        total = a.n * (a.n - 1) // 2
        out["host_pair_ms"] = {k: 1e3 * v for k, v in per.items()}
        out["host_loop_extrapolated_s"] = per["uniform"] * (total - n_ov) + per["same_object"] * n_ov
        out["host_sample_max_abs_diff"] = worst
    del Dh

    if a.e2e:
        from ibloc_amd.object_memory.object_memory import ObjectMemory
        mem = ObjectMemory(device="cuda", get_embeddings_func=lambda **kw: None, log_enabled=False, arena_bytes=64 << 20)
        mem.iou_backend = "device"
        rng = np.random.default_rng(a.seed + 2)
        emb = rng.normal(size=(owner.max() + 1, 32))
        for i, p in enumerate(clouds):
            mem.add_object(f"obj{owner[i]}", [emb[owner[i]] + 0.05 * rng.normal(size=32)], p, np.full_like(p, 0.5))
        torch.cuda.synchronize()
        t = time.perf_counter()
        mem._recluster_IoU(0.3)
        out["e2e_recluster_s"] = time.perf_counter() - t
        out["e2e_objects_after"] = len(mem.memory)
        mem._ctx.close()
    ctx.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
