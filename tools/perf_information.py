"""Cost of the information matrix of a localised pose (`evaluate_information`, ibl_information_kernel) next to its sibling, the
whole-memory evaluation (`evaluate_batch`, ibl_evaluate_kernel), on equal jobs of the default benchmark's shape: the synthetic memory
of bench.py (DeviceWorld: M instances x P surface points, sampled on the device with the benchmark's seed) and one batch of F frames
of Q detections x P points, cleaned by the radius-outlier removal as stage B cleans them.  One job per frame -- what
localise_batch(information=True) adds: the frame's cleaned points under its pose (here the frame's true camera pose).

    python tools/perf_information.py [--memory M] [--points P] [--frames F] [--q Q] [--arena-gb G]

Defaults: 10 000 x 5 000 memory points, 32 frames of 7 x 5 000 points (about 4 930 each after cleaning).  Prints one JSON line:
information_s and evaluate_s = the two calls on the same 32 jobs (median of 10 after 2 warm-ups, host clock; both calls
synchronise), information_points_s = the same with the per-point output, ratio = information_s / evaluate_s, the fitness of the
jobs and whether n_corr / ns equals it.  Both kernels read the same cells; the new one also reads a cell whose bound only ties with
the best distance, carries the matched point and ten fp64 sums.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--memory", type=int, default=10000)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--q", type=int, default=7)
    ap.add_argument("--threshold", type=float, default=0.02)
    ap.add_argument("--arena-gb", type=float, default=8.0, help="scratch arena of the registration context (the grid build of 50 M points sorts in it)")
    a = ap.parse_args()

    import torch
    import bench
    from ibloc_amd.registration import MemGrid, RegContext, evaluate_batch, evaluate_information, radius_outlier_batch
    if not torch.cuda.is_available():
        raise SystemExit("perf_information.py measures device work: no GPU here")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize

    t = time.perf_counter()
    world = bench.DeviceWorld(a.memory, dev, pts_per_object=a.points, E=1, D=8, seed=21, sample_points=False)
    g = torch.Generator(device=dev)
    g.manual_seed(21)
    mem4 = torch.zeros((a.memory * a.points, 4), dtype=torch.float32, device=dev)
    step = max(1, (1 << 22) // a.points)
    for lo in range(0, a.memory, step):                       # the memory's points, in DeviceWorld's own chunks, kept on the device
        hi = min(a.memory, lo + step)
        p, _, _ = world.sample(torch.arange(lo, hi, device=dev), [a.points] * (hi - lo), g)
        mem4[lo * a.points:hi * a.points, :3] = p.reshape(-1, 3).float()
    frng = np.random.default_rng(1000)
    frames = [world.frame(frng, q=a.q) for _ in range(a.frames)]
    g.manual_seed(1000)
    det = world.detections(frames, a.points, g)
    ctx = RegContext(int(a.arena_gb * (1 << 30)))
    keepb = radius_outlier_batch(ctx, det, 0.05, 8).bool()
    clean = det.pts4[keepb].contiguous()
    off = np.concatenate([[0], np.cumsum(keepb.cpu().numpy())])[det.seg_off_host]
    row0 = np.concatenate([[0], np.cumsum([len(f["ids"]) for f in frames])])
    jb, je = off[row0[:-1]].astype(np.int32), off[row0[1:]].astype(np.int32)
    T = np.stack([f["pose"] for f in frames])
    grid = MemGrid(ctx, mem4, cell=2 * a.threshold)
    sync()
    out = {"memory": a.memory, "points": a.points, "frames": a.frames, "q": a.q, "jobs": len(jb), "clean_points_per_detection":
           float((je - jb).sum()) / (a.frames * a.q), "setup_s": time.perf_counter() - t, "grid": grid.info()}

    def median_time(fn, warm=2, reps=10):
        times = []
        for _ in range(warm + reps):
            sync()
            t0 = time.perf_counter()
            res = fn()
            sync()
            times.append(time.perf_counter() - t0)
        return float(np.median(times[warm:])), times[warm:], res

    out["evaluate_s"], out["evaluate_all"], (_, fit) = median_time(lambda: evaluate_batch(ctx, grid, clean, jb, je, T, a.threshold))
    out["information_s"], out["information_all"], (info, n_corr) = median_time(lambda: evaluate_information(ctx, grid, clean, jb, je, T, a.threshold))
    out["information_points_s"], _, _ = median_time(lambda: evaluate_information(ctx, grid, clean, jb, je, T, a.threshold, points=True))
    out["ratio"] = out["information_s"] / out["evaluate_s"]
    out["fitness_mean"] = float(fit.mean())
    out["n_corr_over_ns_is_fitness"] = bool((n_corr / np.maximum(je - jb, 1) == fit).all())
    out["symmetric"] = bool(all(m.tobytes() == m.T.copy().tobytes() for m in info))
    grid.close()
    ctx.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
