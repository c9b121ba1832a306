"""Cost of adding an object to a resident memory, of taking one out and of changing one where it is: MemoryShard.append / .remove /
.replace on a live memory against the rebuild they replace, on a synthetic memory of N instances x 5 000 points (ibloc_amd.synth.SynthWorld).

    python tools/perf_live_memory.py N [--points P] [--seed S] [--compact] [--arena-gb G]

Prints one JSON line: rebuild_s = rebuild_shard_s + rebuild_features_s, the time from "one object added" to "shard ready" without a
live memory (MemoryShard construction from host arrays + features(0.05, 0.4), device synchronised), with rebuild_host_s, the part of it
that is host packing and the host-to-device copy of the clouds (CloudBatch.from_numpy alone); live_build_s, the same construction with
live=True; append_1_s / append_32_s, MemoryShard.append of 1 and of 32 instances (median of 5 after a warm-up append, device
synchronised), with append_*_grid_s, the ibl_memgrid_append part of those appends, and append_*_all the single times; remove_1_s /
remove_32_s, MemoryShard.remove of 1 and of 32 neighbouring instances from the middle of the same memory (median of 5 after a warm-up
removal), with remove_*_grid_s, the ibl_memgrid_remove part, and remove_*_all; replace_1_s, MemoryShard.replace of the middle instance by
another cloud of the same size elsewhere (median of 5 after a warm-up), with replace_1_grid_s, the ibl_memgrid_replace part, and
replace_1_all, against remove_append_1_s, the removal and append a caller had to use instead (it moves the instance to the end);
grid_rebuild_s, a MemGrid built from the kept points
(median of 5 after a warm-up): the re-sort the removal avoids.  Without a live memory a removal costs rebuild_s.  Needs a GPU."""
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
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--compact", action="store_true", help="compact resident features (168 instead of 264 bytes per point)")
    ap.add_argument("--arena-gb", type=float, default=24.0, help="scratch arena of the registration context")
    a = ap.parse_args()

    import torch
    from ibloc_amd.engine import MemoryShard, intensity_from_colors
    from ibloc_amd.registration import CloudBatch, MemGrid, RegContext
    from ibloc_amd.synth import SynthWorld
    if not torch.cuda.is_available():
        raise SystemExit("perf_live_memory.py measures device work: no GPU here")

    extra = 6 * (1 + 32) + 12                                # a warm-up and five timed appends of 1 and of 32 instances, 2 x 6 replacements
    t = time.perf_counter()
    w = SynthWorld(a.n + extra, pts_per_object=a.points, E=2, D=64, seed=a.seed)
    emb = list(w.embeddings)
    ints = [intensity_from_colors(c) for c in w.colors]
    out = {"n": a.n, "points": a.points, "compact": a.compact, "synth_s": time.perf_counter() - t}
    sync = torch.cuda.synchronize
    ctx = RegContext(int(a.arena_gb * (1 << 30)))

    def build(live):
        sync()
        t0 = time.perf_counter()
        m = MemoryShard(ctx, emb[:a.n], w.points[:a.n], intensities=ints[:a.n], compact_features=a.compact, live=live)
        sync()
        t1 = time.perf_counter()
        m.features(0.05, 0.4)
        sync()
        return m, t1 - t0, time.perf_counter() - t1

    build_small = MemoryShard(ctx, emb[:2], w.points[:2], intensities=ints[:2])       # warm-up (code object load)
    build_small.features(0.05, 0.4)
    build_small.close()
    m, out["rebuild_shard_s"], out["rebuild_features_s"] = build(False)
    out["rebuild_s"] = out["rebuild_shard_s"] + out["rebuild_features_s"]
    m.close()
    del m
    sync()
    t = time.perf_counter()
    cb = CloudBatch.from_numpy(w.points[:a.n], ints[:a.n])
    sync()
    out["rebuild_host_s"] = time.perf_counter() - t
    del cb
    torch.cuda.empty_cache()

    m, shard_s, feat_s = build(True)
    out["live_build_s"] = shard_s + feat_s
    grid_times = []
    grid_append = m.grid.append

    def timed_grid_append(p):
        sync()
        t0 = time.perf_counter()
        grid_append(p)
        sync()
        grid_times.append(time.perf_counter() - t0)

    m.grid.append = timed_grid_append
    nxt = a.n
    for k in (1, 32):
        times = []
        for _ in range(6):
            sync()
            t = time.perf_counter()
            m.append(emb[nxt:nxt + k], w.points[nxt:nxt + k], intensities=ints[nxt:nxt + k])
            sync()
            times.append(time.perf_counter() - t)
            nxt += k
        out[f"append_{k}_s"] = float(np.median(times[1:]))
        out[f"append_{k}_all"] = times
        out[f"append_{k}_grid_s"] = float(np.median(grid_times[-5:]))
    out["resident_points"] = m.clouds.n
    grid_times = []
    grid_remove = m.grid.remove

    def timed_grid_remove(ranges):
        sync()
        t0 = time.perf_counter()
        grid_remove(ranges)
        sync()
        grid_times.append(time.perf_counter() - t0)

    m.grid.remove = timed_grid_remove
    for k in (1, 32):
        times = []
        for _ in range(6):
            first = m.M // 2
            sync()
            t = time.perf_counter()
            m.remove(range(first, first + k))
            sync()
            times.append(time.perf_counter() - t)
        out[f"remove_{k}_s"] = float(np.median(times[1:]))
        out[f"remove_{k}_all"] = times
        out[f"remove_{k}_grid_s"] = float(np.median(grid_times[-5:]))
    grid_times = []
    grid_replace = m.grid.replace

    def timed_grid_replace(ranges, counts, p):
        sync()
        t0 = time.perf_counter()
        grid_replace(ranges, counts, p)
        sync()
        grid_times.append(time.perf_counter() - t0)

    m.grid.replace = timed_grid_replace
    times, substitute = [], []
    for _ in range(6):
        mid = m.M // 2
        sync()
        t = time.perf_counter()
        m.replace([mid], emb[nxt:nxt + 1], w.points[nxt:nxt + 1], intensities=ints[nxt:nxt + 1])
        sync()
        times.append(time.perf_counter() - t)
        nxt += 1
    out["replace_1_s"] = float(np.median(times[1:]))
    out["replace_1_all"] = times
    out["replace_1_grid_s"] = float(np.median(grid_times[-5:]))
    for _ in range(6):                                       # what a caller had to do instead, and it moves the instance to the end
        mid = m.M // 2
        sync()
        t = time.perf_counter()
        m.remove([mid])
        m.append(emb[nxt:nxt + 1], w.points[nxt:nxt + 1], intensities=ints[nxt:nxt + 1])
        sync()
        substitute.append(time.perf_counter() - t)
        nxt += 1
    out["remove_append_1_s"] = float(np.median(substitute[1:]))
    out["remove_append_1_all"] = substitute
    times = []
    for _ in range(6):
        sync()
        t = time.perf_counter()
        g = MemGrid(ctx, m.clouds.pts4, cell=2 * m.eval_threshold)
        sync()
        times.append(time.perf_counter() - t)
        g.close()
    out["grid_rebuild_s"] = float(np.median(times[1:]))
    out["points_after_removals"] = m.clouds.n
    out["grid"] = m.grid.info()
    out["rebuild_over_append_1"] = out["rebuild_s"] / out["append_1_s"]
    out["rebuild_over_remove_1"] = out["rebuild_s"] / out["remove_1_s"]
    out["grid_rebuild_over_grid_remove_1"] = out["grid_rebuild_s"] / out["remove_1_grid_s"]
    out["rebuild_over_replace_1"] = out["rebuild_s"] / out["replace_1_s"]
    out["remove_append_over_replace_1"] = out["remove_append_1_s"] / out["replace_1_s"]
    m.close()
    ctx.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
