"""Cost of deciding which detections are resident instances seen again: MemoryShard.overlap + the decision rule of
ObjectMemory.associate_detections on a live synthetic memory (ibloc_amd.synth.SynthWorld), against the host alternative a user
would write -- per detection a bounding-box filter over the instances, a scipy cKDTree per candidate instance, a radius query of
the detection's points, the same decision.

    python tools/perf_associate.py [N] [--points P] [--dets Q] [--det-points K] [--seed S] [--arena-gb G]

Defaults: N = 1 000 instances x 5 000 points, 7 detections x 5 000 points (fresh samples of resident objects, re-noised; every
second one is given a foreign embedding).  Prints one JSON line: device_s = upload of the detections + MemoryShard.overlap + the
decision (median of 10 after 2 warm-ups, host clock, the call synchronises), overlap_s the overlap call alone on resident detections,
stage_ms the device time of its two launches (HIP events: ibloc_amd.prof), host_s the host alternative (median of 3; the instances'
bounding boxes are precomputed outside the timed part, the trees are not -- the memory changes between calls), host_over_device,
and whether both sides decided alike.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_hits(dets, clouds, boxes, radius, k):
    """(inst, hits) candidate lists as MemoryShard.overlap returns them, on the host"""
    from scipy.spatial import cKDTree
    lo, hi = boxes
    inst = np.full((len(dets), k), -1, dtype=np.int32)
    hits = np.zeros((len(dets), k), dtype=np.int32)
    for d, D in enumerate(dets):
        cand = np.flatnonzero(((D.min(0) - radius <= hi) & (D.max(0) + radius >= lo)).all(axis=1))
        found = []
        for m in cand:
            dist, _ = cKDTree(clouds[m]).query(D, k=1, distance_upper_bound=radius)
            h = int(np.isfinite(dist).sum())
            if h:
                found.append((-h, int(m)))
        for j, (h, m) in enumerate(sorted(found)[:k]):
            inst[d, j], hits[d, j] = m, -h
    return inst, hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=1000)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=7)
    ap.add_argument("--det-points", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--arena-gb", type=float, default=2.0, help="scratch arena of the registration context")
    a = ap.parse_args()

    import torch
    from ibloc_amd import prof
    from ibloc_amd.engine import MemoryShard
    from ibloc_amd.object_memory.object_memory import AssociationParams, association_decisions
    from ibloc_amd.registration import CloudBatch, RegContext
    from ibloc_amd.synth import SynthWorld
    if not torch.cuda.is_available():
        raise SystemExit("perf_associate.py measures device work: no GPU here")

    t = time.perf_counter()
    w = SynthWorld(a.n, pts_per_object=a.points, E=2, D=64, seed=a.seed)
    rng = np.random.default_rng(a.seed + 1)
    seen = rng.choice(a.n, size=a.dets, replace=False)
    dets = [w.objects[j].sample(a.det_points, rng)[0].astype(np.float32).astype(np.float64) for j in seen]
    det_emb = [w.base_emb[j] + rng.normal(0, 0.1 / 8.0, size=64) if i % 2 == 0 else rng.normal(size=64) for i, j in enumerate(seen)]
    means = [np.mean(e, axis=0) for e in w.embeddings]
    clouds = [np.ascontiguousarray(p.astype(np.float32).astype(np.float64)) for p in w.points]
    out = {"n": a.n, "points": a.points, "dets": a.dets, "det_points": a.det_points, "synth_s": time.perf_counter() - t}
    sync = torch.cuda.synchronize
    ctx = RegContext(int(a.arena_gb * (1 << 30)))
    mem = MemoryShard(ctx, list(w.embeddings), w.points, live=True)
    params = AssociationParams()
    sizes = [len(d) for d in dets]

    def device(upload=True, batch=None):
        batch = CloudBatch.from_numpy(dets) if upload else batch
        inst, hits, _ = mem.overlap(batch, radius=params.radius, k=params.k)
        return inst, hits, association_decisions(inst, hits, sizes, det_emb, lambda m: means[m], params)

    def median_time(fn, warm, reps):
        times = []
        for i in range(warm + reps):
            sync()
            t0 = time.perf_counter()
            res = fn()
            sync()
            times.append(time.perf_counter() - t0)
        return float(np.median(times[warm:])), times, res

    out["device_s"], out["device_all"], (inst, hits, dec) = median_time(device, 2, 10)
    resident = CloudBatch.from_numpy(dets)
    out["overlap_s"], _, _ = median_time(lambda: mem.overlap(resident, radius=params.radius, k=params.k), 2, 10)
    prof.reset(True)
    for _ in range(10):
        mem.overlap(resident, radius=params.radius, k=params.k)
    ms, _, calls = prof.read(prof.ST_ASSOC)
    prof.reset(False)
    out["stage_ms"] = ms / max(calls, 1)

    boxes = (np.stack([c.min(0) for c in clouds]), np.stack([c.max(0) for c in clouds]))
    radius = mem.eval_threshold if params.radius is None else params.radius

    def host():
        hi, hh = host_hits(dets, clouds, boxes, radius, params.k)
        return hi, hh, association_decisions(hi, hh, sizes, det_emb, lambda m: means[m], params)

    out["host_s"], out["host_all"], (h_inst, h_hits, h_dec) = median_time(host, 0, 3)
    out["host_over_device"] = out["host_s"] / out["device_s"]
    out["decisions"] = dec
    out["decisions_agree"] = dec == h_dec
    out["expected"] = [int(j) if i % 2 == 0 else None for i, j in enumerate(seen)]
    # the tree works in float64 with <=, the device in fp32 with a strict <: counts may differ by pairs at the radius
    same = h_inst == inst
    out["candidates_agree"] = bool(same.all())
    out["hits_max_abs_diff"] = int(np.abs(h_hits - hits)[same].max(initial=0))
    out["hits_first"] = [int(x) for x in hits[:, 0]]
    out["grid"] = mem.grid.info()
    mem.close()
    ctx.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
