"""The world, the removal sets and a numpy model of the spatial hash for the live-memory removal tests: tests/test_live_remove_model.py
shows on the CPU that the sets contain the cases they are named for, tests/test_gpu_live_memory_remove.py runs them on the device.

The world is that of tests/test_gpu_live_memory.py: 8 instances of 300 to 800 points, instance 7 a second observation of instance 0
shifted by 1.5 cm, so that the two share 4 cm cells."""
import copy
import functools

import numpy as np

SIZES = (300, 520, 800, 410, 650, 380, 740, 560)          # points per instance
N_EMB = (2, 3, 4, 2, 3, 4, 2, 3)
CELL = 0.04
THR = 0.02
FINE_CELL, FINE_THR = 0.01, 0.005                         # the cells of the growth test: thousands of cells, a table that changes size
FINE_REMOVED = (1, 2, 3, 4, 5, 6, 7)                      # 7 of 8 go, the smallest instance stays
DUP_OF = 2                                                # the duplicates case: a ninth instance with bit-identical rows of this one

# name -> instances removed from the memory of all 8, and the cases the set is named for
REMOVAL_SETS = {
    "first": ([0], ("partial_cell", "vanished_cell", "begins_at_0")),             # the twin (7) keeps the shared cells
    "last": ([7], ("partial_cell", "vanished_cell", "ends_at_n")),
    "middle": ([3], ("vanished_cell",)),
    "non_adjacent": ([1, 4, 6], ("vanished_cell",)),
    "all_but_one": ([0, 1, 2, 3, 4, 5, 6], ("partial_cell", "vanished_cell", "begins_at_0")),
}


@functools.lru_cache(maxsize=None)
def world():
    """(SynthWorld, embeddings, points, colors, frames) -- read-only: every test shares them"""
    from ibloc_amd.synth import SynthWorld
    w = SynthWorld(8, pts_per_object=800, E=4, D=32, seed=71, extent=(0.06, 0.16))
    twin = copy.copy(w.objects[0])
    twin.world_center = w.objects[0].world_center + np.array([0.015, -0.01, 0.012])
    w.objects[7] = twin
    rng = np.random.default_rng(72)
    w.points[7], w.colors[7] = twin.sample(800, rng)
    emb = [np.ascontiguousarray(w.embeddings[i][:N_EMB[i]]) for i in range(8)]
    pts = [np.ascontiguousarray(w.points[i][:SIZES[i]]) for i in range(8)]
    col = [np.ascontiguousarray(w.colors[i][:SIZES[i]]) for i in range(8)]
    frames = [w.make_frame(rng, q=3, pts_per_object=800, anchor=a) for a in (7, 5, 6, 2)]
    return w, emb, pts, col, frames


def kept(n, removed):
    return [i for i in range(n) if i not in set(removed)]


def point_ranges(sizes, removed):
    """the half-open point ranges of the instances `removed` (ascending), neighbours not joined"""
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(off[i]), int(off[i + 1])) for i in sorted(removed)]


# ---- numpy model of ibl_memgrid_build ------------------------------------------------------------------------------------------------
def pts4_host(clouds, colors):
    """(n, 4) float32 rows x, y, z, intensity as the memory packs them (intensity = (r + g + b) / 3 in float64, rounded)"""
    rows = []
    for p, c in zip(clouds, colors):
        c = np.asarray(c, dtype=np.float64)
        rows.append(np.concatenate([np.asarray(p, dtype=np.float32), ((c[:, 0] + c[:, 1] + c[:, 2]) / 3.0).astype(np.float32)[:, None]], axis=1))
    return np.ascontiguousarray(np.concatenate(rows), dtype=np.float32)


def grid_keys(p4, cell):
    """the 63-bit cell key of every row: floorf(float32(p) * (float32(1) / float32(cell))), 21 bits per axis, offset 2^20"""
    inv = np.float32(1.0) / np.float32(cell)
    c = np.floor(np.asarray(p4[:, :3], dtype=np.float32) * inv).astype(np.int64) + (1 << 20)
    return (c[:, 0].astype(np.uint64) << np.uint64(42)) | (c[:, 1].astype(np.uint64) << np.uint64(21)) | c[:, 2].astype(np.uint64)


def table_slots(n_cells):
    h = 1024
    while h < 3 * n_cells:
        h *= 2
    return h


def model_build(p4, cell):
    """dict(order, sorted, keys (sorted), ukeys, ustart, n_cells, table_slots) of the grid built from the rows p4: a stable sort by key"""
    keys = grid_keys(p4, cell)
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    ukeys, first = np.unique(skeys, return_index=True)
    ustart = np.concatenate([first, [len(p4)]]).astype(np.int32)
    return dict(order=order, sorted=p4[order], keys=skeys, ukeys=ukeys, ustart=ustart, n_cells=len(ukeys), table_slots=table_slots(len(ukeys)))


def model_remove(built, ranges):
    """the contract of ibl_memgrid_remove on a model grid: the sorted rows whose original index lies in no range, in their order"""
    gone = np.zeros(len(built["order"]), dtype=bool)
    for b, e in ranges:
        gone[b:e] = True
    keep = ~gone[built["order"]]
    return built["sorted"][keep], built["keys"][keep], gone
