"""The world, the replacement sets and a numpy model of ibl_memgrid_replace for the live-memory replacement tests:
tests/test_live_replace_model.py shows on the CPU that the model is the build of the spliced rows and that the sets contain the cases
they are named for, tests/test_gpu_live_memory_replace.py runs them on the device.

The world is that of tests/live_remove_cases.py with instance 3 replaced by a SECOND twin of instance 0, shifted by ~1 cm: 4 cm cells
are then shared by the instances 0 < 3 < 7, the smallest case in which the new points of a replaced instance (3) must land BETWEEN
resident points (of 0 and of 7) inside one cell."""
import copy
import functools

import numpy as np

from tests import live_remove_cases as lc
from tests.live_remove_cases import CELL, FINE_CELL, FINE_THR, N_EMB, SIZES, THR, grid_keys, model_build, pts4_host  # noqa: F401

# name -> [(instance, "fresh", points) | (instance, "moved", metres along x)], and the cases the set is named for
REPLACE_SETS = {
    "first": ([(0, "fresh", 640)], ("begins_at_0", "grows")),
    "last": ([(7, "fresh", 200)], ("ends_at_n", "shrinks")),
    "middle_shared": ([(3, "fresh", SIZES[3])], ("same_size", "interleaves")),
    "moved": ([(4, "moved", 3.0)], ("same_size", "cells_vanish", "cells_appear")),
    "touching": ([(1, "fresh", 700), (2, "fresh", 500)], ("adjacent_ranges", "grows", "shrinks")),
    "non_adjacent": ([(1, "fresh", 700), (4, "fresh", 300), (6, "fresh", SIZES[6])], ("grows", "shrinks", "same_size")),
    "all": ([(0, "fresh", 350), (1, "fresh", 480), (2, "fresh", 900), (3, "fresh", 300), (4, "fresh", 650), (5, "fresh", 500),
             (6, "fresh", 600), (7, "fresh", 610)], ("begins_at_0", "ends_at_n", "every_instance", "adjacent_ranges")),
}


@functools.lru_cache(maxsize=None)
def world():
    """(SynthWorld, objects, embeddings, points, colors) -- read-only: every test shares them"""
    w, emb, pts, col, _ = lc.world()
    objects = list(w.objects)
    objects[3] = copy.copy(w.objects[0])
    objects[3].world_center = w.objects[0].world_center + np.array([-0.01, 0.008, 0.009])
    p, c = objects[3].sample(SIZES[3], np.random.default_rng(81))
    pts, col = list(pts), list(col)
    pts[3], col[3] = np.ascontiguousarray(p), np.ascontiguousarray(c)
    return w, tuple(objects), emb, tuple(pts), tuple(col)


@functools.lru_cache(maxsize=None)
def replacements(name):
    """(instances, clouds, colors) of the set: fresh samples of the same objects in other sizes, or the resident cloud moved"""
    _, objects, _, pts, col = world()
    instances, clouds, colors = [], [], []
    for i, kind, arg in REPLACE_SETS[name][0]:
        if kind == "fresh":
            p, c = objects[i].sample(arg, np.random.default_rng(900 + 10 * sorted(REPLACE_SETS).index(name) + i))
        else:
            p, c = pts[i] + np.array([arg, 0.0, 0.0]), col[i]
        instances.append(i)
        clouds.append(np.ascontiguousarray(p))
        colors.append(np.ascontiguousarray(c))
    return tuple(instances), tuple(clouds), tuple(colors)


def fresh_embeddings(i, count, seed=0):
    """`count` new embedding rows for instance i"""
    D = world()[2][0].shape[1]
    return np.random.default_rng(7000 + 31 * i + seed).normal(size=(count, D)).astype(np.float32)


def spliced(items, instances, new_items):
    """the list `items` with new_items[k] in the place instances[k]"""
    out = list(items)
    for i, x in zip(instances, new_items):
        out[i] = x
    return out


def replace_args(sizes, instances, clouds):
    """(ranges, counts) as ibl_memgrid_replace takes them: one range per instance, ascending, neighbours NOT joined"""
    off = np.concatenate([[0], np.cumsum(sizes)])
    by = np.argsort(instances)
    return [(int(off[instances[k]]), int(off[instances[k] + 1])) for k in by], [len(clouds[k]) for k in by]


def ordered(instances, items):
    """`items` in ascending order of their instances"""
    return [items[k] for k in np.argsort(instances)]


def splice_p4(p4, ranges, new_p4, counts):
    """the rows p4 with ranges[r] replaced by the next counts[r] rows of new_p4"""
    parts, at, c = [], 0, 0
    for (b, e), k in zip(ranges, counts):
        parts += [p4[at:b], new_p4[c:c + k]]
        at, c = e, c + k
    return np.ascontiguousarray(np.concatenate(parts + [p4[at:]]))


# ---- numpy model of ibl_memgrid_replace: the position formulas, no sort of resident points -------------------------------------------
def model_replace(built, ranges, counts, new_p4, cell=CELL):
    """dict(sorted, keys, sidx) of the grid `built` (lc.model_build: its `order` is the per-slot original index) after the
    replacement, by the formulas of the device code: every kept resident slot and every sorted new point computes its destination
    from scans and bounded binary searches; every destination must be hit exactly once."""
    rbeg, rend = np.array([r[0] for r in ranges], dtype=np.int64), np.array([r[1] for r in ranges], dtype=np.int64)
    rcum0 = np.concatenate([[0], np.cumsum(rend - rbeg)])              # removed by the ranges before r
    ncum = np.cumsum(np.asarray(counts, dtype=np.int64))
    ncum0 = np.concatenate([[0], ncum])
    sidx, skeys, ukeys, ustart = built["order"], built["keys"], built["ukeys"], built["ustart"]
    n, n_new = len(sidx), len(new_p4)
    nr = np.searchsorted(rbeg, sidx, side="right")                     # ranges that begin at or below the index
    keep = (nr == 0) | (sidx >= rend[np.maximum(nr, 1) - 1])
    kscan = np.concatenate([[0], np.cumsum(keep)])                     # n + 1 entries
    raw = grid_keys(new_p4, cell) if n_new else np.zeros(0, dtype=np.uint64)
    order = np.argsort(raw, kind="stable")
    nkeys = raw[order]
    n_out = int(kscan[-1]) + n_new
    out = np.zeros((n_out, 4), dtype=np.float32)
    keys = np.zeros(n_out, dtype=np.uint64)
    new_sidx = np.full(n_out, -1, dtype=np.int64)
    hit = np.zeros(n_out, dtype=np.int64)
    lo, hi = np.searchsorted(nkeys, skeys, side="left"), np.searchsorted(nkeys, skeys, side="right")
    for i in np.flatnonzero(keep):
        c_before = ncum0[nr[i]]
        d = kscan[i] + lo[i] + np.searchsorted(order[lo[i]:hi[i]], c_before, side="left")
        out[d], keys[d], new_sidx[d] = built["sorted"][i], skeys[i], sidx[i] - rcum0[nr[i]] + c_before
        hit[d] += 1
    for j in range(n_new):
        k, c = nkeys[j], order[j]
        r = int(np.searchsorted(ncum, c, side="right"))
        cell_i = int(np.searchsorted(ukeys, k, side="left"))
        pos = int(ustart[cell_i])
        if cell_i < len(ukeys) and ukeys[cell_i] == k:
            pos += int(np.searchsorted(sidx[pos:ustart[cell_i + 1]], rbeg[r], side="left"))
        d = j + kscan[pos]
        out[d], keys[d], new_sidx[d] = new_p4[c], k, rbeg[r] - rcum0[r] + c
        hit[d] += 1
    assert (hit == 1).all()
    return dict(sorted=out, keys=keys, sidx=new_sidx)
