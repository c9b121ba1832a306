"""-m gpu: live object memory.  A memory that is appended to while resident (ibl_memgrid_build with live = 1 / ibl_memgrid_append,
MemoryShard(live=True).append, ObjectMemory.live_memory) holds, array for array, what a memory rebuilt from all instances holds, and
localises to the same results bit for bit."""
import copy
import functools

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from tests.live_memory_helpers import (assert_same_features, assert_same_grid, assert_same_results, point_distances, pts4_of, run_frames,
                                       same_bits)

pytestmark = pytest.mark.gpu

SIZES = (300, 520, 800, 410, 650, 380, 740, 560)          # points per instance: the first is the smallest (growth test)
N_EMB = (2, 3, 4, 2, 3, 4, 2, 3)
CELL = 0.04
THR = 0.02


@functools.lru_cache(maxsize=None)
def world():
    """8 small instances; the last one is a second observation of instance 0, shifted by 1.5 cm: its points share 4 cm cells with
    instance 0's.  Returns (SynthWorld, embeddings, points, colors, frames)."""
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


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(2 << 30)
    yield c
    c.close()


def cells_of(p, cell=CELL):
    """cell triples as the grid computes them: floorf(float(p) * (1.0f / float(cell)))"""
    inv = np.float32(1.0) / np.float32(cell)
    return [tuple(r) for r in np.floor(np.asarray(p, dtype=np.float32) * inv).astype(np.int64)]


def queries(pts, n_old):
    """~4 000 query points around all memory points (2 mm-1 cm off them) and 400 far from everything, with the count of every case
    the merge has to get right"""
    rng = np.random.default_rng(73)
    allp = np.concatenate(pts).astype(np.float32)
    pick = rng.choice(len(allp), 3600)
    near = allp[pick] + rng.normal(0, 0.004, size=(3600, 3)).astype(np.float32)
    far = allp[rng.choice(len(allp), 400)] + np.array([0, 0, 25.0], dtype=np.float32)
    q = np.concatenate([near, far]).astype(np.float32)
    dmin, nearest = cKDTree(allp.astype(np.float64)).query(q.astype(np.float64))
    within = dmin < THR * 0.999
    old_cells, new_cells = set(cells_of(allp[:n_old])), set(cells_of(allp[n_old:]))
    qc = cells_of(q)
    counts = dict(nearest_old=int((within & (nearest < n_old)).sum()), nearest_new=int((within & (nearest >= n_old)).sum()),
                  mixed_cell=sum(c in old_cells and c in new_cells for c in qc),
                  new_cell=sum(c in new_cells and c not in old_cells for c in qc), none=int((dmin > THR * 1.001).sum()))
    return q, counts


@pytest.mark.parametrize("first,steps", [(7, (1,)), (1, (7,)), (4, (1, 1, 1, 1))], ids=["7+1", "1+7", "4+1+1+1+1"])
def test_appended_grid_equals_fresh_build(ctx, first, steps):
    from ibloc_amd.registration import MemGrid
    _, _, pts, col, _ = world()
    live = MemGrid(ctx, pts4_of(pts[:first], col[:first]), CELL, live=True, reserve_points=1000)
    have = first
    for k in steps:
        live.append(pts4_of(pts[have:have + k], col[have:have + k]))
        have += k
        fresh = MemGrid(ctx, pts4_of(pts[:have], col[:have]), CELL)
        n_old = sum(SIZES[:have - k])
        q, counts = queries(pts[:have], n_old)
        print(f"{first} + {steps}: {have} instances, cases {counts}")
        # (instances 1 .. 6 stand metres apart: only the step that adds instance 7 puts new points into old cells)
        assert all(v > 0 for name, v in counts.items() if name != "mixed_cell" or have == 8), counts
        d2 = assert_same_grid(ctx, live, fresh, q)
        assert np.isinf(d2).sum() >= counts["none"] and np.isfinite(d2).sum() >= counts["nearest_old"] + counts["nearest_new"]
        fresh.close()
    live.close()


def test_growth_noop_and_arena_refusal(ctx):
    from ibloc_amd import _lib
    from ibloc_amd.registration import MemGrid
    _, _, pts, col, _ = world()
    cell, thr = 0.01, 0.005          # 1 cm cells: 267 -> 3 645 occupied cells, so the table goes 1 024 -> 4 096 -> 8 192 -> 16 384 slots
    live = MemGrid(ctx, pts4_of(pts[:1], col[:1]), cell, live=True, reserve_points=0)
    start = live.info()
    assert start["point_capacity"] == start["n"] == SIZES[0]
    caps, tables = {start["point_capacity"]}, {start["table_slots"]}
    q, _ = queries(pts, SIZES[0])
    for have in range(2, 9):                                # one instance at a time: 300 -> 4 360 points
        live.append(pts4_of(pts[have - 1:have], col[have - 1:have]))
        info = live.info()
        assert info["point_capacity"] >= info["n"] == sum(SIZES[:have])
        assert info["table_slots"] >= 3 * info["n_cells"] and (info["table_slots"] == 1024 or info["table_slots"] < 6 * info["n_cells"])
        caps.add(info["point_capacity"])
        tables.add(info["table_slots"])
        fresh = MemGrid(ctx, pts4_of(pts[:have], col[:have]), cell)
        assert_same_grid(ctx, live, fresh, q, thr)
        fresh.close()
    assert live.info()["n"] > 8 * start["n"]
    assert len(caps) >= 3 and len(tables) >= 3, (caps, tables)      # the buffers grew and the table was re-dimensioned, more than once
    # n_new == 0 changes nothing
    before, d_before = live.info(), point_distances(ctx, live, q, thr)[0]
    assert np.isfinite(d_before).sum() > 500 and np.isinf(d_before).sum() >= 400
    live.append(torch.zeros((0, 4), dtype=torch.float32, device="cuda"))
    assert live.info() == before and point_distances(ctx, live, q, thr)[0].tobytes() == d_before.tobytes()
    # a grid of the arena refuses, and evaluates as before
    arena = MemGrid(ctx, pts4_of(pts[:3], col[:3]), CELL)
    before, d_before = arena.info(), point_distances(ctx, arena, q)[0]
    with pytest.raises(_lib.IblError):
        arena.append(pts4_of(pts[3:4], col[3:4]))
    assert arena.info() == before and point_distances(ctx, arena, q)[0].tobytes() == d_before.tobytes()
    arena.close()
    live.close()


@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
def test_resident_state_equals_rebuilt(ctx, compact):
    from ibloc_amd.engine import MemoryShard
    _, emb, pts, col, _ = world()
    plain = MemoryShard(ctx, emb, pts, colors=col, compact_features=compact)
    live = MemoryShard(ctx, emb[:5], pts[:5], colors=col[:5], compact_features=compact, live=True, reserve_points=1200, reserve_rows=7)
    early = live.features(0.05, 0.4)                      # requested before the appends ...
    live.append(emb[5:7], pts[5:7], colors=col[5:7])      # (fits the headroom)
    live.append(emb[7:], pts[7:], colors=col[7:])         # (does not: every buffer grows)
    assert live.features(0.05, 0.4) is early
    assert (live.M, live.lo, live.hi) == (plain.M, plain.lo, plain.hi) == (8, 0, 8)
    assert same_bits(live.mem_emb, plain.mem_emb) and same_bits(live.emb_offsets, plain.emb_offsets)
    assert same_bits(live.emb_offsets_host, plain.emb_offsets_host)
    assert same_bits(live.clouds.pts4, plain.clouds.pts4) and same_bits(live.clouds.seg_off, plain.clouds.seg_off)
    assert same_bits(live.clouds.seg_off_host, plain.clouds.seg_off_host)
    n = sum(SIZES)
    assert_same_features(early, plain.features(0.05, 0.4), n, 8, compact)
    assert_same_features(live.features(0.05, 1.5), plain.features(0.05, 1.5), n, 8, compact)      # ... and after them
    assert live.grid.info()["n"] == plain.grid.info()["n"] == n and live.grid.info()["n_cells"] == plain.grid.info()["n_cells"]
    live.close()
    plain.close()


def test_localise_after_append_equals_rebuilt(ctx):
    from ibloc_amd.engine import LocaliseEngine, MemoryShard
    _, emb, pts, col, frames = world()
    assert any(i >= 5 for f in frames for i in f["ids"])            # true objects among the appended instances
    plain = MemoryShard(ctx, emb, pts, colors=col)
    ref = run_frames(LocaliseEngine(plain), frames)
    assert any(r.best >= 0 and r.records for r in ref)
    live = MemoryShard(ctx, emb[:5], pts[:5], colors=col[:5], live=True)
    eng = LocaliseEngine(live)
    run_frames(eng, frames[3:])                                     # the engine has served a query before the memory grows
    live.append(emb[5:7], pts[5:7], colors=col[5:7])
    live.append(emb[7:], pts[7:], colors=col[7:])
    assert_same_results(run_frames(eng, frames), ref)
    assert any(m >= 5 for r in ref for assn in r.assignments for _, m in assn)
    # a memory that never appends: live or not, the same results
    never = MemoryShard(ctx, emb, pts, colors=col, live=True)
    assert_same_results(run_frames(LocaliseEngine(never), frames), ref)
    for m in (plain, live, never):
        m.close()


def test_object_memory_appends_to_the_resident_engine():
    from ibloc_amd.object_memory.object_memory import ObjectMemory
    _, emb, pts, col, frames = world()

    def memory(n, live=True):
        om = ObjectMemory("cuda", None, None, 300.0, 300.0, get_embeddings_func=lambda **kw: None, log_enabled=False, arena_bytes=2 << 30)
        om.live_memory = live
        for j in range(n):
            om.add_object(f"obj{j}", list(emb[j]), pts[j], col[j])
        return om

    def query(om, f):
        return om.localise_detections(f["det_emb"], f["clouds"], fpfh_global_dist_factor=1.5, fpfh_local_dist_factor=1.5)

    upfront = memory(8)
    query(upfront, frames[3])
    ref = query(upfront, frames[0])
    assert ref.records
    for live in (True, False):
        om = memory(6, live)
        assert om.live_memory is live
        query(om, frames[3])
        eng, shard = om._engine, om._shard
        assert eng is not None
        for j in (6, 7):
            om.add_object(f"obj{j}", list(emb[j]), pts[j], col[j])
        if live:
            assert om._engine is eng and om._shard is shard and shard.M == 8
        else:
            assert om._engine is None
        assert_same_results([query(om, frames[0])], [ref])
        assert (om._engine is eng) == live
        om.downsample_all_objects(0.01)                                # any other mutation still discards the engine
        assert om._engine is None
        om._ctx.close()
    upfront._ctx.close()


def test_append_refusals_touch_nothing(ctx):
    from ibloc_amd.engine import MemoryShard
    _, emb, pts, col, _ = world()

    def state(m):
        return (m.M, m.lo, m.hi, m.emb_offsets_host.tobytes(), m.emb_offsets.cpu().numpy().tobytes(), tuple(m.mem_emb.shape),
                None if m.grid is None else tuple(sorted(m.grid.info().items())), None if m.clouds is None else m.clouds.n)

    def refused(m, *args, **kw):
        before = state(m)
        with pytest.raises(ValueError):
            m.append(*args, **kw)
        assert state(m) == before

    with pytest.raises(ValueError):
        MemoryShard(ctx, emb, pts, colors=col, shard=(0, 1), live=True)
    refused(MemoryShard(ctx, emb[:4], pts[:4], colors=col[:4], shard=(0, 1)), emb[4:5], pts[4:5], colors=col[4:5])      # sharded
    refused(MemoryShard(ctx, emb[:4], pts[:4], colors=col[:4]), emb[4:5], pts[4:5], colors=col[4:5])                    # not live
    live = MemoryShard(ctx, emb[:4], pts[:4], colors=col[:4], live=True)
    refused(live, emb[4:5])                                                                                             # clouds withheld
    refused(live, [e[:, :16] for e in emb[4:5]], pts[4:5], colors=col[4:5])                                             # dimension
    refused(live, emb[4:6], pts[4:5], colors=col[4:5])                                                                  # counts
    emb_only = MemoryShard(ctx, emb[:4], live=True)
    refused(emb_only, emb[4:5], pts[4:5], colors=col[4:5])                                                              # clouds given
    emb_only.append(emb[4:6])                                                                                           # (and the legal form)
    assert emb_only.M == 6 and emb_only.mem_emb.shape[0] == sum(N_EMB[:6])
    live.append(emb[4:5], pts[4:5], colors=col[4:5])
    assert live.M == 5 and live.grid.info()["n"] == sum(SIZES[:5])
    live.close()
