"""-m gpu: live object memory, replacement.  A memory whose instances are changed where they are while it is resident
(ibl_memgrid_replace, MemoryShard(live=True).replace, ObjectMemory.update_objects / merge_objects) holds, array for array, what a
memory built from the edited instance list holds, and localises to the same results bit for bit.  Every comparison is with an object
built fresh from the edited lists.  tests/test_live_replace_model.py shows that the replacement sets contain the cases they are named
for."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from tests import live_replace_cases as rc
from tests.live_replace_cases import CELL, SIZES, THR
from tests.live_memory_helpers import (assert_same_features, assert_same_grid, assert_same_results, exported, frame_of, grid_state, pick,
                                       point_distances, pts4_of, queries, run_frames, same_bits)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(2 << 30)
    yield c
    c.close()


def grid_replace(grid, sizes, instances, clouds, colors):
    """replaces the instances of a grid over clouds of `sizes` points: one range per instance, neighbours not joined"""
    ranges, counts = rc.replace_args(sizes, instances, clouds)
    grid.replace(ranges, counts, pts4_of(rc.ordered(instances, clouds), rc.ordered(instances, colors)))


@pytest.mark.parametrize("name", sorted(rc.REPLACE_SETS))
def test_replaced_grid_equals_fresh_build(ctx, name):
    from ibloc_amd.registration import MemGrid
    _, _, _, pts, col = rc.world()
    instances, clouds, colors = rc.replacements(name)
    pts2, col2 = rc.spliced(pts, instances, clouds), rc.spliced(col, instances, colors)
    q = queries(list(pts) + list(clouds))                   # around the old and the new clouds
    live = MemGrid(ctx, pts4_of(pts, col), CELL, live=True, reserve_points=1000)
    cap = live.info()["point_capacity"]
    before = point_distances(ctx, live, q)[0]
    grid_replace(live, SIZES, instances, clouds, colors)
    fresh = MemGrid(ctx, pts4_of(pts2, col2), CELL)
    d2 = assert_same_grid(ctx, live, fresh, q)
    # the queries see the replacement: the points are where a k-d tree finds them, before and after
    tree = lambda clouds_: cKDTree(np.concatenate(clouds_).astype(np.float32).astype(np.float64))   # noqa: E731
    dmin_old, dmin = tree(pts).query(q.astype(np.float64))[0], tree(pts2).query(q.astype(np.float64))[0]
    assert np.isfinite(before[dmin_old < THR * 0.999]).all() and np.isinf(before[dmin_old > THR * 1.001]).all()
    assert np.isfinite(d2[dmin < THR * 0.999]).all() and np.isinf(d2[dmin > THR * 1.001]).all()
    # fresh samples of a surface: queries 4 mm off a removed point lose it, those off a new one find it (hundreds of each; a moved
    # cloud loses and finds all of them)
    lost, found = (np.isfinite(before) & (dmin_old < dmin)).sum(), (np.isfinite(d2) & (dmin < dmin_old)).sum()
    assert lost > 50 and found > 50, (lost, found)
    if name == "moved":
        assert (np.isfinite(before) & np.isinf(d2)).sum() > 50 and (np.isinf(before) & np.isfinite(d2)).sum() > 50
    assert live.info()["point_capacity"] >= cap             # capacities do not shrink
    fresh.close()
    live.close()


def test_replace_is_append_and_remove(ctx):
    from ibloc_amd.registration import MemGrid
    _, _, _, pts, col = rc.world()
    q = queries(pts)
    n6 = sum(SIZES[:6])

    def grids():
        return [MemGrid(ctx, pts4_of(pts[:6], col[:6]), CELL, live=True, reserve_points=500) for _ in range(2)]

    # one empty range at n is the append (the buffer of 500 spare points has to grow for the 1 300 new ones, in both)
    a, b = grids()
    a.append(pts4_of(pts[6:], col[6:]))
    b.replace([(n6, n6)], [SIZES[6] + SIZES[7]], pts4_of(pts[6:], col[6:]))
    assert_same_grid(ctx, b, a, q)
    assert a.info() == b.info()
    # ... and the index bookkeeping is the append's: the same removal from both gives the same grid
    for g in (a, b):
        g.remove([(300, 820), (n6, n6 + SIZES[6])])
    assert_same_grid(ctx, b, a, q)
    a.close(), b.close()
    # counts of 0 are the removal
    a, b = grids()
    ranges = [(0, 300), (300, 820), (1620, 2030)]
    a.remove(ranges)
    b.replace(ranges, [0, 0, 0], torch.empty((0, 4), dtype=torch.float32, device="cuda"))
    assert_same_grid(ctx, b, a, q)
    assert a.info() == b.info()
    for g in (a, b):
        g.append(pts4_of(pts[:1], col[:1]))
        g.remove([(10, 500)])
    assert_same_grid(ctx, b, a, q)
    a.close(), b.close()
    # insertions at index 0 and in the middle (in front of instance 3), a removal between them
    live = MemGrid(ctx, pts4_of(pts[:6], col[:6]), CELL, live=True, reserve_points=0)
    live.replace([(0, 0), (300, 820), (1620, 1620)], [SIZES[7], 0, SIZES[6]], pts4_of([pts[7], pts[6]], [col[7], col[6]]))
    order = [7, 0, 2, 6, 3, 4, 5]
    fresh = MemGrid(ctx, pts4_of(pick(pts, order), pick(col, order)), CELL)
    assert_same_grid(ctx, live, fresh, q)
    fresh.close()
    # the renumbered indices: instance 6 now sits at [1 660, 2 400) and goes again
    live.remove([(SIZES[7] + SIZES[0] + SIZES[2], SIZES[7] + SIZES[0] + SIZES[2] + SIZES[6])])
    order.remove(6)
    fresh = MemGrid(ctx, pts4_of(pick(pts, order), pick(col, order)), CELL)
    assert_same_grid(ctx, live, fresh, q)
    fresh.close()
    live.close()


@pytest.mark.parametrize("cell,thr", [(CELL, THR), (rc.FINE_CELL, rc.FINE_THR)], ids=["4cm", "1cm"])
def test_edits_interleaved(ctx, cell, thr):
    """replace -> remove -> append -> replace of an appended instance -> a replace that needs the point buffer to grow, each step
    against a fresh build: a wrong renumbering of the per-slot indices shows at the next step that searches them"""
    from ibloc_amd.registration import MemGrid
    _, _, _, pts, col = rc.world()
    q = queries(pts)
    have = [(pts[i], col[i]) for i in range(6)]             # the clouds the grid holds, in order
    live = MemGrid(ctx, pts4_of([p for p, _ in have], [c for _, c in have]), cell, live=True, reserve_points=200)
    caps, tables = [live.info()["point_capacity"]], [live.info()["table_slots"]]

    def check():
        fresh = MemGrid(ctx, pts4_of([p for p, _ in have], [c for _, c in have]), cell)
        assert_same_grid(ctx, live, fresh, q, thr)
        fresh.close()
        caps.append(live.info()["point_capacity"])
        tables.append(live.info()["table_slots"])
        assert caps[-1] >= caps[-2] and caps[-1] >= live.info()["n"] == sum(len(p) for p, _ in have)

    def replace(positions, new):
        grid_replace(live, [len(p) for p, _ in have], positions, [p for p, _ in new], [c for _, c in new])
        for i, x in zip(positions, new):
            have[i] = x
        check()

    s_first, s_mid, s_touch = rc.replacements("first"), rc.replacements("middle_shared"), rc.replacements("touching")
    replace([3, 0], [(s_mid[1][0], s_mid[2][0]), (s_first[1][0], s_first[2][0])])          # (given out of order: 3 same size, 0 grows)
    assert caps[-1] == caps[0] + caps[0] // 2                                               # 340 more points than 200 spare ones: grown by 1.5
    live.remove([(sum(len(p) for p, _ in have[:1]), sum(len(p) for p, _ in have[:2]))])    # instance 1 goes
    del have[1]
    check()
    live.append(pts4_of([pts[6], pts[7]], [col[6], col[7]]))
    have += [(pts[6], col[6]), (pts[7], col[7])]
    check()
    last = rc.replacements("last")
    replace([6], [(last[1][0], last[2][0])])                # the appended twin (was instance 7) shrinks: shares cells with 0 and 3
    back = [3, 1, 2, 4]                                     # (rows of instance 4 are then resident twice, bit for bit)
    replace([1, 2], [(s_touch[1][1], s_touch[2][1]), (np.concatenate(pick(pts, back)), np.concatenate(pick(col, back)))])
    assert caps[-1] == caps[-2] + caps[-2] // 2 and live.info()["n"] > caps[-2]               # 5 490 points into 4 890: grown again
    if cell == rc.FINE_CELL:
        assert len(set(tables)) > 1, tables                 # thousands of 1 cm cells: the table dimension changed on the way
    live.close()


def test_grid_refusals_touch_nothing(ctx):
    from ibloc_amd import _lib
    from ibloc_amd.registration import MemGrid, RegContext
    _, _, _, pts, col = rc.world()
    q = queries(pts)
    n = sum(SIZES)
    new = pts4_of(pts[:1], col[:1])                         # 300 rows
    fixed = MemGrid(ctx, pts4_of(pts, col), CELL)
    live = MemGrid(ctx, pts4_of(pts, col), CELL, live=True, reserve_points=100)
    cases = [(fixed, [(0, 300)], [300], "a grid built without live"),
             (live, [(820, 1620), (0, 300)], [100, 200], "unsorted"),
             (live, [(0, 400), (300, 820)], [100, 200], "overlapping"),
             (live, [(300, 200)], [300], "reversed"),
             (live, [(-5, 10)], [300], "before 0"),
             (live, [(n - 10, n + 1)], [300], "past n"),
             (live, [(n + 1, n + 1)], [300], "an insertion past n"),
             (live, [(300, 300), (300, 820)], [100, 200], "two ranges with the same begin"),
             (live, [(0, 300), (500, 500)], [300, 0], "an empty range with count 0"),
             (live, [(0, 300), (500, 600)], [301, -1], "a negative count"),
             (live, [(0, 300), (300, n)], [0, 0], "an empty result")]
    for grid, ranges, counts, what in cases:
        before = grid_state(ctx, grid, q)
        with pytest.raises(_lib.IblError):
            grid.replace(ranges, counts, new[:sum(counts)])
        assert grid_state(ctx, grid, q) == before, what
    before = grid_state(ctx, live, q)
    one, cnt = (C.c_int64 * 1)(0), (C.c_int64 * 1)(300)       # null pointers with n_ranges > 0, which MemGrid.replace cannot pass
    end = (C.c_int64 * 1)(300)
    for rb, re, nc, p in ((None, end, cnt, new.data_ptr()), (one, None, cnt, new.data_ptr()), (one, end, None, new.data_ptr()),
                          (one, end, cnt, None), (None, None, None, None)):
        assert _lib.lib.ibl_memgrid_replace(ctx.handle, live.handle, rb, re, nc, p, 1, None) != 0
        assert grid_state(ctx, live, q) == before
    assert _lib.lib.ibl_memgrid_replace(None, live.handle, one, end, cnt, new.data_ptr(), 1, None) != 0
    assert _lib.lib.ibl_memgrid_replace(ctx.handle, None, one, end, cnt, new.data_ptr(), 1, None) != 0
    live.replace([], [], new[:0])                             # n_ranges == 0 changes nothing
    assert grid_state(ctx, live, q) == before
    # an arena too small (1 MiB, the smallest there is) for the scratch of 60 000 new points (40 B each): refused before anything is
    # launched, with the other half of the point buffers not yet touched either
    small, many = RegContext(1 << 20), torch.zeros((60000, 4), dtype=torch.float32, device="cuda")
    cnt[0] = 60000
    assert _lib.lib.ibl_memgrid_replace(small.handle, live.handle, one, end, cnt, many.data_ptr(), 1, None) != 0
    assert "arena" in _lib.lib.ibl_last_error().decode()
    small.close()
    assert grid_state(ctx, live, q) == before
    live.replace([(0, 300)], [300], new)                      # (and the grid still works: instance 0 by itself is no change)
    assert grid_state(ctx, live, q) == before
    fixed.close()
    live.close()


def shard_edit():
    """instances [5, 2] (given out of order) of the world: E 4 -> 6 and 4 -> 1, 380 -> 900 and 800 -> 450 points"""
    _, objects, emb, pts, col = rc.world()
    instances = [5, 2]
    new_emb = [rc.fresh_embeddings(5, 6), rc.fresh_embeddings(2, 1)]
    assert [len(emb[i]) for i in instances] == [4, 4]
    samples = [objects[5].sample(900, np.random.default_rng(91)), objects[2].sample(450, np.random.default_rng(92))]
    clouds, colors = [np.ascontiguousarray(s[0]) for s in samples], [np.ascontiguousarray(s[1]) for s in samples]
    return instances, new_emb, clouds, colors


@pytest.mark.parametrize("room", ["headroom", "growing"])
@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
def test_resident_state_equals_rebuilt(ctx, compact, room):
    from ibloc_amd.engine import MemoryShard
    _, _, emb, pts, col = rc.world()
    instances, new_emb, clouds, colors = shard_edit()
    emb2, pts2, col2 = rc.spliced(emb, instances, new_emb), rc.spliced(pts, instances, clouds), rc.spliced(col, instances, colors)
    plain = MemoryShard(ctx, emb2, pts2, colors=col2, compact_features=compact)
    reserve = dict(reserve_points=1200, reserve_rows=7) if room == "headroom" else dict(reserve_points=10, reserve_rows=0)
    live = MemoryShard(ctx, emb, pts, colors=col, compact_features=compact, live=True, **reserve)
    early = live.features(0.05, 0.4)                       # resident before the replacement ...
    bufs = (live.clouds._buf.data_ptr(), early.fpfh.data_ptr(), early.normals.data_ptr())
    cap = live.grid.info()["point_capacity"]
    live.replace(instances, new_emb, clouds, colors=colors)
    assert live.features(0.05, 0.4) is early
    # 4 360 -> 4 530 points: in place with 1 200 spare points, every point buffer grown by 1.5 with 10 (the 23 -> 22 embedding rows
    # fit either way: tests/test_live_replace_model.py and test_replace_refusals_touch_nothing grow such a buffer)
    now = (live.clouds._buf.data_ptr(), early.fpfh.data_ptr(), early.normals.data_ptr())
    if room == "headroom":
        assert now == bufs and live.grid.info()["point_capacity"] == cap
    else:
        assert all(a != b for a, b in zip(now, bufs)) and live.grid.info()["point_capacity"] == cap + cap // 2
        assert live.clouds._buf.shape[0] == early.fpfh.untyped_storage().nbytes() // (33 * 4) == cap + cap // 2
    assert (live.M, live.lo, live.hi) == (plain.M, plain.lo, plain.hi) == (8, 0, 8)
    assert same_bits(live.mem_emb, plain.mem_emb) and same_bits(live.emb_offsets, plain.emb_offsets)
    assert same_bits(live.emb_offsets_host, plain.emb_offsets_host)
    assert same_bits(live.clouds.pts4, plain.clouds.pts4) and same_bits(live.clouds.seg_off, plain.clouds.seg_off)
    assert same_bits(live.clouds.seg_off_host, plain.clouds.seg_off_host)
    n = sum(len(p) for p in pts2)
    assert_same_features(early, plain.features(0.05, 0.4), n, 8, compact)
    assert_same_features(live.features(0.05, 1.5), plain.features(0.05, 1.5), n, 8, compact)      # ... and requested after it
    assert_same_grid(ctx, live.grid, plain.grid, queries(list(pts) + clouds))
    live.close()
    plain.close()


def world_frames():
    """frames of the objects 1, 2, 4, 5, 6 and 7 (instance 3 of this world is a second twin of object 0: no frame asks for it)"""
    w = rc.world()[0]
    rng = np.random.default_rng(74)
    return [frame_of(w, rng, ids) for ids in ([7, 4, 6], [5, 2, 1], [2, 4], [6, 1, 5])]


def test_localise_after_replace_equals_rebuilt(ctx):
    from ibloc_amd.engine import LocaliseEngine, MemoryShard
    _, objects, emb, pts, col = rc.world()
    # the instances 2 and 5 seen again: the stored embeddings stay, one more each, and fresh samples of other sizes as clouds
    instances = [2, 5]
    new_emb = [np.concatenate([emb[i], rc.fresh_embeddings(i, 1, seed=1)]) for i in instances]
    samples = [objects[2].sample(520, np.random.default_rng(93)), objects[5].sample(760, np.random.default_rng(94))]
    clouds, colors = [np.ascontiguousarray(s[0]) for s in samples], [np.ascontiguousarray(s[1]) for s in samples]
    frames = world_frames()
    plain = MemoryShard(ctx, rc.spliced(emb, instances, new_emb), rc.spliced(pts, instances, clouds), colors=rc.spliced(col, instances, colors))
    ref = run_frames(LocaliseEngine(plain), frames)
    assert any(r.best >= 0 and r.records for r in ref)
    assert any(m in instances for r in ref if r.best >= 0 for _, m in r.assignments[r.best])      # a winner names a replaced instance
    live = MemoryShard(ctx, emb, pts, colors=col, live=True)
    eng = LocaliseEngine(live)
    run_frames(eng, frames[3:])                                     # the engine has served a query before the memory changes
    live.replace(instances, new_emb, clouds, colors=colors)
    assert_same_results(run_frames(eng, frames), ref)
    for m in (plain, live):
        m.close()


def test_object_memory_updates_the_resident_engine():
    from ibloc_amd.object_memory.object_memory import ObjectMemory
    from ibloc_amd.utils.fpfh_register import Cloud
    _, objects, emb, pts, col = rc.world()
    frames = world_frames()
    again = objects[4].sample(500, np.random.default_rng(95))       # object 4 seen a second time
    again_emb = rc.fresh_embeddings(4, 1, seed=2)[0]

    def memory(live):
        om = ObjectMemory("cuda", None, None, 300.0, 300.0, get_embeddings_func=lambda **kw: None, log_enabled=False, arena_bytes=2 << 30)
        om.live_memory = live
        for j in range(8):
            om.add_object(f"obj{j}", list(emb[j]), pts[j], col[j])
        return om

    def query(om, f):
        return om.localise_detections(f["det_emb"], f["clouds"], fpfh_global_dist_factor=1.5, fpfh_local_dist_factor=1.5)

    def edits(om, check):
        query(om, frames[3])
        check("start")
        om.memory[4].add_info("obj4 again", again_emb, Cloud(again[0], again[1]))
        om.update_objects([4])
        check("update")
        first = query(om, frames[0])                                # sees 7, 4, 6
        ids = [o.id for o in om.memory]
        om.merge_objects(0, 7)                                      # the twin is the same object
        assert [o.id for o in om.memory] == ids[:7] and len(om.memory[0].embeddings) == len(emb[0]) + len(emb[7])
        assert om.memory[0].pointcloud.points.shape[0] == SIZES[0] + SIZES[7]
        check("merge")
        return first, query(om, frames[1]), query(om, frames[2])    # see 5, 2, 1 and 2, 4

    rebuilt = memory(False)
    ref = edits(rebuilt, lambda what: None)
    assert all(r.records for r in ref) and rebuilt._engine is not None and rebuilt._shard.M == 7
    om = memory(True)
    kept = {}

    def same_engine(what):
        assert om._engine is not None
        kept.setdefault("engine", (om._engine, om._shard))
        assert (om._engine, om._shard) == kept["engine"], what
    assert_same_results(list(edits(om, same_engine)), list(ref))
    assert om._shard.M == 7 and om._shard.clouds.n == sum(SIZES) + 500
    with pytest.raises(ValueError):
        om.update_objects([0, 0])
    with pytest.raises(ValueError):
        om.update_objects([7])
    with pytest.raises(ValueError):
        om.merge_objects(2, 2)
    assert (om._engine, om._shard) == kept["engine"] and len(om.memory) == 7
    om._ctx.close()
    rebuilt._ctx.close()


def test_replace_refusals_touch_nothing(ctx):
    from ibloc_amd.engine import MemoryShard
    _, _, emb, pts, col = rc.world()
    D = emb[0].shape[1]

    def state(m):
        arrays = [m.mem_emb, m.emb_offsets] + ([] if m.clouds is None else [m.clouds.pts4, m.clouds.seg_off])
        for f in m._features.values():
            arrays += [getattr(f, name) for name in f.DEVICE_ARRAYS if getattr(f, name) is not None]
        return (m.M, m.lo, m.hi, m.emb_offsets_host.tobytes(), None if m.clouds is None else m.clouds.seg_off_host.tobytes(),
                None if m.grid is None else tuple(sorted(m.grid.info().items())), [a.cpu().numpy().tobytes() for a in arrays],
                None if m.grid is None else [v.tobytes() for v in exported(m.grid).values()])

    def refused(m, instances, embeddings, clouds="same", colors=None):
        if clouds == "same":
            clouds, colors = pick(pts, [1] * len(embeddings)), pick(col, [1] * len(embeddings))
        before = state(m)
        with pytest.raises(ValueError):
            m.replace(instances, embeddings, clouds, colors=colors)
        assert state(m) == before

    refused(MemoryShard(ctx, emb[:4], pts[:4], colors=col[:4], shard=(0, 1)), [1], [emb[1]])       # sharded
    refused(MemoryShard(ctx, emb[:4], pts[:4], colors=col[:4]), [1], [emb[1]])                     # not live
    live = MemoryShard(ctx, emb[:4], pts[:4], colors=col[:4], live=True)
    live.features(0.05, 0.4)
    refused(live, [4], [emb[1]])                                                                   # out of range
    refused(live, [-1], [emb[1]])
    refused(live, [1, 2, 1], [emb[1]] * 3)                                                         # a duplicate
    refused(live, [1, 2], [emb[1]])                                                                # fewer embeddings than instances
    refused(live, [1], [emb[1]], clouds=[pts[1], pts[2]], colors=[col[1], col[2]])                 # more clouds than instances
    refused(live, [1], [emb[1]], clouds=[pts[1]], colors=[col[1], col[2]])                         # more colours than clouds
    refused(live, [1], [np.zeros((2, D + 1), np.float32)])                                         # another embedding dimension
    refused(live, [1], [np.zeros((0, D), np.float32)])                                             # no embedding
    refused(live, [1], [emb[1]], clouds=[np.zeros((0, 3))], colors=[np.zeros((0, 3))])             # an empty cloud
    refused(live, [1], [emb[1]], clouds=None)                                                      # clouds withheld
    before = state(live)
    live.replace([], [], [], colors=[])                                                            # a no-op
    assert state(live) == before
    emb_only = MemoryShard(ctx, emb[:4], live=True, reserve_rows=0)
    refused(emb_only, [1], [emb[1]])                                                               # clouds given to an embedding-only memory
    more = np.concatenate([emb[6], emb[2]])                                                        # 11 -> 15 rows: the buffer has to grow
    emb_only.replace(iter([2, 0]), [emb[5], more])                                                 # (any iterable, any order: rows only)
    rebuilt = MemoryShard(ctx, [more, emb[1], emb[5], emb[3]])
    assert emb_only.M == 4 and same_bits(emb_only.mem_emb, rebuilt.mem_emb) and same_bits(emb_only.emb_offsets, rebuilt.emb_offsets)
    assert emb_only._emb_buf.shape[0] == 16                                                        # 11 + 11 // 2
    live.replace([0], [emb[5]], [pts[5]], colors=[col[5]])
    assert live.M == 4 and live.grid.info()["n"] == sum(SIZES[1:4]) + SIZES[5]
    live.close()
