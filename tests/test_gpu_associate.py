"""-m gpu: live memory, association.  ibl_memgrid_overlap (MemGrid.overlap, MemoryShard.overlap) returns, for every detection, exactly
the hits of the brute force of tests/associate_cases.py -- an integer per (detection, instance), demanded equal -- on fresh and on
edited grids, and ObjectMemory.process_detections(associate=True) merges re-observations into their instances while the resident
memory stays what a rebuilt one is.  tests/test_associate_model.py shows on the CPU that the cases contain what they are named for."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import associate_cases as ac
from tests.associate_cases import CELL, R_CELL, R_EDGE, R_HALF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(1 << 30)
    yield c
    c.close()


def batch(clouds):
    from ibloc_amd.registration import CloudBatch
    return CloudBatch.from_numpy([np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds])


def device_overlap(ctx, insts, dets, r, k):
    from ibloc_amd.registration import MemGrid
    mem, det = batch(insts), batch(dets)
    grid = MemGrid(ctx, mem.pts4, CELL, live=True)
    out = grid.overlap(det.pts4, det.seg_off_host, mem.seg_off, r, k, inst_off_end=mem.n)
    grid.close()
    return out


def assert_pairs(got, want):
    for g, w, name in zip(got, want, ("inst", "hits", "n_hit_inst")):
        assert g.dtype == np.int32 and g.shape == w.shape and (g == w).all(), (name, g.tolist(), w.tolist())


def assert_equals_brute_force(ctx, insts, dets, r, k=None):
    """the full non-zero list of every detection (k >= n_inst) equals the brute force: every (detection, instance) entry"""
    H = ac.brute_hits(dets, insts, r)
    k = len(insts) + 3 if k is None else k
    assert_pairs(device_overlap(ctx, insts, dets, r, k), ac.expected_pairs(H, k))
    return H


@pytest.mark.parametrize("r", [R_HALF, R_CELL], ids=["half_cell", "cell"])
def test_small_world(ctx, r):
    insts, dets = ac.small_world()
    H = assert_equals_brute_force(ctx, insts, dets, r)
    assert (H > 0).sum() >= 6 and (H[3] == 0).all()
    assert_equals_brute_force(ctx, insts, dets, r, k=1)                 # the cut: the best candidate alone


def test_crowded_point(ctx):
    insts, dets = ac.crowded()
    H = assert_equals_brute_force(ctx, insts, dets, R_HALF)
    assert H.tolist() == [[1] * 12]
    assert_equals_brute_force(ctx, insts, dets, R_CELL)


def test_radius_edge(ctx):
    insts, dets, expect = ac.radius_edge()
    H = assert_equals_brute_force(ctx, insts, dets, R_EDGE)
    assert H.tolist() == [list(expect)]


def test_one_instance_in_all_eight_cells(ctx):
    insts, dets = ac.eight_cells()
    H = assert_equals_brute_force(ctx, insts, dets, R_HALF)
    assert H.tolist() == [[1, 1]]


def test_more_than_k_hits(ctx):
    insts, dets = ac.over_k()
    inst, hits, n_hit = device_overlap(ctx, insts, dets, R_HALF, ac.OVER_K)
    assert n_hit.tolist() == [7]
    assert inst.tolist() == [[0, 1, 3, 5]] and hits.tolist() == [[3, 3, 2, 2]]
    assert_equals_brute_force(ctx, insts, dets, R_HALF, k=ac.OVER_K)
    assert_equals_brute_force(ctx, insts, dets, R_HALF)


def test_empty_and_far_detections(ctx):
    insts, dets = ac.empty_and_far()
    assert len(dets[1]) == 0
    assert_equals_brute_force(ctx, insts, dets, R_HALF)
    inst, hits, n_hit = device_overlap(ctx, insts, dets, R_HALF, 4)
    assert n_hit[1] == 0 and n_hit[3] == 0 and n_hit[0] > 0 and n_hit[2] > 0
    for d in (1, 3):
        assert inst[d].tolist() == [-1] * 4 and hits[d].tolist() == [0] * 4


def test_determinism(ctx):
    insts, dets = ac.small_world()
    a = device_overlap(ctx, insts, dets, R_CELL, 8)
    b = device_overlap(ctx, insts, dets, R_CELL, 8)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_edited_grids(ctx):
    """after append, after remove of a middle instance and after a replace that grows one instance and shrinks another, the edited
    shard answers as a shard freshly built from the same instances does, and as the brute force does: the per-slot original indices
    and their renumbering are what the instance lookup reads"""
    from ibloc_amd.engine import MemoryShard
    insts, dets = ac.small_world()
    have = [np.asarray(p) for p in insts]
    emb = [np.random.default_rng(20 + i).normal(size=(2, 8)).astype(np.float32) for i in range(8)]
    det = batch(dets)
    live = MemoryShard(ctx, emb[:5], have[:5], live=True, reserve_points=100)

    def check(clouds, embs, r):
        k = len(clouds) + 2
        fresh = MemoryShard(ctx, embs, clouds, live=True)
        got, ref = live.overlap(det, radius=r, k=k), fresh.overlap(det, radius=r, k=k)
        fresh.close()
        assert_pairs(got, ref)
        assert_pairs(got, ac.expected_pairs(ac.brute_hits(dets, clouds, r), k))

    live.append(emb[5:6], have[5:6])                                     # 280 points into 100 spare ones: the buffers grow
    cur, cur_emb = have[:6], emb[:6]
    check(cur, cur_emb, R_HALF)
    live.remove([2])                                                     # a middle instance: the later ones are renumbered
    cur, cur_emb = cur[:2] + cur[3:], cur_emb[:2] + cur_emb[3:]
    check(cur, cur_emb, R_HALF)
    check(cur, cur_emb, R_CELL)
    grown = np.concatenate([cur[1], np.asarray(dets[1]), np.asarray(dets[4])[:60]])      # instance 1 takes in two detections' points
    shrunk = cur[3][:90]                                                                  # the former instance 4 loses most of its own
    live.replace([3, 1], [emb[6], emb[7]], [shrunk, grown])
    cur = [cur[0], grown, cur[2], shrunk, cur[4]]
    cur_emb = [cur_emb[0], emb[7], cur_emb[2], emb[6], cur_emb[4]]
    check(cur, cur_emb, R_HALF)
    check(cur, cur_emb, R_CELL)
    assert live.overlap(det)[0].shape == (len(dets), 8)                  # the defaults: radius = eval_threshold, k = 8
    assert_pairs(live.overlap(det), ac.expected_pairs(ac.brute_hits(dets, cur, live.eval_threshold), 8))
    live.close()


S = np.int32(0x5A5A5A5A)


def test_refusals_launch_nothing(ctx):
    from ibloc_amd import _lib, prof
    from ibloc_amd.engine import MemoryShard
    from ibloc_amd.registration import MemGrid, RegContext
    insts, dets = ac.small_world()
    mem, det = batch(insts), batch(dets)
    live, fixed = MemGrid(ctx, mem.pts4, CELL, live=True), MemGrid(ctx, mem.pts4, CELL)
    n_inst, n_det, k = mem.n_seg, det.n_seg, 4
    o_inst, o_hits, o_n = (np.full(n_det * k, S, np.int32), np.full(n_det * k, S, np.int32), np.full(n_det, S, np.int32))
    st = torch.cuda.current_stream().cuda_stream
    call = _lib.lib.ibl_memgrid_overlap
    off = det.seg_off_host
    down = off.copy()
    down[2] = down[1] - 1

    def refused(what, grid=live, end=mem.n, offsets=off, r=R_HALF, k_=k, n_inst_=n_inst, ptrs=None, nd=n_det):
        io, de, oi, oh, on = ptrs or (mem.seg_off.data_ptr(), det.pts4.data_ptr(), o_inst.ctypes.data, o_hits.ctypes.data, o_n.ctypes.data)
        status = call(ctx.handle, grid.handle, io, n_inst_, end, de, offsets.ctypes.data, nd, float(r), k_, oi, oh, on, st)
        assert status < 0, what
        msg = _lib.lib.ibl_last_error().decode()
        assert "ibl_memgrid_overlap" in msg, (what, msg)
        return msg

    prof.reset(True)
    assert "live" in refused("an immutable grid", grid=fixed)
    assert "cell" in refused("radius > cell", r=CELL * 1.001)
    assert "positive" in refused("radius 0", r=0.0)
    assert "positive" in refused("radius < 0", r=-0.02)
    assert "positive" in refused("radius nan", r=float("nan"))
    assert "k = 0" in refused("k = 0", k_=0)
    refused("k < 0", k_=-3)
    assert "end at" in refused("an offset end short of n", end=mem.n - 1)
    refused("an offset end past n", end=mem.n + 1)
    assert "descends" in refused("descending detection offsets", offsets=down)
    refused("no instances", n_inst_=0)
    refused("n_det < 0", nd=-1)
    good = (mem.seg_off.data_ptr(), det.pts4.data_ptr(), o_inst.ctypes.data, o_hits.ctypes.data, o_n.ctypes.data)
    for hole in range(5):
        refused(f"null pointer {hole}", ptrs=tuple(None if i == hole else p for i, p in enumerate(good)))
    assert call(None, live.handle, *good[:1], n_inst, mem.n, good[1], off.ctypes.data, n_det, R_HALF, k, *good[2:], st) < 0
    assert call(ctx.handle, None, *good[:1], n_inst, mem.n, good[1], off.ctypes.data, n_det, R_HALF, k, *good[2:], st) < 0
    # an arena too small (1 MiB, the smallest there is) for 2 x 5 x 200 000 output entries: the arena error, before any launch
    small = RegContext(1 << 20)
    big = np.full(n_det * 200000, S, np.int32)
    assert call(small.handle, live.handle, good[0], n_inst, mem.n, good[1], off.ctypes.data, n_det, R_HALF, 200000, big.ctypes.data,
                big.ctypes.data, o_n.ctypes.data, st) < 0
    assert "arena" in _lib.lib.ibl_last_error().decode()
    small.close()
    assert (big == S).all()
    # no detections: success, and still nothing launched
    assert call(ctx.handle, live.handle, good[0], n_inst, mem.n, None, off.ctypes.data, 0, R_HALF, k, *good[2:], st) == 0
    torch.cuda.synchronize()
    assert (o_inst == S).all() and (o_hits == S).all() and (o_n == S).all()
    assert prof.read(prof.ST_ASSOC)[2] == 0                              # the stage's timer never started
    # ... and the same arrays are written by a call that is accepted (radius == cell included)
    assert call(ctx.handle, live.handle, *good[:1], n_inst, mem.n, good[1], off.ctypes.data, n_det, R_CELL, k, *good[2:], st) == 0
    assert prof.read(prof.ST_ASSOC)[2] == 1
    prof.reset(False)
    assert_pairs((o_inst.reshape(n_det, k), o_hits.reshape(n_det, k), o_n), ac.expected_pairs(ac.brute_hits(dets, insts, R_CELL), k))
    with pytest.raises(_lib.IblError):
        fixed.overlap(det.pts4, off, mem.seg_off, R_HALF, k)
    live.close(), fixed.close()
    # the shard: sharded, not live and embedding-only memories raise ValueError before anything is touched
    emb = [np.random.default_rng(30 + i).normal(size=(2, 8)).astype(np.float32) for i in range(6)]
    clouds = [np.asarray(p) for p in insts]
    for shard in (MemoryShard(ctx, emb, clouds, shard=(0, 1)), MemoryShard(ctx, emb, clouds), MemoryShard(ctx, emb, live=True)):
        with pytest.raises(ValueError):
            shard.overlap(det)
        shard.close()


# ---- the facade ----------------------------------------------------------------------------------------------------------------------
def facade_memory(live):
    from ibloc_amd.object_memory.object_memory import ObjectMemory
    f = ac.facade()
    om = ObjectMemory("cuda", None, None, 300.0, 300.0, get_embeddings_func=lambda **kw: None, log_enabled=False, arena_bytes=2 << 30)
    om.live_memory = live
    for j in range(4):
        om.add_object(f"obj{j}", list(f["embeddings"][j]), f["points"][j], f["colors"][j])
    return om


def facade_frames():
    w = ac.facade()["world"]
    rng = np.random.default_rng(417)
    return [w.make_frame(rng, q=2, pts_per_object=800, anchor=a) for a in (1, 3)]


def facade_query(om, f):
    return om.localise_detections(f["det_emb"], f["clouds"], fpfh_global_dist_factor=1.5, fpfh_local_dist_factor=1.5)


def facade_run(om, associate, after_first=lambda: None):
    """one localise(), the four detections, two more localise(): (decisions, results)"""
    f = ac.facade()
    frames = facade_frames()
    first = facade_query(om, frames[0])
    after_first()
    pose = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    decisions = om.process_detections(list(f["phrases"]), list(f["det_embs"]), list(f["det_clouds"]), pose, associate=associate)
    return decisions, [first, facade_query(om, frames[1]), facade_query(om, frames[0])]


def test_facade_merges_reobservations_in_the_resident_memory():
    from ibloc_amd.engine import MemoryShard
    from tests.test_gpu_live_memory_replace import assert_same_features, assert_same_grid, assert_same_results, queries, same_bits
    f = ac.facade()
    rebuilt = facade_memory(False)
    ref_decisions, ref = facade_run(rebuilt, True)
    assert ref_decisions == f["expect"] and any(r.records and r.best >= 0 for r in ref)
    om = facade_memory(True)
    kept = {}

    def note_engine():
        kept["engine"] = (om._engine, om._shard)
        assert om._shard.live and om._shard._features                   # the features are resident before the memory is edited
    decisions, res = facade_run(om, True, note_engine)
    assert decisions == f["expect"] == [1, 3, None, None]
    assert (om._engine, om._shard) == kept["engine"]                    # edited where it is, never rebuilt
    assert len(om.memory) == 6 and [o.id for o in om.memory] == list(range(6))
    for d, m in ((0, 1), (1, 3)):
        info = om.memory[m]
        assert len(info.embeddings) == 3 and same_bits(info.embeddings[2], f["det_embs"][d])
        assert info.names == [f"obj{m}", f["phrases"][d]]
        assert info.pointcloud.points.shape[0] == 2500 + 1500 and same_bits(info.pointcloud.points[2500:], f["det_clouds"][d][0])
        assert same_bits(info.mean_emb, np.mean(np.array(info.embeddings), axis=0))
    for m in (0, 2):
        assert len(om.memory[m].embeddings) == 2 and om.memory[m].pointcloud.points.shape[0] == 2500
    assert om.memory[4].names == [f["phrases"][2]] and om.memory[5].names == [f["phrases"][3]]
    # the resident arrays are those of a shard built fresh from the list
    embs = [np.stack(m.embeddings).astype(np.float32) for m in om.memory]
    pts = [np.asarray(m.pointcloud.points) for m in om.memory]
    fresh = MemoryShard(om._ctx, embs, pts, colors=[np.asarray(m.pointcloud.colors) for m in om.memory])
    live = om._shard
    assert live.M == fresh.M == 6
    assert same_bits(live.mem_emb, fresh.mem_emb) and same_bits(live.emb_offsets, fresh.emb_offsets)
    assert same_bits(live.clouds.pts4, fresh.clouds.pts4) and same_bits(live.clouds.seg_off, fresh.clouds.seg_off)
    assert same_bits(live.clouds.seg_off_host, fresh.clouds.seg_off_host)
    n = sum(len(p) for p in pts)
    for key, feat in live._features.items():
        assert_same_features(feat, fresh.features(*key), n, 6, False)
    assert_same_grid(om._ctx, live.grid, fresh.grid, queries(pts))
    fresh.close()
    # ... and the next localise() calls are those of a memory rebuilt after every edit, bit for bit
    assert_same_results(res, ref)
    om._ctx.close()
    rebuilt._ctx.close()


def test_facade_without_associate_appends_every_detection():
    f = ac.facade()
    om = facade_memory(True)
    decisions, _ = facade_run(om, False)
    assert decisions is None and len(om.memory) == 8
    assert [o.names for o in om.memory[4:]] == [[p] for p in f["phrases"]]
    assert all(len(o.embeddings) == 2 and o.pointcloud.points.shape[0] == 2500 for o in om.memory[:4])
    # on an empty memory association appends everything, too
    empty = facade_memory(True)
    empty.memory, empty._engine = [], None
    pose = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    assert empty.process_detections(list(f["phrases"]), list(f["det_embs"]), list(f["det_clouds"]), pose, associate=True) == [None] * 4
    assert len(empty.memory) == 4
    # two detections of one call may choose the same instance: merged into it in order
    twice = facade_memory(True)
    d = twice.process_detections(["a", "b"], [f["det_embs"][0], f["det_embs"][0]], [f["det_clouds"][0], f["det_clouds"][0]], pose, associate=True)
    assert d == [1, 1] and len(twice.memory) == 4 and len(twice.memory[1].embeddings) == 4
    assert twice.memory[1].pointcloud.points.shape[0] == 2500 + 2 * 1500
    for m in (om, empty, twice):
        m._ctx.close()
