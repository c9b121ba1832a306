"""-m gpu: the oriented-box IoU matrix of memory consolidation on the device (csrc/obb_iou.hip, ibl_obb_iou_matrix) against the host loop
of ObjectMemory._recluster_IoU (1 - calculate_obj_aligned_3d_IoU pair by pair), closed forms, the driver's consolidation sequence with
iou_backend = "device", argument edges and a 5 000-fragment memory."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from oracle import build_oracle as bo

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(256 << 20)
    yield c
    c.close()


def box_points(rng, half, R=np.eye(3), t=np.zeros(3), n=600):
    p = rng.uniform(-1, 1, size=(n, 3)) * half
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
    return np.vstack([p, corners]) @ R.T + t


def parity_scene(seed):
    """~120 clouds: fragments of one object at small relative rotations, thin objects, nested boxes, exact duplicates, boxes sharing
    faces, boxes touching at a face / edge / vertex, far-apart boxes, and clouds without a box"""
    rng = np.random.default_rng(seed)
    c = []
    for k in range(21):
        ctr = np.array([k % 5 * 1.2, k // 5 * 1.2, 0.0]) + rng.uniform(-0.1, 0.1, 3)
        half = rng.uniform(0.05, 0.4, 3)
        if k % 3 == 0:
            half[k % 2] = 0.004                                                  # thin
        R = Rotation.random(random_state=rng).as_matrix()
        pts = box_points(rng, half, R, ctr, 3000)
        for _ in range(rng.integers(3, 7)):
            sel = rng.random(len(pts)) < 0.5
            Rf = Rotation.from_rotvec(rng.normal(size=3) * 0.05).as_matrix()
            c.append((pts[sel] - ctr) @ Rf.T + ctr)
    o = np.array([10.0, 0.0, 0.0])
    a = box_points(rng, np.array([0.4, 0.3, 0.2]), t=o)
    c += [a, a.copy()]                                                           # exact duplicates
    c += [box_points(rng, np.array([0.2, 0.1, 0.05]), Rotation.random(random_state=rng).as_matrix(), o)]     # nested
    c += [box_points(rng, np.array([0.1, 0.1, 0.1]), t=o + [0.05, -0.1, 0.02])]                           # nested, axis-aligned
    c += [box_points(rng, np.array([0.4, 0.3, 0.2]), t=o + [0.3, 0.0, 0.0])]   # shares four faces' planes with a
    c += [box_points(rng, np.array([0.2, 0.3, 0.2]), t=o + [0.2, 0.0, 0.0])]   # shares five face planes with a
    c += [a + [0.8, 0, 0], a + [0.8, 0.6, 0], a + [0.8, 0.6, 0.4], a + [0, -0.6, 0.4]]   # touching at a face, an edge, a vertex
    R45 = Rotation.from_euler("z", 45, degrees=True).as_matrix()
    c += [box_points(rng, np.array([0.2, 0.1, 0.1]), R45, o + [0.4 + 0.3 * np.sqrt(0.5) - 0.02, 0.0, 0.0])]   # a rotated corner dips in
    c += [box_points(rng, rng.uniform(0.05, 0.3, 3), Rotation.random(random_state=rng).as_matrix(), rng.uniform(-40, 40, 3)) for _ in range(8)]
    c += [a[:3], np.c_[rng.uniform(-1, 1, size=(40, 2)), np.full(40, 0.3)] + o, np.zeros((0, 3))]       # no box: 3 points, coplanar, empty
    return c


def host_matrix(clouds):
    from ibloc_amd.utils.IoU_ops import calculate_obj_aligned_3d_IoU
    n = len(clouds)
    D = np.ones((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            D[i, j] = D[j, i] = 1 - calculate_obj_aligned_3d_IoU(clouds[i], clouds[j])
    return D


@pytest.mark.parametrize("seed", [0, 1])
def test_matrix_equals_the_host_loop(ctx, seed):
    from ibloc_amd.build import oriented_box_distance_matrix
    clouds = parity_scene(seed)
    assert 100 <= len(clouds) <= 140
    Dd = oriented_box_distance_matrix(clouds, ctx)
    Dh = host_matrix(clouds)
    assert Dd.shape == Dh.shape and Dd.dtype == np.float64
    assert np.abs(Dd - Dh).max() <= TOL
    assert np.all(Dd[Dh == 1.0] == 1.0)                          # separated, touching and box-less pairs: exactly 1
    assert np.all(np.diag(Dd) == 1.0) and np.array_equal(Dd, Dd.T)
    assert (Dh < 1.0).sum() > 2 * len(clouds) and (Dh < 0.5).sum() > len(clouds)      # many overlapping pairs, strong ones among them
    assert np.all(Dd[-3:] == 1.0) and np.all(Dd[:, -3:] == 1.0)


def test_device_matrix_is_deterministic(ctx):
    from ibloc_amd.build import obb_iou_matrix
    from ibloc_amd.utils.IoU_ops import oriented_bounding_boxes
    boxes, valid = oriented_bounding_boxes(parity_scene(0))
    D1, n1 = obb_iou_matrix(ctx, boxes, valid, return_overlapping=True)
    D2, n2 = obb_iou_matrix(ctx, boxes, valid, return_overlapping=True)
    assert torch_equal(D1, D2) and n1 == n2 > 0


def torch_equal(a, b):
    import torch
    return bool(torch.equal(a, b))


def _row(c, R, h):
    return np.concatenate([np.asarray(c, float), np.asarray(R, float).reshape(9), np.asarray(h, float)])


def _iou(ctx, rows):
    from ibloc_amd.build import obb_iou_matrix
    D = obb_iou_matrix(ctx, np.array(rows), np.ones(len(rows), dtype=np.int32)).cpu().numpy()
    return 1 - D[0, 1]


def _clip(poly, clip):
    """area of the intersection of two convex polygons given counter-clockwise (Sutherland-Hodgman, written for this test)"""
    out = list(poly)
    for a, b in zip(clip, clip[1:] + clip[:1]):
        inside = lambda p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) >= 0
        src, out = out, []
        for p, q in zip(src, src[1:] + src[:1]):
            if inside(q):
                if not inside(p):
                    out.append(_cross(a, b, p, q))
                out.append(q)
            elif inside(p):
                out.append(_cross(a, b, p, q))
        if not out:
            return 0.0
    x, y = np.array(out).T
    return 0.5 * abs(x @ np.roll(y, -1) - y @ np.roll(x, -1))


def _cross(a, b, p, q):
    d1, d2 = np.subtract(b, a), np.subtract(q, p)
    t = ((a[0] - p[0]) * d1[1] - (a[1] - p[1]) * d1[0]) / (d2[0] * d1[1] - d2[1] * d1[0])
    return (p[0] + t * d2[0], p[1] + t * d2[1])


def test_closed_forms(ctx):
    rng = np.random.default_rng(8)
    for _ in range(20):                                          # identical boxes at random poses
        R = Rotation.random(random_state=rng).as_matrix()
        r = _row(rng.uniform(-50, 50, 3), R, rng.uniform(0.01, 1.0, 3))
        assert abs(_iou(ctx, [r, r]) - 1.0) <= 1e-12
    for _ in range(40):                                          # axis-aligned: product of the overlaps
        ca, cb = rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.5, 0.5, 3)
        ha, hb = rng.uniform(0.1, 0.6, 3), rng.uniform(0.1, 0.6, 3)
        ov = np.clip(np.minimum(ca + ha, cb + hb) - np.maximum(ca - ha, cb - hb), 0, None)
        inter = np.prod(ov)
        want = inter / (8 * np.prod(ha) + 8 * np.prod(hb) - inter)
        P = np.eye(3)[rng.permutation(3)] * rng.choice([-1, 1], 3)      # any labelling / sign of the axes
        P[:, 2] = np.cross(P[:, 0], P[:, 1])
        assert abs(_iou(ctx, [_row(ca, np.eye(3), ha), _row(cb, P, np.abs(P.T) @ hb)]) - want) <= 1e-12
    for deg in (10.0, 30.0, 45.0, 61.0, 90.0, 137.0):           # prisms turned about z: clipped rectangle x common height
        ha, hb = np.array([0.5, 0.2, 0.3]), np.array([0.45, 0.15, 0.2])
        t = np.array([0.05, 0.02, 0.07])
        Rz = Rotation.from_euler("z", deg, degrees=True).as_matrix()
        rect = lambda h, R, c: [tuple(R[:2, :2] @ np.array([sx * h[0], sy * h[1]]) + c[:2]) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        height = min(ha[2], t[2] + hb[2]) - max(-ha[2], t[2] - hb[2])
        inter = _clip(rect(ha, np.eye(3), np.zeros(3)), rect(hb, Rz, t)) * height
        want = inter / (8 * np.prod(ha) + 8 * np.prod(hb) - inter)
        assert 0.05 < want < 0.9
        assert abs(_iou(ctx, [_row(np.zeros(3), np.eye(3), ha), _row(t, Rz, hb)]) - want) <= 1e-12
    # cubes turned 45 deg about y and about x, stacked along z: their crossing edges are separated along z = e_y x e_x, an axis no
    # face normal gives; exactly 0 when apart, the host's exact volume when they dip into each other
    from ibloc_amd.utils.IoU_ops import oriented_box_intersection_volume
    R1 = Rotation.from_euler("y", 45, degrees=True).as_matrix()
    R2 = Rotation.from_euler("x", 45, degrees=True).as_matrix()
    h = np.full(3, 0.5)
    for gap, zero in ((1e-6, True), (0.0, True), (-0.05, False)):
        cb = np.array([0.0, 0.0, 2 * 0.5 * np.sqrt(2) + gap])
        got = _iou(ctx, [_row(np.zeros(3), R1, h), _row(cb, R2, h)])
        if zero:
            assert got == 0.0
        else:
            inter = oriented_box_intersection_volume((np.zeros(3), R1, h), (cb, R2, h))
            assert inter > 0 and abs(got - inter / (2 - inter)) <= 1e-12


def _memory(seed):
    """the consolidation input of the drivers: rotated objects (some thin) seen as 2-4 overlapping fragments, noisy embeddings"""
    rng = np.random.default_rng(seed)
    frags = []
    for k in range(10):
        c = np.array([(k % 4) * 1.5, (k // 4) * 1.5, 0.0]) + rng.uniform(-0.1, 0.1, size=3)
        half = rng.uniform(0.1, 0.35, size=3)
        if k % 4 == 1:
            half[2] = 0.01
        R = Rotation.random(random_state=rng).as_matrix()
        u = rng.uniform(-1, 1, size=(3000, 3))
        ax = rng.integers(0, 3, size=3000)
        u[np.arange(3000), ax] = np.sign(u[np.arange(3000), ax])
        pts = (u * half) @ R.T + c
        cols = np.clip(0.5 + 0.4 * np.sin(pts * 5 + k), 0, 1)
        emb = rng.normal(size=48)
        for f in range(2 + k % 3):
            sel = rng.random(3000) < 0.7
            frags.append((f"obj{k}" if f else f"thing{k}", emb + 0.05 * rng.normal(size=48), pts[sel] + rng.normal(size=(sel.sum(), 3)) * 1e-3, cols[sel]))
    return frags


def _same(a, b):
    assert len(a.memory) == len(b.memory)
    for x, y in zip(a.memory, b.memory):
        assert x.names == y.names and x.id == y.id
        assert len(x.embeddings) == len(y.embeddings) and all(np.array_equal(p, q) for p, q in zip(x.embeddings, y.embeddings))
        assert np.array_equal(x.mean_emb, y.mean_emb)
        assert np.array_equal(x.pointcloud.points, y.pointcloud.points) and np.array_equal(x.pointcloud.colors, y.pointcloud.colors)


def test_driver_sequence_device_equals_host():
    """add_object x N -> downsample_all_objects -> _recluster_IoU(0.3) -> recluster_via_clustering_and_IoU with the default measure
    (tum_localisation_trial.py:137-148): iou_backend "device" and "host" build identical memories, and the first IoU step equals the
    oracle transcript with the object-aligned IoU"""
    from ibloc_amd.object_memory.object_memory import ObjectMemory
    from ibloc_amd.utils.IoU_ops import calculate_obj_aligned_3d_IoU
    from tests.test_gpu_build import _same_memory
    mems = {}
    for backend in ("device", "host"):
        mem = ObjectMemory(device="cuda", get_embeddings_func=lambda **kw: None, log_enabled=False, arena_bytes=1 << 30)
        assert mem.iou_backend == "host"                         # the default is unchanged
        mem.iou_backend = backend
        for name, emb, p, c in _memory(21):
            mem.add_object(name, [emb], p, c)
        mem.downsample_all_objects(0.02)
        mems[backend] = mem
    want = [bo.Obj(name, emb, p, c) for name, emb, p, c in _memory(21)]
    bo.downsample_all(want, 0.02)
    for mem in mems.values():
        mem._recluster_IoU(0.3)
    _same(mems["device"], mems["host"])
    want = bo.recluster_IoU(want, 0.3, calculate_obj_aligned_3d_IoU)
    _same_memory(mems["device"], want)
    n_first = len(want)
    for mem in mems.values():
        mem.recluster_via_clustering_and_IoU(eps=0.08, embedding_distance_threshold=0.5, IoU_threshold=0.25, min_points_per_cluster=20)
    _same(mems["device"], mems["host"])
    assert 5 <= len(mems["device"].memory) <= n_first < 29
    for mem in mems.values():
        mem._ctx.close()


def test_user_iou_func_keeps_the_host_loop_and_bad_backend_raises():
    from ibloc_amd.object_memory.object_memory import ObjectMemory
    mem = ObjectMemory(device="cuda", get_embeddings_func=lambda **kw: None, log_enabled=False, arena_bytes=256 << 20)
    for name, emb, p, c in _memory(22)[:6]:
        mem.add_object(name, [emb], p, c)
    mem.iou_backend = "device"
    calls = []

    def f(a, b):
        calls.append(1)
        return 0.0
    mem._recluster_IoU(0.3, iou_func=f)
    assert len(calls) == 15 and len(mem.memory) == 6             # 6 * 5 / 2 pairs in the host loop; nothing merges at IoU 0
    mem.iou_backend = "gpu"
    with pytest.raises(ValueError):
        mem._recluster_IoU(0.3)
    mem._ctx.close()


def test_edges(ctx):
    import ctypes
    import torch
    from ibloc_amd import _lib
    from ibloc_amd.build import obb_iou_matrix
    from ibloc_amd.registration import _stream
    D, k = obb_iou_matrix(ctx, np.zeros((0, 15)), np.zeros(0, dtype=np.int32), return_overlapping=True)
    assert D.shape == (0, 0) and k == 0
    D, k = obb_iou_matrix(ctx, _row(np.zeros(3), np.eye(3), np.ones(3))[None], np.ones(1, dtype=np.int32), return_overlapping=True)
    assert D.cpu().numpy().tolist() == [[1.0]] and k == 0
    r = _row(np.zeros(3), np.eye(3), np.ones(3))
    D, k = obb_iou_matrix(ctx, np.tile(r, (70, 1)), np.zeros(70, dtype=np.int32), return_overlapping=True)      # every object invalid
    assert torch.all(D == 1.0) and k == 0
    D, k = obb_iou_matrix(ctx, np.tile(r, (70, 1)), np.ones(70, dtype=np.int32), return_overlapping=True)       # all identical, two tiles
    assert k == 70 * 69 // 2
    Dh = D.cpu().numpy()
    assert np.all(np.diag(Dh) == 1.0) and np.abs(Dh[~np.eye(70, dtype=bool)]).max() <= 1e-12
    with pytest.raises(ValueError):
        obb_iou_matrix(ctx, np.zeros((4, 14)), np.ones(4))
    with pytest.raises(ValueError):
        obb_iou_matrix(ctx, np.zeros((4, 15)), np.ones(3))
    out = ctypes.c_int64(7)
    st = _lib.lib.ibl_obb_iou_matrix(ctx.handle, None, None, -1, None, ctypes.addressof(out), _stream())
    assert st == -1 and b"bad argument" in _lib.lib.ibl_last_error()
    st = _lib.lib.ibl_obb_iou_matrix(None, None, None, 0, None, None, _stream())
    assert st == -1
    st = _lib.lib.ibl_obb_iou_matrix(ctx.handle, None, None, 3, None, ctypes.addressof(out), _stream())
    assert st == -1 and b"null" in _lib.lib.ibl_last_error()
    st = _lib.lib.ibl_obb_iou_matrix(ctx.handle, None, None, 0, None, ctypes.addressof(out), _stream())
    assert st == 0 and out.value == 0


def test_scale_5000_fragments(ctx):
    """a memory of 5 000 fragments: 2 000 pairs (1 500 uniformly drawn, 500 of fragments of one object) equal the host loop"""
    from ibloc_amd.build import obb_iou_matrix
    from ibloc_amd.synth import fragment_scene
    from ibloc_amd.utils.IoU_ops import calculate_obj_aligned_3d_IoU, oriented_bounding_boxes
    clouds, owner = fragment_scene(5000, seed=5)
    boxes, valid = oriented_bounding_boxes(clouds)
    D, n_ov = obb_iou_matrix(ctx, boxes, valid, return_overlapping=True)
    D = D.cpu().numpy()
    assert D.shape == (5000, 5000) and np.all(np.diag(D) == 1.0) and np.array_equal(D, D.T)
    rng = np.random.default_rng(6)
    pairs = [tuple(rng.choice(5000, 2, replace=False)) for _ in range(1500)]
    same = [(i, j) for i in range(4999) for j in (i + 1,) if owner[i] == owner[j]]
    pairs += [same[k] for k in rng.choice(len(same), 500, replace=False)]
    for i, j in pairs:
        h = 1 - calculate_obj_aligned_3d_IoU(clouds[i], clouds[j])
        assert abs(D[i, j] - h) <= TOL, (i, j)
        if h == 1.0:
            assert D[i, j] == 1.0, (i, j)
    assert n_ov >= (D < 1.0).sum() // 2 > 5000
