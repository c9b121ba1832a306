"""CPU: utils.IoU_ops.oriented_bounding_boxes, the host half of the device IoU matrix of _recluster_IoU -- one oriented box per cloud on
a thread pool, bit for bit the per-object oriented_bounding_box, and valid = 0 where that raises."""
import numpy as np
import pytest

from ibloc_amd.synth import fragment_scene
from ibloc_amd.utils import IoU_ops as iou


def _clouds():
    clouds, _ = fragment_scene(40, seed=3)
    rng = np.random.default_rng(4)
    clouds.insert(5, clouds[2][:3])                                                   # three points: no hull
    clouds.insert(9, np.c_[rng.uniform(-1, 1, size=(50, 2)), np.zeros(50)])           # coplanar
    clouds.append(np.zeros((0, 3)))                                                   # empty
    return clouds


@pytest.mark.parametrize("threads", [1, 8])
def test_boxes_equal_the_per_object_box(threads):
    clouds = _clouds()
    boxes, valid = iou.oriented_bounding_boxes(clouds, threads=threads)
    assert boxes.shape == (len(clouds), 15) and boxes.dtype == np.float64
    assert valid.shape == (len(clouds),) and valid.dtype == np.int32
    for i, p in enumerate(clouds):
        try:
            c, R, h = iou.oriented_bounding_box(p)
        except Exception:
            assert valid[i] == 0 and not boxes[i].any(), i
            continue
        assert valid[i] == 1
        assert np.array_equal(boxes[i], np.concatenate([c, R.reshape(9), h])), i     # bit for bit
    assert list(np.flatnonzero(valid == 0)) == [5, 9, len(clouds) - 1]


def test_thread_counts_agree_and_the_pool_is_capped():
    clouds = _clouds()
    b1, v1 = iou.oriented_bounding_boxes(clouds, threads=1)
    b64, v64 = iou.oriented_bounding_boxes(clouds, threads=64)                        # capped at MAX_BOX_THREADS
    bd, vd = iou.oriented_bounding_boxes(iter(clouds))                                # default pool, any iterable
    assert iou.MAX_BOX_THREADS == 16
    assert np.array_equal(b1, b64) and np.array_equal(v1, v64) and np.array_equal(b1, bd) and np.array_equal(v1, vd)


def test_empty_list():
    boxes, valid = iou.oriented_bounding_boxes([])
    assert boxes.shape == (0, 15) and valid.shape == (0,)


def test_box_layout_is_centre_rotation_half():
    """row = centre, R row-major (columns are the box axes), half extents: the layout include/ibloc.h documents"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(1)
    half = np.array([0.5, 0.3, 0.1])
    R = Rotation.from_euler("xyz", [0.3, -0.7, 1.1]).as_matrix()
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
    p = np.vstack([rng.uniform(-1, 1, size=(2000, 3)) * half, corners]) @ R.T + [1.0, -2.0, 0.5]
    (row,), (ok,) = iou.oriented_bounding_boxes([p])
    assert ok == 1
    assert np.allclose(row[:3], [1.0, -2.0, 0.5], atol=1e-9)
    Rb = row[3:12].reshape(3, 3)
    assert np.allclose(np.abs(Rb.T @ R), np.eye(3), atol=1e-9) and np.isclose(np.linalg.det(Rb), 1.0)
    assert np.allclose(row[12:], half, atol=1e-9)
