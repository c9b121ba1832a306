"""-m gpu: `ibl_dbscan_batch` and `ibl_voxel_downsample_batch` (csrc/build_memory.hip) and the batch grid builder under them
(csrc/reg_grid.hip) against `oracle.build_oracle`, one call per case of tests/build_cases.py (tests/test_build_model.py shows on the
CPU that every case contains what it is named for).  Every comparison is `np.array_equal`: labels and cluster counts group by group;
points, colours, counts and offsets object by object.

case                         what it holds the kernels to
lattice_at_eps / _above_*    pairs at exactly eps do not count (fp64, ((dx^2 + dy^2) + dz^2), strict <); one ulp more and they do; a point
                             with exactly min_points neighbours is core, with one fewer it is not; lattice points on cell planes
border_between_two_*         a border point takes the LOWEST-numbered cluster among its core neighbours; clusters are numbered by their
                             smallest original index although the kernels walk in cell order; the core neighbour may sit in another cell row
snake_open / _closed         widened cells (extent > 128 cells); a chain where every point has exactly min_points neighbours, cut at a
                             step of exactly eps across a cell plane, and joined when that step is one ulp shorter
many_groups                  320 groups: the second round of the dims kernel and its carried cell prefix; empty groups anywhere, 1 / 255 /
                             256 / 257 points, duplicates, groups lying inside each other stay unlinked
far_from_origin              fp32 binning of coordinates at 4 096 m under fp64 distances
budget_exceeded              the 64 Mi-cell budget: later groups collapse to one cell, labels stay exact, status bit 1 reports it (the
                             collapse rule had never run: its "first group that does not fit" slot could not leave -1, the call failed)
budget_filled_exactly        32 groups fill the budget to the last cell; the 33rd still gets its one cell (the host check refused
                             the one cell past the budget)
on_the_planes_*              floor(p / voxel) for p on a voxel plane, exact and rounded quotients, -0.0
crowded                      5 000 points in one voxel: one running fp64 sum in input order
interleaved                  voxels come out in order of first occurrence, here the reverse of the key order
many_objects                 720 objects: more than one block of the offsets kernel, empty objects anywhere
span_limit (+ 3 refusals)    65 536 voxels along every axis is the last span a key holds; 65 537 along any axis is refused by name
beyond_int32                 voxel indices near +-3e9
"""
import numpy as np
import pytest

from tests import build_cases as bc

pytestmark = pytest.mark.gpu

GRID_OVERFLOW = 1                        # IBL_ST_GRID_OVERFLOW


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(4 << 30)              # the two budget cases take about 0.6 GB for the cell tables
    yield c
    c.close()


@pytest.mark.parametrize("name", list(bc.DBSCAN_CASES))
def test_dbscan_labels_equal_the_oracle(ctx, name):
    from ibloc_amd.build import dbscan_batch
    case = bc.DBSCAN_CASES[name]()
    want = bc.dbscan_expected(name)
    ctx.status()                                                        # clear the sticky bits of earlier tests
    labels, ncl = dbscan_batch(ctx, case["groups"], case["eps"], case["min_points"])
    status = ctx.status()
    assert len(labels) == len(want) and len(ncl) == len(want)
    wrong = [g for g in range(len(want)) if not np.array_equal(labels[g], want[g])]
    assert not wrong, (name, wrong[:10], [int((labels[g] != want[g]).sum()) for g in wrong[:10]])
    assert np.array_equal(ncl, [w.max() + 1 if len(w) and w.max() >= 0 else 0 for w in want]), name
    assert bool(status & GRID_OVERFLOW) == case["overflow"], (name, status)


@pytest.mark.parametrize("with_colors", [True, False], ids=["colours_counts", "points_only"])
@pytest.mark.parametrize("name", list(bc.VOXEL_CASES))
def test_voxel_downsample_equals_the_oracle(ctx, name, with_colors):
    from ibloc_amd.build import voxel_downsample_batch
    case = bc.VOXEL_CASES[name]()
    want = bc.voxel_expected(name, with_colors)
    if with_colors:
        gp, gc, gn = voxel_downsample_batch(ctx, case["points"], case["colors"], case["voxel"], return_counts=True)
    else:
        gp, gc = voxel_downsample_batch(ctx, case["points"], None, case["voxel"])
        assert gc is None
    assert len(gp) == len(want)
    assert np.array_equal(np.cumsum([len(p) for p in gp]), np.cumsum([len(w[0]) for w in want])), name      # the output offsets
    for i, (wp, wc, wn) in enumerate(want):
        assert np.array_equal(gp[i], wp), (name, i)
        if with_colors:
            assert np.array_equal(gc[i], wc), (name, i)
            assert np.array_equal(gn[i], wn), (name, i)


@pytest.mark.parametrize("name", list(bc.VOXEL_REFUSED))
def test_voxel_span_past_the_key_is_refused_by_name(ctx, name):
    from ibloc_amd.build import voxel_downsample_batch
    case = bc.VOXEL_REFUSED[name]()
    obj, axis = case["refused"]
    with pytest.raises(RuntimeError, match=rf"object {obj} spans more than 65536 voxels along axis {axis}\b"):
        voxel_downsample_batch(ctx, case["points"], case["colors"], case["voxel"], return_counts=True)
