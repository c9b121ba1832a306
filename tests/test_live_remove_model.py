"""CPU: the removal sets of tests/live_remove_cases.py contain the cases they are named for, shown with a numpy model of the spatial
hash alone -- a stable sort by the grid key, then the flagged points dropped -- so that a later edit of the world cannot quietly turn
tests/test_gpu_live_memory_remove.py into a test of easy cases.  Also the identity ibl_memgrid_remove rests on: compacting the sorted
array gives the array that sorting the kept points gives."""
import numpy as np
import pytest

from tests import live_remove_cases as lc


def all_rows():
    _, _, pts, col, _ = lc.world()
    return lc.pts4_host(pts, col)


def cell_cases(p4, cell, ranges):
    """which of the named cases the removal of `ranges` from the grid of p4 contains"""
    built = lc.model_build(p4, cell)
    _, kept_keys, gone = lc.model_remove(built, ranges)
    gone_sorted = gone[built["order"]]
    total = np.diff(built["ustart"])
    lost = np.add.reduceat(gone_sorted.astype(np.int64), built["ustart"][:-1])
    found = set()
    if ((lost > 0) & (lost < total)).any():
        found.add("partial_cell")
    if (lost == total).any():
        found.add("vanished_cell")
    if ranges[0][0] == 0:
        found.add("begins_at_0")
    if ranges[-1][1] == len(p4):
        found.add("ends_at_n")
    assert len(np.unique(kept_keys)) == built["n_cells"] - int((lost == total).sum())
    return found, built


def assert_compaction_is_the_build(p4, cell, ranges):
    built = lc.model_build(p4, cell)
    compacted, keys, gone = lc.model_remove(built, ranges)
    fresh = lc.model_build(p4[~gone], cell)
    assert compacted.tobytes() == fresh["sorted"].tobytes() and keys.tobytes() == fresh["keys"].tobytes()
    # ... and the renumbered original indices are the fresh build's sort order
    renumbered = (np.arange(len(p4)) - np.cumsum(gone) * 1)[built["order"]][~gone[built["order"]]]
    assert np.array_equal(renumbered, fresh["order"])
    return fresh


def flag_scan_scatter(built, ranges):
    """the device algorithm restated: per sorted slot a search of its original index in the ranges (rbeg, rend and the running
    count rcum), an exclusive sum of the flags, a scatter with the index renumbered by the removed points below it"""
    rbeg, rend = np.array([r[0] for r in ranges]), np.array([r[1] for r in ranges])
    rcum = np.cumsum(rend - rbeg)
    sidx = built["order"]
    lo = np.searchsorted(rbeg, sidx, side="right")                       # ranges that begin at or below the index
    keep = (lo == 0) | (sidx >= rend[np.maximum(lo, 1) - 1])
    below = np.where(lo == 0, 0, rcum[np.maximum(lo, 1) - 1])
    scan = np.cumsum(keep) - keep
    out = np.zeros((int(keep.sum()), 4), dtype=np.float32)
    new_sidx = np.zeros(int(keep.sum()), dtype=np.int64)
    out[scan[keep]] = built["sorted"][keep]
    new_sidx[scan[keep]] = (sidx - below)[keep]
    return out, new_sidx


@pytest.mark.parametrize("name", sorted(lc.REMOVAL_SETS))
def test_flag_scan_scatter_is_the_build(name):
    removed, _ = lc.REMOVAL_SETS[name]
    p4 = all_rows()
    ranges = lc.point_ranges(lc.SIZES, removed)
    out, new_sidx = flag_scan_scatter(lc.model_build(p4, lc.CELL), ranges)
    gone = np.zeros(len(p4), dtype=bool)
    for b, e in ranges:
        gone[b:e] = True
    fresh = lc.model_build(p4[~gone], lc.CELL)
    assert out.tobytes() == fresh["sorted"].tobytes() and np.array_equal(new_sidx, fresh["order"])


@pytest.mark.parametrize("name", sorted(lc.REMOVAL_SETS))
def test_removal_sets_contain_their_cases(name):
    removed, claimed = lc.REMOVAL_SETS[name]
    p4 = all_rows()
    assert len(p4) == sum(lc.SIZES)
    ranges = lc.point_ranges(lc.SIZES, removed)
    found, built = cell_cases(p4, lc.CELL, ranges)
    print(name, removed, "cases", sorted(found), "cells", built["n_cells"])
    assert set(claimed) <= found, (name, claimed, found)
    fresh = assert_compaction_is_the_build(p4, lc.CELL, ranges)
    assert 0 < fresh["n_cells"] < built["n_cells"]


def test_twin_shares_cells_with_instance_0():
    p4 = all_rows()
    keys = lc.grid_keys(p4, lc.CELL)
    first, twin = set(keys[:lc.SIZES[0]].tolist()), set(keys[-lc.SIZES[7]:].tolist())
    others = set(keys[lc.SIZES[0]:-lc.SIZES[7]].tolist())
    assert len(first & twin) >= 10 and not (first | twin) & others        # (the instances 1 .. 6 stand apart from both)


def test_fine_cells_change_the_table_dimension():
    p4 = all_rows()
    ranges = lc.point_ranges(lc.SIZES, lc.FINE_REMOVED)
    found, built = cell_cases(p4, lc.FINE_CELL, ranges)
    fresh = assert_compaction_is_the_build(p4, lc.FINE_CELL, ranges)
    print("1 cm cells:", built["n_cells"], "->", fresh["n_cells"], "table", built["table_slots"], "->", fresh["table_slots"])
    assert {"vanished_cell", "ends_at_n"} <= found
    assert built["table_slots"] >= 4 * fresh["table_slots"] and fresh["table_slots"] >= 3 * fresh["n_cells"]


def test_duplicates_share_a_cell_bit_for_bit():
    _, _, pts, col, _ = lc.world()
    p4 = lc.pts4_host(list(pts) + [pts[lc.DUP_OF]], list(col) + [col[lc.DUP_OF]])
    sizes = lc.SIZES + (lc.SIZES[lc.DUP_OF],)
    off = np.concatenate([[0], np.cumsum(sizes)])
    original, copy_ = p4[off[lc.DUP_OF]:off[lc.DUP_OF + 1]], p4[off[8]:]
    assert original.tobytes() == copy_.tobytes()
    built = lc.model_build(p4, lc.CELL)
    # a cell that holds two bit-equal rows of different instances: the original's row sits before the copy's
    where = {int(i): s for s, i in enumerate(built["order"])}
    a, b = where[int(off[lc.DUP_OF])], where[int(off[8])]
    assert a < b and built["keys"][a] == built["keys"][b] and built["sorted"][a].tobytes() == built["sorted"][b].tobytes()
    for removed in ([lc.DUP_OF], [8]):
        assert_compaction_is_the_build(p4, lc.CELL, lc.point_ranges(sizes, removed))


def test_interleaved_steps_keep_the_identity():
    """build 4, append 2, remove [1], append 2, remove [0, 5] -- the sequence of the GPU test, on the model"""
    _, _, pts, col, _ = lc.world()
    have = [0, 1, 2, 3, 4, 5]
    for removed, then in (([1], [6, 7]), ([0, 5], [1])):
        p4 = lc.pts4_host([pts[i] for i in have], [col[i] for i in have])
        assert_compaction_is_the_build(p4, lc.CELL, lc.point_ranges([lc.SIZES[i] for i in have], removed))
        have = [have[i] for i in lc.kept(len(have), removed)] + then
