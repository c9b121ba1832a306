"""CPU: the contract of ibl_memgrid_replace and of registration.splice_rows without a device.  The position formulas of the device
code (tests/live_replace_cases.model_replace) give the build of the spliced rows, original indices included; the replacement sets
contain the cases they are named for, so that a later edit of the world cannot quietly turn tests/test_gpu_live_memory_replace.py
into a test of easy cases; and splice_rows, which runs on any torch device, is checked against np.concatenate of the pieces."""
import numpy as np
import pytest
import torch

from tests import live_replace_cases as rc


def set_rows(name):
    _, _, _, pts, col = rc.world()
    instances, clouds, colors = rc.replacements(name)
    ranges, counts = rc.replace_args(rc.SIZES, instances, clouds)
    new_p4 = rc.pts4_host(rc.ordered(instances, clouds), rc.ordered(instances, colors))
    return rc.pts4_host(pts, col), ranges, counts, new_p4


@pytest.mark.parametrize("cell", [rc.CELL, rc.FINE_CELL], ids=["4cm", "1cm"])
@pytest.mark.parametrize("name", sorted(rc.REPLACE_SETS))
def test_model_replace_is_the_build_of_the_spliced_rows(name, cell):
    p4, ranges, counts, new_p4 = set_rows(name)
    got = rc.model_replace(rc.model_build(p4, cell), ranges, counts, new_p4, cell)
    fresh = rc.model_build(rc.splice_p4(p4, ranges, new_p4, counts), cell)
    assert got["sorted"].tobytes() == fresh["sorted"].tobytes() and got["keys"].tobytes() == fresh["keys"].tobytes()
    assert np.array_equal(got["sidx"], fresh["order"])


def test_model_insertions_and_removals():
    """empty ranges (at 0, in the middle, at n) and counts of 0, mixed: the forms that make the call an append or a removal"""
    p4, _, _, new_p4 = set_rows("all")
    n = len(p4)
    for ranges, counts in (([(n, n)], [500]), ([(0, 0)], [300]), ([(0, 300), (820, 1620)], [0, 0]),
                           ([(0, 0), (300, 300), (300 + 520, 300 + 520 + 800), (n - 560, n - 560), (n, n)], [40, 300, 0, 7, 100])):
        rows = new_p4[:sum(counts)]
        got = rc.model_replace(rc.model_build(p4, rc.CELL), ranges, counts, rows)
        fresh = rc.model_build(rc.splice_p4(p4, ranges, rows, counts), rc.CELL)
        assert got["sorted"].tobytes() == fresh["sorted"].tobytes() and np.array_equal(got["sidx"], fresh["order"])


def cases_of(name):
    p4, ranges, counts, new_p4 = set_rows(name)
    old_built = rc.model_build(p4, rc.CELL)
    after = rc.splice_p4(p4, ranges, new_p4, counts)
    built = rc.model_build(after, rc.CELL)
    found = set()
    if ranges[0][0] == 0:
        found.add("begins_at_0")
    if ranges[-1][1] == len(p4):
        found.add("ends_at_n")
    if any(a[1] == b[0] for a, b in zip(ranges, ranges[1:])):
        found.add("adjacent_ranges")
    if len(ranges) == len(rc.SIZES):
        found.add("every_instance")
    for (b, e), c in zip(ranges, counts):
        found.add("grows" if c > e - b else "shrinks" if c < e - b else "same_size")
    old_cells, new_cells = set(old_built["ukeys"].tolist()), set(built["ukeys"].tolist())
    if old_cells - new_cells:
        found.add("cells_vanish")
    if new_cells - old_cells:
        found.add("cells_appear")
    # a cell that holds, in order, a resident point of a lower instance, a new point, and a resident point of a higher instance
    is_new = np.zeros(len(after), dtype=bool)
    shift = 0
    for (b, e), c in zip(ranges, counts):
        is_new[b + shift:b + shift + c] = True
        shift += c - (e - b)
    flags = is_new[built["order"]]
    for s, e in zip(built["ustart"][:-1], built["ustart"][1:]):
        f = flags[s:e]
        if f.any() and not f[0] and not f[-1]:
            found.add("interleaves")
            break
    return found


@pytest.mark.parametrize("name", sorted(rc.REPLACE_SETS))
def test_replacement_sets_contain_their_cases(name):
    found = cases_of(name)
    print(name, sorted(found))
    assert set(rc.REPLACE_SETS[name][1]) <= found, (name, found)


def test_middle_shared_lands_between_instances_0_and_7():
    p4, ranges, counts, new_p4 = set_rows("middle_shared")
    built = rc.model_build(rc.splice_p4(p4, ranges, new_p4, counts), rc.CELL)
    off = np.concatenate([[0], np.cumsum(rc.SIZES)])
    inst = np.searchsorted(off, built["order"], side="right") - 1          # (same size: the offsets are those of the world)
    cells = 0
    for s, e in zip(built["ustart"][:-1], built["ustart"][1:]):
        i = inst[s:e]
        assert (np.diff(i) >= 0).all()
        cells += int(i[0] == 0 and i[-1] == 7 and (i == 3).any())
    assert cells >= 5, cells


# ---- registration.splice_rows on CPU tensors ---------------------------------------------------------------------------------------------
EDITS = [  # (rows used, [(begin, end, new rows)]) in a buffer of 64 rows
    (50, [(10, 20, 10)]),                                   # same size: nothing moves
    (50, [(10, 20, 3)]),                                    # the tail moves down
    (50, [(10, 20, 17)]),                                   # the tail moves up, overlapping itself
    (50, [(0, 5, 9), (5, 12, 1), (30, 30, 4), (45, 50, 0)]),  # begins at 0, touching, an insertion, a removal at the end: up, then down
    (50, [(3, 20, 2), (25, 26, 12), (40, 41, 0)]),          # down, up, and a run that ends where it began
    (50, [(50, 50, 14)]),                                   # an append
    (40, [(0, 40, 64)]),                                    # everything, to the last row of the buffer
    (60, [(0, 0, 1), (1, 2, 0), (20, 22, 5)]),
    # removals alone (the scratch chunks of the test are 1 and 4 rows, and the default, which holds everything):
    (64, [(5, 7, 0), (30, 31, 0)]),                         # a kept prefix that does not move; shifts of 2 and 3 rows, below a chunk of 4
    (60, [(0, 1, 0), (4, 10, 0), (40, 45, 0), (47, 50, 0)]),  # runs of 3 and 2 rows shorter than their shifts of 7 and 12: one copy each
    (64, [(0, 40, 0)]),                                     # 24 rows move down by 40; (0, 3): 61 rows by 3, through the chunk or in pieces
    (64, [(0, 3, 0)]),
    (50, [(0, 2, 0), (9, 11, 0), (20, 33, 0)]),             # shifts of 2, 4 and 17 rows: below, at and above a chunk of 4
    # appends alone
    (64, [(64, 64, 0)]),                                    # nothing, behind a buffer without headroom: it stays
    (63, [(63, 63, 1)]),                                    # the last row of the buffer
]


@pytest.mark.parametrize("shape", [(64, 3), (64,), (64, 2, 5)], ids=["rows", "scalars", "blocks"])
def test_splice_rows_in_place(shape):
    from ibloc_amd.registration import compact_scratch, splice_rows
    host = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) + 0.5
    row_bytes = host[0].nbytes
    rng = np.random.default_rng(5)
    for n_used, spec in EDITS:
        new = [rng.normal(size=(k,) + shape[1:]).astype(np.float32) for _, _, k in spec]
        parts, at = [], 0
        for (b, e, _), rows in zip(spec, new):
            parts += [host[at:b], rows]
            at = e
        want = np.concatenate(parts + [host[at:n_used]])
        assert len(want) <= 64
        for scratch_bytes in (None, row_bytes, 4 * row_bytes, 1):     # the default chunk, one row, a few rows, less than a row
            buf = torch.from_numpy(host.copy())
            scratch = None if scratch_bytes is None else compact_scratch(buf.device, scratch_bytes)
            out_buf, out = splice_rows(buf, n_used, [(b, e, torch.from_numpy(r)) for (b, e, _), r in zip(spec, new)], scratch=scratch)
            assert out_buf is buf and out.data_ptr() == buf.data_ptr() and out.shape == want.shape
            assert out.numpy().tobytes() == want.tobytes(), (n_used, spec, scratch_bytes)
            behind = max(len(want), n_used)
            assert buf[behind:].numpy().tobytes() == host[behind:].tobytes()       # nothing behind the used rows is touched


@pytest.mark.parametrize("shape", [(64, 3), (64,), (64, 2, 5)], ids=["rows", "scalars", "blocks"])
def test_splice_rows_grows_by_half(shape):
    from ibloc_amd.registration import splice_rows
    host = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) + 0.5
    # (the second and third: appends to a buffer without headroom, by less and by more than half of it)
    for n_used, b, e, k, rows_after in ((60, 10, 12, 10, 96), (64, 64, 64, 1, 96), (64, 64, 64, 40, 104), (64, 0, 4, 100, 160)):
        new = np.full((k,) + shape[1:], -1.0, dtype=np.float32)
        buf = torch.from_numpy(host.copy())
        out_buf, out = splice_rows(buf, n_used, [(b, e, torch.from_numpy(new))])
        assert out_buf.shape[0] == rows_after == max(n_used - (e - b) + k, 96) and out_buf.data_ptr() != buf.data_ptr()
        assert out.data_ptr() == out_buf.data_ptr()
        assert out.numpy().tobytes() == np.concatenate([host[:b], new, host[e:n_used]]).tobytes()
        assert buf.numpy().tobytes() == host.tobytes()                                 # the old buffer is read only
