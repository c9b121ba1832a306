"""-m gpu: the whole-memory spatial hash on its own.  Build and append share one merge, so "an appended grid equals a fresh build"
(test_gpu_live_memory.py) no longer checks the build independently: here a fresh build is compared with a float64 brute force, and
the grid's ownership of its device memory is checked (nothing of it in the context arena, `close` gives everything back)."""
import numpy as np
import pytest

from tests.test_gpu_live_memory import CELL, SIZES, THR, point_distances, pts4_of, queries, world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(1 << 30)
    yield c
    c.close()


# 4 cm cells at the evaluation's 2 cm; 1 cm cells at 1 cm (a query's box then spans up to 27 cells, and 159 of the near queries have
# no point within reach).  At both thresholds every query of `queries()` is clear of the threshold by more than 0.1 % -- at 5 mm,
# half of the 1 cm cell, five would not be, and the test compares the pattern of every query.
@pytest.mark.parametrize("cell,thr", [(CELL, THR), (0.01, 0.01)], ids=["4cm", "1cm"])
def test_fresh_build_against_fp64(ctx, cell, thr):
    from ibloc_amd.registration import MemGrid
    _, _, pts, col, _ = world()
    q, _ = queries(pts, sum(SIZES[:7]))
    allp = np.concatenate(pts).astype(np.float32).astype(np.float64)
    q64 = q.astype(np.float64)
    ref = np.concatenate([((q64[i:i + 500, None, :] - allp[None, :, :]) ** 2).sum(-1).min(1) for i in range(0, len(q), 500)])
    # the finite / inf pattern is compared for EVERY query: none may lie so close to the threshold that fp32 rounding decides
    ratio = np.sqrt(ref) / thr
    assert not ((ratio >= 0.999) & (ratio <= 1.001)).any(), np.sort(np.abs(ratio - 1))[:3]
    grid = MemGrid(ctx, pts4_of(pts, col), cell)
    info = grid.info()
    assert info["n"] == info["ustart_end"] == info["point_capacity"] == sum(SIZES)
    d2 = point_distances(ctx, grid, q, thr)[0].astype(np.float64)
    grid.close()
    within = ratio < 1
    assert 500 < within.sum() <= len(q) - 400
    assert np.array_equal(np.isfinite(d2), within)
    # three fp32 subtractions (2^-24 relative each, doubled by the square) and the three roundings of dist2f
    rel = np.abs(d2[within] - ref[within]) / ref[within]
    print(f"cell {cell}: {info['n_cells']} cells, {int(within.sum())} within {thr}, worst relative error {rel.max() * 2 ** 24:.2f} x 2^-24")
    assert rel.max() <= 8 * 2.0 ** -24


def test_grids_do_not_live_in_the_arena(ctx):
    from ibloc_amd.engine import intensity_from_colors
    from ibloc_amd.registration import CloudBatch, MemGrid, radius_outlier_batch
    _, _, pts, col, _ = world()
    q, _ = queries(pts, sum(SIZES[:7]))
    fixed = MemGrid(ctx, pts4_of(pts, col), CELL)
    live = MemGrid(ctx, pts4_of(pts, col), CELL, live=True, reserve_points=1000)
    before = [point_distances(ctx, g, q)[0].tobytes() for g in (fixed, live)]
    assert before[0] == before[1]
    ctx.reset()
    batch = CloudBatch.from_numpy(pts, [intensity_from_colors(c) for c in col])
    assert int(radius_outlier_batch(ctx, batch, 0.05, 8).sum().item()) > 0          # arena-consuming calls over whatever the arena held
    MemGrid(ctx, pts4_of(pts[:5], col[:5]), 0.01).close()
    assert [point_distances(ctx, g, q)[0].tobytes() for g in (fixed, live)] == before
    assert fixed.info()["n"] == live.info()["n"] == sum(SIZES)
    fixed.close()
    live.close()


def test_close_gives_the_memory_back():
    from ibloc_amd.registration import MemGrid, RegContext
    _, _, pts, col, _ = world()
    p4 = pts4_of(pts, col)
    # One build of the 4 360 points has a measured arena high-water of 229 120 bytes (all of it scratch).  The smallest arena the
    # library creates is 1 MiB, so that is the smallest power of two in which the build succeeds.
    small = RegContext(1 << 20)
    MemGrid(small, p4, CELL).close()
    first = small.high_water()
    assert 0 < first < 1 << 20
    for _ in range(199):
        MemGrid(small, p4, CELL).close()
    assert small.high_water() == first
    small.close()


def test_evaluate_transform_is_stable_across_calls():
    from ibloc_amd.utils import fpfh_register as fr
    _, _, pts, col, _ = world()
    shift = np.array([0.004, -0.003, 0.002])
    cases = [(pts[0] + shift, pts[0]), (pts[3] - shift, pts[3])]                   # two different target clouds
    T = np.eye(4)
    first = [fr.evaluate_transform(s, t, T, THR) for s, t in cases]
    assert all(fit > 0.5 and rmse > 0 for rmse, fit in first) and first[0] != first[1]
    for _ in range(3):
        Tr, _, fit = fr.register_point_clouds((pts[0] + shift, col[0]), (pts[0], col[0]), 0.05, 1.5, 1.5)      # (same context)
        assert Tr.shape == (4, 4) and fit > 0
        assert [fr.evaluate_transform(s, t, T, THR) for s, t in cases] == first
