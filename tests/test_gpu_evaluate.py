"""-m gpu: the whole-memory evaluation alone (`ibl_evaluate_kernel`, csrc/reg_eval.hip) through `evaluate_points` and `evaluate_batch`,
EVERY POINT of every family of tests/evaluate_cases.py (tests/test_evaluate_model.py shows with the references alone what each
family is there for), under the default switches (pruned scan) and under ctx.diag(eval_fullscan=1):

    d2        equal BIT FOR BIT to the brute force of the fp32 rule (oracle_nearest_bruteforce: no grid, every memory point), +inf
              included, no point exempt -- a hit outside the query's box, a cell skipped by the pruning bound, a slot of the
              four-at-a-time loop or a job offset that is off shows here
    fp64      every point outside the 2^-20 band around the threshold: finite iff d_fp64 < thr, and |d2 - d2_fp64| <= 2^-21 d2_fp64
              (one rounding of each difference, doubled by the square, and three roundings in dist2f: 5 x 2^-24)
    fitness   == count / ns exactly (count of the brute force), 0.0 for an empty job
    rmse      within ns x 2^-52 relative of sqrt(fsum(d2 of the inliers) / count): the device adds doubles in a fixed order
    paths     evaluate_batch (no d2_out) gives the bits of evaluate_points, so does a second call, and a grid built live = True with
              a reserve gives the same d2 bits as the immutable one
and 65 536 + 3 jobs in one call (more than one launch can number) job by job.

Measured on an MI355X (both scans give the same figures: their d2 are bit-equal to the brute force and so to each other):
    family                  points    jobs  inliers  d2 != brute force  in the band  worst |d2 - d2_fp64| / d2_fp64 outside the band
    slab_origin              41000       3    33039                  0            0  2.835 x 2^-24
    slab_mid                 41000       3    32914                  0            0  1.000 x 2^-24
    slab_far                 41000       3    32641                  0            0  1.000 x 2^-24
    occupancy_cells           2477       2     2097                  0            0  2.400 x 2^-24
    occupancy_single           145       2        8                  0            0  0.771 x 2^-24
    occupancy_many           33334       2    14024                  0            0  2.987 x 2^-24
    jobs                     23962      15    18535                  0            0  2.773 x 2^-24
    jobs_single               5000       1     4997                  0            0  2.468 x 2^-24
    ratio_0.02_0.02          41000       3    33047                  0            0  2.835 x 2^-24
    ratio_0.05_0.02          41000       3    33040                  0            0  2.835 x 2^-24
    ratio_0.01_0.02          41000       3    33047                  0            0  2.835 x 2^-24
    ratio_0.04_0.04          41000       3    33083                  0            0  2.835 x 2^-24
    threshold_0.04_0.02      12854       1     5766                  0         4101  1.969 x 2^-24
    threshold_0.01_0.02      12854       1     5697                  0         5009  2.823 x 2^-24
    threshold_0.04_0.04      12782       1     5529                  0         4487  1.889 x 2^-24
    threshold_0.05_0.075     12854       1     5672                  0         4868  2.382 x 2^-24
    threshold_0.04_0.021     12854       1     5966                  0         4304  1.773 x 2^-24
    threshold_0.01_0.021     12854       1     5966                  0         5200  2.657 x 2^-24
    threshold_0.04_0.036     12854       1     6533                  0         4634  2.217 x 2^-24
    threshold_0.01_0.019     12854       1     6719                  0         5011  2.723 x 2^-24
    many_jobs               383882   65539   224712                  0            0  1.015 x 2^-24
every rmse equal to sqrt(fsum(d2) / count) to the last bit (gap 0 x 2^-52 in all 42 runs), every fitness equal to count / ns.
With the box unpadded, as the kernel was before this test existed, 13 + 13 + 27 + 21 points of threshold_0.04_0.021, _0.01_0.021,
_0.04_0.036 and _0.01_0.019 came back +inf under both scans where the brute force has a hit (the anchor within 4e-10 below 0, the
query at +(float)thr: tests/test_evaluate_model.py has the arithmetic); every other family passed as it does now.
"""
import numpy as np
import pytest
import torch

from tests import evaluate_cases as ec

pytestmark = pytest.mark.gpu

NAMES = [n for n, _, _ in ec.ALL]


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(1 << 30)
    yield c
    c.close()


def pts4(p):
    return torch.from_numpy(np.concatenate([p, np.zeros((len(p), 1), np.float32)], 1)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(ctx, fam, grid, det4, full):
    from ibloc_amd.registration import evaluate_points
    with ctx.diag(eval_fullscan=1 if full else 0):
        d2, rmse, fit = evaluate_points(ctx, grid, det4, fam["jb"], fam["je"], fam["T"], fam["thr"])
    torch.cuda.synchronize()
    return d2.cpu().numpy(), rmse, fit


def check(fam, ref, d2, rmse, fit, scan):
    """every point and every job against the references; prints the family's figures, then asserts"""
    n = len(ref["d2"])
    assert d2.shape == (n,)
    wrong = np.nonzero(bits(d2) != bits(ref["d2"]))[0]
    out = ~ec.in_band(fam, ref)
    thr2 = fam["thr"] * fam["thr"]
    inl64 = ref["d2_64"] < thr2
    fin = np.isfinite(d2)
    both = out & fin & inl64
    rel = np.abs(d2[both].astype(np.float64) - ref["d2_64"][both]) / np.where(ref["d2_64"][both] > 0, ref["d2_64"][both], 1.0)
    print(f"{fam['name']} [{scan}]: {n} points in {len(ref['ns'])} jobs, {int(fin.sum())} inliers ({int(np.isfinite(ref['d2']).sum())} by brute force), "
          f"{len(wrong)} d2 differ from the brute force, {int((~out).sum())} in the band, worst relative error to fp64 "
          f"{(rel.max() if len(rel) else 0.0) * 2 ** 24:.3f} x 2^-24")
    assert len(wrong) == 0, (wrong[:5], d2[wrong[:5]], ref["d2"][wrong[:5]], ref["q"][wrong[:5]])
    assert np.array_equal(fin[out], inl64[out])
    assert np.all(rel <= 2.0 ** -21)
    assert np.all(d2[both][ref["d2_64"][both] == 0] == 0)
    worst_rmse = 0.0
    for j, (cnt, f, r) in enumerate(ec.expected_scores(fam, ref)):
        ns = int(ref["ns"][j])
        assert fit[j] == f and (ns > 0 or fit[j] == 0.0), (j, fam["tags"][j], fit[j], f)
        if cnt == 0:
            assert rmse[j] == 0.0, (j, fam["tags"][j])
        else:
            worst_rmse = max(worst_rmse, abs(rmse[j] - r) / r if r > 0 else abs(rmse[j]))
            assert abs(rmse[j] - r) <= ns * 2.0 ** -52 * r, (j, fam["tags"][j], rmse[j], r)
    print(f"{fam['name']} [{scan}]: worst relative rmse gap {worst_rmse * 2 ** 52:.2f} x 2^-52")


@pytest.mark.parametrize("scan", ["pruned", "full"])
@pytest.mark.parametrize("name", NAMES)
def test_every_point_against_the_brute_force(ctx, name, scan):
    from ibloc_amd.registration import MemGrid, evaluate_batch
    fam = ec.get(name)
    ref = ec.reference(fam)
    mem4, det4 = pts4(fam["mem"]), pts4(fam["det"])
    grid = MemGrid(ctx, mem4, fam["cell"])
    full = scan == "full"
    d2, rmse, fit = run(ctx, fam, grid, det4, full)
    check(fam, ref, d2, rmse, fit, scan)
    # the other call path, a second call, a live grid with a reserve: the same bits
    with ctx.diag(eval_fullscan=1 if full else 0):
        rmse_b, fit_b = evaluate_batch(ctx, grid, det4, fam["jb"], fam["je"], fam["T"], fam["thr"])
    assert rmse_b.tobytes() == rmse.tobytes() and fit_b.tobytes() == fit.tobytes()
    d2_2, rmse_2, fit_2 = run(ctx, fam, grid, det4, full)
    assert d2_2.tobytes() == d2.tobytes() and rmse_2.tobytes() == rmse.tobytes() and fit_2.tobytes() == fit.tobytes()
    grid.close()
    live = MemGrid(ctx, mem4, fam["cell"], live=True, reserve_points=1000)
    d2_l, rmse_l, fit_l = run(ctx, fam, live, det4, full)
    live.close()
    assert d2_l.tobytes() == d2.tobytes() and rmse_l.tobytes() == rmse.tobytes() and fit_l.tobytes() == fit.tobytes()


@pytest.mark.parametrize("scan", ["pruned", "full"])
def test_more_jobs_than_one_launch_holds(ctx, scan):
    """65 536 + 3 jobs: gridDim.y ends at 65 535, so the call launches twice; the jobs of the second launch read their own ranges and
    transforms, write their distances behind those of the first and their scores into their own slots"""
    from ibloc_amd.registration import MemGrid
    fam = ec.many_jobs()
    assert len(fam["jb"]) == ec.GRID_Y_MAX + 4 and len(fam["mem"]) == 9
    ref = ec.reference(fam)
    grid = MemGrid(ctx, pts4(fam["mem"]), fam["cell"])
    d2, rmse, fit = run(ctx, fam, grid, pts4(fam["det"]), scan == "full")
    grid.close()
    check(fam, ref, d2, rmse, fit, scan)
    scores = ec.expected_scores(fam, ref)
    assert all(scores[j][0] > 0 for j in (ec.GRID_Y_MAX - 1, ec.GRID_Y_MAX, ec.GRID_Y_MAX + 1, ec.GRID_Y_MAX + 3))
    assert len({scores[j] for j in range(ec.GRID_Y_MAX - 1, ec.GRID_Y_MAX + 3)}) == 4          # neighbours across the boundary differ
