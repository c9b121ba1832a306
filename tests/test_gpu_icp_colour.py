"""-m gpu: the COLOURED ICP estimator alone (csrc/reg_icp.hip with colored = 1 behind the job assembly of csrc/reg_register.hip) against
`oracle.reg_oracle.icp(..., colored=True)`, job by job, on the job sets of tests/icp_colour_cases.py.  tests/test_icp_colour_model.py
shows with the oracle alone that every set reaches the path it is there for, that no job sits on a rounding boundary and that the slip
a set exists to catch would move T by 100 tolerances or more.

The stage is fed through injected instance features: crafted FPFH rows decide the start (the identity, or a RANSAC transform within
millimetres), crafted target normals and gradients are written over the computed ones, and `reuse[1] == 0` in every call shows that
nothing was recomputed in context -- every row the stage read is a row the family wrote.  The oracle starts from the product's own
`T_ransac` with the same rows; where the family claims the identity start, `T_ransac` must BE the identity, with the oracle's statistics.
Every job is held to the tolerances of tests/test_gpu_icp.py: |T - T_oracle| <= 1e-6 per entry, fitness to 1e-9, rmse to 1e-7; there
is no share of jobs that may miss.  Two runs of a family must be byte-equal.

Largest gap to the oracle per family, measured on an MI355X (the oracle's own sensitivity to a start moved by 1e-13 is 1e-13 .. 1e-12):

family          path it exists for                                                                               T, fitness, rmse
strides         sources of 3 .. 5000 points: the 29-accumulator moments loop goes round once (<= 2048 rows),
                twice (2049) and three times (5000)                                                              1.1e-14, 0, 0
many_active     47 jobs: the coloured step walks the active-job list with a stride (38 listed > 32 block rows
                at iteration 8), reuses its shared sums from job to job, and walks it without (fewer later);
                empty source, empty target, nothing within reach; five jobs alone = in the batch                 3.3e-16, 0, 0
pieces          2 and 3 target instances, an empty middle slot, a source on pieces 2 and 3 only: the row
                offset of a piece into normals[] / grad[], a constant field of its own per piece                  2.3e-12, 0, 0
photometric     planes with a quadratic intensity, sources shifted IN the plane: only the photometric rows
                (ditM, is0, the sign of r) bring the shift back                                                   8.2e-16, 0, 0
singular        exactly zero pivots: solve6_d refuses, T stays T_ransac, the job stops one iteration later;
                the neighbours in the batch are the ones of the call without the singular jobs                    8.2e-16, 0, 0
ties            equal fp32 distances between targets with different normals, gradients and intensities, at
                iteration 0 (thread per point) and at iterations 8 / 10 (grouped search)                          4.2e-17, 0, 0
ties_reordered  the same points in another row order: the other row wins                                          1.1e-16, 0, 0
few             3, 4, 5 sources (6 to 10 Jacobian rows); 1 and 2 sources on the exactly singular targets           1.1e-15, 0, 0
"""
import numpy as np
import pytest

from tests import icp_colour_cases as cc
from tests.test_gpu_icp import check_means, compare

pytestmark = pytest.mark.gpu

I4 = np.eye(4)


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(4 << 30)
    yield c
    c.close()


def check_start(fam, out, jobs=None):
    """where the family claims the identity start, the product's RANSAC returned exactly the identity with the oracle's statistics"""
    for i, j in enumerate(range(len(fam["js"])) if jobs is None else jobs):
        T0, stats = cc.oracle_start(fam, j)
        assert np.array_equal(out["ransac_stats"][i], stats), (fam["tags"][j], out["ransac_stats"][i], stats)
        if fam["start"][j] == "identity":
            assert np.array_equal(out["T_ransac"][i], I4), fam["tags"][j]
        else:
            assert np.abs(out["T_ransac"][i] - T0).max() < 1e-6


def against_the_oracle(ctx, name):
    """the family twice (byte-equal), then every job against the oracle run from the product's own RANSAC transform"""
    fam = cc.FAMILIES[name]()
    p = cc.pools(ctx, fam)
    nrm, grad = p[3].normals[:p[1].n, :3].cpu().numpy(), p[3].grad[:p[1].n, :3].cpu().numpy()
    assert np.array_equal(nrm, np.concatenate(fam["mem_nrm"])) and np.array_equal(grad, np.concatenate(fam["mem_grad"]))
    out = cc.run(ctx, fam, p)
    again = cc.run(ctx, fam, p)
    for k in ("T", "fitness", "rmse", "T_ransac", "ransac_stats", "means"):
        assert np.array_equal(out[k], again[k]), k
    check_start(fam, out)
    check_means(fam, out)
    oracle = [cc.oracle_run(fam, j, out["T_ransac"][j]) for j in range(len(fam["js"]))]
    compare(name, fam, out, oracle)
    return fam, p, out, oracle


@pytest.mark.parametrize("name", ["strides", "pieces", "photometric", "ties", "ties_reordered", "few"])
def test_coloured_family(ctx, name):
    fam, p, out, oracle = against_the_oracle(ctx, name)
    if name == "few":          # the sources on the exactly singular targets stay where RANSAC left them
        for j in range(3, len(oracle)):
            assert np.array_equal(out["T"][j], out["T_ransac"][j]) and out["fitness"][j] == 1.0


def test_many_active_every_job_and_no_job_depends_on_its_neighbours(ctx):
    fam, p, out, oracle = against_the_oracle(ctx, "many_active")
    its = np.array([o[3] for o in oracle])
    assert (its >= cc.GROUP_FROM).sum() > cc.ACT_Y > (its >= 20).sum()
    for j, tag in cc.MANY_SPECIAL.items():
        assert np.array_equal(out["T"][j], out["T_ransac"][j]) and out["fitness"][j] == 0.0 and out["rmse"][j] == 0.0, tag
    # one job per call: byte-equal to the batch's.  The first and the last job, and one each that stops before the lists start, while
    # they are walked, and at the last iteration
    J = len(its)
    alone = [0, J - 1, int(np.flatnonzero(its < cc.GROUP_FROM)[0]), int(np.flatnonzero((its > cc.GROUP_FROM) & (its < 20) & (np.arange(J) > 0))[0]),
             int(np.flatnonzero(its == 30)[0])]
    assert len(set(alone)) == 5
    for j in alone:
        one = cc.run(ctx, fam, p, [j])
        check_start(fam, one, [j])
        for k in ("T", "fitness", "rmse"):
            assert np.array_equal(one[k][0], out[k][j]), (j, fam["tags"][j], k)


def test_singular_jobs_are_refused_and_leave_their_neighbours_alone(ctx):
    fam, p, out, oracle = against_the_oracle(ctx, "singular")
    sing = [j for j, t in enumerate(fam["tags"]) if t != "neighbour"]
    rest = [j for j, t in enumerate(fam["tags"]) if t == "neighbour"]
    assert len(sing) == 2 and len(rest) == 3
    for j in sing:          # refused: T is RANSAC's, bit for bit, though every source has a neighbour 2 cm away
        assert np.array_equal(out["T"][j], out["T_ransac"][j]) and out["fitness"][j] == 1.0 and out["rmse"][j] > 0.01
    without = cc.run(ctx, fam, p, rest)
    for i, j in enumerate(rest):
        for k in ("T", "fitness", "rmse"):
            assert np.array_equal(without[k][i], out[k][j]), (j, k)
