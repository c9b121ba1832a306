"""-m gpu: the RANSAC stage alone (csrc/reg_ransac.hip) against `oracle.reg_oracle.ransac`, job by job, on the job sets of
tests/ransac_cases.py (tests/test_ransac_model.py shows with the oracle alone that every set reaches the path it is named for).  The
stage is fed through injected instance features (tests/regmatch_cases.py): the rows are trivially separable, so the correspondence
list is the full bijection and only the geometry varies.  For EVERY job `ransac_stats` (walked, validated, best inliers) equals the
oracle's and |T_ransac - T_oracle| <= 1e-6 per entry, the bound tests/test_gpu_register.py applies to this output; there is no
tolerance on the statistics and no share of jobs that may miss.  Status bits 1 (grid overflow), 16 and 32 (a call redone with the VALU
search / with a full survivor list) stay clear, and every row comes from the injected features (reuse[1] == 0).

family        path it exists for                                                                                  largest |T_ransac - T_oracle|
stop_rounds   one job per stopping place of the scheduler: round 1, 2, 3, behind the first host read-back         0
              (a 2^20 round of two jobs), and ransac_max_iter = 700 000 off every round boundary
fixed_budget  IBL_REG_FIXED_BUDGET: walked == ransac_max_iter                                                     0
many_active   88 slots: the <RANSAC_BIG_SUBS> flag kernel in the 262 144 round, then a compacted active list      0
              (slot != job); empty / 1 / 2 / 3-point jobs in between; single jobs byte-equal to the batch
tail          six jobs in rounds of 2^20 hypotheses, the budget of 1 500 000 ends inside the second               0
lds_edge      n_corr 1023 / 1024 / 1025 / 3000: correspondences staged in LDS or drawn from global memory         0
dense_fold    30 .. 60 correspondences, all inliers + noise: thousands of survivors per job and round, the        0
              fold walks several 64-chunks, est_k stops it inside one; ties in fitness decided by rmse
dense_fixed   the same with a fixed budget of 20 000: the fold walks every chunk of two rounds                    0
degenerate    n_corr 3, 4, 5: repeated draws, zero-length edges, Kabsch of rank 0 and 1; collinear lists          0
edge_band     squared edge ratios within 3e-6 of 0.81 on both sides: the fp32 test defers to the exact one        0
ids_seed      seed with a high word, job ids >= 2^31 out of order, center=True                                    0
Measured on an MI355X: all 160 jobs agree in the three statistics, and every T_ransac is bit-identical to the oracle's
(largest gap 0 in every family).  No case had to be replaced.  The whole
file takes 5 s, the slowest tests 0.4 s (fixed_budget, tail, many_active with its seven single-job calls).
"""
import numpy as np
import pytest

from tests import ransac_cases as rs
from tests import regmatch_cases as rc

pytestmark = pytest.mark.gpu

TOL_T = 1e-6


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(6 << 30)
    yield c
    c.close()


def compare(name, fam, out, jobs=None):
    """every job against the oracle: statistics equal, T_ransac within TOL_T; prints the largest gap, then asserts all jobs"""
    jobs = list(range(len(fam["js"]))) if jobs is None else list(jobs)
    want = [rc.expected(fam, j) for j in jobs]
    gaps = np.array([np.abs(out["T_ransac"][k] - w[1]).max() for k, w in enumerate(want)])
    print(f"{name}: {len(jobs)} jobs, largest gap in T_ransac {gaps.max():.2e}")
    missed = [(j, fam["tags"][j], out["ransac_stats"][k].tolist(), want[k][2].tolist(), float(gaps[k])) for k, j in enumerate(jobs)
              if not (np.array_equal(out["ransac_stats"][k], want[k][2]) and gaps[k] <= TOL_T)]
    assert not missed, missed
    return gaps.max()


def run_family(ctx, name, pools=None):
    fam = rs.FAMILIES[name]()
    ctx.status()                                               # clear the sticky bits of earlier tests
    p = pools or rc.pools(ctx, fam)
    out = rc.run(ctx, fam, p)
    st = ctx.status()
    assert st & (1 | 16 | 32) == 0, st
    compare(name, fam, out)
    return fam, p, out


@pytest.mark.parametrize("name", ["stop_rounds", "fixed_budget", "tail", "lds_edge", "dense_fold", "dense_fixed", "degenerate", "edge_band"])
def test_family(ctx, name):
    fam, p, out = run_family(ctx, name)
    assert np.array_equal(out["means"], np.zeros_like(out["means"]))          # center=False
    if fam["fixed_budget"]:
        assert (out["ransac_stats"][:, 0] == fam["max_iter"]).all()


def test_many_active_every_job_and_no_job_depends_on_its_neighbours(ctx):
    fam, p, out = run_family(ctx, "many_active")
    for j, t in enumerate(fam["tags"]):
        if t in ("empty source", "empty target", "1 point", "2 points"):
            assert np.array_equal(out["T_ransac"][j], np.eye(4)) and not out["ransac_stats"][j].any(), t
    # one job per call, with its own id: byte-equal to the batch's.  The first and the last slot, a job that stops in round 1, one in the
    # wide round, two that outlive the read-back, the 3-point job
    tag = fam["tags"]
    alone = [0, len(tag) - 1, tag.index("quick"), 50, rs.MANY_SLOW[1], rs.MANY_NEVER, tag.index("3 points")]
    assert len(set(alone)) == len(alone) and tag[0] == tag[50] == "6/150"
    for j in alone:
        one = rc.run(ctx, fam, p, jobs=[j])
        for k in ("T_ransac", "ransac_stats"):
            assert np.array_equal(one[k][0], out[k][j]), (j, tag[j], k)
    assert ctx.status() & (1 | 16 | 32) == 0


def test_ids_seed_centred(ctx):
    fam, p, out = run_family(ctx, "ids_seed")
    for j in range(len(fam["js"])):
        assert np.allclose(out["means"][j], rc.job_arrays(fam, j)["means"], atol=1e-9)
