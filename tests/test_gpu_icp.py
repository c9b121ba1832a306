"""-m gpu: the ICP stage alone (csrc/reg_icp.hip) against `oracle.reg_oracle.icp`, job by job, on the job sets of tests/icp_cases.py
(tests/test_icp_model.py shows with the oracle alone that every set exercises what it is there for and that no job sits on a
rounding boundary).  Every job is held to what test_point_to_point_fallback holds its single job to: |T - T_oracle| <= 1e-6 per
entry, fitness to 1e-9, rmse to 1e-7 -- there is no share of jobs that may miss.

Point-to-point families run through register_batch(have_colors=False): the stage from the identity, nothing in front of it.  The
coloured family runs the whole registration with both sides' instance features; the oracle then starts from the product's own RANSAC
transform and reads the target normals and gradients out of the memory's instance features (nothing is recomputed in context on
that world, so those rows are what the stage read) -- features, matching and RANSAC drop out of the comparison.

family      path it exists for                                                                  largest gap to the oracle (T, fitness, rmse)
many_jobs   40 jobs: the active-job lists walked with a stride (36 listed > 32 block rows at iteration 8)
            and without (fewer later); sources of 0 .. 3000 points; empty / unreachable / single-point jobs   1.7e-13, 0, 0
pieces      2 and 3 instances per side, apart and overlapping, an empty middle slot: the minimum carried
            from piece to piece by the thread-per-point and the grouped search                                  1.5e-14, 0, 0
long_side   5000 sources: more than one stride (2048) of the moments kernel, 20 chunks                          8.9e-15, 0, 0
ties        equal fp32 distances decided by the lowest original index (all 722 sources at iteration 0:
            the thread-per-point search)                                                                         1.8e-15, 0, 0
late_ties   the same rule in the grouped search: ties between different points from iteration 8 / 10 on          0, 0, 0
few_sources a single source with a neighbour: the Kabsch step of rank 0 from one source point                    0, 0, 0
centred     center=True: the means and the centred clouds                                                       1.6e-15, 0, 0
coloured    the coloured estimator (geometric + photometric rows, 6 x 6 solve), wrong assignments that run
            all 30 iterations in the grouped search (the correct jobs stop after 4 to 8 iterations: only the
            three wrong assignments take this estimator past iteration 8)                                        5.6e-16, 0, 0
            (its edges -- strides of the moments loop, the strided active list, pieces, photometric rows,
            refused singular systems, ties, few points -- on injected fields: tests/test_gpu_icp_colour.py)
"""
import numpy as np
import pytest

from tests import icp_cases as ic

pytestmark = pytest.mark.gpu

TOL_T, TOL_FIT, TOL_RMSE = 1e-6, 1e-9, 1e-7


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(4 << 30)
    yield c
    c.close()


def batches(fam):
    from ibloc_amd.registration import CloudBatch
    return CloudBatch.from_numpy(fam["det"], fam["det_int"]), CloudBatch.from_numpy(fam["mem"], fam["mem_int"])


def run_p2p(ctx, fam, pools=None):
    from ibloc_amd.registration import register_batch
    det, mem = pools or batches(fam)
    out = register_batch(ctx, det, mem, fam["js"], fam["jt"], ic.VOXEL, ic.GLOBAL, ic.LOCAL, have_colors=False, center=fam["center"])
    assert ctx.status() & 1 == 0
    return out


def compare(name, fam, out, oracle):
    """every job against its oracle run (T, fitness, rmse, iterations); prints the largest gaps, then asserts all jobs"""
    gaps = np.array([[np.abs(out["T"][j] - o[0]).max(), abs(out["fitness"][j] - o[1]), abs(out["rmse"][j] - o[2])] for j, o in enumerate(oracle)])
    worst = gaps.max(0)
    print(f"{name}: {len(oracle)} jobs, largest gap T {worst[0]:.2e} fitness {worst[1]:.2e} rmse {worst[2]:.2e}; oracle iterations {[o[3] for o in oracle]}")
    missed = [(j, fam["tags"][j], oracle[j][3], gaps[j].tolist()) for j in range(len(oracle))
              if not (gaps[j, 0] <= TOL_T and gaps[j, 1] < TOL_FIT and gaps[j, 2] < TOL_RMSE)]
    assert not missed, missed
    return worst


def oracle_p2p(fam):
    return [ic.oracle_p2p(fam, j) for j in range(len(fam["js"]))]


def check_means(fam, out):
    for j in range(len(fam["js"])):
        assert np.allclose(out["means"][j], ic.job_arrays(fam, j)["means"], atol=1e-9)


def test_many_jobs_every_job_and_no_job_depends_on_its_neighbours(ctx):
    fam = ic.many_jobs()
    pools = batches(fam)
    out = run_p2p(ctx, fam, pools)
    oracle = oracle_p2p(fam)
    compare("many_jobs", fam, out, oracle)
    its = np.array([o[3] for o in oracle])
    assert (its >= ic.GROUP_FROM).sum() > ic.ACT_Y > (its >= 20).sum()
    for j, t in enumerate(fam["tags"]):
        if t in ("empty source", "empty target", "unreachable"):
            assert np.array_equal(out["T"][j], np.eye(4)) and out["fitness"][j] == 0.0 and out["rmse"][j] == 0.0, t
    # one job per call: byte-equal to the batch's.  The first and the last job, and one each that stops before the lists start, while
    # they are walked, and at the last iteration
    J = len(its)
    alone = [0, J - 1, int(np.flatnonzero(its < ic.GROUP_FROM)[0]), int(np.flatnonzero((its > ic.GROUP_FROM) & (its < 20))[0]),
             int(np.flatnonzero(its == 30)[0])]
    assert len(set(alone)) == 5
    for j in alone:
        one = run_p2p(ctx, ic.sub_family(fam, [j]), pools)
        for k in ("T", "fitness", "rmse"):
            assert np.array_equal(one[k][0], out[k][j]), (j, fam["tags"][j], k)


@pytest.mark.parametrize("name", ["pieces", "long_side", "ties", "late_ties", "few_sources"])
def test_point_to_point_family(ctx, name):
    fam = ic.P2P_FAMILIES[name]()
    out = run_p2p(ctx, fam)
    compare(name, fam, out, oracle_p2p(fam))
    assert np.array_equal(out["means"], np.zeros_like(out["means"]))          # center=False


def test_centred(ctx):
    fam = ic.centred()
    out = run_p2p(ctx, fam)
    check_means(fam, out)
    compare("centred", fam, out, oracle_p2p(fam))


def test_coloured_stage_from_the_products_own_ransac_transform(ctx):
    """The 1e-6 / 1e-9 / 1e-7 of the point-to-point path, applied to the coloured estimator (wrong assignments included).
    Measured on an MI355X: the largest gap over the eight jobs is 5.6e-16 in T and none in fitness and rmse, so the tolerances stand as
    they are (the oracle's own sensitivity to a start moved by 1e-13 is 2e-13)."""
    from ibloc_amd.registration import instance_features_batch, register_batch
    fam = ic.coloured()
    det, mem = batches(fam)
    fd = instance_features_batch(ctx, det, ic.VOXEL)
    fm = instance_features_batch(ctx, mem, ic.VOXEL, grad_radius=2 * ic.REACH)
    out = register_batch(ctx, det, mem, fam["js"], fam["jt"], ic.VOXEL, ic.GLOBAL, ic.LOCAL, seed=ic.COL_SEED_RANSAC, job_id_base=ic.COL_JOB_ID_BASE,
                         have_colors=True, center=True, det_features=fd, mem_features=fm)
    assert ctx.status() & 1 == 0
    print("reuse", out["reuse"])
    assert out["reuse"][0] > 0 and out["reuse"][1] == 0          # every row from the cache: the borrowed rows are the ones the stage read
    check_means(fam, out)
    nrm_all, grad_all, off = fm.normals[:mem.n, :3].cpu().numpy(), fm.grad[:mem.n, :3].cpu().numpy(), mem.seg_off_host
    oracle = []
    for j in range(len(fam["js"])):
        rows = np.concatenate([np.arange(off[s], off[s] + n) for s, n in ic.job_arrays(fam, j)["tgt_rows"]])
        oracle.append(ic.oracle_coloured(fam, j, nrm_all[rows], grad_all[rows], out["T_ransac"][j]))
    compare("coloured", fam, out, oracle)
    assert sum(o[3] >= 9 for o in oracle) >= 3
