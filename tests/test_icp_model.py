"""CPU: the job sets of tests/icp_cases.py are what they claim, shown with the oracle alone -- so that a later edit of a case cannot
quietly stop exercising the path it exists for (the grouped search and the active-job lists from iteration 8, the strided walk of
more than 32 listed jobs, ties, pieces, degenerate jobs), and so that holding EVERY job of tests/test_gpu_icp.py to 1e-6 is fair: no
job may sit on a rounding boundary (conditioning)."""
import numpy as np
import pytest

from tests import icp_cases as ic
from oracle import reg_oracle as ro

GPU_TOL_T = 1e-6          # the tolerance tests/test_gpu_icp.py holds T to


def p2p_runs(name):
    fam = ic.P2P_FAMILIES[name]()
    return fam, [ic.oracle_p2p(fam, j) for j in range(len(fam["js"]))]


def test_many_jobs_walks_the_active_list_strided_and_unstrided():
    fam, runs = p2p_runs("many_jobs")
    its = np.array([r[3] for r in runs])
    print("iterations", its.tolist())
    assert len(its) == 40
    sizes = [len(ic.job_arrays(fam, j)["src"]) for j in range(40)]
    assert set(sizes) == set(ic.SIZES)
    # listed at iteration 8 = still running after the update of iteration 7; more than 32 of them even run a ninth update
    assert (its >= 9).sum() >= 33 and (its >= 20).sum() < 32 and (its >= 30).sum() >= 3 and (its < 8).sum() >= 5
    assert (its >= ic.GROUP_FROM).sum() > ic.ACT_Y
    tag = {t: j for j, t in enumerate(fam["tags"])}
    for t in ("empty source", "empty target", "unreachable"):
        T, fit, rmse, it = runs[tag[t]]
        assert fit == 0.0 and rmse == 0.0 and np.array_equal(T, np.eye(4)), t
    assert len(ic.job_arrays(fam, tag["empty source"])["src"]) == 0 and len(ic.job_arrays(fam, tag["empty target"])["tgt"]) == 0
    # never a neighbour, whatever the iteration: the nearest target is further than the reach by more than the job could ever move
    a = ic.job_arrays(fam, tag["unreachable"])
    assert len(a["src"]) > 0 and np.sqrt(((a["src"][:, None].astype(np.float64) - a["tgt"][None]) ** 2).sum(-1).min()) > 10 * ic.REACH
    a = ic.job_arrays(fam, tag["single target point"])
    assert len(a["tgt"]) == 1 and runs[tag["single target point"]][1] == 1.0


@pytest.mark.parametrize("name", ["pieces", "long_side"])
def test_pieces_and_long_side_reach_the_grouped_search(name):
    fam, runs = p2p_runs(name)
    print(name, "iterations", [r[3] for r in runs])
    assert all(r[3] >= 9 for r in runs)
    if name == "long_side":
        assert len(ic.job_arrays(fam, 0)["src"]) == 5000 > 2 * ic.STEP_STRIDE
        return
    assert sorted((int((fam["js"][j] >= 0).sum()), int((fam["jt"][j] >= 0).sum())) for j in range(len(runs))) == [(2, 2)] * 3 + [(3, 3)] * 2
    assert any(list(fam["jt"][j] >= 0) == [True, False, True] for j in range(len(runs)))
    # overlapping pieces: at the identity a good share of the nearest neighbours lies in each piece behind the first
    for j, t in enumerate(fam["tags"]):
        a = ic.job_arrays(fam, j)
        c = ro.correspondences(a["src"], a["tgt"], np.eye(4), ic.REACH)
        bounds = np.cumsum([0] + [n for _, n in a["tgt_rows"]])
        share = [float(((c >= bounds[p]) & (c < bounds[p + 1])).sum()) / max(1, (c >= 0).sum()) for p in range(len(bounds) - 1)]
        print(t, "share of the neighbours per piece", np.round(share, 3))
        if t.startswith("overlap"):
            assert min(share) > 0.15


def test_centred_jobs_run_into_the_grouped_search():
    fam, runs = p2p_runs("centred")
    assert fam["center"] and all(r[3] >= 9 for r in runs)
    assert any((fam["jt"][j] >= 0).sum() == 3 for j in range(len(runs)))
    for j in range(len(runs)):
        assert np.abs(ic.job_arrays(fam, j)["means"]).max() > 0.1          # (a centring that did nothing would prove nothing)


def test_ties_are_ties_and_the_rule_is_observable():
    fam, runs = p2p_runs("ties")
    a = ic.job_arrays(fam, 0)
    d2 = np.empty((len(a["src"]), len(a["tgt"])), np.float32)
    for i, q in enumerate(a["src"]):
        d2[i] = fp32_d2(q, a["tgt"])
    two = np.sort(d2, axis=1)[:, :2]
    tied = two[:, 0] == two[:, 1]
    c = ro.correspondences(a["src"], a["tgt"], np.eye(4), ic.REACH)
    assert np.all(c >= 0) and np.array_equal(d2[np.arange(len(c)), c], two[:, 0])
    print("sources whose two nearest targets tie:", int(tied.sum()), "of", len(tied))
    assert tied.sum() * 2 >= len(tied)
    # "lowest original index" is not "first in cell order": the rule picks the upper layer for some sources and the lower for others
    up = a["tgt"][c][:, 2] > a["src"][:, 2]
    assert 0.25 < up[tied].mean() < 0.75
    assert runs[0][3] >= 9
    rev = ic.ties_reversed()
    T_rev = ic.oracle_p2p(rev, 0)[0]
    print("reversed target rows move T by", np.abs(T_rev - runs[0][0]).max())
    assert np.abs(T_rev - runs[0][0]).max() > 1e-4
    b = ic.job_arrays(fam, 1)
    assert len(b["tgt"]) == 2 * len(a["tgt"]) and len(np.unique(b["tgt"], axis=0)) == len(a["tgt"])


def fp32_d2(q, tgt):
    """the fp32 distance of the oracle and the kernels, fma(dz, dz, fma(dy, dy, dx * dx)), from one float32 query to every target"""
    dx, dy, dz = (q[None] - tgt).T
    return (dz.astype(np.float64) * dz + (dy.astype(np.float64) * dy + (dx * dx).astype(np.float64)).astype(np.float32)).astype(np.float32)


def test_late_ties_fall_in_the_grouped_search_and_the_rule_is_observable():
    """the only ties between points at DIFFERENT coordinates that the grouped search (iteration >= 8) ever has to decide: replayed
    iteration by iteration, the sources whose two nearest targets are equally far are counted under the transform of that iteration"""
    fam, runs = p2p_runs("late_ties")
    other = ic.late_ties_reordered()
    for j, m in enumerate(ic.LATE_TIE_AT):
        a = ic.job_arrays(fam, j)
        T, fit, rmse, its = runs[j]
        assert m >= ic.GROUP_FROM and its == m + 1 >= 9
        tied = []
        for k in range(its + 1):
            Tk = ro.icp(a["src"], None, a["tgt"], None, None, None, ic.REACH, np.eye(4), colored=False, max_iter=k)[0]
            q = (a["src"].astype(np.float64) @ Tk[:3, :3].T + Tk[:3, 3]).astype(np.float32)
            n = 0
            for qi in q:
                d = fp32_d2(qi, a["tgt"])
                o = np.argsort(d, kind="stable")[:2]
                n += int(d[o[0]] == d[o[1]] and not np.array_equal(a["tgt"][o[0]], a["tgt"][o[1]]))
            tied.append(n)
        print("job", j, "tied sources per iteration", tied)
        assert tied[m] == 4 and tied[m + 1] == 4 and sum(tied) == 8
        # the lowest index is the site behind: the job ends e_m short of the site ahead.  With the site ahead in front of the chain it ends on it
        assert np.array_equal(T[:3, :3], np.eye(3)) and np.array_equal(T[:3, 3], [ic.LATE_D * (1.0 - 2.0 ** -m), 0.0, 0.0])
        gap = np.abs(ic.oracle_p2p(other, j)[0] - T).max()
        print("job", j, "another row order moves T by", gap)
        assert gap == ic.LATE_D * 2.0 ** -m >= 50 * GPU_TOL_T


def test_few_sources_find_neighbours():
    fam, runs = p2p_runs("few_sources")
    assert [len(ic.job_arrays(fam, j)["src"]) for j in range(2)] == [1, 1]
    assert all(r[1] == 1.0 for r in runs)          # (the one- and two-point sources of many_jobs never find a neighbour)


# ------------------------------------------------------------------------------------------------
# coloured.  The correct jobs start from a good RANSAC transform and stop after 4 to 8 iterations: only the three wrong assignments take
# the coloured estimator through the grouped search and the active-job lists.
# No `coloured_dup` family (a target side of two instances with the same coordinates and different intensities): coincident instances
# are within each other's influence radius, so the product recomputes that side's normals and gradients in context and does not hand
# them out -- there are no rows to give the oracle, and normals of the oracle's own on a cloud in which every point is double differ
# from the product's by the order of its 30 nearest neighbours, far above 1e-6.  Whether swapping the pieces moves the oracle's T was
# therefore not tried.  Late ties between different points are covered by `late_ties` instead.
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coloured_runs():
    """per job: start (the oracle's RANSAC transform), the oracle's target normals and gradients, and the run from there"""
    fam = ic.coloured()
    out = []
    for j in range(len(fam["js"])):
        a, raw = ic.job_arrays(fam, j), ic.job_arrays(fam, j, center=False)
        T, rmse, fit, Tr, stats = ro.register_point_clouds(a["src"], a["src_int"], a["tgt"], a["tgt_int"], ic.VOXEL, ic.GLOBAL, ic.LOCAL, seed=ic.COL_SEED_RANSAC,
                                                           job_id=ic.COL_JOB_ID_BASE + j, src_raw=raw["src"], tgt_raw=raw["tgt"])
        nrm = ro.normals(raw["tgt"], 2 * ic.VOXEL, 30)
        grad = ro.color_gradient(raw["tgt"], nrm, a["tgt_int"], 2 * ic.REACH, 30)
        run = ic.oracle_coloured(fam, j, nrm, grad, Tr)
        assert np.array_equal(run[0], T)          # (the stage alone, from the RANSAC transform, is what the whole registration ends with)
        out.append(dict(T0=Tr, nrm=nrm, grad=grad, run=run))
    return fam, out


def test_coloured_family(coloured_runs):
    fam, runs = coloured_runs
    its = [r["run"][3] for r in runs]
    print("iterations", its)
    assert 7 <= len(its) <= 9
    assert sum(it >= 9 for it in its) >= 3
    assert sum(t == "wrong" for t in fam["tags"]) >= 3
    assert sorted(int((fam["jt"][j] >= 0).sum()) for j, t in enumerate(fam["tags"]) if t != "wrong") == [1, 1, 1, 2, 3]
    # the photometric term is visible at the GPU test's tolerance: without it a correct job ends 100 tolerances away at the least
    j = 1
    assert fam["tags"][j] == "correct"
    T1 = ic.oracle_coloured(fam, j, runs[j]["nrm"], runs[j]["grad"], runs[j]["T0"], lambda_geometric=1.0)[0]
    print("lambda_geometric = 1 moves T of job", j, "by", np.abs(T1 - runs[j]["run"][0]).max())
    assert np.abs(T1 - runs[j]["run"][0]).max() >= 100 * GPU_TOL_T


# ------------------------------------------------------------------------------------------------
# conditioning: five starts moved by 1e-13 give the same fitness and rmse, bit for bit, and a T within 1e-11 (measured: 2e-13).  A job
# that fails has a correspondence on a rounding boundary: it gets another seed in icp_cases.py, not a tolerance in the GPU test.
# ------------------------------------------------------------------------------------------------
def _conditioned(base, rerun):
    T, fit, rmse, it = base
    worst = 0.0
    for k in range(5):
        Tk, fk, rk, _ = rerun(k)
        assert fk == fit and rk == rmse
        worst = max(worst, float(np.abs(Tk - T).max()))
    assert worst < 1e-11
    return worst


@pytest.mark.parametrize("name,lo,hi", [("many_jobs", 0, 14), ("many_jobs", 14, 28), ("many_jobs", 28, 40), ("pieces", 0, 2), ("pieces", 2, 4), ("pieces", 4, 5), ("long_side", 0, 1),
                                        ("ties", 0, 2), ("late_ties", 0, 2), ("few_sources", 0, 2), ("centred", 0, 2)])
def test_point_to_point_jobs_are_well_conditioned(name, lo, hi):
    fam = ic.P2P_FAMILIES[name]()
    worst = 0.0
    for j in range(lo, hi):
        base = ic.oracle_p2p(fam, j)
        worst = max(worst, _conditioned(base, lambda k: ic.oracle_p2p(fam, j, ic.perturbed(np.eye(4), k))))
    print(name, lo, hi, "T moves by", worst)


def test_coloured_jobs_are_well_conditioned(coloured_runs):
    fam, runs = coloured_runs
    worst = 0.0
    for j, r in enumerate(runs):
        worst = max(worst, _conditioned(r["run"], lambda k: ic.oracle_coloured(fam, j, r["nrm"], r["grad"], ic.perturbed(r["T0"], k))))
    print("coloured: T moves by", worst)
