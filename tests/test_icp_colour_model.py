"""CPU: the job sets of tests/icp_colour_cases.py are what they claim, shown with the oracle alone -- every family reaches the path of
the coloured estimator it exists for, every job that tests/test_gpu_icp_colour.py compares is well conditioned (the rule of
tests/test_icp_model.py, unchanged), a kernel with the slip a family is there to catch would be seen at the GPU tolerance (the oracle
rerun with inputs altered to mimic the slip moves T of some job by 100 tolerances or more), and one Gauss-Newton step of the oracle
agrees with the numpy restatement of oracle/open3d_fp64.py, which shares no statement with oracle_reg.c or the kernel."""
import numpy as np
import pytest

from oracle import open3d_fp64 as o3
from oracle import reg_oracle as ro
from tests import icp_cases as ic
from tests import icp_colour_cases as cc
from tests.test_icp_model import _conditioned, fp32_d2

SEEN = 100 * cc.TOL_T          # the factor tests/test_icp_model.py uses for "visible at the GPU test's tolerance"
I4 = np.eye(4)


def runs_of(name):
    fam = cc.FAMILIES[name]()
    return fam, cc.oracle_all(fam)


def moved_by(fam, runs, j, **altered):
    """how far the altered rerun of job j ends from the plain one"""
    T = cc.oracle_run(fam, j, cc.oracle_start(fam, j)[0], **altered)[0]
    return float(np.abs(T - runs[j][0]).max())


# ------------------------------------------------------------------------------------------------
# the start
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.FAMILIES))
def test_the_start_is_what_the_family_says(name):
    """identity starts: the oracle's matching leaves every source on ONE target, its RANSAC walks the whole (small) budget, validates
    nothing and returns the identity; near starts: every correspondence an inlier of a transform that is not the identity"""
    fam = cc.FAMILIES[name]()
    for j in range(len(fam["js"])):
        fs, ft = cc.job_rows(fam, j)
        a = cc.job_arrays(fam, j)
        corr = ro.feature_match(fs, ft)
        T0, stats = cc.oracle_start(fam, j)
        if fam["start"][j] == "identity":
            assert len(corr) == (len(fs) if len(ft) else 0) and np.all(corr[:, 1] == 0)
            assert np.array_equal(T0, I4), fam["tags"][j]
            assert stats.tolist() == [cc.MAX_ITER if len(corr) >= 3 else 0, 0, 0], (fam["tags"][j], stats)
        else:
            assert len(corr) == len(a["src"]) == len(a["tgt"]) and len(set(corr[:, 1].tolist())) == len(corr)
            assert stats[1] >= 1 and stats[2] == len(corr) and np.abs(T0 - I4).max() > 0.02


# ------------------------------------------------------------------------------------------------
# paths
# ------------------------------------------------------------------------------------------------
def test_strides_walk_the_moments_loop_once_twice_and_three_times():
    fam, runs = runs_of("strides")
    sizes = [len(cc.job_arrays(fam, j)["src"]) for j in range(len(runs))]
    print("iterations", [r[3] for r in runs])
    assert tuple(sizes) == cc.STRIDE_SIZES and all(len(cc.job_arrays(fam, j)["tgt"]) >= 3000 for j in range(len(runs)))
    rounds = [-(-n // cc.STEP_STRIDE) for n in sizes]
    assert rounds[-4:] == [1, 1, 2, 3] and sizes[-3] == cc.STEP_STRIDE
    for j, r in enumerate(runs):          # real work from the identity: every source finds a neighbour and the pose moves by centimetres
        assert r[1] == 1.0 and np.abs(r[0] - I4).max() > 0.03, fam["tags"][j]
    # a moments loop that stops after its first round loses the rows from 2048 on
    gaps = []
    for j in (sizes.index(2049), sizes.index(5000)):
        a = dict(cc.job_arrays(fam, j))
        a["src"], a["src_int"] = a["src"][:cc.STEP_STRIDE], a["src_int"][:cc.STEP_STRIDE]
        gaps.append(moved_by(fam, runs, j, a=a))
    print("first stride only moves T by", gaps)
    assert max(gaps) >= SEEN


def test_many_active_walks_the_active_list_strided_and_unstrided():
    fam, runs = runs_of("many_active")
    its = np.array([r[3] for r in runs])
    print("iterations", its.tolist())
    assert len(its) >= 40
    # listed at iteration 8 = still running after the update of iteration 7; more than 32 of them even run a ninth update
    assert (its >= 9).sum() > cc.ACT_Y > (its >= 20).sum() and (its >= 30).sum() >= 3 and (its < cc.GROUP_FROM).sum() >= 5
    assert ((its > cc.GROUP_FROM) & (its < 20)).any()
    assert all(its[j] < cc.GROUP_FROM for j in cc.MANY_NEAR) and [fam["start"][j] for j in cc.MANY_NEAR] == ["near"] * len(cc.MANY_NEAR)
    for j, tag in cc.MANY_SPECIAL.items():
        assert fam["tags"][j] == tag
        T, fit, rmse, it = runs[j]
        assert fit == 0.0 and rmse == 0.0 and np.array_equal(T, cc.oracle_start(fam, j)[0]), tag
    tag = {t: j for j, t in cc.MANY_SPECIAL.items()}
    assert len(cc.job_arrays(fam, tag["empty source"])["src"]) == 0 and len(cc.job_arrays(fam, tag["empty target"])["tgt"]) == 0
    a = cc.job_arrays(fam, tag["unreachable"])
    assert len(a["src"]) > 0 and np.sqrt(((a["src"][:, None].astype(np.float64) - a["tgt"][None]) ** 2).sum(-1).min()) > 10 * cc.REACH
    assert fam["center"] and np.abs(cc.job_arrays(fam, 0)["means"]).max() > 0.1


def test_pieces_put_correspondences_and_boundary_rows_in_pieces_2_and_3():
    fam, runs = runs_of("pieces")
    assert sorted(int((fam["jt"][j] >= 0).sum()) for j in range(len(runs))) == [2, 2, 3, 3]
    assert any(list(fam["jt"][j] >= 0) == [True, False, True] for j in range(len(runs)))
    rolled = {1: [], cc.PIECE_N: []}
    for j, tag in enumerate(fam["tags"]):
        a = cc.job_arrays(fam, j)
        bounds = np.cumsum([0] + [n for _, n in a["tgt_rows"]])
        # the sides are served from the instance features: pieces further apart than the influence radius (0.6 m)
        for p in range(len(bounds) - 1):
            for q in range(p + 1, len(bounds) - 1):
                d = a["tgt"][bounds[p]:bounds[p + 1], None].astype(np.float64) - a["tgt"][None, bounds[q]:bounds[q + 1]]
                assert np.sqrt((d ** 2).sum(-1).min()) > 0.7
        c = ro.correspondences(a["src"], a["tgt"], I4, cc.REACH)
        share = [float(((c >= bounds[p]) & (c < bounds[p + 1])).sum()) / max(1, (c >= 0).sum()) for p in range(len(bounds) - 1)]
        print(tag, "share of the neighbours per piece", np.round(share, 3), "iterations", runs[j][3])
        assert min(share[1:]) > 0.25 and runs[j][1] == 1.0
        assert all(b in c for b in bounds[1:-1])          # the first row of pieces 2 and 3 is somebody's neighbour
        nrm, grad = cc.job_geometry(fam, j)
        for k in rolled:
            rolled[k].append(moved_by(fam, runs, j, nrm=np.roll(nrm, k, axis=0), grad=np.roll(grad, k, axis=0)))
    print("fields read one row off move T by", rolled[1], "one piece off by", rolled[cc.PIECE_N])
    assert max(rolled[1]) >= SEEN and max(rolled[cc.PIECE_N]) >= SEEN


def in_plane_error(T, frame, centre):
    """what is left of the in-plane shift of a `photometric` source after T, at the patch centre (m)"""
    u, v, n = frame
    start = centre + cc.PHOTO_SHIFT[0] * u + cc.PHOTO_SHIFT[1] * v + cc.PHOTO_LIFT * n
    d = T[:3, :3] @ start + T[:3, 3] - centre
    return float(np.hypot(d @ u, d @ v))


def test_photometric_rows_carry_the_pose():
    fam, runs = runs_of("photometric")
    shift = float(np.hypot(*cc.PHOTO_SHIFT))
    assert 0.02 < shift < cc.REACH
    gaps_l, gaps_g = [], []
    for j, frame in enumerate(cc.photometric_frames()):
        a = cc.job_arrays(fam, j)
        centre = a["tgt"].astype(np.float64).mean(0)
        nrm, grad = cc.job_geometry(fam, j)
        assert np.abs(nrm.astype(np.float64) - frame[2]).max() < 1e-7 and np.abs((grad.astype(np.float64) * nrm).sum(1)).max() < 1e-6
        # the direction of the gradient varies over the patch: the photometric rows alone fix both in-plane shifts and the turn about n
        ang = np.arctan2(grad.astype(np.float64) @ frame[1], grad.astype(np.float64) @ frame[0])
        assert np.ptp(np.unwrap(np.sort(ang))) > 1.0
        left = in_plane_error(runs[j][0], frame, centre)
        T1 = cc.oracle_run(fam, j, I4, lambda_geometric=1.0)[0]
        left1 = in_plane_error(T1, frame, centre) if np.isfinite(T1).all() else np.inf
        print(fam["tags"][j], "in-plane shift", shift, "left with lambda 0.968:", left, "with lambda 1:", left1)
        # the linearised intensity is off by the curvature of the quadratic over a neighbour distance (~1 cm): a fraction of a millimetre
        assert left < 0.002 and left1 > 0.5 * shift
        gaps_l.append(moved_by(fam, runs, j, lambda_geometric=1.0))
        gaps_g.append(moved_by(fam, runs, j, grad=-grad))
    print("lambda_geometric = 1 moves T by", gaps_l, "negated gradients by", gaps_g)
    assert np.nanmax(gaps_l) >= SEEN and max(gaps_g) >= SEEN
    # the axis-aligned plane without photometric rows is the exactly singular system of `singular`: nothing moves
    assert np.array_equal(cc.oracle_run(fam, 0, I4, lambda_geometric=1.0)[0], I4)


def jacobian_rows(a, nrm, grad, T):
    """the 2 n x 6 Jacobian of the correspondences of T, written out from the two residuals (no weights): [s x n, n] and [s x g', g'],
    g' = -(g - (g . n) n)"""
    c = ro.correspondences(a["src"], a["tgt"], T, cc.REACH)
    vs = (a["src"].astype(np.float64) @ T[:3, :3].T + T[:3, 3])[c >= 0]
    n, g = nrm.astype(np.float64)[c[c >= 0]], grad.astype(np.float64)[c[c >= 0]]
    gm = -(g - (g * n).sum(1)[:, None] * n)
    return np.concatenate([np.concatenate([np.cross(vs, n), n], 1), np.concatenate([np.cross(vs, gm), gm], 1)])


def test_singular_jobs_are_singular_with_exact_zeros_and_stop():
    fam, runs = runs_of("singular")
    tags = fam["tags"]
    assert tags.count("neighbour") == 3 and tags[0] == tags[-1] == "neighbour"
    for j, tag in enumerate(tags):
        a = cc.job_arrays(fam, j)
        nrm, grad = cc.job_geometry(fam, j)
        J = jacobian_rows(a, nrm, grad, I4)
        T, fit, rmse, its = runs[j]
        if tag == "neighbour":
            assert np.linalg.matrix_rank(J) == 6 and np.abs(T - I4).max() > 0.01
            continue
        assert fit == 1.0 and len(J) == 2 * len(a["src"])
        zero = [2, 3, 4] if tag == "zero columns" else list(range(6))
        assert np.all(J[:, zero] == 0.0)                       # every ENTRY is zero: so is every sum of products, in any order
        rest = [k for k in range(6) if k not in zero]
        assert not rest or np.linalg.matrix_rank(J[:, rest]) == len(rest)
        assert np.array_equal(T, I4) and its <= 2 and rmse > 0.01          # refused, not converged: the source is 2 cm off its plane


def test_ties_are_ties_under_different_fields_and_the_rule_is_observable():
    fam, runs = runs_of("ties")
    other, runs_o = runs_of("ties_reordered")
    # job 0: at iteration 0 the two nearest targets of most sources tie in fp32; the lowest index wins; the two carry different fields
    a = cc.job_arrays(fam, 0)
    nrm, grad = cc.job_geometry(fam, 0)
    d2 = np.stack([fp32_d2(q, a["tgt"]) for q in a["src"]])
    order = np.argsort(d2, axis=1, kind="stable")[:, :2]
    two = np.take_along_axis(d2, order, 1)
    tied = two[:, 0] == two[:, 1]
    c = ro.correspondences(a["src"], a["tgt"], I4, cc.REACH)
    print("sources whose two nearest targets tie:", int(tied.sum()), "of", len(tied))
    assert tied.sum() * 2 >= len(tied) and np.array_equal(c, order[:, 0])
    w, l = order[tied, 0], order[tied, 1]
    assert np.all(np.abs(nrm[w] - nrm[l]).max(1) > 1e-3) and np.all(np.abs(grad[w] - grad[l]).max(1) > 1e-3)
    assert np.all(a["tgt_int"][w] != a["tgt_int"][l])
    up = a["tgt"][c][:, 2] > a["src"][:, 2]
    assert 0.25 < up[tied].mean() < 0.75
    # jobs 1, 2: replayed iteration by iteration, the only ties between different points fall at iterations m and m + 1
    for j, m in zip((1, 2), ic.LATE_TIE_AT):
        a = cc.job_arrays(fam, j)
        nrm, grad = cc.job_geometry(fam, j)
        T, fit, rmse, its = runs[j]
        assert m >= cc.GROUP_FROM and its == m + 1
        tied = []
        for k in range(its + 1):
            Tk = cc.oracle_run(fam, j, I4, max_iter=k)[0]
            q = (a["src"].astype(np.float64) @ Tk[:3, :3].T + Tk[:3, 3]).astype(np.float32)
            n = 0
            for qi in q:
                d = fp32_d2(qi, a["tgt"])
                o = np.argsort(d, kind="stable")[:2]
                if d[o[0]] == d[o[1]]:
                    n += 1
                    assert o[0] < o[1] and not np.array_equal(nrm[o[0]], nrm[o[1]]) and not np.array_equal(grad[o[0]], grad[o[1]])
                    assert a["tgt_int"][o[0]] != a["tgt_int"][o[1]]
            tied.append(n)
        print("job", j, "tied sources per iteration", tied)
        assert tied[m] == 4 and tied[m + 1] == 4 and sum(tied) == 8
        # the lowest index is the site behind: the job stalls 2^-m of the pull short of the site ahead
        want = I4.copy()
        want[0, 3] = ic.LATE_D * (1.0 - 2.0 ** -m)
        assert np.abs(T - want).max() < 1e-12
    # the same points in the other row order: the other row wins
    for j in range(3):
        for key in ("tgt", "tgt_int"):
            assert np.array_equal(np.sort(cc.job_arrays(fam, j)[key], axis=0), np.sort(cc.job_arrays(other, j)[key], axis=0))
    gaps = [float(np.abs(runs_o[j][0] - runs[j][0]).max()) for j in range(3)]
    print("the other winner moves T by", gaps)
    assert gaps[0] >= SEEN and max(gaps[1:]) >= SEEN


def test_few_points_have_full_rank_or_exact_zeros():
    fam, runs = runs_of("few")
    sizes = [len(cc.job_arrays(fam, j)["src"]) for j in range(len(runs))]
    assert sizes == [3, 4, 5, 1, 2, 1, 2]
    for j, n in enumerate(sizes):
        a = cc.job_arrays(fam, j)
        nrm, grad = cc.job_geometry(fam, j)
        J = jacobian_rows(a, nrm, grad, I4)
        assert len(J) == 2 * n and runs[j][1] == 1.0
        if n >= 3:
            s = np.linalg.svd(J, compute_uv=False)
            print(n, "points: singular values of J", s)
            assert s[-1] > 1e-3 * s[0] and np.abs(runs[j][0] - I4).max() > 0.01
        else:
            zero = [2, 3, 4] if "zero columns" in fam["tags"][j] else list(range(6))
            assert np.all(J[:, zero] == 0.0) and np.array_equal(runs[j][0], I4) and runs[j][3] <= 2


# ------------------------------------------------------------------------------------------------
# conditioning: the rule of tests/test_icp_model.py on every job the GPU test compares
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lo,hi", [("strides", 0, 11), ("many_active", 0, 16), ("many_active", 16, 32), ("many_active", 32, 47), ("pieces", 0, 4),
                                        ("photometric", 0, 2), ("singular", 0, 5), ("ties", 0, 3), ("ties_reordered", 0, 3), ("few", 0, 7)])
def test_coloured_jobs_are_well_conditioned(name, lo, hi):
    fam, runs = runs_of(name)
    assert hi <= len(runs) and (hi == len(runs) or name == "many_active")
    worst = 0.0
    for j in range(lo, hi):
        T0 = cc.oracle_start(fam, j)[0]
        a = cc.job_arrays(fam, j)
        worst = max(worst, _conditioned(runs[j], lambda k: cc.oracle_run(fam, j, ic.perturbed(T0, k), a=a)))
    print(name, lo, hi, "T moves by", worst)


def test_every_job_is_covered_by_the_conditioning_check():
    assert len(cc.many_active()["js"]) == 47 and set(cc.FAMILIES) == {"strides", "many_active", "pieces", "photometric", "singular", "ties", "ties_reordered", "few"}


# ------------------------------------------------------------------------------------------------
# one independent step
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,j", [("photometric", 0), ("photometric", 1), ("strides", 5), ("strides", 9)])
def test_first_iteration_agrees_with_the_numpy_restatement(name, j):
    """oracle_reg.c and the kernel are written from the same statements; oracle/open3d_fp64.colored_icp_step is not (kd-tree neighbours
    in fp64, numpy Jacobians, LAPACK solve).  One step from the start, to 1e-9 in T."""
    fam = cc.FAMILIES[name]()
    a = cc.job_arrays(fam, j)
    nrm, grad = cc.job_geometry(fam, j)
    T0 = cc.oracle_start(fam, j)[0]
    step = o3.colored_icp_step(a["src"], a["src_int"], a["tgt"], nrm, a["tgt_int"], grad, T0, cc.REACH)
    T1 = cc.oracle_run(fam, j, T0, max_iter=1)[0]
    gap = np.abs(step["T_new"] - T1).max()
    print(name, j, "correspondences", step["n_corr"], "one step moves T by", np.abs(T1 - T0).max(), "the two disagree by", gap)
    assert step["n_corr"] >= 200 and np.abs(T1 - T0).max() > 0.01 and gap < 1e-9
