"""-m gpu: grids, hybrid neighbourhoods, normals, FPFH, colour gradients and radius-outlier masks vs the C oracle (csrc/knn_select.h and
its consumers reg_normals.hip, reg_fpfh.hip, reg_colorgrad.hip; reg_radius.hip).

EVERY ROW.  The clouds of tests/feature_cases.py (tests/test_feature_model.py shows with the references alone what each is there for,
and that the two references agree on every row where their neighbour sets do) go through `normals_fpfh_batch` and
`instance_features_batch` under the default switches and under knn_noguess, feat_unfused, spfh_f64 and spfh_qcap=8, each compared with
the ORACLE, no row left out:
    radius-outlier mask   equal
    normals               every component within 2^-22 of ro.normals, sign included (both sides solve in double from identical fp32
                          points: one rounding of a value <= 1 to fp32 each); exactly (0, 0, 1) with fewer than 3 neighbours
    FPFH                  every entry within 2^-14 of ro.fpfh(cloud, DEVICE normals) (integer histograms, weighted sums in double on
                          both sides, values <= 200 where an fp32 ulp is 2^-16; one pair in a wrong bin of a NEIGHBOUR's histogram moves
                          an entry by about 1e-2); exactly zero with k <= 1
    gradients             every row within 1e-4 x max(1, max|g| of the cloud) of ro.color_gradient(cloud, DEVICE normals); exactly zero
                          with fewer than 4 neighbours
The oracle is given the device's normals so that a finding in the normals does not cascade into the other two.

PATHS, observed with knn_debug=1 (`[knn] ... fallback=` per tile search) and ctx.status():
    staged tile              uniform alone: fallback == 0 in every search, status 0
    tile that cannot stage   clump alone: the 2 000 points of the clump exceed the 1 600 / 1 024-candidate cap at every reach: fallback >=
                             the clump in the k = 100 search, 0 < fallback < queries in the k = 30 searches
    sparse-spot fallback     sparse alone (isolated points over a dense plane): no tile near a cap, still 0 < fallback <= 80: queries
                             whose cube cannot show their k nearest
    boundary-bin slow path   boundary alone: status bit 1 (IBL_ST_KNN_SLOWPATH) set, clear after status(clear=True)

Which instantiations the public calls reach (read off reg_api.hip and launch_knn, knn_select.h): every search kernel that is built.
Every search of `normals_fpfh_batch`, `instance_features_batch` and the registration runs on a grid of ibl_build_tile_grid, whose tile
edge (KNN_TILE_NORMAL = 4, KNN_TILE_FEATURE = 2, reg_common.h) is the one the consumer's factory states, and launch_knn instantiates
that factory's one tile kernel + ibl_knn_list_kernel: <4, 1024, NormalFactory> (feat_unfused), <4, 1024, GradFactory>,
<2, 1600, SpfhFactory, packed> (feat_unfused), <2, 1600, ListNormalFactory, packed> (default), ibl_knn_list_kernel of the four factories,
ibl_radius_count_kernel.  The per-query kernel for grids without tiles and the tiles no factory is searched on (<2, 2560, *>,
<4, 1024> of the two packed factories) could not be launched and are no longer built.  If a call ever reached launch_knn with a grid of
another edge or without tiles it would return IBL_ERR_INTERNAL ("k-NN tiles of %d^3 cells are not built", "k-NN search needs a tile
grid") instead of launching: every test here that runs a search asserts, through _lib.check, that none did.

Measured on an MI355X: on every cloud, under every switch and through both calls the worst row of normals, FPFH and gradients differs
from the oracle by 0 (the fp32 outputs are equal bit for bit), and the radius-outlier masks are equal.  With Cramer's rule in the 3 x 3
solve of the gradients, on both sides, the device missed the fp64 least-squares restatement on `clump` by 5.3e-4 x max|g| (44 rows over
1e-4 x max|g|); with the LDL^T solve by 3.4e-8.
fallback of queries per search (r, k, ts):  (0.1, 30, 4)   (0.15, 30, 4)   (0.25, 100, 2)
    uniform   1 500 queries                      0              0               0           status 0
    clump     3 060                          2 156          2 172           2 304           status 2 (dense first bins inside the clump)
    sparse    2 040                             23             31              19           status 0
    boundary  1 911                          1 743          1 826           1 726           status 2
"""
import numpy as np
import pytest
import torch

from ibloc_amd.synth import SynthWorld
from oracle import reg_oracle as ro
from tests import feature_cases as fc

pytestmark = pytest.mark.gpu

SWITCHES = {"default": {}, "knn_noguess": dict(knn_noguess=1), "feat_unfused": dict(feat_unfused=1), "spfh_f64": dict(spfh_f64=1),
            "spfh_qcap": dict(spfh_qcap=8)}

@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(2 << 30)
    yield c
    c.close()


def clouds(sizes, seed):
    w = SynthWorld(len(sizes), pts_per_object=max(sizes), E=1, D=8, seed=seed)
    out = []
    for i, n in enumerate(sizes):
        p = w.points[i][:n]
        out.append((p - p.mean(0)).astype(np.float32))
    return out


# ------------------------------------------------------------------------------------------------
# every row against the oracle
# ------------------------------------------------------------------------------------------------
_oracle_rows = {}


def oracle_given_normals(case, nrm):
    """ro.fpfh and ro.color_gradient of the case with the DEVICE's normals, computed once per distinct set of normals"""
    key = (case["name"], nrm.tobytes())
    if key not in _oracle_rows:
        p = case["pts"]
        _oracle_rows[key] = (ro.fpfh(p, nrm, *fc.FEATURE), ro.color_gradient(p, nrm, case["intensity"], *fc.GRAD))
    return _oracle_rows[key]


def run_calls(ctx, cases, grad=True, **switches):
    """the cases as ONE batch through both public calls -> per case dict(a=(normals, fpfh) of normals_fpfh_batch, b=(normals, fpfh in
    natural bin order, gradients) of instance_features_batch), and the status word (cleared)"""
    from ibloc_amd.registration import FEAT_ORDER, CloudBatch, instance_features_batch, normals_fpfh_batch
    b = CloudBatch.from_numpy([c["pts"] for c in cases], [c["intensity"] for c in cases])
    with ctx.diag(**switches):
        nrm, fpfh = normals_fpfh_batch(ctx, b, fc.NORMAL[0], fc.NORMAL[1], fc.FEATURE[0], fc.FEATURE[1])
        feat = instance_features_batch(ctx, b, fc.VOXEL, grad_radius=fc.GRAD[0] if grad else 0.0)
    torch.cuda.synchronize()
    status = ctx.status(clear=True)
    n = b.n
    nrm, fpfh = nrm.cpu().numpy()[:, :3], fpfh.cpu().numpy()
    nb = feat.normals[:n].cpu().numpy()[:, :3]
    fb = np.empty((n, 33), np.float32)
    fb[:, FEAT_ORDER] = feat.fpfh[:n].cpu().numpy()                      # resident rows are stored in matching order
    gb = feat.grad[:n].cpu().numpy()[:, :3] if grad else None
    off = b.seg_off_host
    out = []
    for i in range(len(cases)):
        lo, hi = off[i], off[i + 1]
        out.append(dict(a=(nrm[lo:hi], fpfh[lo:hi], None), b=(nb[lo:hi], fb[lo:hi], None if gb is None else gb[lo:hi])))
    return out, status


def compare_rows(label, case, nrm, fpfh, grad):
    """one case's device rows against the oracle; prints the worst row of each quantity, returns the list of what missed"""
    n = len(case["pts"])
    assert nrm.shape == (n, 3) and fpfh.shape == (n, 33)
    if n == 0:
        return []
    ref = fc.reference(case)
    missed = []
    for name, rows in (("normals", nrm), ("fpfh", fpfh), ("gradient", grad)):
        if rows is not None and not np.isfinite(rows).all():
            missed.append((label, case["name"], name, "rows that are not finite", int((~np.isfinite(rows).all(1)).sum())))

    def worst(name, err, tol, extra=""):
        w, over = fc.rows_over(err, tol)           # (a NaN row counts as over)
        print(f"{label} {case['name']:>11s} {name:8s} worst row {w:5d} err {err[w]:.3e} (tol {tol:.3e}) rows over {over}{extra}")
        if over:
            missed.append((label, case["name"], name, w, float(err[w]), over))

    worst("normals", np.abs(nrm.astype(np.float64) - ref["normals"]).max(1), fc.TOL_NORMAL)
    few = ref["cnt_normal"] < 3
    if not np.array_equal(nrm[few], np.tile(np.float32([0, 0, 1]), (int(few.sum()), 1))):
        missed.append((label, case["name"], "normals of rows with k < 3 are not (0, 0, 1)"))
    ef, eg = oracle_given_normals(case, np.ascontiguousarray(nrm))
    worst("fpfh", np.abs(fpfh.astype(np.float64) - ef).max(1), fc.TOL_FPFH)
    if fpfh[ref["cnt_feature"] <= 1].any():
        missed.append((label, case["name"], "FPFH of rows with k <= 1 is not zero"))
    if grad is not None:
        scale = max(1.0, float(np.abs(eg).max()))
        worst("gradient", np.abs(grad.astype(np.float64) - eg).max(1), fc.TOL_GRAD * scale, f" max|g| {np.abs(eg).max():.3e}")
        if grad[ref["cnt_grad"] < 4].any():
            missed.append((label, case["name"], "gradients of rows with k < 4 are not zero"))
    return missed


def compare_run(label, cases, out):
    missed = []
    for case, o in zip(cases, out):
        missed += compare_rows(label + "/normals_fpfh_batch     ", case, *o["a"])
        missed += compare_rows(label + "/instance_features_batch", case, *o["b"])
    return missed


def test_radius_outlier_bit_exact(ctx):
    from ibloc_amd.registration import CloudBatch, radius_outlier_batch
    cs = clouds([3000, 1, 0, 2500, 700], 3)
    rng = np.random.default_rng(0)
    cs[0] = np.concatenate([cs[0], rng.uniform(-3, 3, size=(40, 3)).astype(np.float32)])     # sprinkle outliers
    b = CloudBatch.from_numpy(cs)
    keep = radius_outlier_batch(ctx, b, 0.05, 8).cpu().numpy().astype(bool)
    off = b.seg_off_host
    for i, c in enumerate(cs):
        exp = ro.radius_outlier(c, 0.05, 8) if len(c) else np.zeros(0, bool)
        assert np.array_equal(keep[off[i]:off[i + 1]], exp), f"cloud {i}"
    assert keep.sum() > 0 and (~keep).sum() >= 30


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_every_row_of_every_cloud_equals_the_oracle(ctx, switch):
    """all clouds of tests/feature_cases.py in one batch, through both calls, under one switch"""
    cases = fc.all_cases()
    out, status = run_calls(ctx, cases, **SWITCHES[switch])
    missed = compare_run(switch, cases, out)
    assert not missed, missed
    assert status & ~fc.ST_KNN_SLOWPATH == 0 and status & fc.ST_KNN_SLOWPATH          # (the batch holds `boundary`)


def test_radius_outlier_mask_of_every_cloud_equals_the_oracle(ctx):
    from ibloc_amd.registration import CloudBatch, radius_outlier_batch
    cases = fc.all_cases()
    b = CloudBatch.from_numpy([c["pts"] for c in cases])
    keep = radius_outlier_batch(ctx, b, *fc.OUTLIER).cpu().numpy().astype(bool)
    off = b.seg_off_host
    for i, c in enumerate(cases):
        exp = fc.reference(c)["keep"]
        got = keep[off[i]:off[i + 1]]
        print(f"{c['name']:>11s}: kept {int(got.sum())} of {len(got)}, oracle {int(exp.sum())}, rows that differ {int((got != exp).sum())}")
        assert np.array_equal(got, exp), c["name"]
    kept = {c["name"]: int(fc.reference(c)["keep"].sum()) for c in cases}
    assert 0 < kept["clump"] < len(fc.clump()["pts"]) and kept["one"] == 0 and kept["duplicates"] == 50


def knn_records(ctx, capfd, case, **switches):
    """the case ALONE through both calls with knn_debug=1 -> (device rows, status, one record per tile search in call order)"""
    capfd.readouterr()
    out, status = run_calls(ctx, [case], knn_debug=1, **switches)
    recs = fc.parse_knn_debug(capfd.readouterr().err)
    for r in recs:
        print(f"{case['name']} {switches or 'default'}: {r}")
    # default: the fused feature search (twice) and the gradient search; feat_unfused: normals + SPFH (twice) and the gradient search
    expect = [(100, 2), (100, 2), (30, 4)] if not switches.get("feat_unfused") else [(30, 4), (100, 2), (30, 4), (100, 2), (30, 4)]
    assert [(r["k"], r["ts"]) for r in recs] == expect
    assert all(r["queries"] == len(case["pts"]) for r in recs)
    return out, status, recs


@pytest.mark.parametrize("switch", ["default", "feat_unfused"])
def test_uniform_alone_is_answered_from_the_staged_cubes(ctx, capfd, switch):
    case = fc.uniform()
    out, status, recs = knn_records(ctx, capfd, case, **SWITCHES[switch])
    assert [r["fallback"] for r in recs] == [0] * len(recs)
    assert status == 0
    missed = compare_run(switch, [case], out)
    assert not missed, missed


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_clump_alone_its_tile_does_not_stage(ctx, capfd, switch):
    case = fc.clump()
    out, status, recs = knn_records(ctx, capfd, case, **SWITCHES[switch])
    for r in recs:
        if r["k"] == 100:
            assert fc.CLUMP_N <= r["fallback"] <= r["queries"], r
        else:
            assert 0 < r["fallback"] < r["queries"], r
    assert status & ~fc.ST_KNN_SLOWPATH == 0          # (a query inside the clump has hundreds of candidates in its first d2 bin: bit 1 is set)
    missed = compare_run(switch, [case], out)
    assert not missed, missed


@pytest.mark.parametrize("switch", ["default", "feat_unfused"])
def test_sparse_alone_queries_beyond_their_cubes_cover_join_the_fallback(ctx, capfd, switch):
    case = fc.sparse()
    out, status, recs = knn_records(ctx, capfd, case, **SWITCHES[switch])
    for r in recs:
        assert 0 < r["fallback"] <= 2 * fc.SPARSE_HALO, r          # (the isolated points, and a few of the plane's next to them)
    assert status == 0
    missed = compare_run(switch, [case], out)
    assert not missed, missed


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_boundary_alone_takes_the_slow_path_and_flags_it(ctx, capfd, switch):
    case = fc.boundary()
    ctx.status(clear=True)
    out, status, recs = knn_records(ctx, capfd, case, **SWITCHES[switch])
    assert status == fc.ST_KNN_SLOWPATH
    assert ctx.status(clear=False) == 0                                        # run_calls read it with clear=True
    assert all(r["fallback"] >= 1 for r in recs)                               # (the centre at least)
    missed = compare_run(switch, [case], out)
    assert not missed, missed


def test_normals_and_fpfh_vs_oracle(ctx):
    """objects of 4 000, 2 500, 3, 0 and 1 500 points and a concatenation of two objects, like a length-2 assignment (neighbourhoods may
    span both): every row of both calls against the oracle"""
    cs = clouds([4000, 2500, 3, 0, 1500], 5)
    cs.append(np.concatenate([cs[0][:1500] + np.float32([0.4, 0, 0]), cs[1][:1500]]))
    cases = [fc.make_case("object%d" % i, c, "object cloud", 40 + i) for i, c in enumerate(cs)]
    out, status = run_calls(ctx, cases)
    assert status == 0
    missed = compare_run("objects", cases, out)
    assert not missed, missed


def test_knn_slow_path_matches_fast_path(ctx):
    """many equidistant candidates (points on a sphere around the query) overflow the 256-entry boundary list: the slow path is TAKEN
    (status bit 1; the cloud this test had before kept 500 interior points, more than either k, and never reached the sphere) and every
    row equals the oracle, under the one-pass and under the two-pass selection"""
    case = fc.boundary()
    ctx.status(clear=True)
    for switch in ("default", "knn_noguess"):
        out, status = run_calls(ctx, [case], **SWITCHES[switch])
        assert status == fc.ST_KNN_SLOWPATH
        missed = compare_run(switch, [case], out)
        assert not missed, missed


def test_fused_normals_and_feature_search_equals_the_two_searches(ctx):
    """instance features take the normals' <= 30 neighbours from the 100-neighbour list of the feature search (one search instead of two);
    the switch feat_unfused runs the two stand-alone searches: normals and FPFH must agree bit for bit, dense and sparse clouds alike"""
    from ibloc_amd.registration import CloudBatch, instance_features_batch, normals_fpfh_batch
    rng = np.random.default_rng(77)
    cs = clouds([5000, 1200, 40, 3, 0], 9)
    cs.append((rng.uniform(-0.05, 0.05, size=(3000, 3))).astype(np.float32))          # > 100 points inside every normal radius
    b = CloudBatch.from_numpy(cs)
    got = instance_features_batch(ctx, b, 0.05)
    n1, f1 = normals_fpfh_batch(ctx, b, 0.1, 30, 0.25, 100)
    with ctx.diag(feat_unfused=1):
        ref = instance_features_batch(ctx, b, 0.05)
        n2, f2 = normals_fpfh_batch(ctx, b, 0.1, 30, 0.25, 100)
    torch.cuda.synchronize()
    assert ctx.status() == 0
    assert torch.equal(got.normals[:b.n], ref.normals[:b.n]) and torch.equal(got.fpfh[:b.n], ref.fpfh[:b.n])
    assert torch.equal(n1, n2) and torch.equal(f1, f2)


def test_spfh_fp32_bins_with_fp64_for_undecided_pairs_equal_the_fp64_bins(ctx):
    """round 4: the SPFH bins of a pair come from fp32 arithmetic when every decision clears a guard band (pair_bins_f32, csrc/reg_fpfh.hip)
    and from the fp64 pair features otherwise (queue + second kernel).  the switch spfh_f64 evaluates every pair in fp64; spfh_qcap=8
    overflows the queue, which the gated fp64 launch repairs: all three must give the same bytes -- noisy surfaces, exact planes (equal
    normals, theta on a bin boundary for every pair), a cloud 200 m from the origin, tiny and empty clouds"""
    from ibloc_amd.registration import CloudBatch, instance_features_batch
    rng = np.random.default_rng(79)
    cs = clouds([6000, 3000, 1200, 40, 3, 0], 13)
    g = np.stack(np.meshgrid(np.arange(60), np.arange(60), indexing="ij"), -1).reshape(-1, 2) * 0.011
    cs.append(np.concatenate([g, np.zeros((len(g), 1))], 1).astype(np.float32))                           # an exact plane on a lattice
    cs.append((np.concatenate([g, 0.002 * rng.normal(size=(len(g), 1))], 1) + [211.5, -187.25, 3.0]).astype(np.float32))
    cs.append((rng.uniform(-0.05, 0.05, size=(3000, 3))).astype(np.float32))
    box = rng.uniform(-0.2, 0.2, size=(6000, 3))
    box[np.arange(6000), rng.integers(0, 3, 6000)] = rng.choice([-0.2, 0.2], 6000)                        # the six faces of a cube
    cs.append(box.astype(np.float32))
    b = CloudBatch.from_numpy(cs)
    got = instance_features_batch(ctx, b, 0.05)
    with ctx.diag(spfh_f64=1):
        ref = instance_features_batch(ctx, b, 0.05)
    with ctx.diag(spfh_qcap=8):
        over = instance_features_batch(ctx, b, 0.05)
    torch.cuda.synchronize()
    assert ctx.status() == 0
    assert float(ref.fpfh[:b.n].abs().sum()) > 0
    assert torch.equal(got.fpfh[:b.n], ref.fpfh[:b.n]) and torch.equal(got.normals[:b.n], ref.normals[:b.n])
    assert torch.equal(over.fpfh[:b.n], ref.fpfh[:b.n])


def test_guess_threshold_selection_equals_the_two_pass_selection(ctx):
    """round 3: the tile search collects the candidates below a GUESS of the k-th neighbour's distance in one pass and selects from that
    list (tile_select_guess); the switch knn_noguess runs the two-pass histogram selection for every query: neighbour sets, normals, FPFH
    and colour gradients must agree bit for bit -- dense, sparse, tiny and two-object clouds alike"""
    from ibloc_amd.registration import CloudBatch, instance_features_batch, normals_fpfh_batch
    rng = np.random.default_rng(78)
    cs = clouds([5000, 3000, 1200, 40, 3, 0], 11)
    cs.append((rng.uniform(-0.05, 0.05, size=(3000, 3))).astype(np.float32))          # > 100 points inside every normal radius
    cs.append(np.concatenate([cs[0][:2000] + np.float32([0.3, 0, 0]), cs[1][:2000]]))
    ints = [rng.uniform(0, 1, size=len(c)).astype(np.float32) for c in cs]
    b = CloudBatch.from_numpy(cs, ints)
    got = instance_features_batch(ctx, b, 0.05, grad_radius=0.15)
    n1, f1 = normals_fpfh_batch(ctx, b, 0.1, 30, 0.25, 100)
    with ctx.diag(knn_noguess=1):
        ref = instance_features_batch(ctx, b, 0.05, grad_radius=0.15)
        n2, f2 = normals_fpfh_batch(ctx, b, 0.1, 30, 0.25, 100)
    torch.cuda.synchronize()
    assert ctx.status() == 0
    assert torch.equal(got.normals[:b.n], ref.normals[:b.n]) and torch.equal(got.fpfh[:b.n], ref.fpfh[:b.n])
    assert torch.equal(got.grad[:b.n], ref.grad[:b.n]) and torch.equal(got.fpfh_split[:b.n], ref.fpfh_split[:b.n])
    assert torch.equal(n1, n2) and torch.equal(f1, f2)
