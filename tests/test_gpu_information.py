"""-m gpu: the information matrix of a pose from its whole-memory correspondences (`ibl_information_kernel`, csrc/reg_eval.hip) through
`evaluate_information`, the engine and the facade, on the families of tests/evaluate_cases.py and the lattice family of
tests/information_cases.py (tests/test_information_model.py shows with the references alone what each is there for):

    per point   nn_out[:, 3] equals the d2 of `evaluate_points` bit for bit (+inf included); nn_out[:, :3] equals the expected
                coordinates bit for bit -- mem[idx] of the brute force on the tie-free families, the rule's choice (the
                lexicographically smallest of the memory points at the minimal fp32 d2) on slab_far and on the lattice; the pruned
                scan and eval_fullscan give the same bytes
    matrix      n_corr equals the brute force's count, n_corr / ns equals `evaluate_batch`'s fitness exactly, every entry lies within
                (n_corr + 4) 2^-53 A_ij of math.fsum over the same matched points (A_ij: the entry with every term replaced by its
                absolute value -- the terms are the device's own products, a sum of n doubles in any order errs by at most
                (n - 1) 2^-53 sum |t|, and an entry adds up to two such sums), about = None, the inlier centroid and, on slab_far,
                BASES["far"]; symmetric bit for bit; an empty job gives zeros
    determinism a second call gives the same bytes; a live grid built in two appends, with a range removed and put back, gives the
                bytes of the grid built at once (slab_far, where the ties are), and so does `evaluate_points` on it
    jobs        empty jobs first, in the middle and last and overlapping ranges (`jobs`); 65 539 jobs across the launch boundary
    refusals    null pointers, threshold <= 0, n_jobs <= 0, a descending range: IblError, outputs untouched
    engine      localise_batch(information=True) equals a direct call on the staged path's cleaned points, fused and staged alike
    facade      utils.fpfh_register.get_information_matrix
"""
import numpy as np
import pytest
import torch

from tests import evaluate_cases as ec
from tests import information_cases as ic

pytestmark = pytest.mark.gpu

NAMES = ic.TIE_FREE + [ic.DUPLICATES_ONLY, ic.TIE_FAMILY, "lattice_ties"]


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


def expected(fam, ref):
    return ic.lattice_expected(fam, ref)[0] if fam["name"] == "lattice_ties" else ic.expected_match(fam, ref)


def run(ctx, fam, grid, det4, full=False, about=None):
    from ibloc_amd.registration import evaluate_information
    with ctx.diag(eval_fullscan=1 if full else 0):
        info, n_corr, nn = evaluate_information(ctx, grid, det4, fam["jb"], fam["je"], fam["T"], fam["thr"], about=about, points=True)
    torch.cuda.synchronize()
    return info, n_corr, nn.cpu().numpy()


def check_matrix(fam, ref, exp, info, n_corr, about, what):
    """every job's matrix against fsum over the expected matched points; prints the worst ratio to the bound, then asserts"""
    worst = 0.0
    hit = np.isfinite(ref["d2"])
    for j, ns in enumerate(ref["ns"]):
        sl = slice(ref["off"][j], ref["off"][j + 1])
        m = exp[sl][hit[sl]]
        assert n_corr[j] == len(m), (what, j, fam["tags"][j], n_corr[j], len(m))
        assert info[j].tobytes() == info[j].T.copy().tobytes(), (what, j)
        if len(m) == 0:
            assert not info[j].any(), (what, j, fam["tags"][j])
            continue
        A, Aabs = ic.info_reference(m, about)
        gap = np.abs(info[j] - A)
        bound = ic.bound(len(m), Aabs)
        worst = max(worst, float((gap[bound > 0] / bound[bound > 0]).max()))
        assert (gap <= bound).all(), (what, j, fam["tags"][j], gap.max(), np.argwhere(gap > bound)[:3])
    print(f"{fam['name']} [{what}]: {len(ref['ns'])} jobs, {int(n_corr.sum())} correspondences, worst |info - fsum| / bound {worst:.3f}")


@pytest.mark.parametrize("name", NAMES)
def test_every_point_and_every_matrix(ctx, name):
    from ibloc_amd.registration import MemGrid, evaluate_batch, evaluate_points
    fam = ic.get(name)
    ref = ec.reference(fam)
    exp = expected(fam, ref)
    mem4, det4 = pts4(fam["mem"]), pts4(fam["det"])
    grid = MemGrid(ctx, mem4, fam["cell"])
    info, n_corr, nn = run(ctx, fam, grid, det4)
    d2, _, _ = evaluate_points(ctx, grid, det4, fam["jb"], fam["je"], fam["T"], fam["thr"])
    _, fit = evaluate_batch(ctx, grid, det4, fam["jb"], fam["je"], fam["T"], fam["thr"])
    d2 = d2.cpu().numpy()
    # ---- per point
    assert nn.shape == (len(ref["d2"]), 4)
    wrong_d = np.nonzero(bits(nn[:, 3]) != bits(d2))[0]
    wrong_m = np.nonzero((bits(nn[:, :3]) != bits(exp)).any(1))[0]
    print(f"{name}: {len(nn)} points, {int(np.isfinite(nn[:, 3]).sum())} matched, {len(wrong_d)} d2 differ from evaluate_points, "
          f"{len(wrong_m)} matched points differ from the expected")
    assert len(wrong_d) == 0, (wrong_d[:5], nn[wrong_d[:5]], d2[wrong_d[:5]])
    assert np.array_equal(bits(d2), bits(ref["d2"]))
    assert len(wrong_m) == 0, (wrong_m[:5], nn[wrong_m[:5]], exp[wrong_m[:5]], ref["q"][wrong_m[:5]])
    # ---- counts and matrix, about the origin
    ns = ref["ns"]
    for j in range(len(ns)):
        assert (n_corr[j] / ns[j] if ns[j] else 0.0) == fit[j], (j, fam["tags"][j])
    check_matrix(fam, ref, exp, info, n_corr, None, "origin")
    # ---- the full scan and a second call: the same bytes
    info_f, n_f, nn_f = run(ctx, fam, grid, det4, full=True)
    assert info_f.tobytes() == info.tobytes() and n_f.tobytes() == n_corr.tobytes() and nn_f.tobytes() == nn.tobytes()
    info_2, n_2, nn_2 = run(ctx, fam, grid, det4)
    assert info_2.tobytes() == info.tobytes() and n_2.tobytes() == n_corr.tobytes() and nn_2.tobytes() == nn.tobytes()
    # ---- about the inlier centroid (and about the far base where the scene is)
    hit = np.isfinite(ref["d2"])
    abouts = [("centroid", exp[hit].astype(np.float64).mean(0))] if hit.any() else []
    if name == ic.TIE_FAMILY:
        abouts.append(("far base", np.array(ec.BASES["far"])))
    for what, c in abouts:
        info_c, n_c, nn_c = run(ctx, fam, grid, det4, about=c)
        assert n_c.tobytes() == n_corr.tobytes() and nn_c.tobytes() == nn.tobytes()
        check_matrix(fam, ref, exp, info_c, n_c, c, what)
    grid.close()


def test_live_grid_after_edits_gives_the_bytes_of_a_fresh_grid(ctx):
    """slab_far (its ties are between distinct coordinates): a live grid built from the first 40 000 points, the rest appended, a
    range taken out and put back in its place -- the order inside the cells has been rebuilt three times.  The information matrix
    and the evaluation (`evaluate_points`: every d2, rmse and fitness) give the bytes of the grid built at once, pruned scan and
    eval_fullscan alike."""
    from ibloc_amd.registration import MemGrid, evaluate_points

    def evaluated(grid, full):
        with ctx.diag(eval_fullscan=1 if full else 0):
            d2, rmse, fit = evaluate_points(ctx, grid, det4, fam["jb"], fam["je"], fam["T"], fam["thr"])
        return d2.cpu().numpy().tobytes(), rmse.tobytes(), fit.tobytes()

    fam = ec.get(ic.TIE_FAMILY)
    mem4, det4 = pts4(fam["mem"]), pts4(fam["det"])
    fresh = MemGrid(ctx, mem4, fam["cell"])
    info, n_corr, nn = run(ctx, fam, fresh, det4)
    ev = evaluated(fresh, False)
    assert evaluated(fresh, True) == ev
    fresh.close()
    live = MemGrid(ctx, mem4[:40000].contiguous(), fam["cell"], live=True, reserve_points=30000)
    live.append(mem4[40000:].contiguous())
    live.remove([(10000, 25000)])
    assert live.info()["n"] == len(mem4) - 15000
    info_r, _, _ = run(ctx, fam, live, det4)
    assert info_r.tobytes() != info.tobytes()                       # (the removed points were matched by something)
    assert evaluated(live, False) != ev
    live.replace([(10000, 10000)], [15000], mem4[10000:25000].contiguous())
    assert live.info()["n"] == len(mem4)
    for full in (False, True):
        info_l, n_l, nn_l = run(ctx, fam, live, det4, full=full)
        assert info_l.tobytes() == info.tobytes() and n_l.tobytes() == n_corr.tobytes() and nn_l.tobytes() == nn.tobytes()
        assert evaluated(live, full) == ev
    live.close()


@pytest.mark.parametrize("scan", ["pruned", "full"])
def test_more_jobs_than_one_launch_holds(ctx, scan):
    """65 536 + 3 jobs of 7 patterns: the jobs of the second launch read their own ranges and transforms and write their own slots.
    Every job equals the first job of its pattern bit for bit, and that one the closed form of the pattern's matched points."""
    from ibloc_amd.registration import MemGrid
    fam = ec.many_jobs()
    ref = ec.reference(fam)
    tied, _ = ic.near_ties(fam, ref)
    assert len(tied) == 0
    exp = ic.expected_match(fam, ref)
    grid = MemGrid(ctx, pts4(fam["mem"]), fam["cell"])
    info, n_corr, nn = run(ctx, fam, grid, pts4(fam["det"]), full=scan == "full")
    grid.close()
    J = len(fam["jb"])
    assert J == ec.GRID_Y_MAX + 4 and info.shape == (J, 6, 6)
    assert np.array_equal(bits(nn[:, 3]), bits(ref["d2"])) and np.array_equal(bits(nn[:, :3]), bits(exp))
    hit = np.isfinite(ref["d2"])
    for p in range(7):
        sl = slice(ref["off"][p], ref["off"][p + 1])
        m = exp[sl][hit[sl]]
        assert (n_corr[p::7] == len(m)).all()
        assert (info[p::7] == info[p]).all()
        if len(m):
            A, Aabs = ic.info_reference(m)
            assert (np.abs(info[p] - A) <= ic.bound(len(m), Aabs)).all() and (np.abs(ic.info_closed(m) - A) <= ic.bound(len(m), Aabs)).all()
        else:
            assert not info[p].any()
    assert len({info[j].tobytes() for j in range(ec.GRID_Y_MAX - 1, ec.GRID_Y_MAX + 3)}) == 4          # neighbours across the boundary differ


def test_refusals_leave_the_outputs_untouched(ctx):
    from ibloc_amd import _lib
    from ibloc_amd.registration import MemGrid, _stream
    fam = ec.get("occupancy_single")
    grid = MemGrid(ctx, pts4(fam["mem"]), fam["cell"])
    det4 = pts4(fam["det"])
    nn = torch.full((len(fam["det"]), 4), -7.0, device="cuda")
    jb, je = np.array([0, 10], np.int32), np.array([10, 30], np.int32)
    T = np.stack([np.eye(4), np.eye(4)]).reshape(2, 16)
    info, n_corr = np.full((2, 36), -7.0), np.full(2, -7, np.int64)
    good = dict(ctx=ctx.handle, grid=grid.handle, det=det4.data_ptr(), jb=jb.ctypes.data, je=je.ctypes.data, T=T.ctypes.data, J=2, thr=0.02,
                about=None, nn=nn.data_ptr(), info=info.ctypes.data, n=n_corr.ctypes.data)
    down = np.array([10, 5], np.int32)
    cases = [("null " + k, {k: None}) for k in ("ctx", "grid", "det", "jb", "je", "T", "info", "n")]
    cases += [("threshold 0", dict(thr=0.0)), ("threshold < 0", dict(thr=-0.02)), ("no jobs", dict(J=0)), ("n_jobs < 0", dict(J=-1)),
              ("descending range", dict(je=down.ctypes.data))]
    for what, change in cases:
        a = dict(good, **change)
        st = _lib.lib.ibl_evaluate_information(a["ctx"], a["grid"], a["det"], a["jb"], a["je"], a["T"], a["J"], a["thr"], a["about"], a["nn"],
                                               a["info"], a["n"], _stream())
        assert st < 0 and b"ibl_evaluate_information" in _lib.lib.ibl_last_error(), what
        with pytest.raises(_lib.IblError):
            _lib.check(st, what)
        torch.cuda.synchronize()
        assert (info == -7.0).all() and (n_corr == -7).all() and bool((nn == -7.0).all()), what
    # and the same arguments unchanged are accepted
    a = good
    st = _lib.lib.ibl_evaluate_information(a["ctx"], a["grid"], a["det"], a["jb"], a["je"], a["T"], a["J"], a["thr"], a["about"], a["nn"],
                                           a["info"], a["n"], _stream())
    assert st == 0 and (n_corr >= 0).all() and bool((nn[:30] != -7.0).any())
    grid.close()


def test_engine_information():
    """FrameResult.information / n_correspondences / inlier_centroid through the fused and the staged stage B against a direct call on
    the staged path's cleaned points and the best record's T_global"""
    from ibloc_amd.engine import LocaliseEngine, MemoryShard, intensity_from_colors
    from ibloc_amd.registration import CloudBatch, RegContext, evaluate_information, radius_outlier_batch
    from ibloc_amd.synth import SynthWorld
    w = SynthWorld(12, pts_per_object=2500, E=2, D=32, seed=61, spacing=1.6)
    rng = np.random.default_rng(63)
    frames = [w.make_frame(rng, q=q, pts_per_object=2500) for q in (3, 1, 2)]
    ectx = RegContext(6 << 30)
    mem = MemoryShard(ectx, list(w.embeddings), w.points, colors=w.colors)
    clouds = [c[0] for f in frames for c in f["clouds"]]
    clouds[0] = np.concatenate([clouds[0], np.random.default_rng(1).uniform(-3, 3, size=(50, 3))])      # stray points for the outlier removal
    ints = [intensity_from_colors(c[1]) for f in frames for c in f["clouds"]]
    ints[0] = np.concatenate([ints[0], np.zeros(50, np.float32)])
    det = CloudBatch.from_numpy(clouds, ints)
    emb = np.concatenate([f["det_emb"] for f in frames])
    qs = [len(f["ids"]) for f in frames]
    kw = dict(det_emb=emb, fpfh_voxel_size=0.05, fpfh_global_dist_factor=1.5, fpfh_local_dist_factor=1.5, seed=3, job_id_base=17)
    eng = LocaliseEngine(mem, None)
    plain = eng.localise_batch(det, qs, **kw)
    fused = eng.localise_batch(det, qs, information=True, **kw)
    eng.fused_stage_b = False
    staged = eng.localise_batch(det, qs, information=True, **kw)
    # the direct call: the staged path's cleaned points
    keepb = radius_outlier_batch(ectx, det, 0.05, 8).bool()
    clean = det.pts4[keepb].contiguous()
    off = np.concatenate([[0], np.cumsum(keepb.cpu().numpy())])[det.seg_off_host]
    row0 = np.concatenate([[0], np.cumsum(qs)])
    assert any(r.best >= 0 for r in fused)
    for f, (p, a, b) in enumerate(zip(plain, fused, staged)):
        assert p.information is None and p.n_correspondences is None and p.inlier_centroid is None
        assert p.assignments == a.assignments == b.assignments and p.best == a.best == b.best and p.n_clean == a.n_clean == b.n_clean
        assert np.array_equal(p.pose, a.pose) and np.array_equal(p.pose_corrected, a.pose_corrected) and np.array_equal(p.pose, b.pose)
        for x, y in zip(p.records, a.records):
            for k in ("T", "T_global", "full_rmse", "full_fitness", "rmse", "fitness"):
                assert np.array_equal(x[k], y[k]), k
        if a.best < 0:
            assert a.information is None and b.information is None
            continue
        rec = a.records[a.best]
        info, n_corr = evaluate_information(ectx, mem.grid, clean, [off[row0[f]]], [off[row0[f + 1]]], rec["T_global"][None], mem.eval_threshold)
        for r in (a, b):
            assert r.information.shape == (6, 6) and r.information.tobytes() == info[0].tobytes()
            assert r.n_correspondences == int(n_corr[0]) == round(rec["full_fitness"] * r.n_clean) and r.n_correspondences > 0
            c = np.array([info[0, 2, 4], info[0, 0, 5], info[0, 1, 3]]) / n_corr[0]
            assert r.inlier_centroid.tobytes() == c.tobytes()
    # sharded clouds are refused before any work (no second rank here: a stub transport stands for the routed engine)
    eng.route = object()
    with pytest.raises(ValueError, match="information: unsharded memories only"):
        eng.localise_batch(det, qs, information=True, **kw)
    eng.route = None
    ectx.close()


def test_facade_get_information_matrix():
    from ibloc_amd.utils import fpfh_register as fr
    from oracle import reg_oracle as ro
    rng = np.random.default_rng(5)
    tgt = rng.uniform(-0.5, 0.5, size=(3000, 3)).astype(np.float32)
    T = ec.rigid((0.3, -0.2, 0.4), (0.002, -0.001, 0.003))
    src = (np.linalg.inv(T) @ np.concatenate([tgt[:2000] + rng.normal(0, 0.003, size=(2000, 3)), np.ones((2000, 1))], 1).T).T[:, :3].astype(np.float32)
    info = fr.get_information_matrix(src.astype(np.float64), tgt.astype(np.float64), 0.02, T)
    d2, idx = ro.nearest_bruteforce(src, tgt, T, 0.02)
    m = tgt[idx[idx >= 0]]
    A, Aabs = ic.info_reference(m)
    assert info.shape == (6, 6) and info[3, 3] == len(m) > 1000
    assert (np.abs(info - A) <= ic.bound(len(m), Aabs)).all()
    same = fr.get_information_matrix(tgt.astype(np.float64), tgt.astype(np.float64), 0.02, np.eye(4))
    assert same[3, 3] == len(tgt)
    A, Aabs = ic.info_reference(tgt)
    assert (np.abs(same - A) <= ic.bound(len(tgt), Aabs)).all()
