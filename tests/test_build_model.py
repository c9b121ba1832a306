"""(CPU) the cases of tests/build_cases.py contain what they are named for, shown with the oracle and with the grid builder's fp32
arithmetic restated in numpy -- so that a green tests/test_gpu_build_edges.py means the kernels were held to these decisions."""
import numpy as np

from oracle import build_oracle as bo
from tests import build_cases as bc

EPS = bc.EPS


def neighbour_counts(P, eps):
    return np.array([len(v) for v in bo.radius_neighbours(P, eps)])


def test_lattice_pairs_sit_at_exactly_eps_and_one_ulp_decides():
    at, above7, above8 = bc.lattice_at_eps("at"), bc.lattice_at_eps("above7"), bc.lattice_at_eps("above8")
    for gi, P in enumerate(at["groups"]):
        inner = at["info"]["inner"][gi]
        L = P[inner >= 0]
        d2 = bc.oracle_sum_d2(L[:, None, :], L[None, :, :])
        assert (d2 == EPS * EPS).sum() == 2 * 3 * 5 * 36                # every axis-neighbour pair, in the oracle's summation order
        assert ((d2 > 0) & (d2 < bc.EPS_UP * bc.EPS_UP) & (d2 != EPS * EPS)).sum() == 0
        assert (neighbour_counts(P, EPS) == 1).all()                    # at eps = EPS nobody has a neighbour
        cnt = neighbour_counts(P, bc.EPS_UP)
        assert np.array_equal(cnt[inner >= 0], 1 + 3 + inner[inner >= 0]) and cnt[inner < 0] == 1
        # the lattice straddles cell planes of its group: the anchor is the minimum, the lattice starts 8 / 8.5 cells in
        mn, inv, n = bc.seg_dims32(P, EPS)
        cells = bc.cells32(L, mn, inv, n)
        assert np.array_equal(mn.astype(np.float64), P[inner < 0][0]) and cells.min() == 8 and cells.max() == 13
        frac = (L - P[inner < 0][0]) / EPS % 1.0
        assert (frac == (0.0 if gi == 0 else 0.5)).all()                # on the planes / mid-cell
    for name, case, labelled, core in (("lattice_at_eps", at, 0, 0), ("lattice_above_eps_min7", above7, 160, 64),
                                       ("lattice_above_eps_min8", above8, 0, 0)):
        for gi, lab in enumerate(bc.dbscan_expected(name)):
            inner = case["info"]["inner"][gi]
            assert (lab >= 0).sum() == labelled and lab.max() == (0 if labelled else -1)
            if labelled:
                assert np.array_equal(lab >= 0, inner >= 2)             # 64 interior (core) + 96 face-interior (border) points
                assert (neighbour_counts(case["groups"][gi], case["eps"]) >= case["min_points"]).sum() == core


def test_border_point_lies_between_two_clusters_in_the_stated_orders():
    for variant in ("a_first", "b_first", "diagonal"):
        case = bc.border_between_two(variant)
        P, info = case["groups"][0], case["info"]
        x, a, b = info["x"], info["a"], info["b"]
        nbs = bo.radius_neighbours(P, EPS)
        core = np.array([len(v) >= 8 for v in nbs])
        assert core[a].all() and core[b].all() and not core[x] and len(nbs[x]) < 8
        na, nb_ = np.intersect1d(nbs[x], a), np.intersect1d(nbs[x], b)
        assert len(na) >= 1 and len(nb_) >= 1                           # core neighbours in both clusters
        assert bc.oracle_sum_d2(P[a][:, None], P[b][None]).min() >= EPS * EPS        # the clusters themselves are not linked
        lab = bc.dbscan_expected("border_between_two_" + variant)[0]
        assert lab.max() == 1 and len(set(lab[a])) == 1 and len(set(lab[b])) == 1 and lab[a][0] != lab[b][0]
        mn, inv, n = bc.seg_dims32(P, EPS)
        assert inv == 1.0 / EPS                                         # not widened: cell = eps, planes on the integer units
        cell = bc.cells32(P, mn, inv, n)
        cid = (cell[:, 2] * n[1] + cell[:, 1]) * n[0] + cell[:, 0]
        if variant == "a_first":
            assert a.max() < b.min() < x and lab[a][0] == 0 and lab[x] == 0 and cid[a].min() < cid[b].min()
        elif variant == "b_first":
            assert x < b.max() < a.min() and lab[b][0] == 0 and lab[x] == 0
            assert cid[a].min() < cid[b].min() and cid[a].max() < cid[b].max()       # A first in cell order, B first in numbering
        else:
            assert lab[a][0] == 0 and lab[x] == 0 and cid[b].max() < cid[a].min()    # B wholly before A in cell order, A numbered first
            assert len(na) == 1 and len(nb_) == 1
            assert cell[na[0], 1] != cell[x, 1] and cell[na[0], 2] != cell[x, 2]     # another cell row in y and in z
        # taking the highest instead of the lowest cluster would change X's label
        assert {int(lab[na[0]]), int(lab[nb_[0]])} == {0, 1}


def test_snake_is_two_clusters_then_one_and_its_gap_straddles_a_widened_cell():
    opened, closed = bc.snake("open"), bc.snake("closed")
    P, Q = opened["groups"][0], closed["groups"][0]
    g0, g1 = opened["info"]["g0"], opened["info"]["g1"]
    assert len(P) == 8000 and (g0, g1) == (closed["info"]["g0"], closed["info"]["g1"])
    assert bc.oracle_sum_d2(P[g0], P[g1]) == EPS * EPS and P[g1, 0] - P[g0, 0] == EPS
    assert 0 < bc.oracle_sum_d2(Q[g0], Q[g1]) < EPS * EPS and Q[g1, 0] == np.nextafter(P[g1, 0], -1.0)
    assert (np.delete(P, g1, axis=0) == np.delete(Q, g1, axis=0)).all()
    assert not np.array_equal(P, P[np.lexsort(P.T[::-1])])              # shuffled
    mn, inv, n = bc.seg_dims32(P, EPS)
    assert np.ptp(P[:, 0]) > 200 * EPS and inv < 1.0 / EPS and n[0] == 129          # widened cells
    c = bc.cells32(P[[g0, g1]], mn, inv, n)
    assert c[0, 0] != c[1, 0] and (c[0, 1:] == c[1, 1:]).all()
    cnt = neighbour_counts(P, EPS)
    assert cnt[g0] == 2 and cnt[g1] == 2 and np.isin(cnt, (2, 3, 4)).all() and (cnt == 3).sum() > 7800    # exactly min_points nearly everywhere
    assert ((bc.oracle_sum_d2(Q[[g0, g1]][:, None], Q[None]) < EPS * EPS).sum(1) == 3).all()
    lab_open, lab_closed = bc.dbscan_expected("snake_open")[0], bc.dbscan_expected("snake_closed")[0]
    assert lab_open.min() == 0 and lab_open.max() == 1 and lab_open[g0] != lab_open[g1]
    assert min((lab_open == 0).sum(), (lab_open == 1).sum()) > 3000
    assert lab_closed.min() == 0 and lab_closed.max() == 0


def test_many_groups_take_a_second_round_and_do_not_see_each_other():
    case = bc.many_groups()
    groups, info = case["groups"], case["info"]
    sizes = [len(g) for g in groups]
    assert len(groups) >= 300 and len(groups) > 256                     # more than one round of the dims kernel
    assert sizes[:3] == [0, 0, 0] and sizes[-4:] == [0] * 4 and sizes[150:155] == [0] * 5
    assert all(sizes[g] == n for n, g in info["sizes"].items())
    assert any(n > 0 for n in sizes[256:])                              # occupied groups in the second round
    for g in info["duplicates"]:
        assert (groups[g] == groups[g][0]).all()
    a, b = info["twice"]
    assert np.array_equal(groups[a], groups[b]) and abs(a - b) > 1
    assert sum(bc.cell_counts(groups, EPS)) < bc.DBSCAN_BUDGET
    want = bc.dbscan_expected("many_groups")
    assert np.array_equal(want[a], want[b]) and want[a].max() >= 0
    assert want[info["duplicates"][0]].tolist() == [0] * 12 and want[info["duplicates"][1]].tolist() == [-1] * 3
    for g, h in info["pairs"]:
        d2 = bc.oracle_sum_d2(groups[g][:, None], groups[h][None])
        assert (d2.min(1) < EPS * EPS).all() and (d2.min(0) < EPS * EPS).all()       # every point has a point of the other group within eps
        assert (want[g] == -1).all() and (want[h] == -1).all()          # alone each is noise ...
        both = bo.cluster_dbscan(np.concatenate([groups[g], groups[h]]), EPS, case["min_points"])
        assert (both >= 0).all()                                        # ... together they would be clustered
    kinds = np.concatenate([np.sign(w + 1) for w in want])
    assert 0.1 < kinds.mean() < 0.9                                     # a real mix of noise and labelled points
    exact = sum(int((bc.oracle_sum_d2(g[:, None], g[None]) == EPS * EPS).sum()) for g in groups if len(g))
    assert exact > 500                                                  # and many pairs at exactly eps


def test_far_from_origin_collapses_in_fp32_only():
    case = bc.far_from_origin()
    P = case["groups"][0]
    assert len(np.unique(P, axis=0)) == len(P)
    assert len(P) - len(np.unique(P.astype(np.float32), axis=0)) >= 10
    assert np.abs(P).min() > 4000
    lab = bc.dbscan_expected("far_from_origin")[0]
    assert lab.max() >= 3 and (lab == -1).sum() > 50


def test_budget_cases_fill_and_exceed_the_cell_budget():
    exceeded, filled = bc.budget_exceeded(), bc.budget_filled_exactly()
    cells = bc.cell_counts(exceeded["groups"], EPS)
    assert len(cells) == 40 and all(90 <= len(g) <= 110 for g in exceeded["groups"])
    for g in exceeded["groups"]:
        assert (np.ptp(g, axis=0) > 128 * EPS).all() and (bc.seg_dims32(g, EPS)[2] == 129).all()
    assert np.cumsum(cells)[30] <= bc.DBSCAN_BUDGET < np.cumsum(cells)[31]           # 31 fit, the rest collapse
    cells = bc.cell_counts(filled["groups"], EPS)
    assert len(cells) == 33 and len(filled["groups"][32]) == 1
    for g in filled["groups"][:32]:
        mn, inv, n = bc.seg_dims32(g, EPS)
        assert inv == 1.0 / EPS and (n == 128).all()
    assert sum(cells[:32]) == 64 << 20 == bc.DBSCAN_BUDGET and cells[32] == 1
    for name in ("budget_exceeded", "budget_filled_exactly"):
        want = bc.dbscan_expected(name)
        assert all(w.max() >= 2 for w in want if len(w) > 1)            # the lattices of every group are found, collapsed or not


def test_oracle_equals_sklearn_where_no_pair_sits_at_eps():
    """scikit-learn counts a distance == eps as a neighbour, the oracle (like Open3D) does not: only cases without such a pair"""
    from sklearn.cluster import DBSCAN
    for name in ("snake_closed", "far_from_origin"):
        case = bc.DBSCAN_CASES[name]()
        P = case["groups"][0]
        got = DBSCAN(eps=case["eps"], min_samples=case["min_points"], algorithm="brute").fit(P).labels_
        assert np.array_equal(got, bc.dbscan_expected(name)[0]), name
    chain = np.concatenate([bc.many_groups()["groups"][g] for g in bc.many_groups()["info"]["pairs"][0]])
    assert np.array_equal(DBSCAN(eps=EPS, min_samples=4, algorithm="brute").fit(chain).labels_, bo.cluster_dbscan(chain, EPS, 4))


# ---- voxel cases ------------------------------------------------------------------------------------------------------------------------
def vox_index(P, voxel):
    return np.floor(np.asarray(P, np.float64) / voxel).astype(np.int64)


def test_plane_points_are_on_the_planes():
    for voxel in (0.0625, 0.05):
        case = bc.on_the_planes(voxel)
        P = case["points"][0]
        k = np.rint(P / voxel)
        on = (k * voxel == P).all(1)
        assert on.sum() >= 600 and np.signbit(P).any() and (P == 0).any() and np.signbit(P[P == 0]).any()      # -0.0 among them
        assert len(case["points"][1]) == 0
        q = P / voxel
        if voxel == 0.0625:
            assert (q[on] == k[on]).all()                               # exact quotients
        else:
            assert (q[on] != k[on]).any()                               # quotients that round: floor sees k or k - 1
            assert (np.floor(q[on]) != k[on]).any()
        one_off = (~on) & (np.abs(P - k * voxel) < 1e-15).all(1)
        assert one_off.sum() >= 300                                     # the neighbours one ulp away
        third = case["points"][2]
        assert (np.rint(third[:, 2] / voxel) * voxel == third[:, 2]).all()


def test_crowded_voxel_holds_5000_points_and_its_mean_is_sequential():
    case = bc.crowded()
    o = case["info"]["obj"]
    P = case["points"][o]
    idx = vox_index(P, case["voxel"])
    uniq, counts = np.unique(idx, axis=0, return_counts=True)
    assert counts.max() == 5000 and np.sort(counts)[-2] < 50
    rows = P[(idx == uniq[counts.argmax()]).all(1)]
    seq = rows[0].copy()
    for r in rows[1:]:
        seq = seq + r
    wp, _, wn = bc.voxel_expected("crowded", False)[o]
    k = int(wn.argmax())
    assert wn[k] == 5000 and np.array_equal(wp[k], seq / 5000.0)       # the oracle's np.mean = the running sum, bit for bit
    pairwise = np.add.reduce(rows.reshape(8, 625, 3).sum(1)) / 5000.0   # a split sum is another number
    assert not np.array_equal(pairwise, wp[k])
    where = np.flatnonzero((idx == uniq[counts.argmax()]).all(1))
    assert where.min() < 10 and where.max() > len(P) - 10               # spread over the whole input


def test_interleaved_first_occurrence_is_reverse_key_order():
    case = bc.interleaved()
    P = case["points"][0]
    idx = vox_index(P, case["voxel"])
    rel = idx - idx.min(0)
    key = (rel[:, 0] << 32) | (rel[:, 1] << 16) | rel[:, 2]
    _, first = np.unique(key, return_index=True)                        # keys ascending -> index of first occurrence
    assert len(first) == 60 and np.array_equal(first, np.arange(60)[::-1])      # the first voxel has the largest key
    assert key[0] == key.max() and (np.bincount(np.unique(key, return_inverse=True)[1]) == 7).all()
    assert (np.diff(np.flatnonzero(key == key[0])) == 60).all()         # a voxel's points alternate with all the others


def test_many_objects_take_more_than_one_block_of_the_offsets_kernel():
    case = bc.many_objects()
    sizes = np.array([len(p) for p in case["points"]])
    assert len(sizes) >= 700 and sizes.max() <= 40 and (sizes[:4] == 0).all() and (sizes[300:309] == 0).all() and (sizes[-5:] == 0).all()
    assert (sizes[256:] > 0).any() and (sizes[512:] > 0).any()


def test_span_limit_is_the_last_accepted_and_the_first_refused():
    ok = bc.span_limit(None)
    idx = vox_index(ok["points"][bc.SPAN_OBJECT], ok["voxel"])
    assert (np.ptp(idx, axis=0) == 65535).all()
    far = idx - idx.min(0)
    assert ((far == 65535).all(1)).sum() == 2                           # points whose three key fields are all full
    assert 0 < bc.SPAN_OBJECT < len(ok["points"]) - 1 and all(len(p) for p in ok["points"])
    for axis in range(3):
        bad = bc.span_limit(axis)
        span = np.ptp(vox_index(bad["points"][bc.SPAN_OBJECT], bad["voxel"]), axis=0)
        assert span[axis] == 65536 and (np.delete(span, axis) == 65535).all() and bad["refused"] == (bc.SPAN_OBJECT, axis)
        for o in (0, 1, 3, 4):
            assert (np.ptp(vox_index(bad["points"][o], bad["voxel"]), axis=0) < 100).all()


def test_beyond_int32_indices_exceed_int32():
    case = bc.beyond_int32()
    for P in case["points"]:
        idx = vox_index(P, case["voxel"])
        assert (np.abs(idx).max(0) > 2 ** 31).any()
        assert len(np.unique(idx, axis=0)) > 100 and len(np.unique(P, axis=0)) == len(P)
    assert (np.abs(vox_index(case["points"][0], case["voxel"])) > 2 ** 31).all()
