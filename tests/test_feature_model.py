"""The clouds of tests/feature_cases.py under the two references alone (no GPU): oracle/oracle_reg.c -- the fp32 distance rule with
(d2, index) ties the device shares, solvers in double -- and oracle/open3d_fp64.py -- kd-tree, LAPACK, numpy, no shared code.  They
show that every cloud is what it claims to be, and that holding EVERY row of the device's normals, FPFH and gradients to the C oracle
(tests/test_gpu_features.py) is fair: where the two rules select the same neighbours the two references agree on every row, to the
rounding of the fp32 output.

Worst rows measured (same-set rows; normal error up to sign, smallest relative eigen-gap (l1 - l0) / l2; FPFH; gradient / max(1, max|g|)):
    uniform      3.0e-08  gap 8.3e-03   5.5e-06   2.9e-08
    clump        3.0e-08  gap 2.3e-03   1.1e-05   3.4e-08     (gradient with Cramer's rule in the oracle: 5.3e-04, 243 rows over 2.5e-5)
    sparse       3.0e-08  gap 7.2e-03   1.2e-05   3.0e-08
    boundary     3.0e-08  gap 4.6e-03   -         4.2e-08     (the centre's own set is decided by rounding: 1 row left out)
    lattice      0        gap 2.9e-01   -         3.0e-08     (ties by index: C oracle only; 813 of 1 600 sets differ from the kd-tree's)
    far          3.0e-08  gap 2.8e-01   1.1e-05   3.0e-08
    blob         3.0e-08  gap 2.5e-03   5.6e-06   2.9e-08
    two_objects  3.0e-08  gap 9.1e-03   5.3e-06   3.0e-08
    one .. forty 2.9e-08  gap 1.0e-01   5.9e-06   1.6e-08
"""
import numpy as np
import pytest

from oracle import open3d_fp64 as o3
from oracle import reg_oracle as ro
from tests import feature_cases as fc

MIN_GAP = 1e-6                      # relative eigen-gap below which a normal is not determined by its neighbours
TOL_GRAD_MODEL = fc.TOL_GRAD / 4    # a quarter of the GPU test's tolerance
SET_CAP = 0.01                      # share of rows whose fp32-rule set may differ from the kd-tree's on clouds with ties (a cap on the
                                    # rows LEFT OUT of a comparison, not a tolerance of one)

NAMED = [c for c in fc.all_cases() if len(c["pts"])]
IDS = [c["name"] for c in NAMED]
_sets = {}


def sets(case, search):
    """-> (same [n] bool: the fp32 rule and the kd-tree select the same neighbours, cnt32, idx64, cnt64) of one search of one case"""
    key = (case["name"], search)
    if key not in _sets:
        p = case["pts"]
        i32, c32 = ro.hybrid_sets(p, *search)
        i64, c64, _ = o3.hybrid_neighbours(p, *search)
        a = np.sort(np.where(i32 >= 0, i32, np.iinfo(np.int32).max), axis=1)
        b = np.sort(np.where(i64 >= 0, i64, np.iinfo(np.int32).max), axis=1)
        _sets[key] = ((c32 == c64) & (a == b).all(axis=1), c32, i64, c64)
    return _sets[key]


def check_set_cap(case, same):
    left_out = int((~same).sum())
    if case["name"] == "lattice" or case["degenerate"]:
        return left_out                                              # ties everywhere: these clouds are held to the C oracle only
    cap = 0 if case["random"] else int(SET_CAP * len(same))
    assert left_out <= cap, f"{case['name']}: {left_out} rows have another neighbour set under the kd-tree (cap {cap})"
    return left_out


@pytest.mark.parametrize("case", NAMED, ids=IDS)
def test_normals_of_both_references_agree_on_every_row_with_equal_sets(case):
    p = case["pts"]
    same, c32, i64, c64 = sets(case, fc.NORMAL)
    left_out = check_set_cap(case, same)
    en = ro.normals(p, *fc.NORMAL)
    n64, _, _ = o3.normals(p, *fc.NORMAL)
    assert np.isfinite(en).all() and np.abs(np.linalg.norm(en.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert np.array_equal(en[c32 < 3], np.tile(np.float32([0, 0, 1]), (int((c32 < 3).sum()), 1)))
    rows = np.nonzero(same & (c32 >= 3))[0]
    pd = p.astype(np.float64)
    gap = np.ones(len(p))
    for i in rows:
        nb = pd[i64[i, :c64[i]]]
        w = np.linalg.eigvalsh(np.cov(nb.T, bias=True))
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
    err = np.minimum(np.abs(en - n64).max(1), np.abs(en + n64).max(1))
    if case["degenerate"]:
        rows = rows[gap[rows] >= MIN_GAP]           # the declared exceptions: oracle-equal where the gap allows (nowhere on a line)
    worst = int(rows[np.argmax(err[rows])]) if len(rows) else -1
    print(f"{case['name']}: {len(rows)} rows compared, {left_out} left out; worst normal row {worst} err {err[worst] if worst >= 0 else 0:.3e}; "
          f"smallest eigen-gap {gap[rows].min() if len(rows) else float('nan'):.3e}")
    if not case["degenerate"]:
        assert gap[rows].min(initial=1.0) >= MIN_GAP, f"row {rows[np.argmin(gap[rows])]} has an undetermined normal"
    assert (err[rows] <= fc.TOL_NORMAL).all(), (worst, err[worst])


@pytest.mark.parametrize("case", NAMED, ids=IDS)
def test_fpfh_of_both_references_agrees_on_every_row_where_all_sets_agree(case):
    """the FPFH of a row reads the SPFH of its neighbours, so the comparison needs equal sets on the whole cloud; both sides get the C
    oracle's normals"""
    p = case["pts"]
    same, c32, _, _ = sets(case, fc.FEATURE)
    if not same.all():
        assert not case["random"], f"{case['name']}: {int((~same).sum())} feature sets differ on a cloud without ties"
        print(f"{case['name']}: {int((~same).sum())} feature sets differ (ties): held to the C oracle only")
        return
    en = ro.normals(p, *fc.NORMAL)
    ef = ro.fpfh(p, en, *fc.FEATURE)
    f64 = o3.fpfh(p, en, *fc.FEATURE)
    err = np.abs(ef - f64).max(1)
    worst = int(np.argmax(err))
    print(f"{case['name']}: worst FPFH row {worst} err {err[worst]:.3e} (k = {c32[worst]}); largest entry {ef.max():.1f}")
    assert not ef[c32 <= 1].any() and not f64[c32 <= 1].any()
    assert ef.max() <= 200.0 + fc.TOL_FPFH
    assert (err <= fc.TOL_FPFH).all(), (worst, err[worst])


@pytest.mark.parametrize("case", NAMED, ids=IDS)
def test_gradients_of_both_references_agree_on_every_row_with_equal_sets(case):
    """oracle_color_gradient (normal equations, LDL^T with diagonal pivoting) against the least-squares restatement.  With Cramer's rule
    in its place `clump` missed by 5.3e-4 x max|g| and 243 rows exceeded this tolerance."""
    p = case["pts"]
    same, c32, _, _ = sets(case, fc.GRAD)
    check_set_cap(case, same)
    en = ro.normals(p, *fc.NORMAL)
    eg = ro.color_gradient(p, en, case["intensity"], *fc.GRAD)
    assert np.isfinite(eg).all() and not eg[c32 < 4].any()
    if case["degenerate"]:
        assert not eg.any()                                           # exactly singular systems: zero, like a zero determinant was
        return
    g64 = o3.color_gradients(p, en, case["intensity"], *fc.GRAD)
    scale = max(1.0, float(np.abs(g64).max()))
    err = np.abs(eg - g64).max(1)
    rows = np.nonzero(same)[0]
    worst = int(rows[np.argmax(err[rows])])
    print(f"{case['name']}: max|g| {np.abs(g64).max():.3e}; worst gradient row {worst} err {err[worst]:.3e} = {err[worst] / scale:.3e} x scale")
    assert (err[rows] <= TOL_GRAD_MODEL * scale).all(), (worst, err[worst], scale)


def test_boundary_centre_overflows_its_boundary_bin_in_every_search():
    b = fc.boundary()
    assert fc.BOUNDARY_INNER + 1 < min(fc.NORMAL[1], fc.GRAD[1], fc.FEATURE[1])            # fewer interior points than k
    for search in (fc.NORMAL, fc.FEATURE, fc.GRAD):
        pop, below = fc.boundary_bin_population(b["pts"], 0, *search)
        print(f"boundary centre, r = {search[0]} k = {search[1]}: {pop} candidates in the k-th neighbour's bin, {below} below it")
        assert below == fc.BOUNDARY_INNER + 1 and pop > fc.KNN_CAPB
        assert pop == fc.BOUNDARY_SPHERE                             # (the whole sphere in one bin: no share of it on a bin edge)


def test_clump_has_rows_of_every_short_count_and_outnumbers_the_candidate_caps():
    c = fc.clump()
    ref = fc.reference(c)
    kn, kf, kg = ref["cnt_normal"], ref["cnt_feature"], ref["cnt_grad"]
    counts = dict(normal_lt3=int((kn < 3).sum()), normal_lt30=int((kn < fc.NORMAL[1]).sum()), feature_le1=int((kf <= 1).sum()),
                  feature_lt100=int((kf < fc.FEATURE[1]).sum()), grad_lt4=int((kg < 4).sum()), grad_lt30=int((kg < fc.GRAD[1]).sum()))
    print("clump:", counts)
    assert counts == dict(normal_lt3=47, normal_lt30=495, feature_le1=1, feature_lt100=140, grad_lt4=41, grad_lt30=62)
    dense = fc.clump_is_dense(c)
    assert fc.CLUMP_N <= dense.sum() <= fc.CLUMP_N + 20
    # the clump is 2 000 points within 12 cm, more than either candidate cap (1 600 packed, 1 024 unpacked), while the cells are sized from
    # the plane's mean density (ibl_build_tile_grid: about 4 cm for k = 30, 7.5 cm for k = 100); what the device's grid makes of it is
    # observed in tests/test_gpu_features.py
    ext = c["pts"][dense].max(0) - c["pts"][dense].min(0)
    assert ext.max() < 0.12 and dense.sum() > 1600


def test_uniform_blob_and_tiny_clouds_are_what_they_claim():
    ref = fc.reference(fc.blob())
    assert (ref["cnt_normal"] == fc.NORMAL[1]).all() and (ro.hybrid_sets(fc.blob()["pts"], fc.NORMAL[0], 101)[1] > 100).all()
    sizes = [len(c["pts"]) for c in fc.tiny()]
    assert sizes == [0, 1, 2, 3, 40, 50, 200]
    assert max(len(c["pts"]) for c in fc.all_cases()) <= 3100 and sum(len(c["pts"]) for c in fc.all_cases()) <= 16000
    for c in fc.all_cases():
        assert c["pts"].dtype == np.float32 and c["intensity"].dtype == np.float32 and len(c["intensity"]) == len(c["pts"])


def test_a_row_that_is_not_a_number_counts_as_a_row_over_the_tolerance():
    assert fc.rows_over([0.0, 1e-9, 0.0], 1e-6) == (1, 0)
    assert fc.rows_over([0.0, 2e-6, 1e-5], 1e-6) == (2, 2)
    assert fc.rows_over([0.0, np.nan, 1e-5, np.inf], 1e-6) == (1, 3)


def test_knn_debug_lines_are_parsed_one_record_per_search():
    text = ("noise\n[knn] r=0.100 k=30 ts=4 tiles=12 queries=1500 fallback=0 (0.0 %)\nother\n"
            "[knn] r=0.250 k=100 ts=2 tiles=7 queries=3060 fallback=2011 (65.7 %)\n")
    assert fc.parse_knn_debug(text) == [dict(r=0.1, k=30, ts=4, tiles=12, queries=1500, fallback=0),
                                        dict(r=0.25, k=100, ts=2, tiles=7, queries=3060, fallback=2011)]
    assert fc.parse_knn_debug("") == []
