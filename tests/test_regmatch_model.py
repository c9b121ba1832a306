"""CPU: the job sets of tests/regmatch_cases.py are what they claim, shown with numpy and the oracle alone -- so that a later edit of a
case cannot quietly stop exercising the path it exists for -- and the two restatements the GPU tests lean on (the fp32 fmaf chain of the
operand builder, the Philox draw) agree with the oracle's C."""
import numpy as np
import pytest

from tests import regmatch_cases as rc
from oracle import reg_oracle as ro


def runs(name):
    fam = rc.FAMILIES[name]()
    return fam, [rc.expected(fam, j) for j in range(len(fam["js"]))]


@pytest.mark.parametrize("name", sorted(rc.FAMILIES))
def test_rows_are_in_the_domain_and_every_distance_and_norm_is_exact_in_fp32(name):
    fam = rc.FAMILIES[name]()
    d2, n = rc.exactness(fam)
    print(name, "largest squared distance", d2, "largest centred norm", n)
    assert 0 < d2 < 2 ** 24 and 0 < n < 2 ** 24
    # the geometry is trivial: two points of a cloud are further apart than twice the correspondence distance, instances of a side
    # further than the influence radius (0.6 m) -- every row is served from the injected features
    for clouds in (fam["det"], fam["mem"]):
        for c in clouds:
            if len(c) > 1:
                d = np.sqrt(((c[:, None].astype(np.float64) - c[None]) ** 2).sum(-1)) + 10.0 * np.eye(len(c))
                assert d.min() > 2 * rc.MAX_DIST
    for pool, table in ((fam["det"], fam["js"]), (fam["mem"], fam["jt"])):
        for seg in table:
            ids = [s for s in seg if s >= 0 and len(pool[s])]
            for a in ids:
                for b in ids:
                    if a < b:
                        gap = np.maximum(np.maximum(pool[a].min(0) - pool[b].max(0), pool[b].min(0) - pool[a].max(0)), 0.0)
                        assert np.linalg.norm(gap) > 1.0


def test_the_oracles_matching_is_the_first_minimum_of_the_exact_distances():
    """numpy on the exact fp64 distances (what lays out the geometry, `instance_pair`) and the oracle's fp32 chain choose the same rows"""
    for name in sorted(rc.FAMILIES):
        fam = rc.FAMILIES[name]()
        for j in range(len(fam["js"])):
            fs, ft = rc.job_rows(fam, j)
            if len(fs) == 0 or len(ft) == 0:
                continue
            ij, ji = rc.first_nearest(fs, ft), rc.first_nearest(ft, fs)
            keep = np.flatnonzero(ji[ij] == np.arange(len(fs)))
            want = np.stack([keep, ij[keep]], 1) if len(keep) >= 9 else np.stack([np.arange(len(fs)), ij], 1)
            assert np.array_equal(rc.expected(fam, j)[0], want), (name, fam["tags"][j])


def test_sizes_cover_tiles_chunks_and_short_databases():
    fam, res = runs("sizes")
    got = sorted((len(rc.job_rows(fam, j)[0]), len(rc.job_rows(fam, j)[1])) for j in range(len(res)))
    assert got == sorted((a, b) for a in rc.SIZES for b in rc.SIZES)
    assert {1, 31, 32, 33, 255, 256, 257}.issubset(rc.SIZES) and max(rc.SIZES) > 2 * 256
    n_corr = np.array([len(r[0]) for r in res])
    print("n_corr", n_corr.reshape(8, 8))
    # the rows compete: in the equal-size jobs most, but not all, sources keep their own partner
    for k, n in enumerate(rc.SIZES[4:], 4):
        c = res[9 * k][0]
        assert 0.7 * n < len(c) < n and (c[:, 0] == c[:, 1]).mean() > 0.9


def test_ties_exist_where_claimed_and_the_lowest_index_wins():
    fam, res = runs("ties")
    tag = {t: j for j, t in enumerate(fam["tags"])}
    # duplicated database rows: the tied sources choose the first copy
    j = tag["duplicated database rows"]
    fs, ft = rc.job_rows(fam, j)
    exact, band = rc.tie_counts(fs, ft)
    assert exact[3] == 2 and exact[30] == 2 and exact[20] == 3
    c = dict(res[j][0].tolist())
    assert (c[3], c[30], c[20]) == (3, 30, 20)
    # ... also when the reverse search meets them
    j = tag["duplicated rows met by the reverse search"]
    fs, ft = rc.job_rows(fam, j)
    assert rc.tie_counts(ft, fs)[0][[3, 30, 20]].tolist() == [2, 2, 3]
    c = {t: s for s, t in res[j][0].tolist()}
    assert (c[3], c[30], c[20]) == (3, 30, 20)
    # duplicated query rows: the target finds the first copy, the other copies are not mutual
    j = tag["duplicated query rows"]
    fs, ft = rc.job_rows(fam, j)
    assert rc.tie_counts(ft, fs)[0][[7, 12]].tolist() == [2, 3]
    srcs = set(res[j][0][:, 0].tolist())
    assert {7, 12} <= srcs and not ({8, 45, 50} & srcs)
    # the lowest index is the non-mutual one
    j = tag["tie between a non-mutual and a mutual target"]
    fs, ft = rc.job_rows(fam, j)
    d2 = rc.distances(fs, ft)
    assert d2[5, 5] == d2[5, 9] == d2[5].min() == 4 and d2[6, 5] == 1 and d2[:, 9].min() == d2[5, 9] and np.argmin(d2[:, 9]) == 5
    pairs = set(map(tuple, res[j][0].tolist()))
    assert (6, 5) in pairs and not any(s == 5 for s, t in pairs)
    # pieces: the tie is between pieces, and the first piece IN THE JOB'S ORDER wins
    for t in ("ties across 2 pieces", "ties across 3 pieces, other order"):
        j = tag[t]
        fs, ft = rc.job_rows(fam, j)
        n_pieces = int((fam["js"][j] >= 0).sum())
        tgt_bounds = np.cumsum([0] + [len(fam["mem"][s]) for s in fam["jt"][j] if s >= 0])
        for q, d, res_of in ((fs, ft, dict(res[j][0].tolist())), (ft, fs, {t: s for s, t in res[j][0].tolist()})):
            d2 = rc.distances(q, d)
            dup = np.flatnonzero((d2.min(1) == 0) & ((d2 == 0).sum(1) == n_pieces))          # a row that every piece of the other side carries
            assert len(dup) >= 1
            for i in dup:
                tied = np.flatnonzero(d2[i] == 0)
                if q is fs:
                    assert len(set(np.searchsorted(tgt_bounds, tied, side="right"))) == n_pieces          # one copy per piece
                assert res_of.get(int(i), int(tied[0])) == tied[0]
    assert list(fam["jt"][tag["ties across 3 pieces, other order"]]) != sorted(fam["jt"][tag["ties across 3 pieces, other order"]])


def test_near_ties_lie_orders_of_magnitude_inside_the_filters_band():
    fam, res = runs("near_ties")
    for j, (quantum, n_min) in enumerate(((1.0, 30), (1.0, 30), (2.0 ** -12, 30), (2.0 ** -12, 30))):
        fs, ft = rc.job_rows(fam, j)
        if j % 2:
            fs, ft = ft, fs                      # swapped: the near ties are met by the reverse search
        d2 = rc.distances(fs, ft)
        order = np.argsort(d2, axis=1, kind="stable")
        best, second = np.take_along_axis(d2, order[:, :1], 1)[:, 0], np.take_along_axis(d2, order[:, 1:2], 1)[:, 0]
        hit = (second - best == quantum) & (order[:, 0] > order[:, 1])          # the farther row at the lower index
        exact, band = rc.tie_counts(fs, ft)
        nq = ((fs.astype(np.float64) - rc.MU_NAT) ** 2).sum(1)
        width = rc.FM_C * 2 * nq.min()
        print(fam["tags"][j], "near ties", int(hit.sum()), "of", len(fs), "narrowest band", width, "quantum", quantum)
        assert hit.sum() >= n_min and (band[hit] >= 2).all() and (exact[hit] == 1).all()
        assert width > 100 * quantum
    # the first pair of jobs sits at the edge of the domain, the second on values fp16 does not hold
    assert np.concatenate(fam["mem_rows"][:1]).max() == 200.0
    frac = (fam["mem_rows"][2] - rc.MU_NAT).astype(np.float32)
    assert (frac.astype(np.float16).astype(np.float32) != frac).any()


def test_crowded_queries_have_hundreds_of_candidates_and_the_list_cannot_overflow():
    fam, res = runs("crowded")
    fs, ft = rc.job_rows(fam, 0)
    exact, band = rc.tie_counts(fs, ft)
    print("rows inside the band per query", np.sort(band)[-6:])
    assert (band > 192).sum() >= 4                       # more than the 192 entries a wave's queue holds between two flushes
    assert len(fs) * len(ft) < 65536
    fs, ft = rc.job_rows(fam, 1)
    assert (rc.tie_counts(ft, fs)[1] > 192).sum() >= 4   # the same, met by the reverse search
    counts = np.bincount(res[1][0][:, 1], minlength=len(ft)) if len(res[1][0]) else np.zeros(1)
    assert np.bincount(rc.first_nearest(fs, ft), minlength=len(ft)).max() > 100          # a target matched by many sources
    assert counts.max() <= 1


def test_mutual_counts_fallback_and_block_layout():
    fam, res = runs("mutual")
    tag = {t: j for j, t in enumerate(fam["tags"])}
    for j in range(len(res)):
        fs, ft = rc.job_rows(fam, j)
        ij, ji = rc.first_nearest(fs, ft), rc.first_nearest(ft, fs)
        n_mutual = int((ji[ij] == np.arange(len(fs))).sum())
        assert n_mutual == len(fam["mutual_sets"][j]), fam["tags"][j]
        # targets matched by nobody: the reverse search runs on a short need list; and a target matched by many sources
        needed = np.unique(ij)
        assert len(needed) == n_mutual <= len(ft) / 5 and np.bincount(ij).max() >= 3
    assert len(res[tag["8 mutual pairs"]][0]) == 40           # 8 < 9: all ns source matches
    assert len(res[tag["9 mutual pairs"]][0]) == 9
    assert len(res[tag["one mutual pair"]][0]) == 300
    blocks = lambda c: sorted(set((c[:, 0] // 256).tolist()))
    c = res[tag["700, all three blocks"]][0]
    assert blocks(c) == [0, 1, 2] and {0, 63, 64, 255, 256, 511, 512, 699} <= set(c[:, 0].tolist())
    assert blocks(res[tag["700, block 1 empty"]][0]) == [0, 2]


def test_pieces_share_pairs_and_slots():
    fam, res = runs("pieces")
    js, jt = fam["js"], fam["jt"]
    uses = [(int(a), int(b)) for j in range(len(js)) for a in js[j] if a >= 0 for b in jt[j] if b >= 0]
    assert len(set(uses)) < len(uses)                                     # what reuse[4] < reuse[5] reports on the device
    assert any(list(s >= 0) == [True, False, True] for s in js)
    assert any(s[0] == 0 for s in js) and any(s[2] == 0 for s in js) and any(s[0] == 0 for s in jt) and any(s[2] == 0 for s in jt)
    assert sorted({(int((js[j] >= 0).sum()), int((jt[j] >= 0).sum())) for j in range(len(js))}) == [(1, 1), (2, 2), (3, 2), (3, 3)]
    assert len({len(c) for c in fam["det"]}) == len(fam["det"])            # unequal sizes
    # matches cross the pieces: in a multi-piece job some source's nearest row lies in another piece than its own partner's
    for j in (0, 1, 5):
        fs, ft = rc.job_rows(fam, j)
        sb = np.cumsum([0] + [len(fam["det"][s]) for s in js[j] if s >= 0])
        tb = np.cumsum([0] + [len(fam["mem"][s]) for s in jt[j] if s >= 0])
        ij = rc.first_nearest(fs, ft)
        sp = [int(js[j][js[j] >= 0][p]) for p in np.searchsorted(sb, np.arange(len(fs)), side="right") - 1]
        tp = [int(jt[j][jt[j] >= 0][p]) for p in np.searchsorted(tb, ij, side="right") - 1]
        assert sum(a != b for a, b in zip(sp, tp)) >= 1, fam["tags"][j]


def test_fmaf_chain_and_operands_restate_the_c_arithmetic():
    """the numpy fmaf chain (product in fp64, sum rounded to odd, then to fp32) against exact rational arithmetic rounded once, on rows with
    full fp32 mantissas, where double rounding would show"""
    rng = np.random.default_rng(7)
    rows = (rng.uniform(0, 60, size=(4000, 33)) * rng.uniform(0, 1, size=(4000, 1))).astype(np.float32)
    st = rc.stored_rows(rows)
    got = rc.centred_norm(st)
    from fractions import Fraction
    for i in range(0, len(rows), 97):
        acc = np.float32(0)
        for k in range(33):
            v = np.float32(st[i, k] - rc.FEAT_MU[k])
            exact = Fraction(float(v)) * Fraction(float(v)) + Fraction(float(acc))
            lo = np.float32(float(exact))
            cands = sorted({float(lo), float(np.nextafter(lo, np.float32(-np.inf))), float(np.nextafter(lo, np.float32(np.inf)))})
            acc = np.float32(min(cands, key=lambda c: (abs(Fraction(c) - exact), int(np.float32(c).view(np.uint32)) & 1)))
        assert got[i] == acc, (i, got[i], acc)
    op = rc.operand_rows(st, got).astype(np.float64)
    assert (op[:, 33] == 8).all() and (op[:, 34] == 8).all() and not op[:, 38:].any()
    assert (np.abs((op[:, 35] + op[:, 36]) * 8 - got) <= 2.0 ** -20 * np.maximum(got, 1.0)).all()
    cw = 1.0e-3 * got.astype(np.float64) + 4.0e-3
    assert (op[:, 37] >= cw * (1 - 1e-6)).all() and (op[:, 37] <= cw * (1 + 2.0 ** -9) + 1e-6).all()


def test_philox_restatement_draws_what_the_oracle_draws():
    """three correspondences of which only the first is right and the other two targets coincide: a hypothesis passes the edge-length
    test exactly when no edge joins two different correspondences, i.e. when its three draws are equal (zero-length edges pass, the
    rank-0 Kabsch is a pure shift).  With a fixed budget of N the oracle validates as many hypotheses as the restated draw has triples
    of equal picks"""
    src = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]], np.float32)
    tgt = np.array([[0.3, 0.2, 0.1], [5.0, 5, 5], [5.0, 5, 5.001]], np.float32)
    corr = np.array([[0, 0], [1, 1], [2, 2]], np.int32)
    for seed, job in (((7 << 32) | 5, 11), ((0x9E3779B9 << 32) | 0x80000001, 4000000000)):
        N = 3000
        T, stats = ro.ransac(src, tgt, corr, rc.MAX_DIST, seed, job, N, confidence=1.0)
        picks = rc.philox_picks(seed, job, np.arange(N), 3)
        equal = (picks[:, 0] == picks[:, 1]) & (picks[:, 1] == picks[:, 2])
        assert picks.min() == 0 and picks.max() == 2
        assert stats[0] == N and stats[1] == equal.sum() and 200 < equal.sum() < 500


def test_restated_constants_are_the_kernels():
    """the band, the queue and the candidate list as csrc/reg_featnn.hip defines them, the mutual threshold as csrc/reg_match.hip passes it"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instance-based-loc_amd", "csrc")
    nn = open(os.path.join(csrc, "reg_featnn.hip")).read()
    define = lambda name: re.search(r"^#define\s+%s\s+(\S+)" % name, nn, flags=re.M).group(1)
    assert float(define("FM_C").rstrip("f")) == rc.FM_C and int(define("FM_QUEUE")) - 64 == 192 and int(define("FM_SUB")) == 1
    assert "cw = 1.0e-3f * a + 4.0e-3f" in open(os.path.join(csrc, "reg_common.h")).read() and rc.FM_A == 4.0e-3
    assert "out_count * 8 + 65536" in nn                                   # the default candidate list `crowded` and `mutual` stay below
    assert re.search(r"ibl_mutual_kernel,[^;]*ps\.J, 1, 9, ps\.corr", open(os.path.join(csrc, "reg_match.hip")).read())


def _wrong_lists(fs, ft):
    """correspondence lists of matchers that are subtly wrong, by name"""
    d2 = rc.distances(fs, ft)
    n, m = d2.shape
    first_f, first_r = np.argmin(d2, 1), np.argmin(d2, 0)
    last_f, last_r = m - 1 - np.argmin(d2[:, ::-1], 1), n - 1 - np.argmin(d2[::-1], 0)
    nq, nt = ((fs.astype(np.float64) - rc.MU_NAT) ** 2).sum(1), ((ft.astype(np.float64) - rc.MU_NAT) ** 2).sum(1)
    band = d2 <= d2.min(1, keepdims=True) + rc.FM_C * (nq[:, None] + nt[None, :])
    band_f = np.argmax(band, 1)                                            # the first row the filter passes, without the exact re-check

    def listed(ij, ji, min_mutual=9, ordered=True):
        keep = np.flatnonzero(ji[ij] == np.arange(n))
        if len(keep) < min_mutual:
            keep = np.arange(n)
        elif not ordered:                                                  # the 256-source blocks of the mutual compaction in another order
            keep = np.concatenate([keep[keep >= 256], keep[keep < 256]])
        return np.stack([keep, ij[keep]], 1).astype(np.int32)

    return {"right": listed(first_f, first_r), "last minimum, forward": listed(last_f, first_r), "last minimum, reverse": listed(first_f, last_r),
            "no exact re-check": listed(band_f, first_r), "threshold 8": listed(first_f, first_r, 8), "threshold 10": listed(first_f, first_r, 10),
            "blocks out of order": listed(first_f, first_r, ordered=False)}


def test_subtly_wrong_matchers_change_what_the_gpu_tests_compare():
    """the bite of tests/test_gpu_regmatch.py, shown on the CPU: the list a wrong tie rule, a filter without its exact re-check, a wrong
    mutual threshold or a misordered compaction would hand to RANSAC gives other statistics than the right list, in the family that
    exists for it (the oracle's RANSAC on both lists; the device's RANSAC equals the oracle's, tests/test_gpu_ransac.py)"""
    targets = {"last minimum, forward": ("ties", "crowded", "pieces"), "last minimum, reverse": ("ties", "crowded"),
               "no exact re-check": ("near_ties", "crowded"), "threshold 8": ("mutual",), "threshold 10": ("mutual",),
               "blocks out of order": ("mutual", "sizes")}
    caught = {}
    for name in sorted(rc.FAMILIES):
        fam = rc.FAMILIES[name]()
        for j in range(len(fam["js"])):
            fs, ft = rc.job_rows(fam, j)
            if len(fs) == 0 or len(ft) == 0:
                continue
            lists = _wrong_lists(fs, ft)
            corr, T, stats = rc.expected(fam, j)
            assert np.array_equal(lists.pop("right"), corr)
            a = rc.job_arrays(fam, j)
            for rule, wrong in lists.items():
                if np.array_equal(wrong, corr):
                    continue
                Tw, sw = ro.ransac(a["src"], a["tgt"], wrong, rc.MAX_DIST, fam["seed"], int(fam["job_ids"][j]), fam["max_iter"])
                differs = not np.array_equal(sw, stats) or np.abs(Tw - T).max() > 1e-6
                caught.setdefault((rule, name), []).append(differs)
    for rule, names in targets.items():
        for name in names:
            hits = caught.get((rule, name), [])
            print(rule, "/", name, ": jobs whose list changes", len(hits), "of them seen in statistics or T_ransac", sum(hits))
            assert hits and all(hits), (rule, name)
