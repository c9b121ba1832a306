"""CPU: the job sets of tests/ransac_cases.py are what they claim, shown with the oracle alone -- so that a later edit of a case cannot
quietly stop exercising the path of csrc/reg_ransac.hip it exists for: the stopping round of every scheduler job, the number of job
slots a round runs on, the survivors a fold walks, repeated draws, the edge-length ratios inside the fp32 guard band."""
import numpy as np
import pytest

from tests import ransac_cases as rs
from tests import regmatch_cases as rc
from oracle import reg_oracle as ro


def runs(name):
    fam = rs.FAMILIES[name]()
    return fam, [rc.expected(fam, j) for j in range(len(fam["js"]))]


@pytest.mark.parametrize("name", sorted(rs.FAMILIES))
def test_matching_cannot_be_the_variable(name):
    """rows in the domain, exact in fp32, and the correspondence list is the full bijection in source order"""
    fam, res = runs(name)
    rc.exactness(fam)
    for j, (corr, T, stats) in enumerate(res):
        fs, ft = rc.job_rows(fam, j)
        if len(fs) == 0 or len(ft) == 0:
            assert len(corr) == 0
            continue
        assert len(fs) == len(ft) == len(corr) and np.array_equal(corr[:, 0], np.arange(len(fs)))
        assert sorted(corr[:, 1].tolist()) == list(range(len(ft)))
        assert np.array_equal(fs, ft[corr[:, 1]])
        if len(fs) <= 400:
            d2 = rc.distances(fs, ft)
            d2[np.arange(len(fs)), corr[:, 1]] = np.inf
            assert len(fs) == 1 or d2.min() >= 32


def test_restated_constants_are_the_kernels():
    k = rs.kernel_constants()
    print(k)
    first, biggest = k["RANSAC_FIRST_ROUND"], k["RANSAC_MAX_ROUND"]
    assert (first, first * 8, biggest) == (4096, 32768, 262144) and first * 64 == biggest
    assert rs.ROUNDS == (first, first + first * 8, first + first * 8 + biggest)
    assert rs.TAIL_ROUND == k["RANSAC_TAIL_ROUND"] and rs.TAIL_JOBS == k["RANSAC_TAIL_JOBS"] and rs.LDS_CORR == k["RANSAC_LDS_CORR"]
    # the wide flag kernel: rounds of at least 1024 RANSAC_BIG_SUBS hypotheses with (round / 16 384) x slots >= RANSAC_WIDE_MIN_BLOCKS
    assert 1024 * k["RANSAC_BIG_SUBS"] <= biggest and rs.BIG_MIN_JOBS * (biggest // 16384) == k["RANSAC_WIDE_MIN_BLOCKS"]
    assert (first * 8 // 16384) * len(rs.many_active()["js"]) < k["RANSAC_WIDE_MIN_BLOCKS"]          # (only the 262 144 round is wide)


def test_stop_rounds_one_job_per_stopping_place():
    fam, res = runs("stop_rounds")
    walked = {t: int(r[2][0]) for t, r in zip(fam["tags"], res)}
    print(walked, [r[2].tolist() for r in res])
    assert len(res) > rs.TAIL_JOBS                                  # the third round is a 262 144 one and the host reads back after it
    assert rs.stopping_round(walked["600/1500"]) == 0
    assert rs.stopping_round(walked["20/200"]) == 1 and walked["20/200"] == 4603
    assert rs.stopping_round(walked["6/150"]) == 2
    assert rs.ROUNDS[2] < walked["4/200"] < fam["max_iter"]
    never = res[fam["tags"].index("never")][2]
    assert never[0] == fam["max_iter"] == 700000 and 3 <= never[2] <= 6
    assert all(fam["max_iter"] % r for r in (4096, 32768, 262144, rs.TAIL_ROUND))
    # two jobs outlive the read-back: at most RANSAC_TAIL_JOBS, so the rounds behind it are 2^20 ones
    assert sum(int(r[2][0]) > rs.ROUNDS[2] for r in res) == 2


def test_fixed_budget_walks_all_of_it():
    fam, res = runs("fixed_budget")
    for corr, T, stats in res:
        assert stats[0] == fam["max_iter"] and stats[1] > 1000
    # the same jobs stop early with the confidence exit
    assert all(rc.expected(fam, j, fixed_budget=False)[2][0] < 5000 for j in range(len(res)))


def test_many_active_fills_the_wide_round_and_leaves_a_scattered_active_list():
    fam, res = runs("many_active")
    walked = np.array([int(r[2][0]) for r in res])
    n_corr = np.array([len(r[0]) for r in res])
    running_2, running_3 = np.flatnonzero(walked > rs.ROUNDS[1]), np.flatnonzero(walked > rs.ROUNDS[2])
    print("jobs", len(res), "running at 36 864:", len(running_2), "at 299 008:", running_3.tolist())
    assert len(running_2) >= rs.BIG_MIN_JOBS and len(res) * (262144 // 16384) >= 1024
    # after the first read-back: a strict, non-contiguous subset (slot != job), more than one job, not the first slot
    assert 1 < len(running_3) < len(res) and running_3[0] > 0 and (np.diff(running_3) > 1).all()
    assert (walked[fam["tags"].index("never")] == fam["max_iter"])
    # in between: jobs that stop in round 1, and the degenerate ones
    assert (walked[np.array([t == "quick" for t in fam["tags"]])] <= rs.ROUNDS[0]).all()
    tag = {t: j for j, t in enumerate(fam["tags"])}
    for t, n in (("empty source", 0), ("empty target", 0), ("1 point", 1), ("2 points", 2)):
        corr, T, stats = res[tag[t]]
        assert len(corr) == n and not stats.any() and np.array_equal(T, np.eye(4)), t
    assert n_corr[tag["3 points"]] == 3 and res[tag["3 points"]][2][0] > 0
    assert len(rc.job_arrays(fam, tag["empty source"])["src"]) == 0 and len(rc.job_arrays(fam, tag["empty target"])["tgt"]) == 0
    assert len(set(fam["job_ids"].tolist())) == len(res)


def test_tail_reaches_the_rounds_of_2_to_the_20_and_ends_inside_one():
    fam, res = runs("tail")
    walked = np.array([int(r[2][0]) for r in res])
    print(walked.tolist())
    assert len(res) > rs.TAIL_JOBS
    late = walked > rs.ROUNDS[2]
    assert 0 < late.sum() <= rs.TAIL_JOBS
    first_tail_end = rs.ROUNDS[2] + rs.TAIL_ROUND
    assert first_tail_end < fam["max_iter"] < first_tail_end + rs.TAIL_ROUND
    assert (walked[late] > first_tail_end).all() and (walked == fam["max_iter"]).sum() >= 2
    assert ((walked > first_tail_end) & (walked < fam["max_iter"])).sum() >= 1          # and a confidence exit inside a tail round


def test_lds_edge_sizes_and_rounds():
    fam, res = runs("lds_edge")
    n_corr = [len(r[0]) for r in res]
    assert sorted(set(n_corr)) == [rs.LDS_CORR - 1, rs.LDS_CORR, rs.LDS_CORR + 1, 3000]
    for n in set(n_corr):
        rounds = sorted(rs.stopping_round(int(r[2][0])) for r in res if len(r[0]) == n)
        assert rounds == [0, 1], (n, rounds)


def test_dense_fold_has_far_more_than_64_survivors_in_a_round():
    fam, res = runs("dense_fold")
    for j, (corr, T, stats) in enumerate(res):
        a = rc.job_arrays(fam, j)
        # the survivors of the first round = what the loop validates among the first 4 096 hypotheses when nothing stops it
        _, s = ro.ransac(a["src"], a["tgt"], corr, rc.MAX_DIST, fam["seed"], int(fam["job_ids"][j]), 4096, confidence=1.0)
        print(fam["tags"][j], "survivors of the first round", int(s[1]), "walked / validated / best", stats.tolist())
        assert s[1] > 64, fam["tags"][j]
        assert 30 <= len(corr) <= 60
    validated = np.array([int(r[2][1]) for r in res])
    walked = np.array([int(r[2][0]) for r in res])
    # est_k stops some jobs inside the first 64-survivor chunk, others after several chunks
    assert (validated < 64).sum() >= 3 and (validated > 128).sum() >= 2 and (walked < 4096).all()
    # the exact jobs: the best transform changes at equal inlier count (decided by rmse)
    total = 0
    for j, t in enumerate(fam["tags"]):
        if not t.endswith("exact"):
            continue
        a = rc.job_arrays(fam, j)
        hist = [ro.ransac(a["src"], a["tgt"], res[j][0], rc.MAX_DIST, fam["seed"], int(fam["job_ids"][j]), m) for m in range(1, int(res[j][2][0]) + 1)]
        by_rmse = sum(1 for (T0, s0), (T1, s1) in zip(hist, hist[1:]) if s0[2] == s1[2] > 0 and not np.array_equal(T0, T1))
        print(t, "updates at equal inlier count", by_rmse)
        total += by_rmse
    assert total >= 1


def test_dense_fixed_ties_in_fitness_are_decided_by_rmse_again_and_again():
    fam, res = runs("dense_fixed")
    assert fam["fixed_budget"] and all(fam["max_iter"] % r for r in (4096, 32768))
    total = 0
    for j, (corr, T, stats) in enumerate(res):
        assert stats[0] == fam["max_iter"] and stats[1] > 500, fam["tags"][j]
        if not fam["tags"][j].endswith("exact"):
            continue
        a = rc.job_arrays(fam, j)
        hist = [ro.ransac(a["src"], a["tgt"], corr, rc.MAX_DIST, fam["seed"], int(fam["job_ids"][j]), m, confidence=1.0)
                for m in range(250, fam["max_iter"] + 1, 250)]
        by_rmse = sum(1 for (T0, s0), (T1, s1) in zip(hist, hist[1:]) if s0[2] == s1[2] > 0 and not np.array_equal(T0, T1))
        print(fam["tags"][j], "validated", int(stats[1]), "updates at equal inlier count (seen at checkpoints)", by_rmse)
        assert by_rmse >= 1, fam["tags"][j]
        total += by_rmse
    assert total >= 6          # (a lower bound: updates between two checkpoints are seen as one)


def test_degenerate_draws_repeat_among_validated_hypotheses():
    fam, res = runs("degenerate")
    all_equal = two_equal = 0
    for j, (corr, T, stats) in enumerate(res):
        nc = len(corr)
        if nc > 5:
            continue
        picks = rc.philox_picks(fam["seed"], int(fam["job_ids"][j]), np.arange(int(stats[0])), nc)
        distinct = np.array([len(set(p)) for p in picks.tolist()])
        # a hypothesis whose three draws are equal passes both checkers whatever the points (zero-length edges, a pure shift): it is validated
        all_equal += int((distinct == 1).sum())
        two_equal += int((distinct == 2).sum())
        assert stats[1] >= (distinct == 1).sum()
        print(fam["tags"][j], "walked", int(stats[0]), "validated", int(stats[1]), "draws with 1 / 2 distinct", int((distinct == 1).sum()), int((distinct == 2).sum()))
    assert all_equal >= 20 and two_equal >= 100
    assert sorted(set(len(r[0]) for r in res)) == [3, 4, 5, 20]
    tag = {t: j for j, t in enumerate(fam["tags"])}
    corr, T, stats = res[tag["collinear, correct"]]
    assert stats[2] == 20
    a = rc.job_arrays(fam, tag["collinear, correct"])
    s = a["src"].astype(np.float64)
    assert np.linalg.matrix_rank(s - s.mean(0)) == 1
    corr, T, stats = res[tag["collinear, incorrect"]]
    assert 3 <= stats[2] < 20 and stats[1] > 1


def test_edge_band_has_ratios_inside_the_guard_band_on_both_sides():
    fam, res = runs("edge_band")
    for j, (corr, T, stats) in enumerate(res):
        a = rc.job_arrays(fam, j)
        band, ok = rs.edge_band_pairs(a["src"], a["tgt"], corr)
        print(fam["tags"][j], "pairs", len(band), "in the band", int(band.sum()), "of them passing / failing the exact test", int((band & ok).sum()),
              int((band & ~ok).sum()), "stats", stats.tolist())
        if fam["tags"][j] == "ratio 1":
            assert not band.any() and ok.all()
            continue
        assert band.mean() > 0.9 and (band & ok).sum() > 100 and (band & ~ok).sum() > 100
        assert stats[0] > 50 and stats[1] >= 3           # the walk is long enough for the verdicts to decide it


def test_ids_and_seed_use_the_high_bits():
    fam, res = runs("ids_seed")
    ids = fam["job_ids"].astype(np.int64)
    assert (ids >= 2 ** 31).all() and (np.diff(ids) < 0).any() and (np.diff(ids) > 0).any() and (np.abs(np.diff(ids)) > 1).all()
    assert fam["seed"] >> 32 and fam["seed"] & 0x80000000 and fam["center"]
    assert all(r[2][0] > 0 for r in res)
    # the id matters: another id walks another way
    a = rc.job_arrays(fam, 2)
    other = ro.ransac(a["src"], a["tgt"], res[2][0], rc.MAX_DIST, fam["seed"], int(ids[2]) - 2 ** 31, fam["max_iter"])
    assert not np.array_equal(other[1], res[2][2])
