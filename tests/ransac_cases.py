"""Deterministic job sets for the RANSAC stage alone (csrc/reg_ransac.hip), shared by tests/test_ransac_model.py (CPU: the oracle shows
that every family reaches the path it is named for) and tests/test_gpu_ransac.py (GPU: `ransac_stats` and `T_ransac` of every job
against `oracle.reg_oracle.ransac`).  Families are the dicts of tests/regmatch_cases.py, run through its injection helper.

Features are trivially separable here, so matching cannot be the variable: source point i and exactly one target point carry the same
code row (`regmatch_cases.code_rows`; different codes are at least 32 apart, squared), the correspondence list is the full bijection in
source order, n_corr = ns = nt.  The geometry decides everything else: inlier targets are a rigid motion of their sources (plus noise
below the correspondence distance of 0.075 m where the family says so), outlier targets are random, and the target rows are shuffled."""
import numpy as np
from scipy.spatial.transform import Rotation

from tests import regmatch_cases as rc
from tests.regmatch_cases import memo

SEED = (7 << 32) | 5
MAX_ITER = 700000          # no multiple of any round size (4 096, 32 768, 262 144, 2^20), and the oracle stays fast
ROUNDS = (4096, 36864, 299008)          # hypotheses walked after the first three rounds; the host first reads back after the third
TAIL_ROUND = 1 << 20
LDS_CORR = 1024            # RANSAC_LDS_CORR: more correspondences than this are drawn from global memory
BIG_MIN_JOBS = 64          # job slots a 262 144-hypothesis round needs to launch the 8 k-hypothesis blocks (RANSAC_WIDE_MIN_BLOCKS 1024 / 16)
TAIL_JOBS = 8              # RANSAC_TAIL_JOBS: with at most this many jobs left a round walks 2^20 hypotheses


def kernel_constants():
    """the scheduler's constants as csrc/reg_ransac.hip defines them (its `#define NAME value` and `constexpr int NAME = value` lines), so
    that a retune of the kernels cannot leave the restatements above -- and with them the paths the families claim to reach -- behind"""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instance-based-loc_amd", "csrc", "reg_ransac.hip")
    text = open(path).read()
    found = dict(re.findall(r"^\s*#define\s+(RANSAC_\w+)\s+([^/\n]+?)\s*(?://.*)?$", text, flags=re.M))
    found.update(re.findall(r"constexpr\s+int\s+(RANSAC_\w+)\s*=\s*([^;]+);", text))
    return {k: int(eval(v.strip(), {"__builtins__": {}})) for k, v in found.items() if re.fullmatch(r"[\d\s()<+*-]+", v.strip())}


def motion(rng, max_deg=25.0, max_shift=0.3):
    R = Rotation.from_euler("xyz", rng.uniform(-max_deg, max_deg, size=3), degrees=True).as_matrix()
    return R, rng.uniform(-max_shift, max_shift, size=3)


def corr_job(rng, nc, n_inl, noise=0.0, box=1.0, shuffle=True):
    """-> (source (nc, 3), target (nc, 3), rows_s, rows_t): n_inl correspondences are a rigid motion (+- noise per axis), the others
    random; the inliers are spread over the list; target k = partner of source perm[k]"""
    src = rng.uniform(-box, box, size=(nc, 3))
    R, t = motion(rng)
    tgt = rng.uniform(-box, box, size=(nc, 3)) + t
    inl = np.sort(rng.permutation(nc)[:n_inl])
    tgt[inl] = src[inl] @ R.T + t + rng.uniform(-noise, noise, size=(n_inl, 3))
    return _shuffled(rng, src, tgt, shuffle)


def _shuffled(rng, src, tgt, shuffle=True):
    nc = len(src)
    perm = rng.permutation(nc) if shuffle else np.arange(nc)
    return src, tgt[perm], rc.code_rows(np.arange(nc)), rc.code_rows(perm)


class _Jobs:
    """collects single-instance jobs: one detected and one memory instance each"""

    def __init__(self):
        self.det, self.mem, self.det_rows, self.mem_rows, self.tags = [], [], [], [], []

    def add(self, job, tag):
        src, tgt, rs, rt = job
        self.det.append(src); self.mem.append(tgt); self.det_rows.append(rs); self.mem_rows.append(rt); self.tags.append(tag)

    def family(self, **kw):
        J = len(self.tags)
        kw.setdefault("seed", SEED)
        kw.setdefault("max_iter", MAX_ITER)
        return rc.family(self.det, self.mem, self.det_rows, self.mem_rows, [[j] for j in range(J)], [[j] for j in range(J)], self.tags, **kw)


def _random_job(rng, nc):
    return corr_job(rng, nc, 0)


@memo
def stop_rounds():
    """one job per stopping place of the scheduler (inliers / correspondences): 600/1500 stops in the first 4 096; 20/200 at est_k 4 603
    in the 32 k round; 6/150 at ~ 72 k in the 256 k round; 4/200 at est_k ~ 575 k, after the first host read-back (in a 2^20 round:
    two jobs are left); 400 random correspondences never stop: best inliers 3, the walk ends at ransac_max_iter = 700 000 inside a round.
    Four quick jobs bring the call to nine slots: with eight or fewer the third round would already be a 2^20 one and nothing read back."""
    rng = np.random.default_rng(401)
    jobs = _Jobs()
    jobs.add(corr_job(rng, 1500, 600, 0.01), "600/1500")
    jobs.add(corr_job(rng, 200, 20, 0.01), "20/200")
    jobs.add(corr_job(rng, 150, 6, 0.004), "6/150")
    jobs.add(corr_job(rng, 200, 4, 0.004), "4/200")
    jobs.add(_random_job(rng, 400), "never")
    for _ in range(4):
        jobs.add(corr_job(rng, 150, 60, 0.01), "quick")
    return jobs.family()


@memo
def fixed_budget():
    """the benchmark's switch: the 20/200 and the 600/1500 job of `stop_rounds` without the confidence exit: walked == ransac_max_iter"""
    fam = dict(rc.sub_family(stop_rounds(), [1, 0]))
    fam["job_ids"] = stop_rounds()["job_ids"][[1, 0]]
    fam["fixed_budget"] = True
    fam["_expected"] = {}
    return fam


MANY_SLOW = (9, 31, 52, 70)          # slots of the 4/200 jobs of `many_active`
MANY_NEVER = 44


@memo
def many_active():
    """88 job slots in one call.  66 jobs of the 6/150 kind are still running at 36 864 hypotheses, so the 262 144-hypothesis round runs
    on 88 >= 64 slots and launches the 8 k-hypothesis kernel; they all stop in that round.  Four 4/200 jobs and a never-stopping one,
    scattered over the slots, outlive the first read-back: the compacted active list is then a strict, non-contiguous subset (slot !=
    job).  In between: quick jobs (stop in round 1), an empty source, an empty target, jobs of 1 and 2 points (n_corr < 3: identity,
    statistics 0) and one of exactly 3 correspondences."""
    rng = np.random.default_rng(411)
    jobs = _Jobs()
    special = {5: "empty source", 17: "empty target", 26: "1 point", 38: "2 points", 60: "3 points"}
    for j in range(88):
        if j in special:
            n = {"empty source": 0, "empty target": 4, "1 point": 1, "2 points": 2, "3 points": 3}[special[j]]
            src, tgt, rs, rt = corr_job(rng, max(n, 1), max(n, 1))
            if special[j] == "empty source":
                src, rs, tgt, rt = src[:0], rs[:0], rng.uniform(-1, 1, size=(4, 3)), rc.code_rows(np.arange(4))
            elif special[j] == "empty target":
                src, rs, tgt, rt = rng.uniform(-1, 1, size=(4, 3)), rc.code_rows(np.arange(4)), tgt[:0], rt[:0]
            jobs.add((src, tgt, rs, rt), special[j])
        elif j in MANY_SLOW:
            jobs.add(corr_job(rng, 200, 4, 0.004), "4/200")
        elif j == MANY_NEVER:
            jobs.add(_random_job(rng, 400), "never")
        elif j % 8 == 3:
            jobs.add(corr_job(rng, 150, 60, 0.01), "quick")
        else:
            jobs.add(corr_job(rng, 150, 6, 0.004), "6/150")
    ids = (np.arange(88, dtype=np.uint32) * 7 + 1000).astype(np.uint32)
    return jobs.family(job_ids=ids)


@memo
def tail():
    """six never-stopping jobs (400 random correspondences) among six quick ones, ransac_max_iter = 1 500 000: twelve slots run the first
    three rounds (299 008), the read-back leaves six <= 8 jobs, whose rounds are 2^20 hypotheses: one whole tail round (to 1 347 584)
    and the end of the budget inside the second"""
    rng = np.random.default_rng(421)
    jobs = _Jobs()
    for j in range(12):
        if j % 2:
            jobs.add(_random_job(rng, 400), "never")
        else:
            jobs.add(corr_job(rng, 150, 60, 0.01), "quick")
    return jobs.family(max_iter=1500000)


@memo
def lds_edge():
    """n_corr = 1023, 1024, 1025 and 3000 around RANSAC_LDS_CORR = 1024 (staged in LDS up to it, drawn from global memory above), each with an
    inlier share of 0.3 (stops in the first round) and of 0.08 (est_k ~ 9 000: the 32 k round)"""
    rng = np.random.default_rng(431)
    jobs = _Jobs()
    for nc in (1023, 1024, 1025, 3000):
        for share in (0.3, 0.08):
            jobs.add(corr_job(rng, nc, int(round(share * nc)), 0.01), "%d/%d" % (int(round(share * nc)), nc))
    return jobs.family()


DENSE_NOISE = (0.02, 0.05, 0.08, 0.11)


@memo
def dense_fold():
    """small lists (30 .. 60) in which every correspondence is an inlier plus noise: nearly every hypothesis passes both checkers, so far
    more than 64 survivors of one job fall into the first round, the best inlier count grows inside a 64-survivor chunk of the fold and
    est_k drops below indices already listed.  With noise beyond the correspondence distance the fitness stays low and the fold walks
    several chunks before est_k stops it inside one.  Four noise-free jobs (a third of the list exact inliers, the rest random): all-inlier
    hypotheses have the same inlier count, so equal fitness is decided by rmse."""
    rng = np.random.default_rng(441)
    jobs = _Jobs()
    for nc, noise in zip((30, 40, 50, 60), DENSE_NOISE):
        jobs.add(corr_job(rng, nc, nc, noise), "%d noise %g" % (nc, noise))
    for nc, noise in zip((60, 45), (0.14, 0.17)):
        jobs.add(corr_job(rng, nc, nc, noise), "%d noise %g" % (nc, noise))
    for nc, n_inl in ((40, 14), (36, 12), (50, 16), (30, 11)):
        jobs.add(corr_job(rng, nc, n_inl, 0.0), "%d/%d exact" % (n_inl, nc))
    return jobs.family()


DENSE_FIXED_ITER = 20000


@memo
def dense_fixed():
    """the jobs of `dense_fold` with a fixed budget of 20 000 hypotheses (no multiple of a round size): est_k never drops, the fold walks every
    survivor of the first round and half of the second -- thousands per job, chunk after chunk -- and in the noise-free jobs hundreds of
    all-inlier hypotheses tie in fitness, so the best transform is the one of least rmse"""
    fam = dict(dense_fold())
    fam["fixed_budget"] = True
    fam["max_iter"] = DENSE_FIXED_ITER
    fam["_expected"] = {}
    return fam


def _line_job(rng, n, stretch):
    """collinear correspondences whose moments are exact: sources on the x axis at multiples of 1/8, targets on a line along y (a
    quarter turn and a shift, all exactly representable): the cross-covariance has ONE non-zero entry, rank 1 without rounding"""
    x = np.sort(rng.permutation(40)[:n]).astype(np.float64) / 8.0
    src = np.stack([x, np.zeros(n), np.zeros(n)], 1)
    tgt = np.stack([np.full(n, 0.5), x * stretch + 0.25, np.full(n, -0.125)], 1)
    return _shuffled(rng, src, tgt)


@memo
def degenerate():
    """n_corr = 3, 4, 5: draws repeat a correspondence in most hypotheses -- zero-length edges (the fp32 edge test hands them to the exact
    one), Kabsch of rank 0 (all three draws equal: the identity rotation) and rank 1 (two equal).  All-inlier, mixed and all-outlier
    lists, so that walks of 1 to 122 hypotheses occur.  Collinear correspondences: a correct list (rank-1 Kabsch for EVERY
    hypothesis, all points inliers whatever the roll about the line) and an incorrect one (targets spaced 0.95 of the sources)."""
    rng = np.random.default_rng(451)
    jobs = _Jobs()
    for nc in (3, 4, 5):
        jobs.add(corr_job(rng, nc, nc, 0.0, box=0.5), "%d/%d" % (nc, nc))
        jobs.add(corr_job(rng, nc, 2, 0.0, box=0.5), "2/%d" % nc)
        jobs.add(corr_job(rng, nc, 0, 0.0, box=0.5), "0/%d" % nc)
    jobs.add(_line_job(rng, 20, 1.0), "collinear, correct")
    jobs.add(_line_job(rng, 20, 0.9375), "collinear, incorrect")
    return jobs.family()


EDGE_SIM = 0.9
EDGE_BAND = 3e-6


def _scaled_job(rng, n, scale, offset, half):
    """targets = sources scaled about the cloud's centre: every edge ratio is `scale` before rounding; the fp32 rounding of the points
    (coordinates ~ `offset`, edges ~ `half`) moves the squared ratios by ~ 1e-7 .. 1e-6.  A cloud of +- 1.2 m or more leaves only
    the points near a hypothesis' own triangle within the correspondence distance, so the fitness stays low and the walk long"""
    c = np.array([offset, -offset, 0.5 * offset])
    src = (c + rng.uniform(-half, half, size=(n, 3))).astype(np.float32).astype(np.float64)
    tgt = c + scale * (src - c)
    return _shuffled(rng, src, tgt)


@memo
def edge_band():
    """the fp32 guard band of the edge-length test: targets that are the sources scaled by 0.9 and by 1 / 0.9, so that the squared edge
    ratios sit at edge_sim^2 = 0.81 and fp32 rounding of the points puts them on both sides of it, within the 3e-6 band in which the
    flag kernel falls back to the exact fp64 test: a validated hypothesis has passed it on all three edges, so `walked` and `validated`
    (hundreds to thousands here) follow the exact verdicts.  One job at ratio 1 (never in the band)."""
    rng = np.random.default_rng(461)
    jobs = _Jobs()
    jobs.add(_scaled_job(rng, 60, 0.9, 3.0, 1.2), "scale 0.9")
    jobs.add(_scaled_job(rng, 60, 1.0 / 0.9, 3.0, 1.2), "scale 1/0.9")
    jobs.add(_scaled_job(rng, 60, 0.9, 3.0, 1.6), "scale 0.9 wide")
    jobs.add(_scaled_job(rng, 50, 1.0 / 0.9, 1.0, 0.8), "scale 1/0.9 near")
    jobs.add(_scaled_job(rng, 60, 1.0, 3.0, 1.2), "ratio 1")
    return jobs.family()


def edge_band_pairs(src, tgt, corr):
    """the flag kernel's fp32 edge test on every pair of correspondences, restated in numpy fp32 -> (in_band, exact_ok): pairs whose
    squared-edge ratio is neither rejected nor accepted outright, and the exact fp64 verdict of every pair"""
    ps, pd = src[corr[:, 0]].astype(np.float32), tgt[corr[:, 1]].astype(np.float32)
    a, b = np.triu_indices(len(corr), 1)

    def sq(p):
        d = p[a] - p[b]
        return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]          # float32 throughout, left to right as the kernel

    ds2, dt2 = sq(ps), sq(pd)
    e2 = np.float32(EDGE_SIM * EDGE_SIM)
    e2_lo, e2_hi = e2 * (np.float32(1.0) - np.float32(EDGE_BAND)), e2 * (np.float32(1.0) + np.float32(EDGE_BAND))
    rejected = (ds2 < dt2 * e2_lo) | (dt2 < ds2 * e2_lo)
    accepted = (ds2 > dt2 * e2_hi) & (dt2 > ds2 * e2_hi)
    s64, d64 = ps.astype(np.float64), pd.astype(np.float64)
    ds = np.sqrt(((s64[a] - s64[b]) ** 2).sum(1))
    dt = np.sqrt(((d64[a] - d64[b]) ** 2).sum(1))
    exact_ok = ~((ds < dt * EDGE_SIM) | (dt < ds * EDGE_SIM))
    return ~rejected & ~accepted, exact_ok


@memo
def ids_seed():
    """a seed with a non-zero high word and job ids >= 2^31 that are neither monotone nor contiguous (Philox counter word 1), with
    center=True: the clouds the stage sees are the centred ones"""
    rng = np.random.default_rng(471)
    jobs = _Jobs()
    jobs.add(corr_job(rng, 300, 90, 0.01), "90/300")
    jobs.add(corr_job(rng, 200, 20, 0.01), "20/200")
    jobs.add(corr_job(rng, 150, 6, 0.004), "6/150")
    jobs.add(corr_job(rng, 1500, 120, 0.01), "120/1500")
    jobs.add(corr_job(rng, 80, 0), "random 80")
    ids = np.array([4000000000, 2147483648, 4294967295, 3000000001, 2147483649], dtype=np.uint32)
    return jobs.family(seed=(0x9E3779B9 << 32) | 0x80000001, job_ids=ids, center=True, max_iter=200000)


FAMILIES = {"stop_rounds": stop_rounds, "fixed_budget": fixed_budget, "many_active": many_active, "tail": tail, "lds_edge": lds_edge,
            "dense_fold": dense_fold, "dense_fixed": dense_fixed, "degenerate": degenerate, "edge_band": edge_band, "ids_seed": ids_seed}


def stopping_round(walked, rounds=ROUNDS):
    """index of the scheduler round in which a walk of `walked` hypotheses ends: 0, 1, 2 = the 4 k, 32 k, 256 k round, 3 = later"""
    return int(np.searchsorted(np.asarray(rounds), walked, side="left"))
