"""The feature-reuse plan of registration (csrc/reg_match.hip: list_near_candidates, ibl_near_pair_kernel, test_near_pairs,
plan_feature_reuse, plan_feature_pairs, ibl_group_gather_kernel, ibl_feat_assemble_kernel and the fold / need kernels behind them): job
sets built for the edges of the decision "this instance keeps its resident features / is recomputed in the context of its side", and a
float64 numpy restatement of that decision and of its bookkeeping.  Shared by tests/test_reuse_model.py (CPU, oracle only: every family
is what it claims and has the power to see a wrong decision) and tests/test_gpu_reuse.py (GPU: cached == uncached bit for bit, the
device's `reuse` statistics == `plan`, poisoned features).

The rule is stated ONCE, in `near_rule`: an attempt to shrink the radius edits that function (and the product) and is judged by
everything else here unchanged.

A family is the dict of tests/regmatch_cases.py without crafted rows:
    det, mem            lists of (n, 3) float32 clouds: the two pools; mem[k] is ONE rigid motion (`MOTION`, about the centre of all
                        points of the family) of det[k], so every job whose two sides list the same instances is meant to register
    det_int, mem_int    per-cloud intensities (a smooth function of the detected coordinates, carried along by the motion)
    js, jt              (J, 3) int32 job tables, padded with -1 (an empty slot may sit in the middle)
    tags, registers     per job a short name and whether the job is meant to register (pose compared with the known motion)
    center, seed, job_ids (J,) uint32, max_iter        the call
    claims              {(lo id, hi id): (least, most)} the minimum point distance every pair of a side was built for (detected pool; the
                        memory pool is its rigid copy); tests/test_reuse_model.py holds the brute force to it

Objects are surface samples of a box with a smaller box on top of it, off its centre (no symmetry: one pose fits), or blobs.  Two
objects `beside` each other along x carry one designated pair of points, face centre against face centre, so the minimum distance of
the pair is the gap it was built with, to fp32 rounding."""
import os
import re

import numpy as np

from tests.icp_cases import SMALL, job_arrays, moved          # noqa: F401  (job_arrays re-exported)
from tests.regmatch_cases import memo

VOXEL = 0.05
GLOBAL = 1.5
LOCAL = 1.5
MAX_ITER = 100000
SEED = (7 << 32) | 5
PARAMS = dict(voxel=VOXEL, local=LOCAL)
NORMAL_RADIUS, NORMAL_NN = 2 * VOXEL, 30
FPFH_RADIUS, FPFH_NN = 5 * VOXEL, 100
GRAD_RADIUS, GRAD_NN = 2 * VOXEL * LOCAL, 30
MOTION = SMALL                      # ((3, -2, 2) degrees, (0.02, -0.02, 0.01) m)
FAR = 0.7                           # pairs called far are at least this far apart
R_MARGIN, CAP_MARGIN = 0.02, 0.05   # no family sits this close (relative) to the radius / to NEAR_CAP
FEATURE_WAYS = {"det": (True, False, False), "mem": (False, True, False), "both": (True, True, False), "both compact": (True, True, True)}


def near_rule(params=PARAMS):
    """R: a foreign point further than this from every point of an instance cannot change a row of its normals (radius 2 v), FPFH
    (radius 5 v, through the SPFH of neighbours: 2 * 5 v, whose normals reach 2 v further) or colour gradients (radius grad_radius =
    2 v local, normals 2 v further), plus the product's rounding margin (include/ibloc.h at ibl_instance_features, csrc/reg_match.hip
    ibl_reg_match_stage)"""
    v = params["voxel"]
    grad_radius = 2 * v * params["local"]
    return max(2 * 5 * v + 2 * v, grad_radius + 2 * v) * 1.001 + 1e-4


def kernel_constants():
    """NEAR_CAP and NEAR_SPLIT as csrc/reg_match.hip defines them, so that a retune of the kernel cannot leave the families that are
    dimensioned by them behind"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instance-based-loc_amd", "csrc", "reg_match.hip")
    found = dict(re.findall(r"^\s*#define\s+(NEAR_\w+)\s+(\d+)\s*(?://.*)?$", open(path).read(), flags=re.M))
    return {k: int(v) for k, v in found.items()}


# ------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------
def intensity_of(pts):
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    return (0.5 + 0.25 * np.sin(9 * p[:, 0] + 1) * np.cos(7 * p[:, 1]) + 0.2 * np.sin(8 * p[:, 2] + 3 * p[:, 0])).astype(np.float32)


def _box_surface(rng, n, size, centre):
    size, centre = np.asarray(size, np.float64), np.asarray(centre, np.float64)
    area = np.array([size[1] * size[2], size[0] * size[2], size[0] * size[1]])
    axis = rng.choice(3, size=n, p=area / area.sum())
    p = rng.uniform(-0.5, 0.5, size=(n, 3))
    p[np.arange(n), axis] = rng.choice([-0.5, 0.5], size=n)
    return p * size + centre


def thing(rng, n, size, centre, pins=()):
    """n points: the pins (points given by the caller: the designated closest points) first, then four fifths of the rest on the surface
    of the box `size` about `centre` and one fifth on a smaller box on top of it (inside the box's x and y range, off its centre)"""
    size, centre = np.asarray(size, np.float64), np.asarray(centre, np.float64)
    pins = np.asarray(pins, np.float64).reshape(-1, 3)
    n_free = n - len(pins)
    n_top = n_free // 5
    top_size = size * [0.4, 0.35, 0.3]
    top_centre = centre + [-0.2 * size[0], 0.15 * size[1], 0.5 * size[2] + 0.5 * top_size[2]]
    return np.concatenate([pins, _box_surface(rng, n_free - n_top, size, centre), _box_surface(rng, n_top, top_size, top_centre)])


def blob(rng, n, radius, centre):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (radius * rng.uniform(0, 1, size=(n, 1)) ** (1 / 3)) + np.asarray(centre, np.float64)


def beside(rng, origin, specs, gaps):
    """objects in a row along x from `origin` (the centre of the first): specs = [(n, size)], gaps = the minimum point distance between
    neighbours; every neighbouring pair has one designated pair of points, centre of the +x face against centre of the -x face.
    -> clouds, claims of all pairs of the row (by position in the row)"""
    origin = np.asarray(origin, np.float64)
    centres, x = [], origin[0]
    for k, (n, size) in enumerate(specs):
        if k:
            x += specs[k - 1][1][0] / 2 + gaps[k - 1] + size[0] / 2
        centres.append(np.array([x, origin[1], origin[2]]))
    clouds = []
    for k, (n, size) in enumerate(specs):
        pins = []
        if k > 0:
            pins.append(centres[k] - [size[0] / 2, 0, 0])
        if k + 1 < len(specs):
            pins.append(centres[k] + [size[0] / 2, 0, 0])
        clouds.append(thing(rng, n, size, centres[k], pins))
    claims = {}
    for a in range(len(specs)):
        for b in range(a + 1, len(specs)):
            d = sum(gaps[a:b]) + sum(specs[k][1][0] for k in range(a + 1, b))
            claims[(a, b)] = (d - 1e-5, d + 1e-5)
    return clouds, claims


def _pad(rows):
    return np.array([list(r) + [-1] * (3 - len(r)) for r in rows], dtype=np.int32).reshape(-1, 3)


class _Pool:
    """collects the detected clouds of a family and what every pair of them that shares a side was built for"""

    def __init__(self):
        self.det, self.claims = [], {}

    def add(self, clouds, claims=None):
        first = len(self.det)
        self.det += [np.asarray(c, np.float64).reshape(-1, 3) for c in clouds]
        for (a, b), rng_ in (claims or {}).items():
            self.claims[(first + a, first + b)] = rng_
        return list(range(first, first + len(clouds)))

    def far(self, a, b):
        self.claims[(min(a, b), max(a, b))] = (FAR, np.inf)

    def family(self, js, jt, tags, registers=None, center=True, job_ids=None):
        det32 = [c.astype(np.float32) for c in self.det]
        allp = np.concatenate([c for c in self.det if len(c)])
        centre = allp.mean(0)
        mem32 = [moved(c.astype(np.float64), centre, MOTION).astype(np.float32) for c in det32]
        ints = [intensity_of(c) for c in det32]
        js, jt = _pad(js), _pad(jt)
        J = len(js)
        fam = dict(det=det32, mem=mem32, det_int=ints, mem_int=[i.copy() for i in ints], js=js, jt=jt, tags=list(tags), center=center,
                   seed=SEED, max_iter=MAX_ITER, claims=dict(self.claims), centre=centre,
                   job_ids=(np.arange(J, dtype=np.uint32) + 11) if job_ids is None else np.asarray(job_ids, dtype=np.uint32),
                   registers=[bool(np.array_equal(js[j], jt[j]) and (js[j] >= 0).any()) for j in range(J)] if registers is None
                   else [bool(r) for r in registers])
        assert len(jt) == len(fam["tags"]) == len(fam["registers"]) == len(fam["job_ids"]) == J <= 12
        fam["_cache"] = {}
        return fam


def sides(fam):
    """-> [(pool, job, segment ids in slot order (-1 = empty slot))] in the product's order: the source sides, then the target sides"""
    J = len(fam["js"])
    return [(0, j, [int(s) for s in fam["js"][j]]) for j in range(J)] + [(1, j, [int(s) for s in fam["jt"][j]]) for j in range(J)]


def true_pose(fam, j):
    """the known motion between the clouds of job j as the product sees them (centred or not)"""
    from scipy.spatial.transform import Rotation
    R = Rotation.from_euler("xyz", MOTION[0], degrees=True).as_matrix()
    t = fam["centre"] - R @ fam["centre"] + np.asarray(MOTION[1])
    a = job_arrays(fam, j)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = R @ a["means"][0] + t - a["means"][1]
    return T


def oracle_pose(fam, j):
    """the oracle's registration of job j -> (T, rmse, fitness, T_ransac, stats), computed once"""
    from oracle import reg_oracle as ro
    key = ("oracle", j)
    if key not in fam["_cache"]:
        a = job_arrays(fam, j)
        raw = job_arrays(fam, j, center=False)
        fam["_cache"][key] = ro.register_point_clouds(a["src"], a["src_int"], a["tgt"], a["tgt_int"], VOXEL, GLOBAL, LOCAL, seed=fam["seed"],
                                                      job_id=int(fam["job_ids"][j]), ransac_max_iter=fam["max_iter"], src_raw=raw["src"],
                                                      tgt_raw=raw["tgt"])
    return fam["_cache"][key]


def rot_deg(A, B):
    return float(np.degrees(np.arccos(np.clip((np.trace(A[:3, :3].T @ B[:3, :3]) - 1) / 2, -1, 1))))


# ------------------------------------------------------------------------------------------------
# the plan, restated in float64 numpy
# ------------------------------------------------------------------------------------------------
def min_distance(A, B):
    """brute force: the least distance between a point of A and a point of B (float64 on the fp32 coordinates); inf when one is empty"""
    if len(A) == 0 or len(B) == 0:
        return np.inf
    A, B = A.astype(np.float64), B.astype(np.float64)
    best = np.inf
    for i0 in range(0, len(A), 512):
        d = A[i0:i0 + 512, None, :] - B[None, :, :]
        best = min(best, float(np.einsum("ijk,ijk->ij", d, d).min()))
    return float(np.sqrt(best))


def box_count(A, B, R):
    """points of B within R of the bounding box of A (an empty A has the box the product gives it: zeros)"""
    if len(B) == 0:
        return 0
    lo, hi = (A.astype(np.float64).min(0), A.astype(np.float64).max(0)) if len(A) else (np.zeros(3), np.zeros(3))
    b = B.astype(np.float64)
    gap = np.maximum(np.maximum(lo - b, b - hi), 0.0)
    return int(((gap * gap).sum(1) < R * R).sum())


def pair_facts(fam, pool, a, b):
    """-> (minimum point distance, points of the higher-numbered instance within R of the lower-numbered one's box) of two instances
    of a pool, after asserting that neither sits near its threshold"""
    lo, hi = min(a, b), max(a, b)
    key = ("pair", pool, lo, hi)
    if key not in fam["_cache"]:
        clouds = fam["mem" if pool else "det"]
        R, cap = near_rule(), kernel_constants()["NEAR_CAP"]
        d = min_distance(clouds[lo], clouds[hi])
        c = box_count(clouds[lo], clouds[hi], R)
        assert not (R * (1 - R_MARGIN) <= d <= R * (1 + R_MARGIN)), ("a pair on the radius", pool, lo, hi, d, R)
        assert not (cap * (1 - CAP_MARGIN) <= c <= cap * (1 + CAP_MARGIN)), ("a pair on NEAR_CAP", pool, lo, hi, c, cap)
        fam["_cache"][key] = (d, c)
    return fam["_cache"][key]


def is_near(fam, pool, a, b):
    """the rule: some point of one within R of some point of the other, or too many candidates to hold ("call it close")"""
    d, c = pair_facts(fam, pool, a, b)
    return d < near_rule() or c > kernel_constants()["NEAR_CAP"]


def dirty_slots(fam, pool, segs, have_features):
    """per slot of a side: None (empty slot), True (recomputed in the context of the side) or False (served from the instance features)"""
    out = []
    for a, sa in enumerate(segs):
        if sa < 0:
            out.append(None)
        elif not have_features:
            out.append(True)
        else:
            out.append(any(sb >= 0 and is_near(fam, pool, sa, sb) for b, sb in enumerate(segs) if b != a))
    return out


def plan_details(fam, features=(True, True)):
    """-> dict: stats (the six reuse statistics), dirty (per side the list of `dirty_slots`), groups (keys (pool, dirty instances in slot
    order) in the product's order: detected groups first), always_dirty ({pool: instances dirty in every side they appear in, and those
    that appear in none})"""
    key = ("plan", tuple(features))
    if key in fam["_cache"]:
        return fam["_cache"][key]
    size = lambda pool, s: len(fam["mem" if pool else "det"][s])
    S = sides(fam)
    J = len(fam["js"])
    groups = ([], [])
    dirty, sources = [], []
    cached = 0
    for pool, j, segs in S:
        ds = dirty_slots(fam, pool, segs, features[pool])
        dirty.append(ds)
        gkey = (pool,) + tuple(s for s, d in zip(segs, ds) if d)
        if len(gkey) > 1 and gkey not in groups[pool]:
            groups[pool].append(gkey)
        src, pos = [], 0
        for s, d in zip(segs, ds):
            if d is None:
                continue
            if d:
                src.append((("group", gkey, pos), size(pool, s)))      # the pos-th dirty instance of its group
                pos += 1
            else:
                src.append((("pool", pool, s), size(pool, s)))
                cached += size(pool, s)
        sources.append(src)
    all_groups = groups[0] + groups[1]
    recomputed = sum(size(g[0], s) for g in all_groups for s in g[1:])
    pairs, uses = set(), 0
    for sgi in range(2 * J):
        other = sgi + J if sgi < J else sgi - J
        for q, nq in sources[sgi]:
            for d, nd in sources[other]:
                if nq > 0 and nd > 0:
                    pairs.add((q, d))
                    uses += 1
    always = {}
    for pool in (0, 1):
        seen = {}
        for (pl, j, segs), ds in zip(S, dirty):
            if pl == pool:
                for s, d in zip(segs, ds):
                    if d is not None:
                        seen[s] = seen.get(s, True) and d
        always[pool] = [s for s in range(len(fam["det"])) if seen.get(s, True)]
    out = dict(stats=np.array([cached, recomputed, len(all_groups), 2 * J, len(pairs), uses], dtype=np.int64), dirty=dirty, groups=all_groups,
               always_dirty=always)
    fam["_cache"][key] = out
    return out


def plan(fam, features=(True, True)):
    """the expected reuse_stats[0..5] of a call whose pools carry instance features as `features` = (detected, memory) says: points
    served by the instance features, points recomputed, recomputed groups, job sides, distinct (query source, database source) pairs
    with points on both ends over both directions, pair uses"""
    return plan_details(fam, features)["stats"]


# ------------------------------------------------------------------------------------------------
# the oracle's features of an instance alone and in its side
# ------------------------------------------------------------------------------------------------
def oracle_features(pts, ints):
    from oracle import reg_oracle as ro
    if len(pts) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 33), np.float32), np.zeros((0, 3), np.float32)
    nrm = ro.normals(pts, NORMAL_RADIUS, NORMAL_NN)
    return nrm, ro.fpfh(pts, nrm, FPFH_RADIUS, FPFH_NN), ro.color_gradient(pts, nrm, ints, GRAD_RADIUS, GRAD_NN)


def rows_changed(fam, pool, segs, slot):
    """-> rows of the instance in `slot` of the side `segs` whose (normals, FPFH, gradients) in the side's concatenation differ from
    the instance's stand-alone values, by the oracle"""
    clouds, ints = (fam["mem"], fam["mem_int"]) if pool else (fam["det"], fam["det_int"])
    key = ("side", pool, tuple(segs))
    if key not in fam["_cache"]:
        ids = [s for s in segs if s >= 0]
        fam["_cache"][key] = oracle_features(np.concatenate([clouds[s] for s in ids]), np.concatenate([ints[s] for s in ids]))
    s = segs[slot]
    if ("alone", pool, s) not in fam["_cache"]:
        fam["_cache"][("alone", pool, s)] = oracle_features(clouds[s], ints[s])
    b = sum(len(clouds[t]) for t in segs[:slot] if t >= 0)
    return tuple(int((x[b:b + len(clouds[s])] != y).any(1).sum()) for x, y in zip(fam["_cache"][key], fam["_cache"][("alone", pool, s)]))


# ------------------------------------------------------------------------------------------------
# families
# ------------------------------------------------------------------------------------------------
BOX_A, BOX_B = (0.4, 0.3, 0.35), (0.3, 0.3, 0.3)
LONG_B = (0.7, 0.3, 0.3)               # the middle of a chain: its neighbours are more than R + margin apart


@memo
def threshold():
    """the radius itself.  Minimum point distances (detected pool; the memory pool is its rigid copy):
    0-1 0.58 (dirty by the rule)      2-3 0.62 (clean)      4-5 0.58, 5-6 0.62, 4-6 1.50 (4 and 5 dirty, 6 clean)"""
    rng = np.random.default_rng(401)
    p = _Pool()
    a = p.add(*beside(rng, (0, 0, 0), [(1200, BOX_A), (1000, BOX_B)], [0.58]))
    b = p.add(*beside(rng, (0, 4, 0), [(1200, BOX_A), (1000, BOX_B)], [0.62]))
    c = p.add(*beside(rng, (0, 8, 0), [(900, BOX_A), (800, BOX_B), (700, BOX_B)], [0.58, 0.62]))
    js = [a, b, c]
    return p.family(js, js, ["0.58 m: inside", "0.62 m: outside", "0.58 m then 0.62 m"])


@memo
def touching():
    """the only zone in which rows really change.  Minimum point distances:
    0-1 0.02      2-3 0.08 (sparser clouds: 700 / 650 points, so that a point's 30 nearest reach across)
    the chain 4-5 0.05, 5-6 0.03, 4-6 0.78 (4 touches 5, 5 touches 6, 4 is far from 6)"""
    rng = np.random.default_rng(402)
    p = _Pool()
    a = p.add(*beside(rng, (0, 0, 0), [(1200, BOX_A), (1000, BOX_B)], [0.02]))
    b = p.add(*beside(rng, (0, 4, 0), [(700, BOX_A), (650, BOX_B)], [0.08]))
    c = p.add(*beside(rng, (0, 8, 0), [(900, BOX_A), (1100, LONG_B), (800, BOX_B)], [0.05, 0.03]))
    js = [a, b, c, [c[0], c[2]], [c[1], c[2]], [b[1], b[0]]]
    return p.family(js, js, ["0.02 m", "0.08 m", "chain", "the ends of the chain: far", "the chain's second link", "0.08 m, other order"])


@memo
def grey_zone():
    """dirty by today's rule although no row changes.  Minimum point distances:
    0-1 0.30      2-3 0.45      4-5 0.30, 5-6 0.45, 4-6 1.45"""
    rng = np.random.default_rng(403)
    p = _Pool()
    a = p.add(*beside(rng, (0, 0, 0), [(1200, BOX_A), (1000, BOX_B)], [0.30]))
    b = p.add(*beside(rng, (0, 4, 0), [(1200, BOX_A), (1000, BOX_B)], [0.45]))
    c = p.add(*beside(rng, (0, 8, 0), [(900, BOX_A), (1100, LONG_B), (800, BOX_B)], [0.30, 0.45]))
    js = [a, b, c]
    return p.family(js, js, ["0.30 m", "0.45 m", "0.30 m then 0.45 m"])


def _straddled(rng, p, n_blob, blob_first, origin, satellites=0, half=1.0, radius=0.12):
    """A = two clusters 2 * half m apart, ONE instance; B = a blob of that radius in the empty middle of A's box, at least 0.73 m from
    every point of A (half - 0.15 - radius): a candidate by boxes, far by points.  satellites: that many of B's points in each of two small blobs off the axis (0.8 m
    from A), which widen B's box until points of A lie within R of it: the exact test has points to test whichever id is the lower"""
    o = np.asarray(origin, np.float64)
    A = np.concatenate([thing(rng, 600, BOX_B, o + [-half, 0, 0]), thing(rng, 600, BOX_B, o + [half, 0, 0])])
    B = np.concatenate([blob(rng, n_blob - 2 * satellites, radius, o), blob(rng, satellites, 0.05, o + [0.3, -0.8, 0]),
                        blob(rng, satellites, 0.05, o + [-0.3, 0.8, 0])])
    ids = p.add([B, A] if blob_first else [A, B])
    p.far(*ids)
    return ids


@memo
def boxes_only():
    """boxes that overlap while the points are far apart: served from the cache.  Minimum point distances: 0-1 and 2-3 at least 0.73 (the
    blob of 1 500 points -- 1 300 in the middle of the other instance's box, 100 + 100 in two satellites that widen its own).
    0 = the two clusters, 1 = the blob; 2 = the blob, 3 = the clusters: the kernel loads the higher id and sweeps the lower"""
    rng = np.random.default_rng(404)
    p = _Pool()
    js = [_straddled(rng, p, 1500, False, (0, 0, 0), 100), _straddled(rng, p, 1500, True, (0, 4, 0), 100)]
    return p.family(js, js, ["clusters swept, blob loaded", "blob swept, clusters loaded"])


@memo
def cap():
    """the geometry of `boxes_only` (clusters 3 m apart, a blob of radius 0.6 m: the same clearance at a density the oracle walks
    quickly) with more candidates than the kernel holds.  Minimum point distances at least 0.73 throughout.
    0-1 the blob (id 1) has NEAR_CAP + 900 points, all within R of the clusters' box: "too many to hold: call it close", recomputed
    2-3 NEAR_CAP - 600 points: the exact test runs, cached
    4-5 the blob of NEAR_CAP + 900 points has the LOWER id: what is counted are the clusters' points near the blob's box (none): cached"""
    rng = np.random.default_rng(405)
    c = kernel_constants()["NEAR_CAP"]
    p = _Pool()
    wide = dict(half=1.5, radius=0.6)
    js = [_straddled(rng, p, c + 900, False, (0, 0, 0), **wide), _straddled(rng, p, c - 600, False, (0, 4, 0), **wide),
          _straddled(rng, p, c + 900, True, (0, 8, 0), **wide)]
    return p.family(js, js, ["over the cap", "under the cap", "over the cap, counted from the other side"])


def _late(rng, p, late_higher, origin, gap=0.05):
    """A = a body of NEAR_SPLIT * 256 + 800 points and, 0.75 m from it, a plate of 100 points that come LAST; B = a box `gap` beyond the
    plate, 0.8 m from the body"""
    k = kernel_constants()
    o = np.asarray(origin, np.float64)
    body = thing(rng, k["NEAR_SPLIT"] * 256 + 800, BOX_A, o)
    x = 0.2 + 0.75                                                   # the plate's plane
    plate = np.concatenate([[[x, 0, 0]], np.c_[np.full(99, x), rng.uniform(-0.05, 0.05, size=(99, 2))]]) + o
    B = thing(rng, 1000, BOX_B, o + [x + gap + 0.15, 0, 0], pins=[o + [x + gap, 0, 0]])
    ids = p.add([B, np.concatenate([body, plate])] if late_higher else [np.concatenate([body, plate]), B])
    p.claims[(ids[0], ids[1]) if ids[0] < ids[1] else (ids[1], ids[0])] = (gap - 1e-5, gap + 1e-5)
    return ids


@memo
def late_hit():
    """a hit that only a later sweep of the swept instance's points meets.  Minimum point distances: 0-1 and 2-3 0.05, between the
    LAST 100 points (by index) of the instance of NEAR_SPLIT * 256 + 900 points and the box beside them; its first NEAR_SPLIT * 256 + 800
    points are 0.8 m away or more.  0 = the large instance (swept: the hit is in the second sweep of one block), 1 = the box;
    2 = the box, 3 = the large instance (loaded: its near points are the last it reads)"""
    rng = np.random.default_rng(406)
    p = _Pool()
    js = [_late(rng, p, False, (0, 0, 0)), _late(rng, p, True, (0, 4, 0))]
    return p.family(js, js, ["late points swept", "late points loaded"])


@memo
def partial():
    """one clean and two dirty instances in a side.  Minimum point distances: 0-1 (A-B) 0.04, 0-2 (A-C) and 1-2 (B-C) at least 1.5.
    Sides [A, C, B] (C cached in the middle, group (A, B)), [A, B, -1] (the same group again) and [B, A, -1] (a second group: the order
    of a concatenation decides index ties)"""
    rng = np.random.default_rng(407)
    p = _Pool()
    A, B = p.add(*beside(rng, (0, 0, 0), [(1200, BOX_A), (1000, BOX_B)], [0.04]))
    (C,) = p.add([thing(rng, 900, BOX_A, (0, 2.0, 0))])
    p.far(A, C)
    p.far(B, C)
    js = [[A, C, B], [A, B], [B, A]]
    return p.family(js, js, ["[A, C, B]", "[A, B, -1]", "[B, A, -1]"])


@memo
def mixed_use():
    """an instance that is clean in one job and dirty in another job of the same call.  Minimum point distances: 0-1 (A-B) 0.04.
    Jobs [A] (A from the cache), [A, B] (both recomputed), [B] (B from the cache)"""
    rng = np.random.default_rng(408)
    p = _Pool()
    A, B = p.add(*beside(rng, (0, 0, 0), [(1200, BOX_A), (1000, BOX_B)], [0.04]))
    js = [[A], [A, B], [B]]
    return p.family(js, js, ["A alone", "A beside B", "B alone"])


@memo
def degenerate():
    """duplicated, empty and tiny instances, empty slots, empty sides.  Instances: 0 = A (800 points, its box reaches to 0.2 m from the
    origin, where the box of an empty instance lies), 1 = B (700), 2 = E (0 points), 3 = F and 4 = G (600 each, 5 m from the origin),
    5 = P1 (1 point), 6 = P2 (2 points).  Minimum point distances: A-A 0 (an instance is always near its own copy), A-B 0.04, F-G 0.04,
    P1-A 0.05, P2-A 0.9; every pair with E: none (inf)"""
    rng = np.random.default_rng(409)
    p = _Pool()
    A, B = p.add(*beside(rng, (0.4, 0, 0), [(800, BOX_A), (700, BOX_B)], [0.04]))
    (E,) = p.add([np.zeros((0, 3))])
    F, G = p.add(*beside(rng, (5.0, 3.0, 0), [(600, BOX_A), (600, BOX_B)], [0.04]))
    (P1,) = p.add([np.array([[0.4 - 0.2 - 0.05, 0.0, 0.0]])])                       # 0.05 m off the centre of A's -x face ...
    p.det[A][5] = [0.2, 0.0, 0.0]                                                   # ... where A gets a point
    p.claims[(A, P1)] = (0.05 - 1e-5, 0.05 + 1e-5)
    (P2,) = p.add([np.array([[0.4, 0.9 + 0.15, 0.0], [0.42, 0.9 + 0.15, 0.01]])])   # 0.9 m off the centre of A's +y face ...
    p.det[A][6] = [0.4, 0.15, 0.0]                                                  # ... where A gets a point
    p.claims[(A, P2)] = (0.9 - 1e-5, 0.9 + 1e-5)
    p.claims[(A, A)] = (0.0, 0.0)
    for x in (A, B, F, G):
        p.claims[(min(x, E), max(x, E))] = (np.inf, np.inf)
    js = [[A, A], [A, B, A], [E, A], [A, E, B], [F, G, E], [E, F], [P1, A], [A, P2], [-1, A, -1], [A, -1, B], [-1, -1, -1], [A]]
    jt = js[:10] + [[A], [-1, -1, -1]]
    tags = ["[A, A, -1]", "[A, B, A]", "empty first, near the origin", "empty in the middle", "empty last, far from the origin",
            "empty first, far from the origin", "1 point beside A", "2 points far from A", "[-1, A, -1]", "[A, -1, B]", "empty source side",
            "empty target side"]
    return p.family(js, jt, tags, registers=[True] * 10 + [False, False])


@memo
def both_pools():
    """groups on the detected and on the memory pool in one call: detected groups come first, memory groups carry gradients.  Minimum
    point distances: 0-1 0.03; the chain 2-3 0.05, 3-4 0.04, 2-4 0.79; 5-6 0.06.  Five groups on the detected pool ((0, 1), (2, 3, 4), (5, 6),
    (3, 4), (2, 3)) of 1 350 to 3 150 points and, through the two jobs whose sides list different instances, another set of four on the
    memory pool ((0, 1), (2, 3, 4), (5, 6), (2, 3))"""
    rng = np.random.default_rng(410)
    p = _Pool()
    a = p.add(*beside(rng, (0, 0, 0), [(750, BOX_A), (600, BOX_B)], [0.03]))
    b = p.add(*beside(rng, (0, 4, 0), [(1050, BOX_A), (1200, LONG_B), (900, BOX_B)], [0.05, 0.04]))
    c = p.add(*beside(rng, (0, 8, 0), [(1500, BOX_A), (1350, BOX_B)], [0.06]))
    js = [a, b, c, [b[1], b[2]], [a[0]], [b[0], b[1]]]
    jt = [a, b, c, [b[0], b[1]], [a[0], a[1]], [b[0], b[1]]]
    tags = ["2 instances", "3 instances", "2 larger instances", "other links of the chain on the two sides", "A onto A and its neighbour",
            "the chain's first link"]
    return p.family(js, jt, tags, registers=[True, True, True, False, False, True])


FAMILIES = {"threshold": threshold, "touching": touching, "grey_zone": grey_zone, "boxes_only": boxes_only, "cap": cap, "late_hit": late_hit,
            "partial": partial, "mixed_use": mixed_use, "degenerate": degenerate, "both_pools": both_pools}


# ------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------
def batches(fam):
    from ibloc_amd.registration import CloudBatch
    return CloudBatch.from_numpy(fam["det"], fam["det_int"]), CloudBatch.from_numpy(fam["mem"], fam["mem_int"])


def features(ctx, det, mem, compact=False):
    """-> (detected features, memory features): the memory features with the gradients the coloured ICP reads; compact: the memory
    features without their resident fp16 operands"""
    from ibloc_amd.registration import instance_features_batch
    return instance_features_batch(ctx, det, VOXEL), instance_features_batch(ctx, mem, VOXEL, grad_radius=GRAD_RADIUS, compact=compact)


def poisoned(feat, batch, segments):
    """a copy of the features in which every row of the instances `segments` is NaN in every device array; the boxes stay"""
    from ibloc_amd.registration import InstanceFeatures
    arrays = {name: (None if getattr(feat, name) is None else getattr(feat, name).clone()) for name in InstanceFeatures.DEVICE_ARRAYS}
    rows = 0
    for s in segments:
        b, e = int(batch.seg_off_host[s]), int(batch.seg_off_host[s + 1])
        rows += e - b
        for a in arrays.values():
            if a is not None:
                a[b:e] = float("nan")
    out = InstanceFeatures(arrays["normals"], arrays["fpfh"], arrays["fpfh_split"], arrays["fpfh_norm"], arrays["grad"], feat.bbox.copy(),
                           feat.voxel_size, feat.grad_radius, n=feat.n, n_seg=feat.n_seg)
    return out, rows


def run(ctx, fam, det, mem, fd=None, fm=None, jobs=None):
    """one register_batch call: all jobs of the family, or only `jobs` (with their own job ids)"""
    from ibloc_amd.registration import register_batch
    sel = np.arange(len(fam["js"])) if jobs is None else np.asarray(jobs, dtype=np.int64)
    return register_batch(ctx, det, mem, fam["js"][sel], fam["jt"][sel], VOXEL, GLOBAL, LOCAL, seed=fam["seed"], ransac_max_iter=fam["max_iter"],
                          have_colors=True, center=fam["center"], det_features=fd, mem_features=fm, job_ids=fam["job_ids"][sel])
