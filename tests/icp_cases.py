"""Deterministic job sets for the ICP stage alone (csrc/reg_icp.hip), shared by tests/test_icp_model.py (CPU: the oracle shows that
every family exercises the path it exists for) and tests/test_gpu_icp.py (GPU: the stage against `oracle.reg_oracle.icp`, job by job).

A family is a dict
    det, mem          lists of (n, 3) float32 clouds: the two pools a `register_batch` call sees
    det_int, mem_int  lists of (n,) float32 intensities (coloured families) or None
    js, jt            (J, 3) int32: per job the source / target instances, padded with -1 (an empty slot may sit in the middle)
    center            whether the family is run with center=True
    tags              per job a short name of what the job is there for
`job_arrays(fam, j)` gives the job's concatenated float32 source and target in slot order -- the order the oracle's tie rule
(lowest index among equal fp32 distances) is defined on -- after the centring the product applies.

Sources and targets are DIFFERENT samplings of an object: a detection from `SynthWorld.make_frame`, brought back into the world frame
by the frame's pose and then moved by a known rigid offset about the object's centre, against the memory cloud.  (Rigid copies
converge in 5-13 iterations to rmse ~ 1e-9 and exercise little.)  Oracle iterations of the point-to-point estimator at voxel 0.05,
local_dist_factor 1.5 (reach 0.075 m) on 3000-point objects: SMALL 18-21, MEDIUM 25-30, SHIFT 30 (never converges)."""
import numpy as np
from scipy.spatial.transform import Rotation

from ibloc_amd.synth import SynthWorld

VOXEL = 0.05
LOCAL = 1.5
GLOBAL = 1.5
REACH = VOXEL * LOCAL                    # ICP correspondence distance
GROUP_FROM = 8                           # ICP_GROUP_FROM: first iteration of the grouped search and of the active-job lists
ACT_Y = 32                               # ICP_ACT_Y: block rows that walk the active-job list
STEP_STRIDE = 8 * 256                    # ICP_BPJ * 256: one stride of the step kernel over a source side

IDENTITY = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
SMALL = ((3.0, -2.0, 2.0), (0.02, -0.02, 0.01))
MEDIUM = ((8.0, -6.0, 5.0), (0.05, -0.04, 0.03))
SHIFT = ((0.0, 0.0, 0.0), (0.4, 0.0, 0.0))
_NAMES = {IDENTITY: "identity", SMALL: "small", MEDIUM: "medium", SHIFT: "shift"}
SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 700, 1500, 3000)

_cache = {}


def _memo(fn):
    def wrapped(*args):
        key = (fn.__name__,) + args
        if key not in _cache:
            _cache[key] = fn(*args)
        return _cache[key]
    wrapped.__name__ = fn.__name__
    wrapped.__doc__ = fn.__doc__
    return wrapped


def intensity(colors):
    return ((colors[:, 0] + colors[:, 1] + colors[:, 2]) / 3.0).astype(np.float32)


def moved(pts, centre, offset):
    """the cloud turned by offset[0] (xyz Euler angles, degrees) about `centre` and shifted by offset[1], in fp64"""
    R = Rotation.from_euler("xyz", offset[0], degrees=True).as_matrix()
    return (np.asarray(pts, np.float64) - centre) @ R.T + centre + np.asarray(offset[1])


def thinned(pts, n):
    """n rows spread evenly over the cloud (its rows are ordered primitive by primitive: a leading block would be one face)"""
    return pts[(np.arange(n) * len(pts)) // max(n, 1)] if n < len(pts) else pts


@_memo
def _world(seed, spacing, pts=3000):
    return SynthWorld(9, pts_per_object=pts, E=1, D=8, seed=seed, spacing=spacing)


@_memo
def _frames(seed, spacing, n_frames, pts):
    """n_frames detections of all nine objects, every cloud back in the world frame: (frame, object) -> (points fp64, colours)"""
    w = _world(seed, spacing, min(pts, 3000))
    rng = np.random.default_rng(seed + 1000)
    out = []
    for _ in range(n_frames):
        f = w.make_frame(rng, q=9, pts_per_object=pts, anchor=4)
        R, t = f["pose"][:3, :3], f["pose"][:3, 3]
        clouds = {}
        for k, (pc, col) in zip(f["ids"], f["clouds"]):
            clouds[k] = (pc @ R.T + t, col)
        out.append(clouds)
    return out


def _pad(rows):
    return np.array([list(r) + [-1] * (3 - len(r)) for r in rows], dtype=np.int32).reshape(-1, 3)


def _family(det, mem, js, jt, tags, center=False, det_int=None, mem_int=None, **extra):
    f32 = lambda L: [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3) for c in L]
    fam = dict(det=f32(det), mem=f32(mem), det_int=det_int, mem_int=mem_int, js=_pad(js), jt=_pad(jt), tags=list(tags), center=center)
    fam.update(extra)
    assert len(fam["js"]) == len(fam["jt"]) == len(fam["tags"])
    return fam


def job_arrays(fam, j, center=None):
    """-> dict src, tgt (float32, slot order, centred as the product centres them), src_int, tgt_int, means (2, 3) fp64, tgt_rows (for
    every target row its (instance, row in the instance): the rows of instance features that belong to it)"""
    center = fam["center"] if center is None else center
    out = {}
    for side, pool, ints, seg in (("src", fam["det"], fam["det_int"], fam["js"][j]), ("tgt", fam["mem"], fam["mem_int"], fam["jt"][j])):
        ids = [int(s) for s in seg if s >= 0]
        cat = np.concatenate([pool[s] for s in ids]) if ids else np.zeros((0, 3), np.float32)
        mean = cat.astype(np.float64).mean(0) if (center and len(cat)) else np.zeros(3)
        out[side] = (cat.astype(np.float64) - mean).astype(np.float32)
        out[side + "_int"] = None if ints is None else (np.concatenate([ints[s] for s in ids]) if ids else np.zeros(0, np.float32))
        out[side + "_mean"] = mean
        out[side + "_rows"] = [(s, len(pool[s])) for s in ids]
    out["means"] = np.stack([out.pop("src_mean"), out.pop("tgt_mean")])
    return out


def sub_family(fam, jobs, center=None):
    """the same pools with only `jobs`, optionally with another centring switch"""
    sub = dict(fam)
    sub["js"], sub["jt"] = fam["js"][list(jobs)], fam["jt"][list(jobs)]
    sub["tags"] = [fam["tags"][j] for j in jobs]
    if center is not None:
        sub["center"] = center
    return sub


# ------------------------------------------------------------------------------------------------
# point-to-point families (register_batch(..., have_colors=False): the ICP stage from the identity, nothing in front of it)
# ------------------------------------------------------------------------------------------------
P2P_SEED = 51
P2P_SPACING = 1.0          # objects 1 m apart: a multi-instance side turned by a few degrees about its centre stays within reach

# (source size, offset) of the ordinary jobs of `many_jobs`; the special jobs are appended behind them
_ROUND = [(3000, SMALL), (3000, MEDIUM), (3000, SHIFT), (1500, SMALL), (1500, MEDIUM), (700, SMALL), (700, MEDIUM), (257, SMALL),
          (256, SMALL), (255, SMALL), (65, SMALL), (64, SMALL), (63, MEDIUM)]
_MANY = _ROUND + _ROUND + _ROUND[:8]


@_memo
def many_jobs():
    """40 jobs in one call: more than ICP_ACT_Y = 32 of them still run at iteration 8 (the active-job list is walked with a stride) and
    fewer later (walked without); sources of every size class of the kernels (a group of 8 lanes, a wave, a block of 256 +- 1, several
    blocks), the three offsets and the identity, and the degenerate jobs: empty source, empty target, no target within reach, a single
    target point"""
    w = _world(P2P_SEED, P2P_SPACING)
    frames = _frames(P2P_SEED, P2P_SPACING, 4, 3000)
    det, js, jt, tags = [], [], [], []
    mem = [p for p in w.points]

    def add(src, tgt_ids, tag):
        det.append(src)
        js.append([len(det) - 1])
        jt.append(tgt_ids)
        tags.append(tag)

    for i, (n, off) in enumerate(_MANY):
        k = i % 9
        pts = thinned(frames[i // 9][k][0], n)
        add(moved(pts, w.objects[k].world_center, off), [k], "%d/%s" % (n, _NAMES[off]))
    add(frames[3][5][0], [5], "3000/identity")
    add(thinned(frames[3][1][0], 1500), [1], "1500/identity")
    add(np.zeros((0, 3)), [1], "empty source")
    mem.append(np.zeros((0, 3)))
    add(thinned(frames[3][2][0], 1), [len(mem) - 1], "empty target")
    add(thinned(frames[3][0][0], 2), [8], "unreachable")                  # object 8 is 2.8 m from object 0
    m0 = w.points[3][1234]
    mem.append(m0[None])
    d3 = frames[3][3][0]
    near = np.argsort(((d3 - m0) ** 2).sum(1), kind="stable")[:3]
    add(d3[np.sort(near)], [len(mem) - 1], "single target point")
    return _family(det, mem, js, jt, tags)


@_memo
def pieces():
    """sides of 2 and 3 instances: the minimum of the neighbour search is carried from one target piece to the next.  Apart: the
    instances of the side are different objects.  Overlapping: the target pieces are samplings of ONE object shifted by 2 cm against
    each other, so the nearest neighbour of many sources lies in the second or third piece.  One job leaves its middle slot empty."""
    w = _world(P2P_SEED, P2P_SPACING)
    frames = _frames(P2P_SEED, P2P_SPACING, 4, 3000)
    rng = np.random.default_rng(P2P_SEED + 7)
    mem = [p for p in w.points]
    for shift in ((0.02, 0.0, 0.0), (0.0, -0.014, 0.014)):                 # further samplings of object 4, 2 cm off
        mem.append(w.objects[4].sample(3000, rng)[0] + np.asarray(shift))
    det, js, jt, tags = [], [], [], []

    def group(ids, frame, off):
        centre = np.mean([w.objects[k].world_center for k in ids], axis=0)
        first = len(det)
        for k in ids:
            det.append(moved(frames[frame][k][0], centre, off))
        return list(range(first, first + len(ids)))

    js.append(group([0, 1], 0, SMALL)); jt.append([0, 1]); tags.append("apart 2+2")
    js.append(group([3, 4, 5], 1, SMALL)); jt.append([3, 4, 5]); tags.append("apart 3+3")
    s = group([6, 7], 3, MEDIUM)
    js.append([s[0], -1, s[1]]); jt.append([6, -1, 7]); tags.append("middle slot empty")
    first = len(det)
    for fr in (0, 1):
        det.append(moved(frames[fr][4][0], w.objects[4].world_center, SMALL))
    js.append([first, first + 1]); jt.append([4, 9]); tags.append("overlap 2+2")
    first = len(det)
    for fr in (2, 3, 0):
        det.append(moved(thinned(frames[fr][4][0], 2000), w.objects[4].world_center, MEDIUM))
    js.append([first, first + 1, first + 2]); jt.append([4, 9, 10]); tags.append("overlap 3+3")
    return _family(det, mem, js, jt, tags)


@_memo
def long_side():
    """one job whose source side (5000 points) is longer than one stride of the step kernel (ICP_BPJ * 256 = 2048) and spans 20 chunks"""
    w = _world(P2P_SEED, P2P_SPACING)
    f = _frames(P2P_SEED, P2P_SPACING, 1, 5000)[0]
    return _family([moved(f[2][0], w.objects[2].world_center, SMALL)], [w.points[2]], [[0]], [[0]], ["5000/small"])


TIE_PITCH = 31.0 / 1024.0          # 0.0303 m: the pitch nearest to 0.03 m whose lattice sites and cell midpoints are exact in fp32


def _lattice(order_seed):
    i, j, k = np.meshgrid(np.arange(20), np.arange(20), np.arange(3), indexing="ij")
    pts = np.stack([i.ravel(), j.ravel(), k.ravel()], 1) * TIE_PITCH
    return pts[np.random.default_rng(order_seed).permutation(len(pts))]


@_memo
def ties():
    """equal fp32 distances.  Job 0: the target is a 20 x 20 x 3 lattice in shuffled row order, the source the midpoints of its cells
    turned by 2 degrees IN the lattice plane: z stays exactly half-way between two layers, so for every source point the nearest
    site of the layer below and the one of the layer above are at the same fp32 distance, and "lowest original index" decides the
    layer.  The Kabsch step of that iteration moves the source out of the mid-planes; later iterations are ordinary.  Job 1: the same
    source against a target in which every site is present twice (a tie at every iteration)."""
    tgt = _lattice(5)
    i, j, k = np.meshgrid(np.arange(19), np.arange(19), np.arange(2), indexing="ij")
    mid = (np.stack([i.ravel(), j.ravel(), k.ravel()], 1) + 0.5) * TIE_PITCH
    c = np.array([9.5, 9.5, 0.0]) * TIE_PITCH
    R = Rotation.from_euler("z", 2.0, degrees=True).as_matrix()
    src = (mid - c) @ R.T + c
    src[:, 2] = mid[:, 2]                                                   # (exact)
    assert np.array_equal(src[:, 2].astype(np.float32).astype(np.float64), mid[:, 2])
    twice = np.concatenate([tgt, tgt])[np.random.default_rng(6).permutation(2 * len(tgt))]
    return _family([src], [tgt, twice], [[0], [0]], [[0], [1]], ["lattice", "every site twice"])


def ties_reversed():
    """`ties` with the rows of both targets in reverse order: the same point sets, another lowest index"""
    fam = dict(ties())
    fam["mem"] = [m[::-1].copy() for m in fam["mem"]]
    return fam


LATE_D = 2.0 ** -4          # 0.0625 m: the pull on the back face of `late_ties`, inside the reach
LATE_TIE_AT = (8, 10)       # iterations at which the two jobs of `late_ties` meet their tie


def _late_tie_job(m):
    """-> (source (8, 3), target) of a job whose arithmetic is exact, so that a tie between two DIFFERENT points can be placed at
    iteration m.  The source is the eight corners of a box.  Every back corner (x = -a) has one target, LATE_D further along x; every
    front corner has a chain of targets along x at x_n = LATE_D (1 - 2^-n), n < m, and one at LATE_D.  All coordinates are small
    binary fractions, the cross-covariance is exactly diagonal, so every update is a pure shift along x by the mean residual: at
    iteration n < m the front corners sit on their site x_n, the back corners are e_n = LATE_D 2^-n short, and the shift is e_n / 2.
    At iteration m the front corners sit on no site: x_(m-1) behind and LATE_D ahead are both exactly e_m away.  The rows of LATE_D come
    BEHIND the chain, so the lowest index is the site behind: the residuals cancel, the shift is zero, the same tie comes back at
    iteration m + 1 and the job ends e_m short of LATE_D.  The other choice ends on LATE_D.  (Behind the chain also because the cell
    order then puts the two tied rows next to each other, where one lane of the grouped search meets both.)"""
    a, b, c = 0.25, 0.3125, 0.375
    src, ahead, back, chain = [], [], [], []
    for sy in (-1, 1):
        for sz in (-1, 1):
            src.append([-a, sy * b, sz * c])
            back.append([-a + LATE_D, sy * b, sz * c])
    for sy in (-1, 1):
        for sz in (-1, 1):
            src.append([a, sy * b, sz * c])
            ahead.append([a + LATE_D, sy * b, sz * c])
            chain += [[a + LATE_D * (1.0 - 2.0 ** -n), sy * b, sz * c] for n in range(m)]
    tgt = np.array(back + chain + ahead)
    assert np.array_equal(tgt.astype(np.float32).astype(np.float64), tgt)
    return np.array(src), tgt


@_memo
def late_ties():
    """ties between points at different coordinates in the GROUPED search: from iteration 8 (its first) and from iteration 10 on; see
    _late_tie_job.  (The ties of `ties` job 0 all fall in iteration 0, and those of its job 1 are between coincident points.)"""
    jobs = [_late_tie_job(m) for m in LATE_TIE_AT]
    return _family([j[0] for j in jobs], [j[1] for j in jobs], [[0], [1]], [[0], [1]], ["tie at iteration %d" % m for m in LATE_TIE_AT])



def late_ties_reordered():
    """`late_ties` with the rows of the site ahead IN FRONT of the chain: the same point sets, another lowest index"""
    fam = dict(late_ties())
    fam["mem"] = [np.concatenate([m[-4:], m[:-4]]) for m in fam["mem"]]
    return fam


@_memo
def few_sources():
    """sources of ONE point against a whole object within reach: every correspondence from one source point, the Kabsch step of
    rank 0 with cnt > 0.  (A two-point source has no place here: its rotation about the line through the two points is free, and the
    oracle's own answer moves by 1.7 when the start moves by 1e-13.)"""
    w = _world(P2P_SEED, P2P_SPACING)
    frames = _frames(P2P_SEED, P2P_SPACING, 4, 3000)
    det = [moved(thinned(frames[3][k][0], 1), w.objects[k].world_center, off) for k, off in ((6, SMALL), (7, MEDIUM))]
    return _family(det, [w.points[6], w.points[7]], [[0], [1]], [[0], [1]], ["1/small", "1/medium"])


@_memo
def centred():
    """two jobs of the families above with center=True: the means path (sides moved to their centroids before the stage)"""
    a, b = many_jobs(), pieces()
    det = [a["det"][0], a["det"][4]] + [b["det"][s] for s in b["js"][1]]
    mem = [a["mem"][0], a["mem"][4]] + [b["mem"][s] for s in b["jt"][1]]
    return _family(det, mem, [[0], [2, 3, 4]], [[0], [2, 3, 4]], ["3000/small", "apart 3+3"], center=True)


P2P_FAMILIES = {"many_jobs": many_jobs, "pieces": pieces, "long_side": long_side, "ties": ties, "late_ties": late_ties, "few_sources": few_sources,
                "centred": centred}


# ------------------------------------------------------------------------------------------------
# coloured families (register_batch(..., have_colors=True, center=True, det_features=fd, mem_features=fm))
# ------------------------------------------------------------------------------------------------
COL_SEED = 61
COL_PTS = 2000
COL_SPACING = 2.5          # every instance further than the influence radius from the next: all features come from the cache


@_memo
def coloured():
    """eight jobs on a world whose instances are all served from the feature cache, so the target normals and gradients the stage reads
    are the rows of the memory's instance features: three correct single-instance jobs, one of 2 and one of 3 instances, and three
    wrong assignments (they keep the ICP running into the grouped search)"""
    w = _world(COL_SEED, COL_SPACING, COL_PTS)
    f = _frames(COL_SEED, COL_SPACING, 1, COL_PTS)[0]
    ids = [4, 0, 1, 2, 3, 5]
    det = [f[k][0] for k in ids]
    det_int = [intensity(f[k][1]) for k in ids]
    mem = [p for p in w.points]
    mem_int = [intensity(c) for c in w.colors]
    js = [[0], [1], [2], [0, 1], [2, 3, 4], [0], [1], [5]]
    jt = [[4], [0], [1], [4, 0], [1, 2, 3], [0], [7], [6]]
    tags = ["correct"] * 3 + ["correct 2", "correct 3"] + ["wrong"] * 3
    return _family(det, mem, js, jt, tags, center=True, det_int=det_int, mem_int=mem_int)


COL_SEED_RANSAC = 5
COL_JOB_ID_BASE = 20


# ------------------------------------------------------------------------------------------------
# the oracle on one job
# ------------------------------------------------------------------------------------------------
def oracle_p2p(fam, j, T0=None):
    """-> (T, fitness, rmse, iterations) of the point-to-point estimator from T0 (identity)"""
    from oracle import reg_oracle as ro
    a = job_arrays(fam, j)
    return ro.icp(a["src"], None, a["tgt"], None, None, None, REACH, np.eye(4) if T0 is None else T0, colored=False)


def oracle_coloured(fam, j, nrm, grad, T0, lambda_geometric=0.968):
    """-> (T, fitness, rmse, iterations) of the coloured estimator from T0 with the given target normals and gradients (n, 3)"""
    from oracle import reg_oracle as ro
    a = job_arrays(fam, j)
    return ro.icp(a["src"], a["src_int"], a["tgt"], nrm, a["tgt_int"], grad, REACH, T0, colored=True, lambda_geometric=lambda_geometric)


def perturbed(T0, k):
    """start k of the conditioning check: the rotation and translation entries of T0 moved by up to 1e-13"""
    T = np.array(T0, dtype=np.float64)
    T[:3, :] += np.random.default_rng(900 + k).uniform(-1.0, 1.0, size=(3, 4)) * 1e-13
    return T
