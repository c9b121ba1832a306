"""Deterministic inputs for the whole-memory evaluation alone (`ibl_evaluate_kernel`, csrc/reg_eval.hip), shared by
tests/test_evaluate_model.py (CPU: the references alone show that every family does what it is there for) and
tests/test_gpu_evaluate.py (GPU: every point of every family against the brute force).

A family is a dict
    name       its name
    mem        (n, 3) float32: the memory points the grid is built from
    det        (m, 3) float32: one detection array
    jb, je     (J,) int32: per job the half-open range of `det` it evaluates
    T          (J, 4, 4) float64: per job the transform applied to its points
    cell, thr  the grid's cell and the evaluation's threshold
    tags       per job a short name of what the job is there for
`reference(fam)` gives, jobs back to back in the layout of `evaluate_points`,
    d2, idx    `oracle.reg_oracle.nearest_bruteforce`: the fp32 rule with no grid (float32, +inf / -1 when none)
    d2_64      the fp64 truth: squared distance of the fp32-rounded transformed point to its nearest memory point (cKDTree on the
               fp32 values widened to double, as oracle/open3d_fp64.py does), thresholded nowhere
    q          the fp32-rounded transformed points, off the job offsets, ns the job sizes
and `in_band(fam, ref)` the points whose fp64 distance lies within 2^-20 (relative, squared) of the threshold: there, and only
there, the fp32 rule and fp64 may decide differently (each difference is rounded once -- 2^-24 relative, doubled by the square --
and dist2f rounds three times: less than 2^-21 in all)."""
import numpy as np
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

CELL, THR = 0.04, 0.02                  # the product's: 4 cm cells, evaluation at 2 cm
BAND = 2.0 ** -20
BASES = {"origin": (0.0, 0.0, 0.0), "mid": (241.37, -229.91, 3.03), "far": (-4000.5, 3999.7, 12.3)}
RATIOS = ((0.04, 0.02), (0.02, 0.02), (0.05, 0.02), (0.01, 0.02), (0.04, 0.04))
JOB_SIZES = (0, 1, 255, 256, 257, 2047, 2048, 2049, 5000)
OCCUPANCIES = (1, 2, 3, 4, 5, 8, 9)
BIG_CELL = 3000
F32 = np.float32

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


def rigid(euler_deg, shift, centre=(0.0, 0.0, 0.0)):
    """4 x 4 double: a turn by the xyz Euler angles about `centre`, then a shift"""
    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("xyz", euler_deg, degrees=True).as_matrix()
    c = np.asarray(centre, np.float64)
    T[:3, 3] = c - T[:3, :3] @ c + np.asarray(shift, np.float64)
    return T


def shifted(shift):
    return rigid((0, 0, 0), shift)


def _family(name, mem, det, jobs, cell, thr):
    """jobs: (begin, end, T, tag) each"""
    return dict(name=name, mem=np.ascontiguousarray(mem, F32), det=np.ascontiguousarray(det, F32),
                jb=np.array([j[0] for j in jobs], np.int32), je=np.array([j[1] for j in jobs], np.int32),
                T=np.stack([np.asarray(j[2], np.float64) for j in jobs]), cell=cell, thr=thr, tags=[j[3] for j in jobs])


# ---- slab / ratios -------------------------------------------------------------------------------------------------------------
def _slab_clouds(base, cell, seed):
    """a noisy slab plus a lattice; queries near memory points, snapped to cell faces and corners, and mostly outliers"""
    rng = np.random.default_rng(seed)
    base = np.asarray(base, np.float64)
    mem = (rng.uniform(-0.4, 0.4, size=(60000, 3)) * [1, 1, 0.02] + base).astype(F32)
    lattice = (np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), -1).reshape(-1, 2) * 0.01 + base[:2] + 0.5).astype(F32)
    mem = np.concatenate([mem, np.concatenate([lattice, np.full((len(lattice), 1), base[2], F32)], 1)])
    det = np.concatenate([mem[rng.integers(0, len(mem), 20000)] + rng.normal(0, 0.004, size=(20000, 3)).astype(F32),
                          (np.round(mem[rng.integers(0, len(mem), 4000)] / F32(cell)) * F32(cell)).astype(F32),
                          (rng.uniform(-1, 1, size=(4000, 3)) + base).astype(F32)])
    return mem, det


@_memo
def slab(base_name, cell=CELL, thr=THR, seed=91):
    """the slab at one of BASES ("origin" straddles all eight sign octants): every point under the identity, the back half (near,
    snapped and outlying queries alike) under a small rigid motion about the base, and an empty job"""
    base = BASES[base_name]
    mem, det = _slab_clouds(base, cell, seed)
    n = len(det)
    jobs = [(0, n, np.eye(4), "identity"), (15000, n, rigid((0.4, -0.3, 0.5), (0.013, -0.007, 0.004), base), "small motion"),
            (5, 5, np.eye(4), "empty")]
    return _family(f"slab_{base_name}" if (cell, thr) == (CELL, THR) else f"ratio_{cell}_{thr}", mem, det, jobs, cell, thr)


def ratios(i):
    """the slab near the origin under RATIOS[i] = (cell, thr): the product's, thr = cell, thr < cell / 2, thr = 2 cell (a box of up to
    5^3 cells) and both doubled"""
    return slab("origin", *RATIOS[i])


# ---- jobs -----------------------------------------------------------------------------------------------------------------------
@_memo
def jobs(single=False):
    """one detection array of 12 000 points; ranges of JOB_SIZES points that begin mid-array, overlap and repeat, an empty job first,
    in the middle and last, transforms in turn (identity, small motion, a 90 degree turn about z, a shift out of reach)"""
    mem, det = _slab_clouds(BASES["origin"], CELL, 17)
    det = np.concatenate([det[:8000], det[20000:24000]])[np.random.default_rng(18).permutation(12000)]
    tf = dict(identity=np.eye(4), small=rigid((0.4, -0.3, 0.5), (0.003, -0.004, 0.002)), turn=rigid((0, 0, 90), (0.002, 0.001, -0.001)),
              far=shifted((3.0, -2.0, 1.0)))
    if single:
        return _family("jobs_single", mem, det, [(500, 5500, tf["small"], "J = 1")], CELL, THR)
    plan = [(0, 0, "identity", "empty first"), (0, 1, "identity", "1"), (100, 255, "small", "255"), (200, 256, "turn", "256 overlaps 255"),
            (300, 257, "far", "257 out of reach"), (1000, 2047, "identity", "2047"), (7000, 0, "small", "empty middle"),
            (2000, 2048, "small", "2048 overlaps 2047"), (2000, 2048, "small", "2048 repeated"), (3000, 2049, "turn", "2049"),
            (6000, 5000, "identity", "5000"), (6000, 5000, "turn", "5000 turned"), (6000, 5000, "far", "5000 out of reach"),
            (11999, 1, "small", "last point"), (12000, 0, "identity", "empty last")]
    return _family("jobs", mem, det, [(b, b + n, tf[t], f"{tag} ({t})") for b, n, t, tag in plan], CELL, THR)


GRID_Y_MAX = 65535                       # HIP's limit on gridDim.y: one launch of the evaluation holds that many jobs


@_memo
def many_jobs():
    """GRID_Y_MAX + 1 + 3 tiny jobs over a nine-point cloud (more than one launch can number): job j takes pattern j mod 7 of (range,
    transform), so the jobs on either side of the launch boundary differ and none of them is empty"""
    rng = np.random.default_rng(23)
    mem = np.concatenate([_in_cell(rng, (0, 0, 0), 4, CELL), _in_cell(rng, (-1, 0, 0), 3, CELL), _in_cell(rng, (-1, -1, 1), 2, CELL)])
    det = np.concatenate([_around(rng, mem, 0.004), _in_cell(rng, (0, -1, 0), 3, CELL, 0.0, 1.0)])
    small, far = rigid((0.5, 0.2, -0.4), (0.002, -0.003, 0.001)), shifted((1.0, 1.0, 1.0))
    pats = [(0, 12, np.eye(4), "all"), (0, 9, small, "near, moved"), (2, 5, np.eye(4), "three"), (0, 12, far, "out of reach"),
            (8, 12, np.eye(4), "tail"), (4, 4, small, "empty"), (11, 12, small, "last point")]
    J = GRID_Y_MAX + 1 + 3
    assert all(pats[j % 7][3] != "empty" for j in range(GRID_Y_MAX - 2, J))
    return _family("many_jobs", mem, det, [pats[j % 7] for j in range(J)], CELL, THR)


# ---- occupancy ------------------------------------------------------------------------------------------------------------------
def _in_cell(rng, c, n, cell, lo=0.1, hi=0.9):
    """n points inside cell c (integer coordinates), clear of its faces"""
    return ((np.asarray(c, np.float64) + rng.uniform(lo, hi, size=(n, 3))) * cell).astype(F32)


def _around(rng, pts, r):
    return (pts.astype(np.float64) + rng.normal(0, r, size=pts.shape)).astype(F32)


@_memo
def occupancy(kind):
    """kind "cells": isolated cells of exactly OCCUPANCIES points in every sign octant (some of their points duplicated), one cell of
    BIG_CELL points, a block of 26 full cells around an empty one; a query beside every point of every small cell (each slot of the
    four-at-a-time loop is the minimum once), on some points exactly, and spread over each cell and the empty one.
    kind "single": a grid of one occupied cell.  kind "many": more than 50 000 occupied cells."""
    rng = np.random.default_rng({"cells": 5, "single": 6, "many": 7}[kind])
    cell = CELL
    mem, det = [], []
    if kind == "cells":
        octants = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
        for rep, (sx, sy, sz) in enumerate(octants):
            for i, k in enumerate(OCCUPANCIES):
                c = (sx * (3 + 3 * i) - (sx < 0), sy * (2 + rep) - (sy < 0), sz - (sz < 0))
                p = _in_cell(rng, c, k, cell)
                if rep % 2 == 1 and k >= 2:
                    p[-1] = p[0]                                     # a duplicated point: first and last slot of the cell
                if rep % 4 == 2 and k >= 8:
                    p[3] = p[4] = p[5]
                mem.append(p)
                det += [_around(rng, p, 0.003), p[: (k + 1) // 2], _in_cell(rng, c, 6, cell, 0.0, 1.0)]
        big = _in_cell(rng, (-30, 7, 2), BIG_CELL, cell)
        big[-60:] = big[:60]
        mem.append(big)
        det += [_around(rng, big[rng.integers(0, BIG_CELL, 150)], 0.002), _in_cell(rng, (-30, 7, 2), 150, cell, -0.4, 1.4)]
        centre = np.array([20, 20, -1])
        for d in np.ndindex(3, 3, 3):
            if d != (1, 1, 1):
                mem.append(_in_cell(rng, centre + np.array(d) - 1, 6, cell, 0.0, 1.0))
        det += [_in_cell(rng, centre, 400, cell, 0.0, 1.0), _in_cell(rng, (0, 0, 40), 50, cell)]          # the empty cell; far from everything
    elif kind == "single":
        c = (-3, 5, 0)
        mem.append(_in_cell(rng, c, 7, cell))
        det += [_around(rng, mem[0], 0.004), _in_cell(rng, c, 60, cell, -1.0, 2.0), _in_cell(rng, (40, -40, 3), 20, cell)]
    else:
        cells = np.stack(np.meshgrid(np.arange(-20, 20), np.arange(-20, 20), np.arange(-17, 18), indexing="ij"), -1).reshape(-1, 3)
        mem.append(((cells + rng.uniform(0.1, 0.9, size=cells.shape)) * cell).astype(F32))
        extra = cells[rng.integers(0, len(cells), 4000)]
        mem.append(((extra + rng.uniform(0.1, 0.9, size=extra.shape)) * cell).astype(F32))
        det.append((rng.uniform(-21, 21, size=(20000, 3)) * [1, 1, 18.5 / 21] * cell).astype(F32))
    mem, det = np.concatenate(mem), np.concatenate(det)
    n = len(det)
    return _family(f"occupancy_{kind}", mem, det, [(0, n, np.eye(4), "identity"), (n // 3, n, shifted((0.004, -0.003, 0.002)), "shifted")],
                   cell, THR)


def cell_of(x, cell):
    """floorf(x * inv) as the device computes it (inv = 1.0f / (float)cell), in numpy fp32"""
    inv = F32(1) / F32(cell)
    return np.floor(np.asarray(x, F32) * inv).astype(np.int64)


def occupancy_histogram(fam):
    """{points in a cell: number of such cells} of the family's grid"""
    _, counts = np.unique(cell_of(fam["mem"], fam["cell"]), axis=0, return_counts=True)
    k, n = np.unique(counts, return_counts=True)
    return dict(zip(k.tolist(), n.tolist()))


# ---- threshold ------------------------------------------------------------------------------------------------------------------
def _step(x, k):
    """the float32 k ulps above (k > 0) or below x"""
    x = F32(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf))
    return x


def first_in_cell(k, cell):
    """the smallest float32 x with floorf(x * inv) >= k (for k = 0: +0.0 -- nothing denormal is ever used)"""
    if k == 0:
        return F32(0.0)
    inv = F32(1) / F32(cell)
    x = F32(k * cell)
    while np.floor(x * inv) >= k:
        x = np.nextafter(x, F32(-np.inf))
    while np.floor(x * inv) < k:
        x = np.nextafter(x, F32(np.inf))
    return x


# (cell, thr) of the threshold families.  (float)(thr * thr) lies 0.35 ulp BELOW thr * thr for 0.02 and 0.04 -- the fp32 rule then rejects
# what fp64 accepts, hardly ever the reverse -- and 0.48 ulp ABOVE for 0.075 (the reach of the ICP stage), where both happen.
# 0.021, 0.036 and 0.019 are thresholds whose float, squared in fp32, lies BELOW (float)(thr * thr): a difference of exactly
# (float)thr is then accepted, and the box floorf((q -+ thr) * inv) has to hold an anchor that far away (box_is_exact below).
THRESHOLDS = ((0.04, 0.02), (0.01, 0.02), (0.04, 0.04), (0.05, 0.075), (0.04, 0.021), (0.01, 0.021), (0.04, 0.036), (0.01, 0.019))
TINY = (2.5e-38, 1e-30, 1e-20, 1e-12, 1e-11, 1e-10, 4e-10, 1e-9)     # normal float32 values that stand for "a little beyond the face at 0"
WALK = 12                                # ulp steps to either side of thr along an axis


@_memo
def threshold(cell=CELL, thr=THR):
    """Isolated anchors (no other memory point within 3 thr; asserted) and queries at distance thr -+ a few ulps from them.
    Plain anchors: queries along -+x, -+y, -+z (WALK ulps to either side) and the eight diagonals (every combination of -1 .. 1 ulps
    per component; -3 .. 3 around the anchor at the origin, whose queries have the finest ulps) -- the fp32 rule's d2 lands below, on
    and above thr2.  Face anchors: the anchor is the first float32 beyond a cell face as floorf(x * inv) sees it, or 1, 2, 5 ulps
    further, and the queries walk towards it from inside along that axis (with and without a perpendicular offset below the rounding
    of d2): the anchor's cell is the outermost of the query's box or just outside it.  Faces on both sides of 0, at 0, and at the mid
    and far bases.  One job, identity."""
    thrf = F32(thr)
    L = max(0.2, 10 * thr)
    mem, det = [], []
    slot = [0]

    def lane(base, ax):
        """the next isolated place: every coordinate but `ax` is moved by a multiple of L that no other anchor shares"""
        s = slot[0]
        slot[0] += 1
        i = (s + 1) // 2 * (1 if s % 2 else -1)
        p = np.asarray(base, np.float64) + i * L
        return ((np.floor(p / cell) + 0.37) * cell).astype(F32)

    def plain(base, wide):
        a = lane(base, -1) if base is not None else np.array([0.0011, -0.0023, 0.0017], F32)
        if base is None:
            slot[0] += 1
        mem.append(a)
        for ax in range(3):
            for s in (1, -1):
                q0 = F32(a[ax] + F32(s) * thrf)
                for k in range(-WALK, WALK + 1):
                    q = a.copy()
                    q[ax] = _step(q0, k)
                    det.append(q)
        r = 3 if wide else 1
        d = thrf / F32(np.sqrt(3.0))
        for sg in np.ndindex(2, 2, 2):
            q0 = np.array([F32(a[t] + F32(1 - 2 * sg[t]) * d) for t in range(3)], F32)
            for ks in np.ndindex(2 * r + 1, 2 * r + 1, 2 * r + 1):
                det.append(np.array([_step(q0[t], ks[t] - r) for t in range(3)], F32))

    def face(base, ax, k, s, u):
        a = lane(base, ax)
        if k == 0:
            a[ax] = F32(0.0) if (s > 0 and u == 0) else F32(s * TINY[u])
        else:
            edge = first_in_cell(k, cell) if s > 0 else np.nextafter(first_in_cell(k, cell), F32(-np.inf))
            a[ax] = _step(edge, s * u)
        mem.append(a)
        q0 = F32(a[ax] - F32(s) * thrf)
        for k2 in range(-WALK, WALK + 1):
            for perp in ((0, 0), (3e-6, 0), (3e-6, -3e-6)):
                q = a.copy()
                q[ax] = _step(q0, k2)
                q[(ax + 1) % 3] += F32(perp[0])
                q[(ax + 2) % 3] += F32(perp[1])
                det.append(q)

    plain(None, True)
    for _ in range(6):
        plain(BASES["origin"], False)
    for name in ("mid", "far"):
        plain(BASES[name], False)
        plain(BASES[name], False)
    n = 0
    for k in (0, 1, -1, 3, -3):
        for s in (1, -1):
            for u in (range(8) if k == 0 else (0, 1, 2, 5)):
                face(BASES["origin"], n % 3, k, s, u)
                n += 1
    for name in ("mid", "far"):
        for ax in range(3):
            k = int(round(BASES[name][ax] / cell))
            for s in (1, -1):
                for u in (0, 1, 3):
                    face(BASES[name], ax, k, s, u)
    mem, det = np.stack(mem), np.stack(det)
    assert not cKDTree(mem.astype(np.float64)).query_pairs(3 * thr), "anchors are not isolated"
    det = det[~((np.abs(det) < np.finfo(F32).tiny) & (det != 0)).any(1)]          # (a walk across 0 steps through denormals: left out)
    assert not ((np.abs(mem) < np.finfo(F32).tiny) & (mem != 0)).any(), "denormal anchor"
    return _family(f"threshold_{cell}_{thr}", mem, det, [(0, len(det), np.eye(4), "identity")], cell, thr)


def box_is_exact(thr):
    """fl(thrf * thrf) >= (float)(thr * thr): every point the fp32 rule accepts then lies in a cell of floorf((q -+ thrf) * inv) with
    no padding (tests/test_evaluate_model.py has the argument)"""
    return bool(F32(F32(thr) * F32(thr)) >= F32(thr * thr))


def outside_box(fam, ref):
    """accepted points whose anchor's cell lies outside floorf((q -+ thr) * inv) on some axis, all in numpy fp32 as the kernel does"""
    inv, thrf = F32(1) / F32(fam["cell"]), F32(fam["thr"])
    q = ref["q"]
    hit = ref["idx"] >= 0
    c = cell_of(fam["mem"][np.maximum(ref["idx"], 0)], fam["cell"])
    lo = np.floor((q - thrf) * inv).astype(np.int64)
    hi = np.floor((q + thrf) * inv).astype(np.int64)
    return hit & ((c < lo) | (c > hi)).any(1)


# ---- the references ---------------------------------------------------------------------------------------------------------------
def transformed(det, T):
    """xform of oracle_reg.c and the device -- double, left to right, no contraction -- rounded to fp32"""
    x, y, z = (det[:, t].astype(np.float64) for t in range(3))
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1).astype(F32)


def reference(fam):
    key = ("reference", fam["name"])
    if key in _cache:
        return _cache[key]
    from oracle import reg_oracle as ro
    mem64 = fam["mem"].astype(np.float64)
    tree = cKDTree(mem64)
    parts, done = [], {}
    for b, e, T in zip(fam["jb"], fam["je"], fam["T"]):
        k = (int(b), int(e), T.tobytes())
        if k not in done:                                            # a repeated (range, transform) is computed once
            src = fam["det"][b:e]
            q = transformed(src, T)
            if len(src):
                d2, idx = ro.nearest_bruteforce(src, fam["mem"], T, fam["thr"])
                _, near = tree.query(q.astype(np.float64))
                d2_64 = ((q.astype(np.float64) - mem64[near]) ** 2).sum(1)
            else:
                d2, idx, d2_64 = np.zeros(0, F32), np.zeros(0, np.int32), np.zeros(0)
            done[k] = (d2, idx, d2_64, q)
        parts.append(done[k])
    ns = (fam["je"] - fam["jb"]).astype(np.int64)
    ref = dict(d2=np.concatenate([p[0] for p in parts]), idx=np.concatenate([p[1] for p in parts]),
               d2_64=np.concatenate([p[2] for p in parts]), q=np.concatenate([p[3] for p in parts]),
               ns=ns, off=np.concatenate([[0], np.cumsum(ns)]))
    for v in ref.values():
        v.setflags(write=False)
    _cache[key] = ref
    return ref


def in_band(fam, ref):
    return np.abs(ref["d2_64"] / (fam["thr"] * fam["thr"]) - 1.0) <= BAND


def expected_scores(fam, ref):
    """per job (count, fitness, rmse) of the brute force: fitness = count / ns (0 for an empty job), rmse = sqrt(fsum(d2) / count)"""
    import math
    out = []
    for j, n in enumerate(ref["ns"]):
        d2 = ref["d2"][ref["off"][j]:ref["off"][j + 1]]
        inl = d2[np.isfinite(d2)].astype(np.float64)
        out.append((len(inl), len(inl) / n if n else 0.0, math.sqrt(math.fsum(inl) / len(inl)) if len(inl) else 0.0))
    return out


RANDOM = [("slab_origin", slab, ("origin",)), ("slab_mid", slab, ("mid",)), ("slab_far", slab, ("far",)),
          ("occupancy_cells", occupancy, ("cells",)), ("occupancy_single", occupancy, ("single",)), ("occupancy_many", occupancy, ("many",)),
          ("jobs", jobs, ()), ("jobs_single", jobs, (True,))] + [(f"ratio_{c}_{t}", slab, ("origin", c, t)) for c, t in RATIOS[1:]]
THRESHOLD = [(f"threshold_{c}_{t}", threshold, (c, t)) for c, t in THRESHOLDS]
ALL = RANDOM + THRESHOLD


def get(name):
    for n, fn, args in ALL:
        if n == name:
            return fn(*args)
    raise KeyError(name)
