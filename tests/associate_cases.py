"""Live memory, association -- what tests/test_associate_model.py (CPU) and tests/test_gpu_associate.py (device) share: the measure of
ibl_memgrid_overlap restated in numpy, the case generators, and the decision rule of ObjectMemory.associate_detections restated from
the brute-force hits.

    hits(D, m) = #{ p in D : some point q of instance m has d2(p, q) < r2 },   r2 = float32(r * r),
    d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32  (the device's dist2f; DESIGN.md (c) convention 2), strict <.

Exactness: every test coordinate is a multiple of STEP = 2^-16 m below 8 m in absolute value.  Such values and every difference of two
of them are exact in fp32 (at most 20 significant bits), a square of a difference has at most 40 bits and is exact in float64, and so
is every partial sum of the chain.  `dist2_emulated` therefore rounds exactly where fmaf rounds -- once per step, from the exact
value -- and is the device's chain bit for bit; `dist2_integer` is the same chain in integer arithmetic (round-to-nearest-even to 24
bits by hand), and the model test holds the two equal.  Where a case needs a pair exactly at the radius it uses R_EDGE = 1280 STEP:
1280^2 = 768^2 + 1024^2 and 1280^2 < 2^24, so r2 and the d2 of such pairs are the same fp32 number and the strict < decides."""
import functools

import numpy as np

STEP = 2.0 ** -16
CELL = 0.04                      # the cell of a MemoryShard's grid: 2 * eval_threshold
R_HALF = 0.02                    # cell / 2: the default radius (eval_threshold); boxes of at most 8 cells
R_CELL = 0.04                    # the largest radius the entry point takes: boxes of 27 cells
R_EDGE = 1280 * STEP             # 0.01953125
CORNER = 5243                    # lattice steps: floor(25 * 5243 / 65536) = 2 and floor(25 * 5242 / 65536) = 1 -- a cell face lies between


def lattice(steps):
    """integer lattice steps -> float64 metres (exact, and exact again as fp32)"""
    a = np.asarray(steps, dtype=np.int64)
    assert np.abs(a).max(initial=0) < 8 * 65536
    return a.astype(np.float64) * STEP


def snap(points):
    """points rounded to the lattice"""
    return lattice(np.rint(np.asarray(points, dtype=np.float64) / STEP).astype(np.int64))


def steps_of(points):
    s = np.asarray(points, dtype=np.float64) / STEP
    assert (s == np.rint(s)).all(), "not on the lattice"
    return s.astype(np.int64)


def cell_of(points):
    """the grid cell of every row, as the device forms it: floorf(x * (1.0f / 0.04f))"""
    inv = np.float32(1.0) / np.float32(CELL)
    return np.floor(np.asarray(points, dtype=np.float32) * inv).astype(np.int64)


def r2_of(r):
    return np.float32(float(r) * float(r))


def dist2_emulated(p, q):
    """dist2f of the rows p (n, 3) against the rows q (m, 3): (n, m) float32, the fmaf chain with one rounding per step"""
    p, q = np.asarray(p, dtype=np.float32), np.asarray(q, dtype=np.float32)
    d = (p[:, None, :] - q[None, :, :]).astype(np.float32)
    dx, dy, dz = (d[..., i].astype(np.float64) for i in range(3))
    t = (dx * dx).astype(np.float32)
    t = (dy * dy + t.astype(np.float64)).astype(np.float32)
    return (dz * dz + t.astype(np.float64)).astype(np.float32)


def _round24(n):
    """non-negative integers rounded to 24 significant bits, ties to even -- what one fp32 rounding does to an exact value"""
    n = np.asarray(n, dtype=np.int64)
    bits = np.frexp(n.astype(np.float64))[1]                 # bit length (exact below 2^53)
    sh = np.maximum(bits - 24, 0)
    q, rem = n >> sh, n & ((np.int64(1) << sh) - 1)
    half = np.where(sh > 0, np.int64(1) << np.maximum(sh - 1, 0), np.int64(0))
    up = (sh > 0) & ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    return (q + up.astype(np.int64)) << sh


def dist2_integer(p_steps, q_steps):
    """the same chain on integer lattice steps: (n, m) int64 in units of STEP^2"""
    d = np.asarray(p_steps, dtype=np.int64)[:, None, :] - np.asarray(q_steps, dtype=np.int64)[None, :, :]
    t = _round24(d[..., 0] * d[..., 0])
    t = _round24(d[..., 1] * d[..., 1] + t)
    return _round24(d[..., 2] * d[..., 2] + t)


def brute_hits(dets, insts, r):
    """(n_det, n_inst) int64: hits of every detection on every instance, by the definition -- every pair of points of every pair of
    clouds whose bounding boxes come within 2 r of each other"""
    r2 = r2_of(r)
    H = np.zeros((len(dets), len(insts)), dtype=np.int64)
    for d, D in enumerate(dets):
        D = np.asarray(D, dtype=np.float64).reshape(-1, 3)
        if not len(D):
            continue
        for m, Q in enumerate(insts):
            Q = np.asarray(Q, dtype=np.float64).reshape(-1, 3)
            if not len(Q) or (D.min(0) > Q.max(0) + 2 * r).any() or (Q.min(0) > D.max(0) + 2 * r).any():
                continue
            near = np.zeros(len(D), dtype=bool)
            for a in range(0, len(D), 512):
                near[a:a + 512] = (dist2_emulated(D[a:a + 512], Q) < r2).any(axis=1)
            H[d, m] = int(near.sum())
    return H


def expected_pairs(H, k):
    """(inst (n_det, k), hits (n_det, k), n_hit (n_det,)) the entry point owes for the hits matrix H: the instances with hits > 0 by
    hits descending, then instance ascending, cut to k; -1 / 0 padded"""
    inst = np.full((len(H), k), -1, dtype=np.int32)
    hits = np.zeros((len(H), k), dtype=np.int32)
    n_hit = np.zeros(len(H), dtype=np.int32)
    for d, row in enumerate(H):
        nz = [m for m in sorted(range(len(row)), key=lambda m: (-row[m], m)) if row[m] > 0]
        n_hit[d] = len(nz)
        inst[d, :len(nz[:k])] = nz[:k]
        hits[d, :len(nz[:k])] = [row[m] for m in nz[:k]]
    return inst, hits, n_hit


def decide(H, det_sizes, det_embs, mean_embs, min_overlap=0.6, min_similarity=0.6, k=8):
    """the rule of ObjectMemory.associate_detections restated from the hits matrix: of the first k candidates of `expected_pairs`
    those with hits / len(D) >= min_overlap, of these the highest cosine with the instance's mean embedding if it is >=
    min_similarity; ties to the lower index"""
    inst, hits, _ = expected_pairs(H, k)
    out = []
    for d in range(len(H)):
        e = np.asarray(det_embs[d], dtype=np.float64).reshape(-1)
        cands = [int(m) for m, h in zip(inst[d], hits[d]) if m >= 0 and det_sizes[d] > 0 and h / det_sizes[d] >= min_overlap]
        cos = {m: float(np.dot(e, np.asarray(mean_embs[m], np.float64).reshape(-1)) /
                        (np.linalg.norm(e) * np.linalg.norm(np.asarray(mean_embs[m], np.float64)))) for m in cands}
        best = min(cands, key=lambda m: (-cos[m], m)) if cands else None
        out.append(best if best is not None and cos[best] >= min_similarity else None)
    return out


# ---- the cases: each returns (insts, dets) = lists of (n, 3) float64 lattice arrays -----------------------------------------------------
def _shell(rng, centre, radius, n):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return snap(v * radius * rng.uniform(0.9, 1.1, size=3) + np.asarray(centre))


@functools.lru_cache(maxsize=None)
def small_world():
    """6 instances of 200-400 surface points around the origin (coordinates on both sides of zero on every axis; 1 and 2 intersect)
    and 5 detections: a shifted copy, a partial view that also touches a second instance, a copy shifted by about cell / 2, one far
    from everything, and a union of parts of two instances"""
    rng = np.random.default_rng(411)
    spec = [((-0.15, -0.10, -0.05), 0.09, 300), ((0.15, 0.10, 0.05), 0.10, 400), ((0.19, 0.13, 0.07), 0.08, 250),
            ((-0.30, 0.25, -0.20), 0.07, 200), ((0.40, -0.30, 0.20), 0.11, 350), ((0.0, 0.0, 0.0), 0.06, 280)]
    insts = [_shell(rng, c, r, n) for c, r, n in spec]
    half = insts[1][insts[1][:, 0] > 0.15]
    dets = [insts[0] + lattice([200, -150, 100]),
            half + lattice([-90, 60, 130]),
            insts[5] + lattice([1100, -700, 300]),
            insts[3][:150] + lattice([5 * 65536, 0, 0]),
            np.concatenate([insts[4][:120] + lattice([40, 40, -40]), insts[2][100:220] + lattice([-300, 0, 250])])]
    return tuple(insts), tuple(dets)


@functools.lru_cache(maxsize=None)
def crowded():
    """one detection point (the first of 4) within r of 12 instances of 1-3 points each: it sits next to a cell corner, the instances'
    points on all sides of it, every second instance with points in two or three different cells.  r = R_HALF."""
    rng = np.random.default_rng(412)
    P = np.array([CORNER, CORNER, CORNER], dtype=np.int64)
    insts = []
    for j in range(12):
        n = 1 + j % 3
        sign = np.array([1 if (j >> b) & 1 else -1 for b in range(3)])
        offs = [sign * rng.integers(150, 500, size=3)]                   # < 500 sqrt(3) = 866 steps: within 1310
        for t in range(1, n):
            flip = np.ones(3, dtype=np.int64)
            flip[(j + t) % 3] = -1                                       # across a face: another cell
            offs.append(sign * flip * rng.integers(150, 500, size=3))
        insts.append(lattice(P + np.array(offs)))
    det = lattice(np.array([P, P + [30000, 0, 0], P + [0, 30000, 0], P - [0, 0, 30000]]))
    return tuple(insts), (det,)


@functools.lru_cache(maxsize=None)
def radius_edge():
    """six one-point instances 0.5 m apart and one detection of six points, one per instance: pairs at exactly R_EDGE (along an
    axis, and 768 / 1024 steps along two) and pairs one lattice step inside.  Returns (insts, dets, expected hits per instance)."""
    offs = [(1280, 0, 0), (768, 1024, 0), (1279, 0, 0), (767, 1024, 0), (0, 768, -1024), (0, -768, 1023)]
    expect = [0, 0, 1, 1, 0, 1]
    insts, det = [], []
    for j, o in enumerate(offs):
        base = np.array([CORNER - 32768 * (j % 2), CORNER + 32768 * (j // 2), -CORNER], dtype=np.int64)
        det.append(base)
        insts.append(lattice(base + np.array(o))[None])
    return tuple(insts), (lattice(np.array(det)),), tuple(expect)


@functools.lru_cache(maxsize=None)
def eight_cells():
    """a detection point next to a cell corner with the SAME instance (8 points, all within r) in all 8 cells of its box, a second
    instance in one of them, and two more detection points that see nothing.  r = R_HALF."""
    P = np.array([CORNER, CORNER, CORNER], dtype=np.int64)
    corners = np.array([[sx, sy, sz] for sx in (-400, 400) for sy in (-400, 400) for sz in (-400, 400)], dtype=np.int64)
    insts = [lattice(P + np.array([[500, 300, 200]])), lattice(P + corners)]
    det = lattice(np.array([P, P + [20000, 0, 0], P - [0, 20000, 0]]))
    return tuple(insts), (det,)


OVER_K = 4
_OVER_SETS = [(0, 1, 2), (1, 2, 3), (4,), (0, 5), (3,), (2, 4), (5,)]          # detection points each instance is near: hits 3 3 1 2 1 2 1


@functools.lru_cache(maxsize=None)
def over_k():
    """one detection of 6 points 0.1 m apart and 7 instances, instance m with one point next to every detection point of
    _OVER_SETS[m]: 7 > OVER_K instances hit, with ties in hits (3 3 1 2 1 2 1)"""
    base = np.array([[-3 * 6554 + 6554 * i, 1000 * (i % 2), -2000] for i in range(6)], dtype=np.int64)
    insts = []
    for m, near in enumerate(_OVER_SETS):
        off = np.array([(m + 1) * 100, -(m + 1) * 60, 90 * (m % 3 - 1)])
        insts.append(lattice(base[list(near)] + off))
    return tuple(insts), (lattice(base),)


@functools.lru_cache(maxsize=None)
def empty_and_far():
    """the small world's instances; detections: a copy, an EMPTY one, another copy, one far from everything"""
    insts, dets = small_world()
    return insts, (dets[0], np.zeros((0, 3)), dets[2], dets[3])


@functools.lru_cache(maxsize=None)
def facade():
    """The facade scenario: a SynthWorld of 4 objects of 2 500 points (snapped to the lattice) and four detections in the world frame
    (the pose is the identity): re-observations of the objects 1 and 3 (a 1 500-point view moved by a few lattice steps, an embedding
    next to the object's), a new object far from all four, and an impostor -- points of object 0 with an embedding orthogonal to its
    mean.  dict(world, points, colors, embeddings, phrases, det_embs, det_clouds [(points, colors)], expect)."""
    from ibloc_amd.synth import SynthObject, SynthWorld
    w = SynthWorld(4, pts_per_object=2500, E=2, D=32, seed=413)
    pts = [snap(p) for p in w.points]
    rng = np.random.default_rng(414)
    mean = [np.mean(np.asarray(w.embeddings[j], dtype=np.float32), axis=0) for j in range(4)]

    def view(j, shift):
        keep = np.sort(rng.choice(2500, 1500, replace=False))
        return pts[j][keep] + lattice(shift), w.colors[j][keep]

    new_obj = SynthObject(np.random.default_rng(415), np.array([6.0, 6.0, 0.5]))
    p_new, c_new = new_obj.sample(1800, np.random.default_rng(416))
    other = rng.normal(size=32)
    m0 = mean[0].astype(np.float64)
    other -= m0 * (other @ m0) / (m0 @ m0)                               # orthogonal to the mean embedding of object 0
    near = [w.base_emb[j] + rng.normal(0, 0.1 / np.sqrt(32), size=32) for j in (1, 3)]
    det_embs = [near[0].astype(np.float32), near[1].astype(np.float32), rng.normal(size=32).astype(np.float32), other.astype(np.float32)]
    det_clouds = [view(1, [3, -2, 4]), view(3, [-5, 1, 2]), (snap(p_new), c_new), view(0, [2, 2, -3])]
    return dict(world=w, points=pts, colors=list(w.colors), embeddings=[np.asarray(e, dtype=np.float32) for e in w.embeddings], means=mean,
                phrases=["chair again", "lamp again", "a new plant", "impostor"], det_embs=det_embs, det_clouds=det_clouds,
                expect=[1, 3, None, None])
