"""Deterministic clouds for the memory-build kernels alone (csrc/build_memory.hip: `ibl_dbscan_batch`, `ibl_voxel_downsample_batch`, and
under them the batch grid builder of csrc/reg_grid.hip), shared by tests/test_build_model.py (CPU: every case contains what it is named
for) and tests/test_gpu_build_edges.py (GPU: one call per case, compared with `oracle.build_oracle` by `np.array_equal`).

Random clouds almost never land where these kernels decide, so the cases are built on the decisions: pairs at exactly `eps`, points with
exactly `min_points` neighbours, a border point between two clusters whose numbering disagrees with the cell order, groups that lie inside
each other, the three paths of the grid's dims kernel (second round, widened cells, cell budget), points on voxel planes, voxel
indices past 2^31 and spans at the 16-bit limit of a key field.  Coordinates that decide at a boundary are exact binary fractions
(multiples of EPS / 8 of moderate size), so the fp64 distances and the fp32 binning are exact on both sides of the comparison.

A DBSCAN case is a dict  groups (list of (n, 3) float64), eps, min_points, overflow (whether the cell budget must be reported), info
(what the model test looks at).  A voxel case is a dict  points, colors (lists of (n, 3) float64), voxel, refused (None, or the
(object, axis) the call must name when it refuses the batch), info."""
import numpy as np

from oracle import build_oracle as bo

EPS = 0.0625
EPS_UP = float(np.nextafter(EPS, 1.0))
DBSCAN_BUDGET = 64 << 20                 # cells ibl_dbscan_batch gives the grid builder
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


# ---- the grid builder's arithmetic in numpy fp32 (reg_grid.hip: ibl_bbox_kernel, seg_dims, cell_clamp) -------------------------------
def seg_dims32(points, cell):
    """(min, inv, n) of one segment: the fp32 bounding box of the fp32-rounded points, the cell widened to emax / 128, cells per axis"""
    P = np.asarray(points, np.float64).astype(F32)
    mn, mx = P.min(0), P.max(0)
    e = (mx - mn).astype(F32)
    c = F32(cell)
    if e.max() / F32(128.0) > c:
        c = F32(e.max() / F32(128.0))
    inv = F32(F32(1.0) / c)
    n = np.floor((e * inv).astype(F32)).astype(np.int64) + 1
    return mn, inv, n


def cells32(points, mn, inv, n):
    c = np.floor(((np.asarray(points, np.float64).astype(F32) - mn).astype(F32) * inv).astype(F32)).astype(np.int64)
    return np.clip(c, 0, n - 1)


def cell_counts(groups, cell):
    """cells of every group's full-size grid (1 for an empty group: its box reads as zeros)"""
    return [int(np.prod(seg_dims32(g, cell)[2])) if len(g) else 1 for g in groups]


def oracle_sum_d2(a, b):
    """the squared distance in the order both sides sum it: ((dx^2 + dy^2) + dz^2) in fp64"""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    d2 = d[..., 0] * d[..., 0]
    d2 = d2 + d[..., 1] * d[..., 1]
    return d2 + d[..., 2] * d[..., 2]


def lattice(n, spacing):
    g = np.arange(n, dtype=np.float64) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


# ---- DBSCAN -------------------------------------------------------------------------------------------------------------------------
@_memo
def lattice_at_eps(variant):
    """6 x 6 x 6 lattice with spacing exactly EPS, twice: once with every lattice point ON a cell plane of its group (the group's minimum
    is an anchor 8 cells away), once in the middle of its cell (anchor 8.5 cells away).  variant: "at" (eps = EPS: the six axis neighbours
    sit at exactly eps and do not count), "above7" (eps one ulp larger, min_points 7 = the neighbour count of an interior point),
    "above8" (one more than any point has)."""
    eps, mp = {"at": (EPS, 2), "above7": (EPS_UP, 7), "above8": (EPS_UP, 8)}[variant]
    rng = np.random.default_rng(101)
    groups, interior = [], []
    for away in (8.0, 8.5):
        origin = np.array([1.0, -2.0, 0.5])
        L = origin + lattice(6, EPS)
        P = np.concatenate([L, (origin - away * EPS)[None]])
        perm = rng.permutation(len(P))
        groups.append(P[perm])
        idx = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        inner = ((idx >= 1) & (idx <= 4)).sum(1)                        # 3: interior, 2: inside a face, 1: edge, 0: corner
        interior.append(np.concatenate([inner, [-1]])[perm])
    return dict(groups=groups, eps=eps, min_points=mp, overflow=False, info=dict(inner=interior))


@_memo
def border_between_two(variant):
    """Two 3 x 3 x 3 lattices of spacing EPS / 2 (every point has at least 8 neighbours: all are core at min_points 8) at least eps apart,
    and one point X within eps of a core point of each, with fewer than 8 neighbours itself.  A lies at lower cell ids than B in
    "a_first" / "b_first" (A at lower x; cells are numbered z, y, x), and
      a_first   A holds the lowest original indices, X is last:  A = cluster 0, X takes 0 from A
      b_first   B holds the lowest original indices, X is first: B = cluster 0 although A comes first in cell order, X takes 0 from B
      diagonal  X sits off a corner of each lattice, half a cell away in x, y and z: its only core neighbour in A (the lower-numbered
                cluster, which comes LATER in cell order here) lies in another cell row (other y and other z cell) than X"""
    rng = np.random.default_rng(102)
    h = 0.5
    A = lattice(3, h)
    if variant == "diagonal":
        X = np.array([1.5, -0.5, -0.5])
        B = np.array([2.0, -1.0, -1.0]) + lattice(3, h) * np.array([1.0, -1.0, -1.0])
    else:
        X = np.array([1.75, 0.0, 0.0])
        B = np.array([2.5, 0.0, 0.0]) + lattice(3, h)
    A, B = A[rng.permutation(27)], B[rng.permutation(27)]
    if variant == "b_first":
        units, ix, ia, ib = np.concatenate([X[None], B, A]), 0, np.arange(28, 55), np.arange(1, 28)
    else:
        units, ix, ia, ib = np.concatenate([A, B, X[None]]), 54, np.arange(0, 27), np.arange(27, 54)
    P = (units + np.array([48.0, -16.0, 4.0])) * EPS                    # integer units: cell planes stay on the integers
    return dict(groups=[P], eps=EPS, min_points=8, overflow=False, info=dict(x=ix, a=ia, b=ib))


SNAKE_STEP = 0.6 * EPS
SNAKE_RUN, SNAKE_SEP, SNAKE_LAYER, SNAKE_N, SNAKE_GAP_RUN = 340, 3, 5, 8000, 12


def _snake_path():
    pts, x, y, z, dx, dy, r = [(0, 0, 0)], 0, 0, 0, 1, 1, 0
    while len(pts) < SNAKE_N:
        for _ in range(SNAKE_RUN - 1):
            x += dx
            pts.append((x, y, z))
        dx = -dx
        r += 1
        for _ in range(SNAKE_SEP):
            if r % SNAKE_LAYER == 0:
                z += 1
            else:
                y += dy
            pts.append((x, y, z))
        if r % SNAKE_LAYER == 0:
            dy = -dy
    return np.array(pts[:SNAKE_N], dtype=np.int64)


def _snake_points(ig, closed):
    path = _snake_path()
    pg = SNAKE_GAP_RUN * (SNAKE_RUN - 1 + SNAKE_SEP) + ig               # run 12 walks towards +x: ix = position in the run
    assert path[pg, 0] == ig and path[pg + 1, 0] == ig + 1
    after = np.arange(len(path)) > pg
    P = np.empty((len(path), 3))
    P[:, 0] = np.where(after, EPS + (path[:, 0] - ig - 1) * SNAKE_STEP, (path[:, 0] - ig) * SNAKE_STEP)
    P[:, 1:] = path[:, 1:] * SNAKE_STEP
    if closed:
        P[pg + 1, 0] = np.nextafter(P[pg + 1, 0], -1.0)
    return P, pg


@_memo
def snake(variant):
    """8 000 points along a serpentine (runs of 340 points along x, 3 steps apart in y, 5 runs per layer, layers 3 steps apart in z) at
    spacing 0.6 EPS: every point has exactly min_points = 3 neighbours (itself and its two chain neighbours; four at a corner).  Between
    two points of run 12 the step is exactly EPS ("open": two clusters, the points at the gap are border points) or one ulp less
    ("closed": one cluster).  The extent along x is over 200 EPS, so the cell is widened to emax / 128, and the gap is put where its
    two ends fall into different cells.  The input order is shuffled."""
    for ig in range(150, 200):
        P, pg = _snake_points(ig, False)
        mn, inv, n = seg_dims32(P, EPS)
        c = cells32(P[pg:pg + 2], mn, inv, n)
        if c[0, 0] != c[1, 0]:
            break
    else:
        raise AssertionError("no gap position straddles a cell plane")
    P, pg = _snake_points(ig, variant == "closed")
    perm = np.random.default_rng(103).permutation(len(P))
    inv_perm = np.argsort(perm)
    return dict(groups=[P[perm]], eps=EPS, min_points=3, overflow=False, info=dict(g0=int(inv_perm[pg]), g1=int(inv_perm[pg + 1])))


def _quantised(rng, n, box_units):
    """n points on the EPS / 4 lattice inside a box: many pairs at exactly eps, about eps^-3 points per unit volume"""
    origin = rng.integers(-800, 800, size=3) * EPS
    return origin + rng.integers(0, box_units, size=(n, 3)) * (EPS / 4)


@_memo
def many_groups():
    """320 groups in one call (the dims kernel takes 256 segments per round): empty groups at the head, in the middle and at the tail,
    groups of 1 / 255 / 256 / 257 points, all-duplicate groups, one cloud twice, and pairs of groups that lie inside each other -- the
    even and the odd points of one chain (alone each is noise, together they would be one cluster) and two shifted lattices."""
    rng = np.random.default_rng(104)
    empty = np.zeros((0, 3))
    groups = [empty] * 3
    for n in (1, 255, 256, 257):
        groups.append(_quantised(rng, n, 24))
    groups.append(np.repeat(_quantised(rng, 1, 8), 12, axis=0))         # 12 copies of one point: one cluster
    groups.append(np.repeat(_quantised(rng, 1, 8), 3, axis=0))          # 3 copies: below min_points, noise
    twice = _quantised(rng, 120, 14)
    groups.append(twice)
    chain = np.array([5.0, 5.0, -3.0]) + np.arange(60)[:, None] * np.array([0.375 * EPS, 0.0, 0.0])
    groups += [chain[0::2], chain[1::2]]                                # interleaved pair 1
    lat = np.array([-7.0, 2.0, 2.0]) + lattice(5, 1.125 * EPS)          # alone: spacing 1.125 eps, all noise
    groups += [lat, lat + 0.5625 * EPS]                                 # interleaved pair 2: body-centred, 0.97 eps to the other group
    while len(groups) < 150:
        groups.append(_quantised(rng, int(rng.integers(10, 41)), 10))
    groups += [empty] * 5
    groups.append(twice.copy())
    while len(groups) < 316:
        groups.append(_quantised(rng, int(rng.integers(10, 41)), 10))
    groups += [empty] * 4
    return dict(groups=groups, eps=EPS, min_points=4, overflow=False,
                info=dict(twice=(9, 155), pairs=((10, 11), (12, 13)), duplicates=(7, 8), sizes={1: 3, 255: 4, 256: 5, 257: 6}))


@_memo
def far_from_origin():
    """a cloud 4 096 m from the origin, eps 0.01: one fp32 step there is 4.9e-4, so the grid bins coordinates that moved by up to 2.4 % of
    eps and several distinct points share one fp32 position; the distances must still be those of the fp64 points"""
    rng = np.random.default_rng(105)
    c = rng.uniform(-0.1, 0.1, size=(6, 3))
    P = np.concatenate([c[i] + rng.normal(size=(200, 3)) * 0.008 for i in range(6)] + [rng.uniform(-0.15, 0.15, size=(300, 3))])
    P[1:40:2] = P[0:40:2] + 1e-5                                        # pairs far closer than an fp32 step
    P = P[rng.permutation(len(P))] + np.array([4096.0, -4096.0, 4096.5])
    return dict(groups=[P], eps=0.01, min_points=5, overflow=False, info={})


def _budget_group(rng, extent_units):
    """100 points: the two corners of a cube of extent_units * EPS, three 3 x 3 x 3 lattices of spacing EPS / 2 (clusters at
    min_points 8) and 17 points on the EPS / 4 lattice"""
    origin = rng.integers(-400, 400, size=3) * EPS
    E = extent_units * EPS
    parts = [np.array([[0.0, 0.0, 0.0], [E, E, E]])]
    for _ in range(3):
        parts.append(rng.integers(1, int(extent_units) - 2, size=3) * EPS + lattice(3, EPS / 2))
    parts.append(rng.integers(0, int(extent_units) * 4, size=(17, 3)) * (EPS / 4))
    P = np.concatenate(parts)
    return origin + P[rng.permutation(len(P))]


@_memo
def budget_exceeded():
    """40 groups of 100 points whose extent is 130 EPS on all three axes: the cell is widened and each takes 129^3 cells, 31 fit into the
    64 Mi-cell budget, the other nine collapse to one cell each"""
    rng = np.random.default_rng(106)
    return dict(groups=[_budget_group(rng, 130.0) for _ in range(40)], eps=EPS, min_points=8, overflow=True, info={})


@_memo
def budget_filled_exactly():
    """32 groups of extent 127.5 EPS: 128^3 cells each, together exactly the 64 Mi-cell budget; the 33rd group (one point) finds no
    cell left inside the budget and collapses"""
    rng = np.random.default_rng(107)
    groups = [_budget_group(rng, 127.5) for _ in range(32)]
    groups.append(np.array([[3.0, 4.0, 5.0]]))
    return dict(groups=groups, eps=EPS, min_points=8, overflow=True, info={})


DBSCAN_CASES = {
    "lattice_at_eps": lambda: lattice_at_eps("at"),
    "lattice_above_eps_min7": lambda: lattice_at_eps("above7"),
    "lattice_above_eps_min8": lambda: lattice_at_eps("above8"),
    "border_between_two_a_first": lambda: border_between_two("a_first"),
    "border_between_two_b_first": lambda: border_between_two("b_first"),
    "border_between_two_diagonal": lambda: border_between_two("diagonal"),
    "snake_open": lambda: snake("open"),
    "snake_closed": lambda: snake("closed"),
    "many_groups": many_groups,
    "far_from_origin": far_from_origin,
    "budget_exceeded": budget_exceeded,
    "budget_filled_exactly": budget_filled_exactly,
}


@_memo
def dbscan_expected(name):
    """the oracle, group by group (computed once per process and shared)"""
    case = DBSCAN_CASES[name]()
    return [bo.cluster_dbscan(g, case["eps"], case["min_points"]) if len(g) else np.zeros(0, dtype=np.int32) for g in case["groups"]]


# ---- voxel down-sampling --------------------------------------------------------------------------------------------------------------
def _colors(rng, points):
    return [rng.uniform(0, 1, size=p.shape) for p in points]


@_memo
def on_the_planes(voxel):
    """points whose coordinates are multiples k * voxel, k in -12 .. 12 (for 0.0625 the quotient is k exactly; for 0.05 the product and
    the quotient both round, and floor sees k or k - 1), their neighbours one ulp to either side, and -0.0"""
    rng = np.random.default_rng(201)
    k = rng.integers(-12, 13, size=(600, 3))
    k[:5] = 0
    on = k * voxel
    on[:5] = [[-0.0, 0.0, 0.0], [0.0, -0.0, -0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [-0.0, voxel, -voxel]]
    below, above = np.nextafter(on[5:205], -np.inf), np.nextafter(on[205:405], np.inf)
    P = np.concatenate([on, below, above])
    P = P[rng.permutation(len(P))]
    P[0] = [-0.0, -0.0, 0.0]
    inside = rng.uniform(-12 * voxel, 12 * voxel, size=(300, 3))
    inside[:, 2] = rng.integers(-12, 13, size=300) * voxel              # one coordinate on a plane, two inside
    points = [P, np.zeros((0, 3)), inside]
    return dict(points=points, colors=_colors(rng, points), voxel=voxel, refused=None, info={})


@_memo
def crowded():
    """one voxel with 5 000 points among 400 ordinary ones, its points spread over the whole input: the mean is one running fp64 sum in
    input order (a pairwise or a split sum differs in the last bits)"""
    rng = np.random.default_rng(202)
    voxel = 0.05
    crowd = np.array([0.35, -0.2, 1.0]) + rng.uniform(0.001, 0.049, size=(5000, 3))
    rest = rng.uniform(-0.5, 0.5, size=(400, 3))
    P = np.concatenate([crowd, rest])[rng.permutation(5400)]
    points = [rng.uniform(-0.2, 0.2, size=(150, 3)), P]
    return dict(points=points, colors=_colors(rng, points), voxel=voxel, refused=None, info=dict(obj=1, crowd=5000))


@_memo
def interleaved():
    """60 voxels of 7 points each; the input walks the voxels from the largest key (x, then y, then z) to the smallest, seven times: every
    voxel's points are 60 rows apart, and the order of first occurrence is the reverse of the key order"""
    rng = np.random.default_rng(203)
    voxel = 0.05
    idx = np.array(sorted({tuple(v) for v in rng.integers(-6, 7, size=(200, 3)).tolist()}, reverse=True)[:60])
    rounds = [(idx + rng.uniform(0.05, 0.95, size=idx.shape)) * voxel for _ in range(7)]
    points = [np.concatenate(rounds), np.concatenate(rounds[:3]) + 40 * voxel]
    return dict(points=points, colors=_colors(rng, points), voxel=voxel, refused=None, info=dict(n_vox=60))


@_memo
def many_objects():
    """720 objects of 0 .. 40 points, runs of empty objects at the head, in the middle and at the tail: the offsets kernel takes 256
    objects per block"""
    rng = np.random.default_rng(204)
    points = []
    for i in range(720):
        n = 0 if (i < 4 or 300 <= i < 309 or i >= 715) else int(rng.integers(0, 41))
        points.append(rng.uniform(-5, 5, size=3) + rng.uniform(-0.15, 0.15, size=(n, 3)))
    return dict(points=points, colors=_colors(rng, points), voxel=0.05, refused=None, info={})


SPAN_OBJECT = 2


@_memo
def span_limit(axis):
    """object 2 of 5 spans voxel indices b .. b + 65 535 on all three axes at once (axis None: the largest span a key holds; its far point
    has all three 16-bit fields full, next to object 3's keys), or b .. b + 65 536 on `axis` (refused)"""
    rng = np.random.default_rng(205)
    voxel = 0.0625
    b = np.array([-30000, 10, -65000])
    far = b + 65535
    if axis is not None:
        far[axis] += 1
    mid = b + rng.integers(0, 65536, size=(60, 3))
    idx = np.concatenate([b[None], far[None], mid, b[None], far[None], mid[:20]])
    wide = (idx + rng.uniform(0.1, 0.9, size=idx.shape)) * voxel
    wide = wide[rng.permutation(len(wide))]
    ordinary = [rng.uniform(-0.4, 0.4, size=(n, 3)) + s for n, s in ((300, 0.0), (40, 2.0), (200, -3.0), (90, 1.0))]
    points = ordinary[:2] + [wide] + ordinary[2:]
    return dict(points=points, colors=_colors(rng, points), voxel=voxel, refused=None if axis is None else (SPAN_OBJECT, axis),
                info=dict(base=b, far=far))


@_memo
def beyond_int32():
    """coordinates near +-3e7 with 1 cm voxels: indices near +-3e9, past int32"""
    rng = np.random.default_rng(206)
    points = [rng.uniform(0, 0.2, size=(800, 3)) + np.array([3.0e7, -3.0e7, 3.0000001e7]),
              rng.uniform(0, 0.1, size=(300, 3)) + np.array([-2.9e7, 2.5e7, 2.2e7])]
    return dict(points=points, colors=_colors(rng, points), voxel=0.01, refused=None, info={})


VOXEL_CASES = {
    "on_the_planes_exact": lambda: on_the_planes(0.0625),
    "on_the_planes_inexact": lambda: on_the_planes(0.05),
    "crowded": crowded,
    "interleaved": interleaved,
    "many_objects": many_objects,
    "span_limit": lambda: span_limit(None),
    "beyond_int32": beyond_int32,
}
VOXEL_REFUSED = {f"span_limit_over_axis{a}": (lambda a=a: span_limit(a)) for a in range(3)}


@_memo
def voxel_expected(name, with_colors):
    """(points, colors or None, counts) per object from the oracle"""
    case = VOXEL_CASES[name]()
    return [bo.voxel_down_sample_with_colors(p, c if with_colors else None, case["voxel"]) for p, c in zip(case["points"], case["colors"])]
