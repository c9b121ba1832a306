"""The information matrix of a pose from its whole-memory correspondences (`ibl_information_kernel`, csrc/reg_eval.hip) -- what
tests/test_information_model.py (CPU) and tests/test_gpu_information.py (device) share: the matrix restated in numpy three ways, the
tie rule restated from the brute force, and a lattice family of exact ties.

    correspondences   those of the evaluation: q = (float)(T p), the memory point m with the smallest fp32 d2 = dist2f(q, m),
                      accepted when d2 < (float)(thr * thr)
    ties              among memory points at the same minimal fp32 d2 the lexicographically smallest (x, y, z), compared as floats
    matrix            sum of G1^T G1 + G2^T G2 + G3^T G3 with (x, y, z) = (double)m - about,
                      G1 = [0, z, -y, 1, 0, 0], G2 = [-z, 0, x, 0, 1, 0], G3 = [y, -x, 0, 0, 0, 1]

The families of tests/evaluate_cases.py are used as they are.  `oracle.reg_oracle.nearest_bruteforce` names the LOWEST INDEX among
equal distances, the rule the lexicographically smallest coordinates: the two agree on a family without ties between distinct
coordinates (exact duplicates contribute the same terms), which `near_ties` decides in fp64 with a margin -- fp32 d2 carries less
than 2^-21 of relative error (evaluate_cases), so two candidates whose fp64 squared distances differ by more than 2^-18 are ordered
alike by both.  For the queries `near_ties` does flag, `rule_match` applies the rule to `associate_cases.dist2_emulated`, which is
dist2f bit for bit wherever the coordinate differences are exact in fp32 and their squares' partial sums in fp64: on the lattice, and
near +-4000 where fp32 steps in 2^-12 and the differences are small multiples of that."""
import math

import numpy as np
from scipy.spatial import cKDTree

from tests import associate_cases as ac
from tests import evaluate_cases as ec

F32 = np.float32
TIE_MARGIN = 2.0 ** -18
TIE_FREE = (["slab_origin", "slab_mid", "jobs", "jobs_single", "occupancy_single", "occupancy_many"]
            + [n for n, _, _ in ec.ALL if n.startswith("ratio_") or n.startswith("threshold_")])
DUPLICATES_ONLY = "occupancy_cells"
TIE_FAMILY = "slab_far"

_cache = {}


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------
def rows_of(points, about=None):
    """(n, 3, 6) float64: G1, G2, G3 of every point, (x, y, z) = (double)m - about"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if about is not None:
        p = p - np.asarray(about, dtype=np.float64).reshape(3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    o, l = np.zeros(len(p)), np.ones(len(p))
    return np.stack([np.stack([o, z, -y, l, o, o], 1), np.stack([-z, o, x, o, l, o], 1), np.stack([y, -x, o, o, o, l], 1)], 1)


def info_loop(points, about=None):
    """the definition, literally: one point and one row at a time"""
    A = np.zeros((6, 6))
    for G in rows_of(points, about):
        for r in range(3):
            A += np.outer(G[r], G[r])
    return A


def info_closed(points, about=None):
    """the closed form from the ten sums n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz (what the library assembles on the host)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if about is not None:
        p = p - np.asarray(about, dtype=np.float64).reshape(3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    n, sx, sy, sz = float(len(p)), x.sum(), y.sum(), z.sum()
    sxx, syy, szz, sxy, sxz, syz = (x * x).sum(), (y * y).sum(), (z * z).sum(), (x * y).sum(), (x * z).sum(), (y * z).sum()
    A = np.zeros((6, 6))
    A[:3, :3] = [[syy + szz, -sxy, -sxz], [-sxy, sxx + szz, -syz], [-sxz, -syz, sxx + syy]]
    A[:3, 3:] = [[0, -sz, sy], [sz, 0, -sx], [-sy, sx, 0]]
    A[3:, :3] = A[:3, 3:].T
    A[3:, 3:] = n * np.eye(3)
    return A


def info_reference(points, about=None):
    """(A, Aabs): every entry as math.fsum of its 3 n terms G_r[i] G_r[j] (each product rounded once, as the device rounds it), and
    the same sum with every term replaced by its absolute value -- the scale of the error bound"""
    G = rows_of(points, about)
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            t = (G[:, :, i] * G[:, :, j]).reshape(-1)
            A[i, j] = A[j, i] = math.fsum(t.tolist())
            B[i, j] = B[j, i] = math.fsum(np.abs(t).tolist())
    return A, B


def bound(n_corr, Aabs):
    """a sum of n doubles in any order errs by at most (n - 1) 2^-53 sum |t|; the entries are sums of up to two such sums"""
    return (n_corr + 4) * 2.0 ** -53 * Aabs


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def near_ties(fam, ref):
    """indices (into the jobs-back-to-back point layout of `ref`) of the queries whose second-nearest memory point WITH DIFFERENT
    COORDINATES lies within a factor 1 + 2^-18 of the nearest squared distance in fp64, and the number of matched queries whose match
    has exact duplicates in the memory (a tie that no choice makes visible).  Only queries whose nearest point can be accepted count -- nearest fp64 d2 <= thr^2 (1 + 2^-20),
    the band of evaluate_cases.in_band: beyond it the fp32 rule rejects every candidate, and which of them is nearer decides nothing
    (a query a metre above the slab is nearly equidistant to many of its points)."""
    key = ("near_ties", fam["name"])
    if key not in _cache:
        uniq, inv, cnt = np.unique(fam["mem"], axis=0, return_inverse=True, return_counts=True)
        repeated = cnt[inv.reshape(-1)] > 1
        dup = int(((ref["idx"] >= 0) & repeated[np.maximum(ref["idx"], 0)]).sum())
        q = ref["q"].astype(np.float64)
        if len(uniq) < 2 or not len(q):
            _cache[key] = (np.zeros(0, np.int64), dup)
        else:
            u64 = uniq.astype(np.float64)
            _, nb = cKDTree(u64).query(q, k=2)
            d1 = ((q - u64[nb[:, 0]]) ** 2).sum(1)
            d2 = ((q - u64[nb[:, 1]]) ** 2).sum(1)
            lo, hi = np.minimum(d1, d2), np.maximum(d1, d2)
            reach = lo <= fam["thr"] * fam["thr"] * (1.0 + ec.BAND)
            _cache[key] = (np.nonzero(reach & (hi <= lo * (1.0 + TIE_MARGIN)))[0], dup)
    return _cache[key]


def lex_smallest(rows):
    """the row of (k, 3) that comes first by (x, y, z)"""
    rows = np.asarray(rows)
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))[0]]


def rule_match(fam, q_rows):
    """the rule applied to dist2_emulated for the fp32 query rows: (xyz (k, 3) float32, d2 (k,) float32, ties (k,) int = the number of
    distinct coordinates at the minimal d2); (0, 0, 0), +inf and 0 where nothing lies below (float)(thr * thr)"""
    uniq = np.unique(fam["mem"], axis=0)
    tree = cKDTree(uniq.astype(np.float64))
    thr2 = F32(fam["thr"] * fam["thr"])
    xyz = np.zeros((len(q_rows), 3), F32)
    d2 = np.full(len(q_rows), np.inf, F32)
    ties = np.zeros(len(q_rows), np.int64)
    for i, q in enumerate(np.asarray(q_rows, F32)):
        cand = uniq[tree.query_ball_point(q.astype(np.float64), 1.5 * fam["thr"])]
        if not len(cand):
            continue
        d = ac.dist2_emulated(q[None], cand)[0]
        if d.min() < thr2:
            best = cand[d == d.min()]
            xyz[i], d2[i], ties[i] = lex_smallest(best), d.min(), len(best)
    return xyz, d2, ties


def expected_match(fam, ref):
    """(n, 3) float32: the matched coordinates the kernel owes for every point of `ref` -- mem[idx] of the brute force, and the rule's
    choice for the queries `near_ties` flags; (0, 0, 0) where there is no match"""
    key = ("expected", fam["name"])
    if key not in _cache:
        out = np.where((ref["idx"] >= 0)[:, None], fam["mem"][np.maximum(ref["idx"], 0)], F32(0)).astype(F32)
        tied, _ = near_ties(fam, ref)
        if len(tied):
            xyz, d2, _ = rule_match(fam, ref["q"][tied])
            assert d2.view(np.uint32).tolist() == ref["d2"][tied].view(np.uint32).tolist(), "dist2_emulated is not the brute force's d2 here"
            out[tied] = xyz
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


# ---- the lattice family: exact ties -----------------------------------------------------------------------------------------------------
HALF = 400                               # lattice steps from a query to each of its candidates: 400 sqrt(3) = 693 < 1310 = thr
METRE = 65536                            # 25 cells exactly: the cell faces repeat
MID = ac.CORNER + 1310                   # the middle of the cell that begins at CORNER (a cell is 2621.44 steps wide)
KINDS = {"x": [(1, 0, 0), (-1, 0, 0)], "y": [(0, 1, 0), (0, -1, 0)], "z": [(0, 0, 1), (0, 0, -1)],
         "diagonal": [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]}          # (each listed in DESCENDING order)


def lattice_steps():
    """(mem steps (24, 3), query steps (8, 3), kinds, candidate counts): per kind one query in the middle of a cell and one at
    CORNER, where a cell face passes between the candidates on every axis that differs; the groups lie a metre or more apart, on
    both sides of zero.  A group's candidates are stored in DESCENDING (x, y, z) order: the lowest index is never the rule's choice."""
    mem, qs, kinds, counts = [], [], [], []
    for k, (kind, offs) in enumerate(KINDS.items()):
        for place, at in (("inside", MID), ("face", ac.CORNER)):
            base = np.array([(k - 2) * METRE, (1 - k) * METRE, (k % 2 - 1) * METRE], np.int64)
            P = base + at
            mem += [P + HALF * np.array(o, np.int64) for o in offs]
            qs.append(P)
            kinds.append(f"{kind} {place}")
            counts.append(len(offs))
    return np.array(mem), np.array(qs), kinds, counts


def lattice_family():
    """jobs: all queries under the identity; the four queries inside a cell; the four at a face (candidates in different cells);
    the four at a face again, stored shifted by (3, -2, 5) lattice steps and brought back by the job's transform"""
    key = ("family", "lattice_ties")
    if key not in _cache:
        mem, qs, kinds, _ = lattice_steps()
        inside = [i for i, k in enumerate(kinds) if k.endswith("inside")]
        face = [i for i, k in enumerate(kinds) if k.endswith("face")]
        shift = np.array([3, -2, 5], np.int64)
        det = np.concatenate([qs, qs[inside], qs[face], qs[face] - shift])
        back = ec.shifted(ac.lattice(shift))
        jobs = [(0, 8, np.eye(4), "all"), (8, 12, np.eye(4), "inside a cell"), (12, 16, np.eye(4), "across faces"), (16, 20, back, "across faces, shifted")]
        _cache[key] = ec._family("lattice_ties", ac.lattice(mem), ac.lattice(det), jobs, ec.CELL, ec.THR)
    return _cache[key]


def lattice_expected(fam, ref):
    """(n, 3) float32 by the rule, in integer arithmetic: of the memory points at the minimal `dist2_integer` the first by (x, y, z)"""
    mem = ac.steps_of(fam["mem"].astype(np.float64))
    q = ac.steps_of(ref["q"].astype(np.float64))
    d = ac.dist2_integer(q, mem)
    out = np.zeros((len(q), 3), F32)
    counts = []
    for i in range(len(q)):
        best = mem[d[i] == d[i].min()]
        counts.append(len(best))
        out[i] = ac.lattice(lex_smallest(best)).astype(F32)
    return out, counts


def get(name):
    return lattice_family() if name == "lattice_ties" else ec.get(name)
