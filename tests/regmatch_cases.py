"""Feature matching and RANSAC alone, on INJECTED instance features: the helper that writes crafted FPFH rows into an `InstanceFeatures`
object, the numpy restatement of the fp16 search operands, the expected values from the oracle, and the job sets of the matching stage
(csrc/reg_match.hip + csrc/reg_featnn.hip).  Shared by tests/test_regmatch_model.py (CPU: every family is what it claims),
tests/test_gpu_regmatch.py (GPU) and tests/ransac_cases.py (the RANSAC families use the same helper with trivially separable rows).

The way in: `ibl_register_jobs` uses the FPFH rows of caller-supplied instance features as they are for every instance that is further
than the influence radius from the other instances of its job side (include/ibloc.h; `reuse[1] == 0` shows it happened).  Rows written
into the features therefore decide the correspondence list exactly; `ransac_stats` and `T_ransac` are read back before ICP touches
anything, and hypothesis i draws floor(r * n_corr) from the ORDERED list, so those two outputs pin content, order and length of the list.

A family is a dict
    det, mem            lists of (n, 3) float32 clouds: the two pools
    det_rows, mem_rows  lists of (n, 33) float32 crafted FPFH rows in NATURAL bin order (what the oracle takes; the features store
                        rows[:, FEAT_ORDER])
    js, jt              (J, 3) int32 job tables, padded with -1 (an empty slot may sit in the middle)
    tags                per job a short name of what the job is there for
    center, seed, job_ids (J,) uint32, max_iter, fixed_budget      the call

Rule for crafted rows: non-negative, every 11-bin histogram sums to at most 200 (the domain the fp16 operands are dimensioned for), and
values such that every squared distance between two rows of a job and every centred norm is exactly representable in fp32 (integers, or
multiples of 2^-6 with bounded sums): summation order cannot matter, a tie is a true tie, and the oracle's fp32 chain equals the fp64
value.  `exactness(fam)` measures this; the CPU model tests assert it for every family, the GPU tests do not assume it."""
import numpy as np
from scipy.spatial.transform import Rotation

from ibloc_amd.registration import FEAT_MU, FEAT_ORDER
from tests.icp_cases import job_arrays, sub_family          # noqa: F401  (re-exported: the same job conventions as the ICP families)

VOXEL = 0.05
GLOBAL = 1.5
LOCAL = 1.5
MAX_DIST = VOXEL * GLOBAL                  # RANSAC correspondence distance
GRAD_RADIUS = 2 * VOXEL * LOCAL            # what memory features need their colour gradients for
FM_C, FM_A = 1.0e-3, 4.0e-3                # the filter's band E = FM_C (|q|^2 + |t|^2) + FM_A (csrc/reg_featnn.hip)

MU_NAT = np.empty(33, np.float32)          # the centring constant in natural bin order
MU_NAT[FEAT_ORDER] = FEAT_MU
# the row every crafted row starts from: MU with the centre bins of histograms 0 and 2 one lower (MU's histograms sum to 201, 199, 201)
BASE = MU_NAT.copy().reshape(3, 11)
BASE[0, 5] -= 1
BASE[2, 5] -= 1
assert BASE.sum(1).max() <= 200

_cache = {}


def memo(fn):
    def wrapped(*args):
        key = (fn.__module__, fn.__name__) + args
        if key not in _cache:
            _cache[key] = fn(*args)
        return _cache[key]
    wrapped.__name__ = fn.__name__
    wrapped.__doc__ = fn.__doc__
    return wrapped


# ------------------------------------------------------------------------------------------------
# the fp16 search operands (numpy restatement of fm_centred_norm / fm_operand_piece, csrc/reg_common.h)
# ------------------------------------------------------------------------------------------------
def _fmaf(v, a):
    """fp32 fmaf(v, v, a) of float32 arrays: the product is exact in fp64; the fp64 sum is rounded TO ODD (TwoSum gives the exact error of
    the nearest sum), so the second rounding to fp32 is the correct rounding of the exact value"""
    p = v.astype(np.float64) * v.astype(np.float64)
    a = a.astype(np.float64)
    s = a + p
    bb = s - a
    err = (a - (s - bb)) + (p - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def stored_rows(rows):
    """natural bin order -> the matching order instance features store"""
    return np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 33)[:, FEAT_ORDER])


def centred_norm(stored):
    """squared norm of the centred rows: the fp32 fmaf chain over the bins in matching order"""
    x = np.asarray(stored, np.float32).reshape(-1, 33)
    a = np.zeros(len(x), np.float32)
    for k in range(33):
        a = _fmaf(x[:, k] - FEAT_MU[k], a)
    return a


def operand_rows(stored, norm):
    """-> (n, 48) float16: 33 centred values | 8 8 | norm / 8 as hi + lo | 1e-3 norm + 4e-3 rounded UP | zeros"""
    x = np.asarray(stored, np.float32).reshape(-1, 33)
    a = np.asarray(norm, np.float32)
    op = np.zeros((len(x), 48), np.float16)
    op[:, :33] = (x - FEAT_MU[None, :]).astype(np.float16)
    op[:, 33] = op[:, 34] = 8.0
    w = a * np.float32(0.125)
    nh = w.astype(np.float16)
    op[:, 35] = nh
    op[:, 36] = (w - nh.astype(np.float32)).astype(np.float16)
    cw = np.float32(1.0e-3) * a + np.float32(4.0e-3)
    cu = cw.astype(np.float16)
    low = cu.astype(np.float32) < cw
    op[:, 37] = np.where(low, (cu.view(np.uint16) + low.astype(np.uint16)).view(np.float16), cu)
    return op


# ------------------------------------------------------------------------------------------------
# injection
# ------------------------------------------------------------------------------------------------
def inject(feat, rows_list):
    """overwrites fpfh (rows in matching order), fpfh_norm and, for the resident form, fpfh_split of an InstanceFeatures object made by
    instance_features_batch; its normals, gradients and bbox stay the computed ones unless `inject_geometry` overwrites them too (the
    coloured ICP behind RANSAC reads normals and gradients, the planner reads bbox)"""
    import torch
    rows = np.concatenate([np.asarray(r, np.float32).reshape(-1, 33) for r in rows_list]) if rows_list else np.zeros((0, 33), np.float32)
    assert len(rows) == feat.n
    if feat.n == 0:
        return feat
    st = stored_rows(rows)
    norm = centred_norm(st)
    dev = feat.fpfh.device
    feat.fpfh[:feat.n].copy_(torch.from_numpy(st).to(dev))
    feat.fpfh_norm[:feat.n].copy_(torch.from_numpy(norm).to(dev))
    if feat.fpfh_split is not None:
        feat.fpfh_split[:feat.n].copy_(torch.from_numpy(operand_rows(st, norm).view(np.int16)).to(dev).view(torch.float16))
    return feat


def inject_geometry(feat, nrm_list, grad_list):
    """overwrites the x, y, z lanes of the normals and colour gradients of an InstanceFeatures object made by instance_features_batch
    with grad_radius > 0 (one (n, 3) array per instance): what the coloured ICP reads of its target side (tests/icp_colour_cases.py).
    The w lanes stay as computed."""
    import torch
    if feat.n == 0:
        return feat
    for dst, rows_list in ((feat.normals, nrm_list), (feat.grad, grad_list)):
        rows = np.concatenate([np.asarray(r, np.float32).reshape(-1, 3) for r in rows_list])
        assert len(rows) == feat.n
        dst[:feat.n, :3].copy_(torch.from_numpy(rows).to(dst.device))
    return feat


def pools(ctx, fam, compact=False):
    """-> (det batch, mem batch, det features, mem features) with the family's rows injected"""
    from ibloc_amd.registration import CloudBatch, instance_features_batch
    det, mem = CloudBatch.from_numpy(fam["det"]), CloudBatch.from_numpy(fam["mem"])
    fd = inject(instance_features_batch(ctx, det, VOXEL, compact=compact), fam["det_rows"])
    fm = inject(instance_features_batch(ctx, mem, VOXEL, grad_radius=GRAD_RADIUS, compact=compact), fam["mem_rows"])
    return det, mem, fd, fm


def run(ctx, fam, p, jobs=None, fixed_budget=None):
    """one register_batch call on the pools `p` of `pools()`: all jobs of the family, or only `jobs` (with their own job ids)"""
    from ibloc_amd.registration import register_batch
    sel = np.arange(len(fam["js"])) if jobs is None else np.asarray(jobs, dtype=np.int64)
    det, mem, fd, fm = p
    out = register_batch(ctx, det, mem, fam["js"][sel], fam["jt"][sel], VOXEL, GLOBAL, LOCAL, seed=fam["seed"], ransac_max_iter=fam["max_iter"],
                         have_colors=True, center=fam["center"], det_features=fd, mem_features=fm, job_ids=fam["job_ids"][sel],
                         fixed_budget=fam["fixed_budget"] if fixed_budget is None else fixed_budget)
    assert out["reuse"][1] == 0, out["reuse"]              # every row was served from the (injected) instance features
    return out


# ------------------------------------------------------------------------------------------------
# families and their expected values
# ------------------------------------------------------------------------------------------------
def _pad(rows):
    return np.array([list(r) + [-1] * (3 - len(r)) for r in rows], dtype=np.int32).reshape(-1, 3)


def family(det, mem, det_rows, mem_rows, js, jt, tags, center=False, seed=(7 << 32) | 5, job_ids=None, max_iter=100000, fixed_budget=False):
    f32 = lambda L, w: [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, w) for c in L]
    fam = dict(det=f32(det, 3), mem=f32(mem, 3), det_rows=f32(det_rows, 33), mem_rows=f32(mem_rows, 33), det_int=None, mem_int=None,
               js=_pad(js), jt=_pad(jt), tags=list(tags), center=center, seed=int(seed), max_iter=int(max_iter), fixed_budget=fixed_budget)
    J = len(fam["js"])
    fam["job_ids"] = (np.arange(J, dtype=np.uint32) + 11) if job_ids is None else np.asarray(job_ids, dtype=np.uint32)
    assert len(fam["jt"]) == len(fam["tags"]) == len(fam["job_ids"]) == J
    for clouds, rows in ((fam["det"], fam["det_rows"]), (fam["mem"], fam["mem_rows"])):
        assert [len(c) for c in clouds] == [len(r) for r in rows]
    fam["_expected"] = {}
    return fam


def job_rows(fam, j):
    """-> (source rows, target rows) of job j, concatenated in slot order (natural bin order)"""
    out = []
    for rows, seg in ((fam["det_rows"], fam["js"][j]), (fam["mem_rows"], fam["jt"][j])):
        ids = [int(s) for s in seg if s >= 0]
        out.append(np.concatenate([rows[s] for s in ids]) if ids else np.zeros((0, 33), np.float32))
    return out


def expected(fam, j, fixed_budget=None):
    """the oracle on job j -> (corr (n_corr, 2), T_ransac, stats): feature_match on the job's concatenated rows, ransac on the job's
    clouds (centred the way the product centres them) with the job's id"""
    from oracle import reg_oracle as ro
    fixed = fam["fixed_budget"] if fixed_budget is None else fixed_budget
    key = (j, fixed)
    if key not in fam["_expected"]:
        fs, ft = job_rows(fam, j)
        a = job_arrays(fam, j)
        corr = ro.feature_match(fs, ft)
        # a fixed budget is the loop without its confidence exit: with confidence 1 the bound log(0) / log(..) never tightens est_k
        T, stats = ro.ransac(a["src"], a["tgt"], corr, MAX_DIST, fam["seed"], int(fam["job_ids"][j]), fam["max_iter"],
                             confidence=1.0 if fixed else 0.99)
        fam["_expected"][key] = (corr, T, stats)
    return fam["_expected"][key]


def exactness(fam):
    """-> (largest squared distance between two rows of a job, largest centred norm), after asserting that every one of them -- and with it
    every partial sum of its chain -- is exactly representable in fp32 and that the rows lie in the operands' domain"""
    worst_d2 = worst_n = 0.0
    for rows in fam["det_rows"] + fam["mem_rows"]:
        if len(rows) == 0:
            continue
        assert (rows >= 0).all() and rows.reshape(-1, 3, 11).sum(2).max() <= 200.0
        assert np.array_equal(rows * 64, np.round(rows * 64))               # the grid `distances` is exact on
        n = ((rows.astype(np.float64) - MU_NAT) ** 2).sum(1)
        assert np.array_equal(n, n.astype(np.float32).astype(np.float64))
        assert np.array_equal(centred_norm(stored_rows(rows)).astype(np.float64), n)
        worst_n = max(worst_n, n.max())
    for j in range(len(fam["js"])):
        fs, ft = job_rows(fam, j)
        if len(fs) == 0 or len(ft) == 0:
            continue
        d2 = distances(fs, ft)
        assert np.array_equal(d2, d2.astype(np.float32).astype(np.float64)), fam["tags"][j]
        worst_d2 = max(worst_d2, d2.max())
    return worst_d2, worst_n


def distances(fs, ft):
    """(ns, nt) squared distances in fp64 as |a|^2 + |b|^2 - 2 a.b: exact for crafted rows (multiples of 2^-6 up to 200: every product and
    partial sum fits fp64's 53 bits, in any order), which `exactness` relies on"""
    fs, ft = fs.astype(np.float64), ft.astype(np.float64)
    return (fs * fs).sum(1)[:, None] + (ft * ft).sum(1)[None, :] - 2.0 * (fs @ ft.T)


def tie_counts(fs, ft):
    """per query row of fs: (rows of ft at exactly the minimum distance, rows inside the filter's band 1e-3 (|q|^2 + |t|^2) of it), fp64"""
    d2 = distances(fs, ft)
    nq = ((fs.astype(np.float64) - MU_NAT) ** 2).sum(1)
    nt = ((ft.astype(np.float64) - MU_NAT) ** 2).sum(1)
    m = d2.min(1, keepdims=True)
    return (d2 == m).sum(1), (d2 <= m + FM_C * (nq[:, None] + nt[None, :])).sum(1)


# ------------------------------------------------------------------------------------------------
# row builders
# ------------------------------------------------------------------------------------------------
CODE_BINS = ((0, 3), (1, 3), (2, 3), (0, 7), (1, 7), (2, 7))          # (histogram, bin) of the six base-5 digits of a code row


def code_rows(idx):
    """well-separated rows: BASE with the six base-5 digits of idx (< 15 625) written as 4 * digit into six bins and taken off the centre
    bin of the same histogram.  Two different codes are at least 16 + 16 apart (squared), equal codes at 0."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < 5 ** 6)
    rows = np.tile(BASE[None], (len(idx), 1, 1))
    for k, (h, c) in enumerate(CODE_BINS):
        d = ((idx // 5 ** k) % 5).astype(np.float32)
        rows[:, h, c] += 4 * d
        rows[:, h, 5] -= 4 * d
    return rows.reshape(-1, 33)


def _settle(rows):
    """takes what a perturbation added to a histogram off its largest bins again, so that no histogram sums to more than 200"""
    r = rows.reshape(-1, 11).copy()
    over = np.maximum(r.sum(1) - 200.0, 0.0)
    while over.any():
        k = r.argmax(1)
        take = np.minimum(over, np.floor(r[np.arange(len(r)), k] / 2))
        r[np.arange(len(r)), k] -= take
        over -= take
    assert (r >= 0).all() and r.sum(1).max() <= 200.0
    return r.reshape(-1, 33)


def cluster_rows(rng, n, n_centres=30, spread=6, noise=2, centres=None):
    """rows that compete: integer rows drawn around n_centres centres (BASE +- spread; or the given ones), each +- noise"""
    if centres is None:
        centres = rng.integers(-spread, spread + 1, size=(n_centres, 33))
    rows = BASE.reshape(1, 33) + centres[rng.permutation(n) % len(centres)] + rng.integers(-noise, noise + 1, size=(n, 33))
    return _settle(np.maximum(rows, 0).astype(np.float32))


def jitter(rng, rows, amp=1):
    return _settle(np.maximum(rows + rng.integers(-amp, amp + 1, size=rows.shape), 0).astype(np.float32))


# ------------------------------------------------------------------------------------------------
# geometry of the matching families: trivial on purpose
# ------------------------------------------------------------------------------------------------
PITCH = 0.2           # lattice pitch of the clouds; with a jitter of +- 0.02 two points are at least 0.16 m > 2 MAX_DIST apart
G_ROT = Rotation.from_euler("xyz", [4.0, -3.0, 6.0], degrees=True).as_matrix()
G_SHIFT = np.array([0.11, -0.07, 0.05])
PLACE_NOISE = 0.002   # a right target lies within 2 mm (per axis) of its source's rigid copy: an inlier, and T depends on the draw


def lattice_cloud(rng, n, slot=0):
    """n points of a jittered 12 x 12 x 12 lattice (a 2.4 m cube), `slot` cubes of 4 m further along x: instances of one side are 1.6 m apart"""
    assert n <= 1728
    sites = rng.permutation(1728)[:n]
    ijk = np.stack([sites // 144, (sites // 12) % 12, sites % 12], 1).astype(np.float64)
    return ijk * PITCH + rng.uniform(-0.02, 0.02, size=(n, 3)) + np.array([4.0 * slot, 0.0, 0.0])


def copy_of(cloud):
    return np.asarray(cloud, np.float64).reshape(-1, 3) @ G_ROT.T + G_SHIFT


def first_nearest(fq, fd):
    """per row of fq the index of its nearest row of fd, the lowest among equals: numpy on the exact fp64 distances of crafted rows"""
    return np.argmin(distances(fq, fd), axis=1)


def instance_pair(rng, ns, nt, rows_s, rows_t, slot=0):
    """-> (source cloud, target cloud) of an instance pair whose geometry tells WHICH target row a source was matched to: target k lies on
    the rigid copy of the first source whose nearest row (lowest index among equals) it carries, within PLACE_NOISE; a target that is
    nobody's nearest row lies on a lattice site of its own.  The correspondence (i, k) is then an inlier exactly when k is the right
    answer for i and i is the first source with that answer; every other pairing is at least 0.16 m - noise off.  A wrong choice between
    tied or nearly tied rows therefore costs an inlier, a wrong mutual verdict changes the length of the list and with it every draw."""
    pts = lattice_cloud(rng, ns + nt, slot)
    src, tgt = pts[:ns], copy_of(pts[ns:])
    if ns and nt:
        nn = first_nearest(rows_s, rows_t)
        for i in range(ns - 1, -1, -1):
            tgt[nn[i]] = copy_of(src[i])[0] + rng.uniform(-PLACE_NOISE, PLACE_NOISE, size=3)
    return src, tgt


# ------------------------------------------------------------------------------------------------
# matching families
# ------------------------------------------------------------------------------------------------
SIZES = (1, 31, 32, 33, 255, 256, 257, 600)


@memo
def sizes():
    """ns / nt of 1, 31, 32, 33, 255, 256, 257, 600 against each other (64 jobs, 8 + 8 instances, every (query instance, database
    instance) pair once per direction): query tiles of 32 / 64 / 256, 32-row database chunks and the last partial chunk, nt < 32, the
    chunks pass 1 skips.  Instances are leading parts of one 600-point master cloud whose rows compete (30 centres); both sides carry
    the master rows with their own +- 2 jitter, so most but not all nearest rows are the right ones.  The geometry of target instance b
    is laid out against source instance b (`instance_pair`); in the jobs a != b the leading min(ns, nt) rows still correspond."""
    rng = np.random.default_rng(301)
    master = cluster_rows(rng, 600)
    det_rows = [jitter(rng, master[:n], 2) for n in SIZES]
    mem_rows = [jitter(rng, master[:n], 2) for n in SIZES]
    clouds = [instance_pair(rng, n, n, det_rows[k], mem_rows[k]) for k, n in enumerate(SIZES)]
    det, mem = [c[0] for c in clouds], [c[1] for c in clouds]
    js = [[a] for a in range(8) for b in range(8)]
    jt = [[b] for a in range(8) for b in range(8)]
    tags = ["%d x %d" % (SIZES[a], SIZES[b]) for a in range(8) for b in range(8)]
    return family(det, mem, det_rows, mem_rows, js, jt, tags, max_iter=60000)


def _tie_side(n, g):
    """rows of a side of n points: point k carries code g.get(k, k)"""
    return code_rows([g.get(k, k) for k in range(n)])


@memo
def ties():
    """exact ties, decided by the lowest concatenated index in both directions.
    job 0  duplicated database rows: inside a chunk (targets 3, 17), across a chunk boundary (30, 34) and between a chunk pass 1 reads and
           one it skips (20 in chunk 0, 40 in chunk 1, 66 in chunk 2); the tied sources are 3, 30, 20
    job 1  duplicated query rows (sources 7, 8 and 12, 45, 50): every copy finds the same target, the target finds the first copy
    job 2  source 5 is equally far (4) from targets 5 and 9; target 5 is nearer (1) to source 6, so the lowest index is NOT mutual and
           source 5 leaves the list although target 9 would have kept it
    job 3  job 0's rows with the roles swapped (the ties are met by the reverse search, on a short need list)
    jobs 4, 5  2 and 3 pieces per side; a row of target piece 0 comes again in pieces 1 and 2, and a source row in source pieces 1 / 2;
           job 5 lists its pieces in another order than the pool does: lowest CONCATENATED index, not lowest pool index"""
    rng = np.random.default_rng(311)
    det, mem, det_rows, mem_rows, js, jt, tags = [], [], [], [], [], [], []

    def add_pair(n_s, n_t, rows_s, rows_t, slot=0):
        src, tgt = instance_pair(rng, n_s, n_t, rows_s, rows_t, slot)
        det.append(src); mem.append(tgt); det_rows.append(rows_s); mem_rows.append(rows_t)
        return len(det) - 1

    g0 = {17: 3, 34: 30, 40: 20, 66: 20}
    k = add_pair(70, 70, _tie_side(70, {}), _tie_side(70, g0))
    js.append([k]); jt.append([k]); tags.append("duplicated database rows")
    k = add_pair(60, 60, _tie_side(60, {8: 7, 45: 12, 50: 12}), _tie_side(60, {}))
    js.append([k]); jt.append([k]); tags.append("duplicated query rows")
    # job 2: offsets in two bins the codes leave alone (histogram 0, bins 0 and 1), downwards so that no sum grows
    rs, rt = _tie_side(40, {}), _tie_side(40, {})
    rt[9] = rs[5]
    rt[5, 0] -= 2              # target 5 = code 5 + (-2, 0)
    rt[9, 1] -= 2              # target 9 = code 5 + (0, -2): source 5 is 4 from both
    rs[6] = rs[5]
    rs[6, 0] -= 2
    rs[6, 1] -= 1              # source 6 = code 5 + (-2, -1): 1 from target 5, 5 from target 9
    k = add_pair(40, 40, rs, rt)
    js.append([k]); jt.append([k]); tags.append("tie between a non-mutual and a mutual target")
    k = add_pair(70, 70, _tie_side(70, g0), _tie_side(70, {}))
    js.append([k]); jt.append([k]); tags.append("duplicated rows met by the reverse search")
    # pieces: codes 100 + .. so that nothing collides with the jobs above
    first = len(det)
    sizes_p = (40, 33, 50)
    for p, n in enumerate(sizes_p):
        base = 100 + 100 * p
        g_s = {k: k for k in range(n)}
        g_t = {k: k for k in range(n)}
        if p > 0:
            g_t[2 * p] = 100 + 7 - base           # target piece p row 2p = code 107 = row 7 of target piece 0
            g_s[3 * p] = 100 + 11 - base          # source piece p row 3p = code 111 = row 11 of source piece 0
        rows_s = code_rows([base + g_s[k] for k in range(n)])
        rows_t = code_rows([base + g_t[k] for k in range(n)])
        add_pair(n, n, rows_s, rows_t, slot=p)
    js.append([first, first + 1]); jt.append([first, first + 1]); tags.append("ties across 2 pieces")
    js.append([first + 2, first, first + 1]); jt.append([first + 1, first + 2, first]); tags.append("ties across 3 pieces, other order")
    return family(det, mem, det_rows, mem_rows, js, jt, tags)


def _square_pairs(lo, hi, limit):
    """pairs ((x, y), (x2, y2)), 0 <= y <= x <= limit, with x2^2 + y2^2 = x^2 + y^2 + 1 and lo <= x^2 + y^2 < hi"""
    by_sum = {}
    for x in range(limit + 1):
        for y in range(x + 1):
            by_sum.setdefault(x * x + y * y, (x, y))
    return [(by_sum[s], by_sum[s + 1]) for s in sorted(by_sum) if lo <= s < hi and s + 1 in by_sum]


def _edge_row(h_main, moves):
    """a row at the edge of the domain: 200 in bin h_main[h] of histogram h, nothing elsewhere; moves[h] = (x, y): x taken off that
    bin, y put into the bin behind it (x >= y: the sum does not grow)"""
    r = np.zeros((3, 11), np.float32)
    for h in range(3):
        x, y = moves[h]
        r[h, h_main[h]] = 200 - x
        r[h, h_main[h] + 1] = y
    return r.reshape(33)


def _frac_row(k_main, k_small):
    """a row whose fp16 operands are INEXACT: the centre bins of histograms 0 and 1 lowered by 32 .. 40 in steps of 2^-6 (fp16 keeps
    2^-5 there), the rest of BASE lowered by k_small / 64; k in units of 2^-6"""
    r = BASE.copy()
    r[0, 5] -= 32 + k_main[0] / 64.0
    r[1, 5] -= 32 + k_main[1] / 64.0
    r = r.reshape(33)
    r[np.array([0, 1, 2, 11, 12, 22, 23])] -= np.asarray(k_small, np.float32) / 64.0
    return r


@memo
def near_ties():
    """pairs of database rows whose exact distances to a query differ by the smallest amount the rows' grid allows, the FARTHER one at
    the lower index: the filter must pass both (the difference is orders of magnitude inside its band), the exact re-check must choose.
    jobs 0, 1  rows at the edge of the domain (200 in one bin per histogram, centred norms ~ 1.2e5, band ~ 240): integer rows, distances
               d and d + 1 for d from 1 to ~ 40 000; job 1 = job 0 with the roles swapped (the reverse search)
    jobs 2, 3  rows on a 2^-6 grid around -32 .. -40 centred, which fp16 does not hold exactly (the operands really are approximate):
               distances d and d + 2^-12 for d from 2^-12 to 0.5; job 3 = job 2 swapped"""
    rng = np.random.default_rng(321)
    det, mem, det_rows, mem_rows, js, jt, tags = [], [], [], [], [], [], []

    def add(rows_s, rows_t, tag):
        for swap in (False, True):
            a, b = (rows_t, rows_s) if swap else (rows_s, rows_t)
            src, tgt = instance_pair(rng, len(a), len(b), a, b)
            det.append(src); mem.append(tgt); det_rows.append(a); mem_rows.append(b)
            js.append([len(det) - 1]); jt.append([len(det) - 1]); tags.append(tag + (", swapped" if swap else ""))

    # edge rows: query q (200 in the main bins of its group), then per pair the farther row first.  Groups of queries use different
    # main bins, so that rows of different groups are ~ 2.4e5 apart and do not interfere
    pairs = _square_pairs(1, 40000, 199)
    pairs = [pairs[i] for i in np.linspace(0, len(pairs) - 1, 36).astype(int)]
    rows_s, rows_t = [], []
    for gi, p in enumerate(pairs):
        h_main = ((gi % 9) + 0, ((gi // 3) % 3) * 3, (gi % 4) * 2)
        near, far = p
        h = gi % 3
        zero = [(0, 0)] * 3
        # every query gets its own offset in another histogram, so that the 36 queries are distinct rows
        q_moves = list(zero); q_moves[(h + 1) % 3] = (gi // 9 + 1, 0)
        mv_far = list(q_moves); mv_far[h] = far
        mv_near = list(q_moves); mv_near[h] = near
        rows_s.append(_edge_row(h_main, q_moves))
        rows_t += [_edge_row(h_main, mv_far), _edge_row(h_main, mv_near)]
    add(np.array(rows_s), np.array(rows_t), "edge of the domain")
    # fractional rows: in units of 2^-6, query k_main = (128, 128); pairs differ by 1 in the sum of squares of their offsets
    pairs = _square_pairs(1, 2000, 60)                 # distances below 0.5: nearer than any row of another query (>= 1)
    pairs = [pairs[i] for i in np.linspace(0, len(pairs) - 1, 30).astype(int)]
    rows_s, rows_t = [], []
    for gi, (near, far) in enumerate(pairs):
        small = [(gi >> b) & 1 for b in range(5)] + [gi // 32, 0]
        small = [64 * s for s in small]                # queries differ by 1 or more in some bin
        rows_s.append(_frac_row((256, 256), small))
        rows_t += [_frac_row((256 + far[0], 256 - far[1]), small), _frac_row((256 + near[0], 256 - near[1]), small)]
    add(np.array(rows_s), np.array(rows_t), "fp16-inexact rows")
    return family(det, mem, det_rows, mem_rows, js, jt, tags)


@memo
def crowded():
    """a few queries with several hundred candidates each: the database holds a cluster of 600 near-identical rows (3^6 = 729 patterns of
    0 / -1 / -2 in six bins around a centre whose centred norm is ~ 5 000: band ~ 10, distances inside the cluster <= 24), so a wave's
    256-entry candidate queue flushes more than once.  ns * nt = 40 * 640 stays far below the default candidate list (8 outputs +
    65 536): the list cannot overflow, status bit 16 stays clear.  Job 1 = the roles swapped: 600 sources match the same few targets
    (targets matched by many sources; their reverse search is the crowded one)."""
    rng = np.random.default_rng(331)
    centre = BASE.copy()
    centre[0, 5] -= 40; centre[0, 4] += 20; centre[0, 6] += 20          # centred norm 1600 + 400 + 400 + ...
    centre[1, 5] -= 40; centre[1, 4] += 20; centre[1, 6] += 20
    centre[2, 5] -= 30; centre[2, 4] += 15; centre[2, 6] += 15
    centre = centre.reshape(33)
    bins = np.array([0, 1, 2, 11, 22, 23])
    pat = rng.permutation(729)[:600]
    cluster = np.tile(centre, (600, 1))
    for b in range(6):
        cluster[:, bins[b]] -= (pat // 3 ** b) % 3
    near = np.tile(centre, (4, 1))
    near[1, 0] -= 1
    near[2, 8] -= 1                      # (a bin the cluster does not vary)
    near[3, 1] -= 2; near[3, 11] -= 1
    far = code_rows(np.arange(36) + 50)
    q = np.concatenate([far[:10], near[:2], far[10:30], near[2:], far[30:]])
    db = np.concatenate([cluster[:300], jitter(rng, code_rows(np.arange(40) + 50), 1), cluster[300:]])
    a, b = instance_pair(rng, 40, 640, q, db), instance_pair(rng, 640, 40, db, q)
    det, mem = [a[0], b[0]], [a[1], b[1]]
    return family(det, mem, [q, db], [db, q], [[0], [1]], [[0], [1]], ["few queries, crowded database", "crowded queries, few database rows"])


def _mutual_job(ns, M):
    """sources carry code(i); the targets are code(m) for m in M, then four more copies of each: exactly |M| pairs are mutual (per code
    the source that owns it and the first target that carries it); every other target is matched by nobody.  (Few targets on purpose:
    every source has all copies of its nearest code as candidates, and the default candidate list must not overflow.)"""
    M = sorted(M)
    assert max(M) < ns
    return code_rows(np.arange(ns)), code_rows(M + [M[k % len(M)] for k in range(4 * len(M))])


@memo
def mutual():
    """the mutual filter and its ordered compaction (ibl_mutual_kernel), and the reverse search on short need lists.
    job 0  exactly 8 mutual pairs: fewer than 9, so ALL ns source matches are the list      job 1  exactly 9: the 9 are the list
    job 2  ns = 700, 30 mutual pairs in all three 256-blocks of the compaction, on block and wave edges (0, 63, 64, 255, 256, 511, 512, 699)
    job 3  ns = 700, mutual pairs in blocks 0 and 2 only      job 4  ns = 300 with ONE mutual pair (there is always one: the closest pair
           with the lowest indices), so the fallback again
    Only the first target of every code is matched (a need list of |M| of 5 |M| targets), most of them by many sources."""
    rng = np.random.default_rng(341)
    spread = sorted(set([0, 63, 64, 255, 256, 300, 511, 512, 699] + rng.permutation(700)[:21].tolist()))
    ends = sorted(set([1, 2, 60, 64, 65, 200, 255] + [512, 513, 600, 640, 698, 699]))
    spec = [(40, list(range(3, 11)), "8 mutual pairs"), (40, list(range(3, 12)), "9 mutual pairs"),
            (700, spread, "700, all three blocks"), (700, ends, "700, block 1 empty"), (300, [137], "one mutual pair")]
    det, mem, det_rows, mem_rows, js, jt, tags = [], [], [], [], [], [], []
    for ns, M, tag in spec:
        rs, rt = _mutual_job(ns, M)
        src, tgt = instance_pair(rng, ns, len(rt), rs, rt)
        det.append(src); mem.append(tgt); det_rows.append(rs); mem_rows.append(rt)
        js.append([len(det) - 1]); jt.append([len(det) - 1]); tags.append(tag)
    fam = family(det, mem, det_rows, mem_rows, js, jt, tags)
    fam["mutual_sets"] = [sorted(set(s[1])) for s in spec]
    return fam


@memo
def pieces():
    """2 and 3 instances per side of unequal size (40, 75, 33, 257 points), 1.6 m apart; every instance draws its rows around the same 30
    centres, so a point's nearest row may lie in any piece of the other side.  The same (query instance, database instance) pair
    serves several jobs (fewer distinct pairs than pair uses), instance 0 is slot 0 of one job and slot 2 of another, one job leaves
    its middle slot empty, one lists its pieces in reverse, one has sides of 3 and 2 pieces."""
    rng = np.random.default_rng(351)
    n = (40, 75, 33, 257)
    centres = rng.integers(-6, 7, size=(30, 33))
    master = [cluster_rows(rng, k, centres=centres) for k in n]
    det_rows = [jitter(rng, m, 2) for m in master]
    mem_rows = [jitter(rng, m, 2) for m in master]
    clouds = [instance_pair(rng, k, k, det_rows[slot], mem_rows[slot], slot) for slot, k in enumerate(n)]
    det, mem = [c[0] for c in clouds], [c[1] for c in clouds]
    js = [[0, 1], [0, 1, 2], [2, -1, 0], [1, 0], [0], [3, 1, 0], [3]]
    jt = [[0, 1], [0, 1, 2], [2, -1, 0], [1, 0], [0], [1, 3], [3]]
    tags = ["2 + 2", "3 + 3", "middle slot empty", "reversed", "single", "3 + 2", "single 257"]
    return family(det, mem, det_rows, mem_rows, js, jt, tags)


FAMILIES = {"sizes": sizes, "ties": ties, "near_ties": near_ties, "crowded": crowded, "mutual": mutual, "pieces": pieces}


# ------------------------------------------------------------------------------------------------
# the draw, restated (a disagreement is traced on the CPU: which hypothesis is the first whose draw differs)
# ------------------------------------------------------------------------------------------------
def philox_picks(seed, job_id, i, nc):
    """-> (len(i), 3) the three correspondences hypothesis i of a job draws: Philox4x32-10 on counter (i lo, job id, i hi, 0) with the
    seed's two words as key; pick = (r * nc) >> 32"""
    i = np.asarray(i, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c = [i & m32, np.full_like(i, np.uint64(job_id)), i >> np.uint64(32), np.zeros_like(i)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([((c[t] * np.uint64(nc)) >> np.uint64(32)).astype(np.int64) for t in range(3)], 1)
