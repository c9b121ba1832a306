"""-m gpu: the feature-reuse plan of ibl_register_jobs (csrc/reg_match.hip) held to the uncached schedule, on the job sets of
tests/reuse_cases.py (tests/test_reuse_model.py shows on the CPU, with the oracle alone, that every set is what it claims and can see
a wrong decision).  include/ibloc.h promises, at ibl_instance_features, results bit-identical to features == NULL; per family:

  1. uncached (no instance features) is the reference schedule `base`: reuse[0] == 0, means within 1e-9 of the fp64 means of the fp32
     coordinates, every job that is meant to register within 1 cm / 0.5 degrees of the oracle's pose (tests/test_gpu_register.py's two
     tolerances -- the only ones in this file; everything else is equality).  The RANSAC statistics are printed beside the oracle's, not
     asserted: a last-bit difference in a device FPFH row may move a correspondence;
  2. cached == uncached bit for bit (T, rmse, fitness, means, T_ransac, ransac_stats) with features on the detected pool only, the
     memory pool only, both, and both with compact memory features;
  3. the device's `reuse` equals `reuse_cases.plan` -- the float64 numpy restatement of the rule -- in all six entries, each way: a
     planner that marks everything dirty, or one instance too many clean, fails here;
  4. poison: the rows of every instance the plan has dirty in every side it appears in are NaN in every device array of a copy of the
     features (the boxes stay): the call still returns `base`, bit for bit and finite.  A planner that serves one dirty instance
     from the cache fails loudly;
  5. a job alone equals the job in its batch (same job ids, so the same Philox draws), with and without features;
  6. status: no grid collapsed (bit 1), no call redone (bits 16, 32) after any call.

family      path it exists for; minimum point distance of every pair of a side (m; the memory pool is a rigid copy of the detected)
threshold   the radius itself: 0-1 0.58 (dirty), 2-3 0.62 (clean); 4-5 0.58, 5-6 0.62, 4-6 1.50
touching    where rows really change: 0-1 0.02, 2-3 0.08; the chain 4-5 0.05, 5-6 0.03, 4-6 0.78
grey_zone   dirty by the rule, no row changes: 0-1 0.30, 2-3 0.45; 4-5 0.30, 5-6 0.45, 4-6 1.45
boxes_only  boxes overlap, points >= 0.73 apart, either id the lower: cached after the exact test
cap         the same with NEAR_CAP + 900 candidates (called close), NEAR_CAP - 600 (exact test, cached), and the large instance as
            the lower id (nothing to load: cached); points >= 0.73 apart
late_hit    0.05, met only by the last 100 of NEAR_SPLIT * 256 + 900 points: a second sweep of one block; and with the ids swapped
partial     A-B 0.04, C >= 1.5 from both: [A, C, B], [A, B, -1] (one shared group), [B, A, -1] (a second one)
mixed_use   A-B 0.04: A alone (cached), A beside B (recomputed) and B alone in one call
degenerate  [A, A, -1], [A, B, A] (A-A 0, A-B 0.04); an instance of 0 points first / in the middle / last, near and far from the
            origin; 1 point 0.05 from A, 2 points 0.9 from A; [-1, A, -1], [A, -1, B]; an empty source side, an empty target side
both_pools  0-1 0.03; 2-3 0.05, 3-4 0.04, 2-4 0.79; 5-6 0.06: five detected groups, then four memory groups (with gradients)

The oracle on these families (tests/test_reuse_model.py prints every instance; voxel 0.05, normals 0.1 / 30, FPFH 0.25 / 100, gradients
0.15 / 30): rows of an instance that differ between the instance alone and the instance in its side --
  gap (m)        normals / gradients, rows changed          FPFH, rows changed            (instances of 650 to 1 200 points)
  0.02           202-204 / 202-204                          674-862
  0.03           133-255 / 137-259                          461-961
  0.04           177-196 / 177-196                          651-815
  0.05           129 / 130 (late_hit: 3-60 / 3-60)          546 (late_hit: 100 of the 100-point plate, 609-664 of the box)
  0.08           91-102 / 91-105                            462-573
  0.30, 0.45, 0.58 (dirty by the rule)                      0 / 0 / 0: every row bit-equal to stand-alone
  0.62 and above, and every instance the plan calls clean   0 / 0 / 0 (asserted)
so only the touching families can see a wrong "clean" by equality; the others are held by the plan and by the poison.

`reuse` (points cached, points recomputed, groups, sides, distinct pairs, pair uses) with features on both pools, poisoned rows
(detected + memory pool) and wall time of the family's tests, as measured on an MI355X; device == plan in every entry, every way:
family      reuse (both pools)                       poisoned rows        wall time, all 13 tests of the family (slowest test)
both_pools  [750, 21300, 9, 12, 54, 54]              6 600 + 7 350        0.38 s (0.19 s)
boxes_only  [10800, 0, 0, 4, 16, 16]                 0 + 0                0.33 s (0.16 s)
cap         [25880, 14440, 2, 6, 24, 24]             7 220 + 7 220        1.47 s (0.69 s: the oracle on 7 220-point sides)
degenerate  [7604, 14802, 10, 24, 60, 72]            1 301 + 1 301        0.26 s (0.19 s)
grey_zone   [0, 14400, 6, 6, 34, 34]                 7 200 + 7 200        0.33 s (0.13 s)
late_hit    [0, 15792, 4, 4, 16, 16]                 7 896 + 7 896        0.46 s (0.23 s)
mixed_use   [4400, 4400, 2, 6, 12, 12]               0 + 0 (1 000 + 1 000 in the test without the job "B alone")     0.13 s (0.08 s)
partial     [1800, 8800, 4, 6, 26, 34]               2 200 + 2 200        0.32 s (0.15 s)
threshold   [5800, 7800, 4, 6, 34, 34]               3 900 + 3 900        0.29 s (0.12 s)
touching    [3400, 19200, 10, 12, 58, 58]            4 650 + 4 650        0.33 s (0.19 s)
All 101 tests pass; the file takes 9 s with the start of the process.  No product defect was found.  The device's RANSAC statistics equal the
oracle's in about half of the 39 registering jobs (printed, not asserted: the sources are exact copies, so the oracle's first hypothesis already
validates and one differing correspondence moves it); every pose agrees with the oracle's far inside 1 cm / 0.5 degrees.
Negative controls, run once against deliberately wrong planners (not kept): radius 0.01 m -> 82 of the 101 tests fail; only the first sweep
of the swept instance -> the 9 late_hit tests of points 2, 4 and 5; an overflow of NEAR_CAP called far -> the 9 cap tests of points 3, 4, 5;
everything dirty -> 70; group key without its order -> 19 (partial and touching, the two families that list a pair in both orders); radius 0.5 m -> the 9 threshold tests of
points 3, 4 and 5, equality untouched.
"""
import time

import numpy as np
import pytest

from tests import reuse_cases as uc

pytestmark = pytest.mark.gpu

NAMES = sorted(uc.FAMILIES)
WAYS = tuple(uc.FEATURE_WAYS)
KEYS = ("T", "rmse", "fitness", "means", "T_ransac", "ransac_stats")
TOL_MEANS, TOL_T, TOL_DEG = 1e-9, 0.01, 0.5           # tests/test_gpu_register.py
ST_BAD = 1 | 16 | 32                                  # grid collapsed | redone with the VALU search | redone with a full survivor list


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(2 << 30)
    yield c
    c.close()


_state = {}


def state(ctx, name):
    """per family, once: the batches, the features (resident and compact) and the uncached reference `base`; nothing here is changed
    by a test"""
    if name not in _state:
        fam = uc.FAMILIES[name]()
        det, mem = uc.batches(fam)
        ctx.status()                                           # clear the sticky bits of earlier tests
        t0 = time.perf_counter()
        base = uc.run(ctx, fam, det, mem)
        dt = time.perf_counter() - t0
        assert ctx.status() & ST_BAD == 0
        fd, fm = uc.features(ctx, det, mem)
        _, fc = uc.features(ctx, det, mem, compact=True)
        assert fc.fpfh_split is None and fm.fpfh_split is not None
        _state[name] = dict(fam=fam, det=det, mem=mem, base=base, fd=fd, fm=fm, fc=fc, base_s=dt)
    return _state[name]


def features_of(s, way):
    use_det, use_mem, compact = uc.FEATURE_WAYS[way]
    return (s["fd"] if use_det else None), ((s["fc"] if compact else s["fm"]) if use_mem else None)


def same_bits(base, out, what, rows=None):
    for k in KEYS:
        b = base[k] if rows is None else base[k][rows]
        assert np.array_equal(b, out[k]), (what, k, np.argwhere(np.asarray(b != out[k]).reshape(len(b), -1).any(1)).ravel().tolist())
        assert np.isfinite(out[k]).all(), (what, k)


@pytest.mark.parametrize("name", NAMES)
def test_uncached_is_the_reference_schedule(ctx, name):
    s = state(ctx, name)
    fam, base = s["fam"], s["base"]
    assert base["reuse"][0] == 0 and np.array_equal(base["reuse"], uc.plan(fam, (False, False))), base["reuse"]
    same = 0
    for j in range(len(fam["js"])):
        a = uc.job_arrays(fam, j)
        assert np.abs(base["means"][j] - a["means"]).max() <= TOL_MEANS, (name, j)
        if not fam["registers"][j]:
            continue
        T, rmse, fit, Tr, stats = uc.oracle_pose(fam, j)
        dt, dr = float(np.linalg.norm(T[:3, 3] - base["T"][j][:3, 3])), uc.rot_deg(T, base["T"][j])
        same += int(np.array_equal(stats, base["ransac_stats"][j]))
        print(f"{name} job {j} ({fam['tags'][j]}): RANSAC stats oracle {stats.tolist()} device {base['ransac_stats'][j].tolist()} "
              f"fitness {fit:.4f} / {base['fitness'][j]:.4f} dt {dt:.2e} m drot {dr:.4f} deg")
        assert dt <= TOL_T and dr <= TOL_DEG, (name, j, fam["tags"][j], dt, dr)
    for k in KEYS:
        assert np.isfinite(base[k]).all(), k
    print(f"{name}: RANSAC statistics equal to the oracle's in {same} of {sum(fam['registers'])} registering jobs; "
          f"uncached reuse {base['reuse'].tolist()}; uncached call {s['base_s']:.3f} s")


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("name", NAMES)
def test_cached_equals_uncached_and_the_plan_is_the_stated_one(ctx, name, way):
    s = state(ctx, name)
    fam = s["fam"]
    fd, fm = features_of(s, way)
    out = uc.run(ctx, fam, s["det"], s["mem"], fd, fm)
    st = ctx.status()
    want = uc.plan(fam, uc.FEATURE_WAYS[way][:2])
    print(f"{name} / {way}: reuse {out['reuse'].tolist()} plan {want.tolist()}")
    same_bits(s["base"], out, (name, way))
    assert np.array_equal(out["reuse"], want), (name, way, out["reuse"].tolist(), want.tolist())
    assert st & ST_BAD == 0, st


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("name", NAMES)
def test_poisoned_rows_of_dirty_instances_are_never_read(ctx, name, way):
    s = state(ctx, name)
    fam = s["fam"]
    use = uc.FEATURE_WAYS[way][:2]
    always = uc.plan_details(fam, use)["always_dirty"]
    fd, fm = features_of(s, way)
    rows = [0, 0]
    if fd is not None:
        fd, rows[0] = uc.poisoned(fd, s["det"], always[0])
    if fm is not None:
        fm, rows[1] = uc.poisoned(fm, s["mem"], always[1])
    if name in ("boxes_only", "mixed_use"):                    # nothing is dirty / A and B are each clean in a job of their own
        assert sum(rows) == 0, (name, way, always)
    else:
        assert sum(rows) > 0, (name, way, always)
    out = uc.run(ctx, fam, s["det"], s["mem"], fd, fm)
    st = ctx.status()
    print(f"{name} / {way}: poisoned instances {always[0] if use[0] else '-'} + {always[1] if use[1] else '-'}, rows {rows[0]} + {rows[1]}")
    same_bits(s["base"], out, (name, way, "poisoned"))
    assert np.array_equal(out["reuse"], uc.plan(fam, use))
    assert st & ST_BAD == 0, st


def test_mixed_use_with_b_poisoned_where_it_is_dirty(ctx):
    """`mixed_use` without the job in which B is alone: B is then dirty wherever it appears and its rows are poisoned, while A is
    served from the cache in one job and recomputed in the other"""
    s = state(ctx, "mixed_use")
    fam = dict(s["fam"])
    for k in ("js", "jt", "job_ids"):
        fam[k] = s["fam"][k][:2]
    fam["tags"], fam["registers"], fam["_cache"] = s["fam"]["tags"][:2], s["fam"]["registers"][:2], {}
    d = uc.plan_details(fam)
    assert d["always_dirty"] == {0: [1], 1: [1]} and d["dirty"][0][0] is False and d["dirty"][1][0] is True
    fd, rows_d = uc.poisoned(s["fd"], s["det"], [1])
    fm, rows_m = uc.poisoned(s["fm"], s["mem"], [1])
    out = uc.run(ctx, fam, s["det"], s["mem"], fd, fm)
    print(f"mixed_use, B poisoned: rows {rows_d} + {rows_m}, reuse {out['reuse'].tolist()}")
    same_bits(s["base"], out, "mixed_use, B poisoned", rows=slice(0, 2))
    assert np.array_equal(out["reuse"], d["stats"]) and ctx.status() & ST_BAD == 0


@pytest.mark.parametrize("name", NAMES)
def test_a_job_alone_equals_the_job_in_its_batch(ctx, name):
    s = state(ctx, name)
    fam = s["fam"]
    J = len(fam["js"])
    for j in sorted({0, J // 2, J - 1}):
        sub = dict(fam)
        for k in ("js", "jt", "job_ids"):
            sub[k] = fam[k][j:j + 1]
        sub["tags"], sub["registers"], sub["_cache"] = fam["tags"][j:j + 1], fam["registers"][j:j + 1], {}
        for fd, fm, use in ((None, None, (False, False)), (s["fd"], s["fm"], (True, True))):
            out = uc.run(ctx, fam, s["det"], s["mem"], fd, fm, jobs=[j])
            same_bits(s["base"], out, (name, j, use), rows=slice(j, j + 1))
            assert np.array_equal(out["reuse"], uc.plan(sub, use)), (name, j, use, out["reuse"].tolist())
            assert ctx.status() & ST_BAD == 0
