"""CPU, oracle only: every family of tests/reuse_cases.py is what it claims, and has the power to see a wrong decision of the
feature-reuse plan (csrc/reg_match.hip).

  * `plan` passes its own margin assertions (no pair within 2 % of the radius, no box count within 5 % of NEAR_CAP), and the brute-force
    minimum distance of every pair that shares a side is the one the family's docstring states;
  * every family reaches the path it is named for (the box count on both sides of NEAR_CAP, the hit beyond the first sweep, ...);
  * detection power: by the oracle, the FPFH rows (at 0.08 m or less also the normals and gradients) of every touching instance differ
    between the instance alone and the instance in its side -- a wrong "clean" changes the inputs of matching -- and all three arrays
    of every clean instance are bit-equal to stand-alone -- bit-identity with the uncached schedule is a fair demand;
  * the oracle registers every job that is meant to register within 1 cm / 0.5 degrees of the known motion (tests/test_gpu_register.py's
    tolerance), so the GPU half compares poses with substance."""
import numpy as np
import pytest

from tests import reuse_cases as uc

NAMES = sorted(uc.FAMILIES)
BOTH = (True, True)


def _pairs_of_sides(fam):
    """(pool, a, b) of every two instances that share a side, once"""
    seen = set()
    for pool, j, segs in uc.sides(fam):
        ids = [(k, s) for k, s in enumerate(segs) if s >= 0]
        for x, (ka, a) in enumerate(ids):
            for kb, b in ids[x + 1:]:
                seen.add((pool, min(a, b), max(a, b)))
    return sorted(seen)


def test_the_rule_and_the_kernel_constants():
    assert abs(uc.near_rule() - 0.6007) < 1e-12
    assert abs(uc.near_rule(dict(voxel=0.05, local=5.0)) - (0.6 * 1.001 + 1e-4)) < 1e-12          # the gradient term takes over
    k = uc.kernel_constants()
    assert set(k) >= {"NEAR_CAP", "NEAR_SPLIT"} and k["NEAR_CAP"] > 1500 and k["NEAR_SPLIT"] >= 1


@pytest.mark.parametrize("name", NAMES)
def test_family_is_what_its_docstring_states(name):
    fam = uc.FAMILIES[name]()
    R = uc.near_rule()
    assert len(fam["js"]) <= 12
    for combo in ((True, False), (False, True), BOTH, (False, False)):
        stats = uc.plan(fam, combo)                                    # (asserts its margins)
        assert stats[3] == 2 * len(fam["js"]) and stats[4] <= stats[5]
    assert uc.plan(fam, (False, False))[0] == 0
    for pool, a, b in _pairs_of_sides(fam):
        d, c = uc.pair_facts(fam, pool, a, b)
        assert (a, b) in fam["claims"], (name, a, b, d)
        lo, hi = fam["claims"][(a, b)]
        tol = 2e-6 * (1 + np.abs(fam["mem" if pool else "det"][b]).max(initial=0))          # fp32 coordinates (and, in the memory pool, a motion)
        assert lo - tol <= d <= hi + tol, (name, pool, a, b, d, lo, hi)
        print(f"{name}: pool {pool} pair {a}-{b}: minimum distance {d:.4f}, box count {c}, {'near' if uc.is_near(fam, pool, a, b) else 'far'}")
    sizes = [len(c) for c in fam["det"]]
    print(f"{name}: instance sizes {sizes}, plan (both pools) {uc.plan(fam).tolist()}, R = {R:.4f}")


def _dirty(fam, pool, segs):
    return uc.dirty_slots(fam, pool, segs, True)


def test_threshold_paths():
    fam = uc.threshold()
    for pool in (0, 1):
        assert _dirty(fam, pool, [0, 1, -1]) == [True, True, None] and _dirty(fam, pool, [2, 3, -1]) == [False, False, None]
        assert _dirty(fam, pool, [4, 5, 6]) == [True, True, False]
        assert abs(uc.pair_facts(fam, pool, 0, 1)[0] - 0.58) < 1e-5 and abs(uc.pair_facts(fam, pool, 2, 3)[0] - 0.62) < 1e-5


def test_touching_and_grey_zone_paths():
    fam = uc.touching()
    assert _dirty(fam, 0, [4, 5, 6]) == [True, True, True] and _dirty(fam, 0, [4, 6, -1]) == [False, False, None]
    assert max(uc.pair_facts(fam, 0, a, b)[0] for a, b in ((0, 1), (2, 3), (4, 5), (5, 6))) <= 0.08 + 1e-5
    fam = uc.grey_zone()
    assert _dirty(fam, 1, [4, 5, 6]) == [True, True, True]
    assert all(0.3 - 1e-5 <= uc.pair_facts(fam, 0, a, b)[0] <= 0.45 + 1e-5 for a, b in ((0, 1), (2, 3), (4, 5), (5, 6)))


def _box_gap(A, B):
    gap = np.maximum(np.maximum(A.min(0) - B.max(0), B.min(0) - A.max(0)), 0.0)
    return float(np.sqrt((gap * gap).sum()))


def test_boxes_only_and_cap_paths():
    cap = uc.kernel_constants()["NEAR_CAP"]
    fam = uc.boxes_only()
    for pool in (0, 1):
        clouds = fam["mem" if pool else "det"]
        for a, b in ((0, 1), (2, 3)):
            assert _box_gap(clouds[a], clouds[b]) == 0.0                       # a candidate by boxes ...
            d, c = uc.pair_facts(fam, pool, a, b)
            assert d >= uc.FAR and 0 < c < cap and not uc.is_near(fam, pool, a, b)          # ... with points to test, and far by points
    assert len(fam["det"][1]) == len(fam["det"][2]) == 1500 and uc.pair_facts(fam, 0, 0, 1)[1] >= 1300      # the blob's middle is loaded whole
    assert uc.plan(fam)[1] == 0
    fam = uc.cap()
    for pool in (0, 1):
        counts = [uc.pair_facts(fam, pool, a, b)[1] for a, b in ((0, 1), (2, 3), (4, 5))]
        assert counts[0] == cap + 900 and counts[1] == cap - 600 and counts[2] == 0, counts
        assert min(uc.pair_facts(fam, pool, a, b)[0] for a, b in ((0, 1), (2, 3), (4, 5))) >= uc.FAR
        assert [uc.is_near(fam, pool, a, b) for a, b in ((0, 1), (2, 3), (4, 5))] == [True, False, False]
    assert len(fam["det"][4]) == cap + 900


def test_late_hit_paths():
    k = uc.kernel_constants()
    first = k["NEAR_SPLIT"] * 256
    fam = uc.late_hit()
    R = uc.near_rule()
    for pool in (0, 1):
        clouds = fam["mem" if pool else "det"]
        for big, box in ((0, 1), (3, 2)):
            assert len(clouds[big]) == first + 900
            assert uc.min_distance(clouds[big][:first + 800], clouds[box]) > R * (1 + uc.R_MARGIN)      # nothing in the first sweep, nor before the last 100
            assert uc.min_distance(clouds[big][first + 800:], clouds[box]) < R * (1 - uc.R_MARGIN)
            d = np.sqrt(((clouds[big][first + 800:, None, :].astype(np.float64) - clouds[box][None].astype(np.float64)) ** 2).sum(2)).min(1)
            assert (d < R).all()                                                 # all 100 late points are hits
            assert uc.is_near(fam, pool, big, box)
    # the last 100 points lie in one block's second sweep: block x reads i0 = 256 x + 2048 k
    assert (first + 800) // 256 % k["NEAR_SPLIT"] == (first + 899) // 256 % k["NEAR_SPLIT"] and (first + 800) // (256 * k["NEAR_SPLIT"]) == 1


def test_partial_mixed_use_and_both_pools_paths():
    fam = uc.partial()
    d = uc.plan_details(fam)
    assert d["dirty"][0] == [True, False, True] and d["groups"] == [(0, 0, 1), (0, 1, 0), (1, 0, 1), (1, 1, 0)]      # one group for two sides
    assert d["stats"][2] == 4 and d["stats"][0] == 2 * len(fam["det"][2])
    fam = uc.mixed_use()
    d = uc.plan_details(fam)
    assert d["dirty"][:3] == [[False, None, None], [True, True, None], [False, None, None]] and d["always_dirty"] == {0: [], 1: []}
    fam = uc.both_pools()
    d = uc.plan_details(fam)
    det_groups, mem_groups = [g for g in d["groups"] if g[0] == 0], [g for g in d["groups"] if g[0] == 1]
    assert d["groups"] == det_groups + mem_groups and len(det_groups) >= 3 and len(mem_groups) >= 3 and set(g[1:] for g in det_groups) != set(g[1:] for g in mem_groups)
    sizes = [sum(len(fam["det"][s]) for s in g[1:]) for g in d["groups"]]
    assert len(set(sizes[:len(det_groups)])) >= 3 and len(set(sizes[len(det_groups):])) >= 3, sizes


def test_degenerate_paths():
    fam = uc.degenerate()
    A, B, E, F, G, P1, P2 = range(7)
    assert [len(c) for c in fam["det"]] == [800, 700, 0, 600, 600, 1, 2]
    d = uc.plan_details(fam)
    assert d["dirty"][:10] == [[True, True, None], [True, True, True], [False, False, None], [True, False, True], [True, True, False],
                               [False, False, None], [True, True, None], [False, False, None], [None, False, None], [True, None, True]]
    for pool in (0, 1):
        clouds = fam["mem" if pool else "det"]
        zero = np.zeros((1, 3), np.float32)
        # the box the product gives an empty instance (zeros) is a candidate beside A and none beside F
        assert _box_gap(clouds[A], zero) < uc.near_rule() < _box_gap(clouds[F], zero)
    # without instance features an empty instance is a member of its side's group like any other
    assert (0, E, A) in uc.plan_details(fam, (False, False))["groups"]


@pytest.mark.parametrize("name", NAMES)
def test_detection_power(name):
    """rows that differ between an instance alone and the instance in its side, by the oracle: some for every touching instance, none
    for every instance the plan serves from the cache"""
    fam = uc.FAMILIES[name]()
    details = uc.plan_details(fam)
    done = set()
    for (pool, j, segs), dirty in zip(uc.sides(fam), details["dirty"]):
        if (pool, tuple(segs)) in done:
            continue
        done.add((pool, tuple(segs)))
        for slot, s in enumerate(segs):
            if s < 0:
                continue
            n = len(fam["det"][s])
            changed = uc.rows_changed(fam, pool, segs, slot)
            nearest = min([uc.pair_facts(fam, pool, s, t)[0] for k, t in enumerate(segs) if t >= 0 and k != slot], default=np.inf)
            print(f"{name}: pool {pool} side {segs} instance {s} ({n} points, nearest other {nearest:.3f} m, {'dirty' if dirty[slot] else 'clean'}): "
                  f"rows changed normals {changed[0]} FPFH {changed[1]} gradients {changed[2]}")
            if not dirty[slot] or name == "grey_zone":           # (grey_zone: dirty by the rule although nothing changes)
                assert changed == (0, 0, 0), (name, pool, segs, s, changed)
            elif name in ("touching", "partial", "mixed_use") and n > 0:
                assert changed[1] > 0, (name, pool, segs, s, changed)
                if nearest <= 0.08 + 1e-5:
                    assert changed[0] > 0 and changed[2] > 0, (name, pool, segs, s, changed)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_registers_the_jobs_that_are_meant_to(name):
    fam = uc.FAMILIES[name]()
    assert any(fam["registers"])
    for j, reg in enumerate(fam["registers"]):
        if not reg:
            continue
        T, rmse, fit, Tr, stats = uc.oracle_pose(fam, j)
        want = uc.true_pose(fam, j)
        dt, dr = float(np.linalg.norm(T[:3, 3] - want[:3, 3])), uc.rot_deg(T, want)
        print(f"{name} job {j} ({fam['tags'][j]}): oracle fitness {fit:.4f} rmse {rmse:.2e} stats {stats.tolist()} dt {dt:.2e} m drot {dr:.4f} deg")
        assert dt <= 0.01 and dr <= 0.5, (name, j, fam["tags"][j], dt, dr)
