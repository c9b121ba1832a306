"""CPU: the inputs of tests/evaluate_cases.py, judged by the two references alone (the brute-force fp32 rule of oracle_reg.c and the
fp64 kd-tree truth) -- each family does what tests/test_gpu_evaluate.py needs it for.

Random families (slab, ratios, occupancy, jobs): NO query lies within 2^-20 (relative, squared) of the threshold, and outside
that band the fp32 rule and fp64 agree on every inlier decision and to 2^-21 relative on every distance.

Threshold families: the band is where they live.  Every one holds at least 20 queries with d2 == thr2 exactly (rejected: the test is
strict) and at least 20 that the two references decide differently.  Which way depends on the threshold: (float)(thr * thr) lies 0.35
ulp BELOW thr * thr for 0.02 and 0.04, so the fp32 rule rejects what fp64 accepts (341 to 958 queries) and would have to lose more
than 1.35 ulp in three roundings for the reverse (0 queries; a search over 49 000 further ulp combinations around anchors with
inexact differences found none either); for 0.075, 0.021 and 0.036 it lies above, and both happen (56 / 105, 60 / 83, 33 / 336).  At
least 20 of either kind are asserted over the families together.

The unpadded box floorf((q -+ thr) * inv) of the evaluation kernel as it was, computed in numpy fp32: does it hold the cell of every
anchor the fp32 rule accepts?  Each family walks 84 faces (at 0, on both sides of it, at the mid and far bases; the anchor 0 .. 5 ulps
beyond the face; 25 ulp steps of the query, with and without perpendicular offsets).
  * For thr = 0.02, 0.04, 0.075 (and 0.05, 0.01) no accepted anchor lies outside, and none can: there fl(thrf * thrf) >= thr2 =
    (float)(thr * thr) (`box_is_exact`).  dist2f only adds squares to dx * dx and rounding is monotone, so an accepted point has
    fl(dx * dx) < thr2 <= fl(thrf * thrf), hence |dx| < thrf with dx = fl(a - q); thrf is a float, so a - q < thrf exactly, so
    a < q + thrf and a <= fl(q + thrf) because a is a float; floorf(x * inv) is monotone, so the anchor's cell is at most the
    box's upper cell (and likewise below).
  * For thr = 0.021, 0.036, 0.019, where fl(thrf * thrf) < thr2, a difference of exactly thrf is accepted, and 74 queries are: the
    anchor within 4e-10 BELOW 0 (cell -1), the query at +thrf: fl(q - a) = thrf, fl(q - thrf) = 0 -- the box begins at cell 0.  At
    least 20 such queries over these families are asserted; the kernel pads its box as the overlap kernel does.
"""
import numpy as np
import pytest

from tests import evaluate_cases as ec


def _summary(fam, ref):
    hist = ec.occupancy_histogram(fam)
    share = float(np.isfinite(ref["d2"]).mean())
    print(f"{fam['name']}: {len(fam['mem'])} memory points in {sum(hist.values())} cells, {len(ref['d2'])} queries in {len(fam['jb'])} jobs, "
          f"inlier share {share:.4f}, points per cell: cells {dict(list(hist.items())[:12])}{' ...' if len(hist) > 12 else ''}")
    assert 0.0 < share < 1.0
    return hist, share


@pytest.mark.parametrize("name", [n for n, _, _ in ec.RANDOM])
def test_random_family_is_clear_of_the_threshold_and_the_references_agree(name):
    fam = ec.get(name)
    assert len(fam["mem"]) <= 62000 and len(fam["det"]) <= 30000
    ref = ec.reference(fam)
    hist, _ = _summary(fam, ref)
    band = ec.in_band(fam, ref)
    assert band.sum() == 0, (name, ref["d2_64"][band])
    thr2 = fam["thr"] * fam["thr"]
    inl = ref["d2_64"] < thr2
    assert np.array_equal(np.isfinite(ref["d2"]), inl)
    d2 = ref["d2"][inl].astype(np.float64)
    err = np.abs(d2 - ref["d2_64"][inl])
    assert np.all(err <= 2.0 ** -21 * ref["d2_64"][inl]), float((err / np.maximum(ref["d2_64"][inl], 1e-300)).max())
    if name == "occupancy_cells":
        assert all(hist.get(k, 0) >= 8 for k in ec.OCCUPANCIES) and hist.get(ec.BIG_CELL, 0) == 1
        dup = len(fam["mem"]) - len(np.unique(fam["mem"], axis=0))
        assert dup >= 60
        empty = ec.cell_of(fam["det"], fam["cell"])
        occupied = {tuple(c) for c in ec.cell_of(fam["mem"], fam["cell"])}
        in_empty = np.array([tuple(c) == (20, 20, -1) for c in empty])
        assert in_empty.sum() >= 300 and (20, 20, -1) not in occupied
        assert all((20 + d[0] - 1, 20 + d[1] - 1, -1 + d[2] - 1) in occupied for d in np.ndindex(3, 3, 3) if d != (1, 1, 1))
        hit_in_empty = np.isfinite(ref["d2"][:len(fam["det"])][in_empty])
        assert 0 < hit_in_empty.sum() < in_empty.sum()
        assert (ref["d2"] == 0).sum() >= 100                         # queries that ARE memory points
    if name == "occupancy_single":
        assert sum(hist.values()) == 1
    if name == "occupancy_many":
        assert sum(hist.values()) >= 50000
    if name.startswith("slab") or name.startswith("ratio"):
        assert 0.85 < np.isfinite(ref["d2"][:ref["off"][1]]).mean() < 0.99
    if name == "slab_origin":
        signs = {tuple(s) for s in np.sign(fam["mem"]).astype(int) if 0 not in s}
        assert len(signs) == 8
    if name == "jobs":
        assert sorted(set(ref["ns"].tolist())) == sorted(ec.JOB_SIZES)
        assert ref["ns"][0] == 0 and ref["ns"][-1] == 0 and 0 in ref["ns"][1:-1].tolist()
        assert fam["jb"].min() == 0 and (fam["jb"] > 0).sum() >= 10
        scores = ec.expected_scores(fam, ref)
        assert all(scores[j][0] == 0 for j, t in enumerate(fam["tags"]) if "out of reach" in t)
        assert all(scores[j][0] > 0 for j, t in enumerate(fam["tags"]) if "5000 (" in t or "5000 turned" in t)


_stats = {}


def threshold_stats(name):
    """per threshold family: the masks of the three classes, of the accepted points outside the unpadded box and of those on its edge"""
    if name in _stats:
        return _stats[name]
    from oracle import reg_oracle as ro
    fam = ec.get(name)
    ref = ec.reference(fam)
    thr2_64 = fam["thr"] * fam["thr"]
    thr2f = np.float32(thr2_64)
    # the fp32 rule's d2 against the query's anchor, thresholded nowhere: the brute force with twice the reach (anchors are isolated)
    d2_open, idx_open = ro.nearest_bruteforce(fam["det"], fam["mem"], np.eye(4), 2 * fam["thr"])
    assert (idx_open >= 0).all()
    accepted = np.isfinite(ref["d2"])
    assert np.array_equal(accepted, d2_open < thr2f)
    fp64_in = ref["d2_64"] < thr2_64
    inv, thrf = np.float32(1) / np.float32(fam["cell"]), np.float32(fam["thr"])
    c = ec.cell_of(fam["mem"][np.maximum(ref["idx"], 0)], fam["cell"])
    own = ec.cell_of(ref["q"], fam["cell"])
    lo, hi = np.floor((ref["q"] - thrf) * inv).astype(np.int64), np.floor((ref["q"] + thrf) * inv).astype(np.int64)
    st = dict(accepted=accepted, acc_out=accepted & ~fp64_in, rej_in=~accepted & fp64_in, equal=d2_open == thr2f,
              outside=ec.outside_box(fam, ref), edge=accepted & (((c == hi) & (c > own)) | ((c == lo) & (c < own))).any(1),
              band=ec.in_band(fam, ref))
    _stats[name] = st
    return st


@pytest.mark.parametrize("name", [n for n, _, _ in ec.THRESHOLD])
def test_threshold_family_sits_on_the_threshold(name):
    fam = ec.get(name)
    _summary(fam, ec.reference(fam))
    st = threshold_stats(name)
    print(f"{name}: accepted {int(st['accepted'].sum())} of {len(st['accepted'])}; fp32 accepts / fp64 rejects {int(st['acc_out'].sum())}, fp32 rejects / "
          f"fp64 accepts {int(st['rej_in'].sum())}, d2 == thr2 {int(st['equal'].sum())}, accepted outside the unpadded box {int(st['outside'].sum())}, "
          f"accepted in the outermost cell of the box {int(st['edge'].sum())}; in the 2^-20 band {int(st['band'].sum())}")
    assert st["equal"].sum() >= 20 and not (st["accepted"] & st["equal"]).any()
    assert st["rej_in"].sum() + st["acc_out"].sum() >= 20
    assert (st["outside"].sum() == 0) == ec.box_is_exact(fam["thr"])           # see the module docstring
    assert st["edge"].sum() >= 200
    assert (fam["mem"] < 0).any() and (fam["mem"] > 3000).any() and (fam["det"] < -3000).any()


def test_threshold_families_hold_both_kinds_of_disagreement():
    """(float)(thr * thr) lies below thr * thr for 0.02 and 0.04 (the fp32 rule rejects what fp64 accepts) and above it for 0.075"""
    acc_out = sum(int(threshold_stats(n)["acc_out"].sum()) for n, _, _ in ec.THRESHOLD)
    rej_in = sum(int(threshold_stats(n)["rej_in"].sum()) for n, _, _ in ec.THRESHOLD)
    assert acc_out >= 20 and rej_in >= 20, (acc_out, rej_in)


def test_accepted_anchors_outside_the_unpadded_box():
    outside = {n: int(threshold_stats(n)["outside"].sum()) for n, _, _ in ec.THRESHOLD}
    print(outside)
    assert sum(outside.values()) >= 20
    assert all(ec.box_is_exact(t) for t in (0.02, 0.04, 0.05, 0.01, 0.075)) and not any(ec.box_is_exact(t) for t in (0.021, 0.036, 0.019))
