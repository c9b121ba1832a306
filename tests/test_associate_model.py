"""CPU: the association cases of tests/associate_cases.py contain what they are named for, the numpy restatement of the device's
distance chain equals integer arithmetic on the lattice, the decision rule restated from the brute-force hits gives the facade
scenario's stated decisions, and the entry point is exported and declared.  tests/test_gpu_associate.py runs the cases on the device."""
import os
import re

import numpy as np

from tests import associate_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_case_points():
    out = []
    for case in (ac.small_world, ac.crowded, ac.eight_cells, ac.over_k, ac.empty_and_far):
        insts, dets = case()
        out += list(insts) + list(dets)
    out += list(ac.radius_edge()[0]) + list(ac.radius_edge()[1])
    f = ac.facade()
    return out + list(f["points"]) + [c[0] for c in f["det_clouds"]]


def test_every_coordinate_is_on_the_lattice_below_8m():
    for p in all_case_points():
        p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
        s = p / ac.STEP
        assert (s == np.rint(s)).all() and (np.abs(p) < 8).all()
        assert (p.astype(np.float32).astype(np.float64) == p).all()


def test_emulation_equals_integer_arithmetic():
    rng = np.random.default_rng(5)
    a = rng.integers(-8 * 65536 + 1, 8 * 65536, size=(500, 3))
    b = rng.integers(-8 * 65536 + 1, 8 * 65536, size=(400, 3))
    near = a[:400] + rng.integers(-3000, 3001, size=(400, 3))          # the range the radius decides in
    near = np.clip(near, -8 * 65536 + 1, 8 * 65536 - 1)
    for p, q in ((a, b), (a[:400], near), (near, near)):
        emu = ac.dist2_emulated(ac.lattice(p), ac.lattice(q)).astype(np.float64)
        exact = ac.dist2_integer(p, q).astype(np.float64) * ac.STEP * ac.STEP
        assert (emu == exact).all()
    # ties to even are met: a value exactly between two fp32 neighbours (2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4)
    assert ac._round24(np.array([(1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6])).tolist() == [1 << 24, (1 << 24) + 4, 1 << 25, (1 << 25) + 8]
    # R_EDGE: r2 is the fp32 number 1280^2 STEP^2, and the emulated distance of a pair at the radius is that number
    assert float(ac.r2_of(ac.R_EDGE)) == 1280.0 ** 2 * ac.STEP ** 2
    assert ac.dist2_emulated(ac.lattice([[0, 0, 0]]), ac.lattice([[768, 1024, 0]]))[0, 0] == ac.r2_of(ac.R_EDGE)


def test_small_world_is_what_it_says():
    insts, dets = ac.small_world()
    assert len(insts) == 6 and all(200 <= len(p) <= 400 for p in insts) and len(dets) == 5
    allp = np.concatenate(insts)
    assert (allp.min(0) < 0).all() and (allp.max(0) > 0).all()
    for r in (ac.R_HALF, ac.R_CELL):
        H = ac.brute_hits(dets, insts, r)
        assert (H[3] == 0).all()                                        # the far one
        assert H[0, 0] == len(dets[0])                                  # a shifted copy: every point
        assert 0 < H[2, 5] and (r == ac.R_CELL or H[2, 5] < len(dets[2]))   # shifted by about cell / 2: a partial overlap at r = cell / 2
        assert (H[1] > 0).sum() >= 2 and (H[4] > 0).sum() >= 2          # detections that touch two instances
    assert (ac.brute_hits(dets, insts, ac.R_CELL) >= ac.brute_hits(dets, insts, ac.R_HALF)).all()
    assert (ac.brute_hits(dets, insts, ac.R_CELL) != ac.brute_hits(dets, insts, ac.R_HALF)).any()


def test_crowded_point_sees_12_instances_in_several_cells():
    insts, dets = ac.crowded()
    P = dets[0][:1]
    within = [ac.dist2_emulated(P, q)[0] < ac.r2_of(ac.R_HALF) for q in insts]
    assert len(insts) == 12 and all(w.any() for w in within) and all(1 <= len(q) <= 3 for q in insts)
    cells = {tuple(c) for q, w in zip(insts, within) for c in ac.cell_of(q[w])}
    assert len(cells) >= 6
    # instances whose points within r lie in more than one cell: the ones a per-cell count would count twice
    assert sum(len({tuple(c) for c in ac.cell_of(q[w])}) > 1 for q, w in zip(insts, within)) >= 4
    assert ac.brute_hits(dets, insts, ac.R_HALF).tolist() == [[1] * 12]


def test_radius_edge_has_pairs_at_and_inside_the_radius():
    insts, dets, expect = ac.radius_edge()
    r2 = ac.r2_of(ac.R_EDGE)
    d2 = np.array([ac.dist2_emulated(dets[0][j:j + 1], insts[j])[0, 0] for j in range(6)])
    assert (d2 == r2).sum() == 3 and (d2 < r2).sum() == 3
    one_inside = (ac.steps_of(dets[0]) - np.array([ac.steps_of(q)[0] for q in insts]))
    assert sorted(np.abs(one_inside).max(axis=1).tolist()) == [1023, 1024, 1024, 1024, 1279, 1280]
    assert ac.brute_hits(dets, insts, ac.R_EDGE).tolist() == [list(expect)]
    assert len({tuple(c) for c in ac.cell_of(dets[0])}) == 6           # nothing else is near: six separate neighbourhoods


def test_eight_cells_holds_one_instance_in_all_cells_of_the_box():
    insts, dets = ac.eight_cells()
    P = dets[0][:1]
    assert (ac.dist2_emulated(P, insts[1])[0] < ac.r2_of(ac.R_HALF)).all()
    assert len({tuple(c) for c in ac.cell_of(insts[1])}) == 8
    assert ac.brute_hits(dets, insts, ac.R_HALF).tolist() == [[1, 1]]


def test_over_k_has_more_than_k_hits_with_ties():
    insts, dets = ac.over_k()
    H = ac.brute_hits(dets, insts, ac.R_HALF)
    assert H.tolist() == [[3, 3, 1, 2, 1, 2, 1]]
    inst, hits, n_hit = ac.expected_pairs(H, ac.OVER_K)
    assert n_hit.tolist() == [7] and n_hit[0] > ac.OVER_K
    assert inst.tolist() == [[0, 1, 3, 5]] and hits.tolist() == [[3, 3, 2, 2]]      # ties in hits go to the lower instance


def test_expected_pairs_pads_and_counts():
    H = np.array([[0, 2, 0], [0, 0, 0], [5, 5, 1]])
    inst, hits, n_hit = ac.expected_pairs(H, 2)
    assert inst.tolist() == [[1, -1], [-1, -1], [0, 1]] and hits.tolist() == [[2, 0], [0, 0], [5, 5]] and n_hit.tolist() == [1, 0, 3]


def test_decision_rule_on_the_facade_scenario():
    f = ac.facade()
    dets = [c[0] for c in f["det_clouds"]]
    H = ac.brute_hits(dets, f["points"], ac.R_HALF)
    sizes = [len(d) for d in dets]
    assert ac.decide(H, sizes, f["det_embs"], f["means"]) == f["expect"] == [1, 3, None, None]
    # for the reasons the scenario names: the impostor overlaps object 0 entirely and fails on the embedding alone, the new object
    # overlaps nothing, and the re-observations pass both tests with room
    assert H[3, 0] == sizes[3] and (H[2] == 0).all() and H[0, 1] == sizes[0] and H[1, 3] == sizes[1]
    cos = lambda a, b: float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))      # noqa: E731
    assert abs(cos(f["det_embs"][3].astype(np.float64), f["means"][0].astype(np.float64))) < 1e-6
    assert cos(f["det_embs"][0], f["means"][1]) > 0.8 and cos(f["det_embs"][1], f["means"][3]) > 0.8
    # the thresholds decide: nothing is accepted at an unreachable similarity, the impostor is at none
    assert ac.decide(H, sizes, f["det_embs"], f["means"], min_similarity=1.01) == [None] * 4
    assert ac.decide(H, sizes, f["det_embs"], f["means"], min_similarity=-1.0) == [1, 3, None, 0]
    assert ac.decide(H, sizes, f["det_embs"], f["means"], min_overlap=1.01, min_similarity=-1.0) == [None] * 4
    # ties in the cosine go to the lower instance
    same = [np.ones(4), np.ones(4)]
    assert ac.decide(np.array([[4, 4]]), [4], [np.ones(4)], same) == [0]


def test_entry_point_is_exported_and_declared():
    from ibloc_amd import _lib
    assert hasattr(_lib.lib, "ibl_memgrid_overlap") and "ibl_memgrid_overlap" in _lib.declared_symbols()
    text = open(os.path.join(ROOT, "include", "ibloc.h")).read()
    assert re.search(r"\bint\s+ibl_memgrid_overlap\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    # refused without a device: null pointers are decided before any HIP call
    assert _lib.lib.ibl_memgrid_overlap(None, None, None, 0, 0, None, None, 0, 0.02, 8, None, None, None, None) < 0
    assert b"ibl_memgrid_overlap" in _lib.lib.ibl_last_error()


def test_facade_signatures():
    import inspect
    from ibloc_amd.engine import MemoryShard
    from ibloc_amd.object_memory.object_memory import AssociationParams, ObjectMemory
    from ibloc_amd.registration import MemGrid
    assert list(inspect.signature(MemGrid.overlap).parameters)[1:6] == ["det_pts4", "det_off_host", "inst_off", "radius", "k"]
    sig = inspect.signature(MemoryShard.overlap).parameters
    assert sig["radius"].default is None and sig["k"].default == 8
    p = AssociationParams()
    assert (p.min_overlap, p.min_similarity, p.radius, p.k) == (0.6, 0.6, None, 8)
    for fn in (ObjectMemory.process_detections, ObjectMemory.process_image):
        assert inspect.signature(fn).parameters["associate"].default is False
    assert inspect.signature(ObjectMemory.process_detections).parameters["association"].default is None
