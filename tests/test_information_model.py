"""CPU: what tests/test_gpu_information.py relies on, shown with the references alone (tests/information_cases.py).

    closed form   the matrix from the ten sums equals the literal three-row loop; about = c is the origin matrix of the points - c
    tie-free      the evaluation families named in information_cases.TIE_FREE have no query with two candidates of different
                  coordinates within 1 + 2^-18 (squared, fp64): the brute force's lowest index names the rule's coordinates
    duplicates    occupancy_cells has 186 queries matched to a memory point that is stored more than once, and no other tie
    slab_far      has ties between distinct coordinates (fp32 steps in 2^-12 near +-4000); there the rule is applied to
                  dist2_emulated, which reproduces the brute force's d2 bit for bit; the rule's coordinates never come after the
                  lowest index's
    lattice       a query midway between 2, 2, 2 and 8 candidates, inside one cell and across cell faces: the ties are exact in
                  integer arithmetic, and the rule's choice is never the lowest index
and the binding: the symbol is declared, exported and bound, and refuses null arguments before any HIP call."""
import re

import numpy as np
import pytest

from tests import associate_cases as ac
from tests import evaluate_cases as ec
from tests import information_cases as ic


def test_closed_form_equals_the_three_row_loop():
    rng = np.random.default_rng(7)
    for n, scale, centre in ((1, 1.0, (0, 0, 0)), (37, 2.0, (0.3, -0.2, 0.1)), (500, 0.5, (-4000.5, 3999.7, 12.3))):
        pts = (rng.normal(size=(n, 3)) * scale + centre).astype(np.float32)
        loop, closed = ic.info_loop(pts), ic.info_closed(pts)
        ref, scale_abs = ic.info_reference(pts)
        assert np.array_equal(loop, loop.T) and np.array_equal(closed, closed.T)
        for A in (loop, closed):
            assert (np.abs(A - ref) <= ic.bound(n, scale_abs)).all()
        assert loop[3, 3] == loop[4, 4] == loop[5, 5] == n
        # about = c: the origin matrix of the shifted points (the subtraction is the same float64 operation in both)
        c = np.array([0.25, -1.5, 3.0]) + centre
        assert np.array_equal(ic.info_closed(pts, c), ic.info_closed(pts.astype(np.float64) - c))
        assert np.array_equal(ic.info_loop(pts, c), ic.info_loop(pts.astype(np.float64) - c))
        a, b = ic.info_reference(pts, c)
        assert (np.abs(ic.info_closed(pts, c) - a) <= ic.bound(n, b)).all()


def test_the_matrix_is_the_gauss_newton_hessian_of_the_left_perturbation():
    """sum |exp(xi^) m - m|^2 = xi^T info xi to second order: G = d(exp(xi^) m) / d xi at 0 = [-[m]x | I]"""
    rng = np.random.default_rng(8)
    pts = rng.normal(size=(20, 3))
    A = ic.info_loop(pts)
    xi = rng.normal(size=6) * 1e-5
    w, v = xi[:3], xi[3:]
    moved = pts + np.cross(w, pts) + v                     # first order of exp(xi^) m
    assert abs(((moved - pts) ** 2).sum() - xi @ A @ xi) <= 1e-12 * (xi @ A @ xi)


@pytest.mark.parametrize("name", ic.TIE_FREE)
def test_tie_free_families_have_no_near_tie(name):
    fam = ec.get(name)
    ref = ec.reference(fam)
    tied, dup = ic.near_ties(fam, ref)
    print(f"{name}: {len(ref['q'])} queries, {len(tied)} near-ties, {dup} matches with exact duplicates")
    assert len(tied) == 0
    exp = ic.expected_match(fam, ref)
    hit = ref["idx"] >= 0
    assert np.array_equal(exp[hit], fam["mem"][ref["idx"][hit]]) and not exp[~hit].any()


def test_occupancy_cells_has_duplicates_and_no_other_tie():
    fam = ec.get(ic.DUPLICATES_ONLY)
    tied, dup = ic.near_ties(fam, ec.reference(fam))
    print(f"{fam['name']}: {len(tied)} near-ties between distinct coordinates, {dup} matches with exact duplicates")
    assert dup == 186 and len(tied) == 0


def test_slab_far_has_ties_between_distinct_coordinates():
    fam = ec.get(ic.TIE_FAMILY)
    ref = ec.reference(fam)
    tied, _ = ic.near_ties(fam, ref)
    xyz, d2, n_best = ic.rule_match(fam, ref["q"][tied])
    print(f"{fam['name']}: {len(tied)} near-tied queries, candidates at the minimal fp32 d2: {n_best.tolist()}, "
          f"matched by the brute force: {(ref['idx'][tied] >= 0).tolist()}")
    assert len(tied) >= 1 and (n_best[np.isfinite(d2)] >= 1).all()
    assert (n_best >= 2).any(), "no exact fp32 tie between distinct coordinates"
    # the emulated chain is the brute force's on these queries (the differences are small multiples of 2^-12)
    assert d2.view(np.uint32).tolist() == ref["d2"][tied].view(np.uint32).tolist()
    exp = ic.expected_match(fam, ref)
    assert np.array_equal(exp[tied], xyz)
    # where the brute force has a match its coordinates are at the same fp32 distance as the rule's, and never before them
    for i, t in enumerate(tied):
        if ref["idx"][t] >= 0:
            m = fam["mem"][ref["idx"][t]]
            assert ac.dist2_emulated(ref["q"][t][None], m[None])[0, 0] == d2[i]
            assert tuple(xyz[i]) <= tuple(m)
    rest = np.setdiff1d(np.arange(len(ref["q"])), tied)
    hit = rest[ref["idx"][rest] >= 0]
    assert np.array_equal(exp[hit], fam["mem"][ref["idx"][hit]])


def test_lattice_family_ties_by_integer_arithmetic():
    mem, qs, kinds, counts = ic.lattice_steps()
    d = ac.dist2_integer(qs, mem)
    for i, (kind, n) in enumerate(zip(kinds, counts)):
        at_min = np.nonzero(d[i] == d[i].min())[0]
        assert len(at_min) == n and n == (8 if kind.startswith("diagonal") else 2), kind
        cells = {tuple(c) for c in ac.cell_of(ac.lattice(mem[at_min]))}
        assert len(cells) == (1 if kind.endswith("inside") else n), (kind, cells)       # across faces: every candidate in a cell of its own
        assert d[i].min() == (3 if n == 8 else 1) * ic.HALF ** 2                           # (below 2^24: exact in fp32)
        assert np.float32(d[i].min() * ac.STEP ** 2) < np.float32(ec.THR * ec.THR)
        # the candidates are stored in descending order: the lowest index is the LAST by (x, y, z)
        assert tuple(mem[at_min[0]]) == max(tuple(m) for m in mem[at_min])
    fam = ic.lattice_family()
    ref = ec.reference(fam)
    exp, n_best = ic.lattice_expected(fam, ref)
    assert np.isfinite(ref["d2"]).all() and sorted(n_best[:8]) == [2] * 6 + [8] * 2 and len(exp) == 20
    # the integer chain, the emulated chain and the brute force agree on d2; the rule's coordinates differ from the lowest index's
    assert np.array_equal(ac.dist2_emulated(ref["q"], fam["mem"]).min(1), ref["d2"])
    assert (exp != fam["mem"][ref["idx"]]).any(1).all()
    xyz, d2, ties = ic.rule_match(fam, ref["q"])
    assert np.array_equal(xyz, exp) and np.array_equal(d2, ref["d2"]) and ties.tolist() == n_best
    # the query's own cell holds one candidate of the "face" groups, and not the rule's: a walk that keeps the first minimum fails here
    own = ac.cell_of(ref["q"][12:16])
    assert (ac.cell_of(exp[12:16]) != own).any(1).all()


def test_symbol_is_declared_exported_and_bound():
    import os
    from ibloc_amd import _lib
    assert hasattr(_lib.lib, "ibl_evaluate_information") and "ibl_evaluate_information" in _lib.declared_symbols()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ibloc.h")).read()
    assert re.search(r"\bint\s+ibl_evaluate_information\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    info = np.full(36, -7.0)
    n = np.full(1, -7, np.int64)
    one = np.zeros(16)
    seg = np.zeros(1, np.int32)
    # a null context: refused before any HIP call, outputs untouched
    st = _lib.lib.ibl_evaluate_information(None, None, None, seg.ctypes.data, seg.ctypes.data, one.ctypes.data, 1, 0.02, None, None,
                                           info.ctypes.data, n.ctypes.data, None)
    assert st < 0 and b"ibl_evaluate_information" in _lib.lib.ibl_last_error()
    assert (info == -7.0).all() and n[0] == -7


def test_python_layers_take_the_flag():
    import inspect
    from ibloc_amd import engine, registration
    from ibloc_amd.object_memory.object_memory import ObjectMemory
    from ibloc_amd.utils import fpfh_register
    sig = inspect.signature(registration.evaluate_information)
    assert [sig.parameters[k].default for k in ("threshold", "about", "points")] == [0.02, None, False]
    assert inspect.signature(engine.LocaliseEngine.localise_batch).parameters["information"].default is False
    assert inspect.signature(ObjectMemory.localise_detections).parameters["information"].default is False
    assert "information" not in inspect.signature(ObjectMemory.localise).parameters
    assert list(inspect.signature(fpfh_register.get_information_matrix).parameters) == ["source", "target", "max_correspondence_distance",
                                                                                        "transformation"]
    r = engine.FrameResult(np.zeros(7), np.zeros(7))
    assert r.information is None and r.n_correspondences is None and r.inlier_centroid is None
