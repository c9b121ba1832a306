"""CPU: the error bound tests/test_gpu_attention.py holds `ibl_attention_kernel` to is reachable -- a numpy emulation of the kernel's
arithmetic (tests/attention_cases.py::emulate: fp32 scores, fp32 exp2 and row sum, fp16 p into the PV product, one fp16 rounding of
o / sum) stays at or under 0.75 of it against the float64 reference, on the very inputs the GPU test runs.

Worst ratio error / bound of the emulation per family over all 18 token counts, C_REST = 2^-14:
    diffuse 0.47   peaked 0.71   two_level 0.21   offset 0.54   ramp 0.68   ramp_diffuse 0.34
(with 2^-15: peaked 0.77, with 2^-16: 0.81 -- attention_cases.py says which roundings those are).  Three-term rows, a + lo / 64 against
the bound with 2^-21 |ref| in place of 2^-11 |ref|: worst 0.69 (peaked)."""
import numpy as np
import pytest

from tests import attention_cases as AC


@pytest.mark.parametrize("family", AC.FAMILIES)
def test_emulation_within_bound(family):
    worst, worst3, at = 0.0, 0.0, None
    for T in AC.T_ALL:
        c = AC.case(family, T)
        ref, A, plain = AC.reference(c.get("q0", c["q"]), c.get("k0", c["k"]), c["v"])
        a, value = AC.emulate(c["q"], c["k"], c["v"])
        bnd = AC.bound(ref, A, c["v"])
        r = float((np.abs(a.astype(np.float64) - ref) / bnd).max()) if T > 1 else 0.0
        if r > worst:
            worst, at = r, T
        # three-term rows: the second term carries the rounding residue of the first
        _, lo = AC.split_terms(a, value)
        b3 = AC.bound(ref, A, c["v"], out_rel=2.0 ** -21)
        worst3 = max(worst3, float((np.abs(a.astype(np.float64) + lo.astype(np.float64) / AC.SPLIT - ref) / b3).max()))
        if T == 1:       # one key: the result is v itself, exactly
            assert np.array_equal(a, c["v"])
        if family in AC.DECISIVE and T >= 15:
            # not vacuous: the plain mean of v (a kernel that ignored the logits) misses the bound at least 50-fold somewhere, and on
            # most elements by a wide margin
            miss = np.abs(plain - ref) / bnd
            assert miss.max() >= 50.0 and np.median(miss) >= 10.0, (T, miss.max(), np.median(miss))
    print(f"attention emulation vs fp64, {family}: worst error / bound {worst:.3f} (T = {at}), three-term {worst3:.3f}")
    assert worst <= 0.75, (family, at, worst)
    assert worst3 <= 0.75, (family, worst3)


def test_offset_rows_have_the_reference_of_the_plain_rows():
    """the +60 offset is exact in the fp16 inputs: the float64 softmax of the shifted rows is that of the unshifted ones"""
    c = AC.case("offset", 65)
    r1 = AC.reference(c["q"], c["k"], c["v"])[0]
    r0 = AC.reference(c["q0"], c["k0"], c["v"])[0]
    assert np.abs(r1 - r0).max() <= 1e-12 * np.abs(r0).max()
    s = np.einsum("bhqd,bhkd->bhqk", c["q"].astype(np.float64), c["k"].astype(np.float64)) / 8.0
    assert s.min() > 40.0


def test_families_are_what_they_claim():
    c = AC.case("peaked", 271)
    s = np.einsum("bhqd,bhkd->bhqk", c["q"].astype(np.float64), c["k"].astype(np.float64)) / 8.0
    top = np.sort(s, axis=-1)
    gap = top[..., -1] - top[..., -3]                 # the winner (and at most one runner-up) against the rest
    assert gap.min() >= 10.0 and gap.max() <= 40.0
    win = s.argmax(axis=-1)
    assert {3, 256, 263, 270} <= set(np.unique(win).tolist())     # first tile; first / middle / last key of the last (partial) tile
    c = AC.case("two_level", 257)
    s = np.einsum("bhqd,bhkd->bhqk", c["q"].astype(np.float64), c["k"].astype(np.float64)) / 8.0
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    sub = (p < 2.0 ** -14) & (p > 2.0 ** -25)
    assert 0.4 < sub.mean() < 0.6                     # half of the p are fp16 subnormals
    c = AC.case("diffuse", 257)
    s = np.einsum("bhqd,bhkd->bhqk", c["q"].astype(np.float64), c["k"].astype(np.float64)) / 8.0
    assert 0.2 < s.std() < 0.4


def test_entry_refuses_before_touching_the_device():
    """the argument checks of ibl_attention_f16 come before any launch, so they run here without a GPU (the pointers are never followed)"""
    from ibloc_amd import _lib
    call, P = _lib.lib.ibl_attention_f16, 0x10000
    assert call(P, P, 1, 273, 128, 2, 0, 1, None) < 0            # one token beyond the widest tier
    assert call(P, P, 2, 50, 128, 3, 0, 1, None) < 0             # dim != 64 * heads
    assert call(P, P, 2, 50, 128, 2, 0, 0, None) < 0 and call(P, P, 2, 50, 128, 2, 0, 4, None) < 0
    assert call(None, P, 2, 50, 128, 2, 0, 1, None) < 0 and b"null" in _lib.lib.ibl_last_error()
    assert call(P, None, 2, 50, 128, 2, 0, 1, None) < 0
    assert call(P, P, -1, 50, 128, 2, 0, 1, None) < 0 and call(P, P, 2, -1, 128, 2, 0, 1, None) < 0
    assert call(P + 2, P, 2, 50, 128, 2, 0, 1, None) < 0 and call(P, P + 4, 2, 50, 128, 2, 0, 1, None) < 0
    assert call(P, P, 0, 50, 128, 2, 0, 1, None) == 0 and call(P, P, 2, 0, 128, 2, 0, 1, None) == 0
