"""CPU: the error bound tests/test_gpu_layernorm.py holds `ibl_layernorm_kernel` to is reachable with a factor 4 to spare -- a numpy fp32
emulation of the kernel's two-pass sums in the kernel's own summation order (tests/layernorm_cases.py::emulate) against the float64
reference.

Worst ratio error / bound of the emulation, fp32 result: normal 0.13, offset 0.16, outliers 0.14 (with the mean's term at its first
estimate 2^-21 the offset rows reached 0.32: that term was widened to 2^-20, layernorm_cases.py).  fp16 result against ulp / 2 + the fp32
bound: 0.998 (the half ulp is exact rounding).  Three-term rows, a + lo / 64 against the fp32 bound + 2^-21 |ref|: 0.16."""
import numpy as np
import pytest

from tests import layernorm_cases as LC


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_emulation_within_bound(family):
    w32 = w16 = w3 = 0.0
    for affine in LC.AFFINE:
        for dim in LC.DIMS + (132, 1020):
            for n_rows in (5, 1030):
                for eps in LC.EPS:
                    x = LC.make_rows(family, n_rows, dim, 5)
                    g, b = LC.make_affine(affine, dim, 5)
                    ref, bnd = LC.reference(x, g, b, eps)
                    y = LC.emulate(x, g, b, eps)
                    w32 = max(w32, float((np.abs(y - ref) / bnd).max()))
                    h = y.astype(np.float16)
                    w16 = max(w16, float((np.abs(h.astype(np.float64) - ref) / (LC.ulp16(ref) / 2 + bnd)).max()))
                    _, lo = LC.split_terms(h, y)
                    w3 = max(w3, float((np.abs(h.astype(np.float64) + lo.astype(np.float64) / LC.SPLIT - ref) / (bnd + 2.0 ** -21 * np.abs(ref))).max()))
    print(f"layernorm emulation vs fp64, {family}: worst error / bound fp32 {w32:.3f}, fp16 {w16:.3f}, three-term {w3:.3f}")
    assert w32 <= 0.25, (family, w32)
    assert w16 <= 1.0 and w3 <= 0.25, (family, w16, w3)


def test_one_pass_variance_would_fail_the_offset_rows():
    """the offset family is there for a reason: E[x^2] - mean^2 in fp32 misses the bound several times over (xhat is simply wrong: var comes out 0 or a rounding artefact)"""
    x = LC.make_rows("offset", 5, 768, 5)
    g, b = LC.make_affine("identity", 768, 5)
    ref, bnd = LC.reference(x, g, b, 1e-6)
    f32 = np.float32
    mean = x.mean(axis=1, keepdims=True, dtype=f32)
    var = np.maximum((x * x).mean(axis=1, keepdims=True, dtype=f32) - mean * mean, f32(0))
    y = (x - mean) / np.sqrt(var + f32(1e-6))
    assert (np.abs(y - ref) / bnd).max() > 4.0


def test_entry_refuses_before_touching_the_device():
    """the argument checks of ibl_layernorm_f32 come before any launch, so they run here without a GPU (the pointers are never followed)"""
    from ibloc_amd import _lib
    call, P = _lib.lib.ibl_layernorm_f32, 0x10000
    assert call(P, 1280, 4, 1280, P, P, 1e-6, P, 1280, 0, None) < 0      # a lane holds four float4: columns beyond 1024 would be dropped
    assert call(P, 136, 4, 130, P, P, 1e-6, P, 136, 0, None) < 0         # not a multiple of 4
    assert call(None, 256, 4, 256, P, P, 1e-6, P, 256, 1, None) < 0 and b"null" in _lib.lib.ibl_last_error()
    assert call(P, 252, 4, 256, P, P, 1e-6, P, 256, 1, None) < 0         # input stride shorter than the row
    assert call(P, 256, 4, 256, P, P, 1e-6, P, 512, 3, None) < 0         # three terms need ld_out >= 768
    assert call(P, 256, 4, 256, P, P, 1e-6, P, 258, 1, None) < 0         # stride not a multiple of 4 elements
    assert call(P, 256, 4, 256, P, P, 1e-6, P, 256, 4, None) < 0         # unknown out_kind
    assert call(P, 256, 4, 256, P + 4, P, 1e-6, P, 256, 1, None) < 0     # gamma not 16-byte aligned
    assert call(P, 256, 4, 256, P, P, -1.0, P, 256, 1, None) < 0
    assert call(P, 256, 4, 256, P, P, 1e-6, P, 256, 1, None) < 0         # in place is fp32 only
    assert call(P, 256, 0, 256, P, P, 1e-6, P, 256, 1, None) == 0        # no rows: nothing to do
