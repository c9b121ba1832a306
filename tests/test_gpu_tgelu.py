"""-m gpu: the tanh-GELU epilogues of `ibl_gemm_f16_tn` (SigLIP's gelu_pytorch_tanh) alone, through `ibl_linear_f16_act`.

The three fp16 GELU epilogues with IBL_ACT_GELU_TANH against float64 -- every element, on both tile shapes, between sentinel rows and
columns, exactly as tests/test_gpu_gemm.py holds the erf form and tests/test_gpu_qgelu.py the QuickGELU one (bound and constants:
tests/siglip_cases.py; tests/test_siglip_model.py shows on the CPU where they come from).  Activations 0 and 1 through the new entry are
`ibl_linear_f16_ex` bit for bit, and on `gelu_span` the erf run breaks the tanh bound."""
import numpy as np
import pytest
import torch

from tests import gemm_cases as GC
from tests import siglip_cases as SC
from tests.test_gpu_gemm import Out, _assert_coverage, _bits, _shape, _upload

pytestmark = pytest.mark.gpu

# shapes of tests/test_gpu_qgelu.py: the 128 x 128 form (one row; both sides of a tile; 9 tiles, nk = 3), the 256 x 256 form with one tile
# per workgroup (last tile one row; 34 tiles, last 255 rows) and the persistent walk in which a workgroup writes a full tile and then the
# one-row tile, so that the counted tile-top wait of the fp16 epilogues runs
EPI_SHAPES = [(1, 128, 64), (129, 128, 128), (257, 384, 192), (4097, 256, 128), (4351, 512, 192), "cus+8"]


def _ratio(got, ref, bnd, valid=None):
    ratio = (got.double() - ref).abs() / bnd
    if valid is not None:
        ratio = torch.where(valid, ratio, torch.zeros_like(ratio))
    return ratio


def _judge(got, ref, bnd, what, valid=None):
    assert bool(torch.isfinite(got).all()), f"{what}: NaN or infinity in the result"
    ratio = _ratio(got, ref, bnd, valid)
    r = float(ratio.max())
    print(f"tanh-gelu gemm vs fp64: {what}: worst error / bound {r:.3f}")
    assert r <= 1.0, (what, r, np.unravel_index(int(ratio.argmax()), ratio.shape))


@pytest.mark.parametrize("family", ("normal", "gelu_span", "saturate"))
@pytest.mark.parametrize("shape", EPI_SHAPES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_tanh_gelu_epilogues_vs_fp64(shape, family):
    from ibloc_amd import vit as V
    M, N, K = _shape(shape)
    _assert_coverage(shape, M, N, K)
    c = GC.make(family, M, N, K, resid=False)
    x, W = _upload(c)
    bias = torch.from_numpy(c["bias"]).cuda()
    b64 = bias.double()
    y, S = GC.products(x, W)
    ref, bnd = SC.expected(y, S, K, bias=b64)
    if family == "saturate":       # the family reaches both extremes: results of exactly -0 / 0 far below, the clamp far above
        assert float((y + b64).min()) < -65520.0 and float((y + b64).max()) > 65520.0
    for epi in (GC.EPI_GELU, GC.EPI_X2, GC.EPI_X3):
        what = f"{M} x {N} x {K} {family} tanh {GC.EPI_NAMES[epi]}"
        terms = {GC.EPI_X2: 2, GC.EPI_X3: 3}.get(epi, 1)
        o = Out(M, terms * N, True)
        V.linear_f16_act(x, W, o.win, epi, V.ACT_GELU_TANH, bias=bias)
        assert o.intact(), f"{what}: wrote outside its rows / columns"
        h = o.win[:, :N]
        _judge(h, ref, bnd, what)
        assert bool(torch.isfinite(o.win).all()), f"{what}: NaN or infinity in a later column block"
        if terms > 1:
            assert torch.equal(_bits(o.win[:, (terms - 1) * N:]), _bits(GC.split_of(h))), f"{what}: h / 64 block"
        if terms == 3:
            ref3, bnd3, valid = SC.expected_two_term(y, S, K, bias=b64)
            two = h.double() + o.win[:, N:2 * N].double() / GC.SPLIT
            _judge(two, ref3, bnd3, what + " h + lo / 64", valid=valid)
        # activations 0 and 1 through the new entry are ibl_linear_f16_ex's runs, bit for bit
        for act in (V.ACT_GELU_ERF, V.ACT_QUICK_GELU):
            o0, o1 = Out(M, terms * N, True), Out(M, terms * N, True)
            V.linear_f16_ex(x, W, o0.win, epi, bias=bias, activation=act)
            V.linear_f16_act(x, W, o1.win, epi, act, bias=bias)
            assert torch.equal(o0.buf, o1.buf), f"{what}: activation {act} through ibl_linear_f16_act is not ibl_linear_f16_ex's run"
            assert not torch.equal(o0.win[:, :N], h), f"{what}: the activation argument is ignored"
            if act == V.ACT_GELU_ERF and family == "gelu_span" and epi == GC.EPI_GELU:
                # the erf form is up to 4.7e-4 away: it breaks the tanh bound somewhere on the span
                r = float(_ratio(o0.win[:, :N], ref, bnd).max())
                print(f"tanh-gelu gemm vs fp64: {what}: the erf run against the tanh bound: {r:.1f}")
                assert r > 1.0, f"{what}: the bound cannot tell the erf form from the tanh form"
    # an epilogue without an activation through the new entry: ibl_linear_f16_ex's run too
    o0, o1 = Out(M, N, True), Out(M, N, True)
    V.linear_f16_ex(x, W, o0.win, GC.EPI_F16, bias=bias)
    V.linear_f16_act(x, W, o1.win, GC.EPI_F16, V.ACT_GELU_ERF, bias=bias)
    assert torch.equal(o0.buf, o1.buf)
    torch.cuda.synchronize()
