"""`ibl_layernorm_f32` (the encoder's LayerNorm kernel on its own: fp32 rows, in place or not, and fp16 rows of one, two or three terms)
against a float64 LayerNorm of the same fp32 rows -- every element.

fp32 bound (tests/layernorm_cases.py::reference): 2^-20 (|g xhat| + |b|) + 2^-20 max|x_row| rstd |g|; fp16: half an fp16 ulp of the
reference on top.  A CPU emulation of the kernel's sums reaches 0.16 of the fp32 bound (tests/test_layernorm_model.py).
Measured on the MI355X, worst error / bound over all dims, row counts, strides and eps (each case prints its own, run with -s):
    fp32: normal 0.11, offset 0.17, outliers 0.12   fp16: 0.998 (exact rounding)   three-term a + lo / 64: 0.17"""
import numpy as np
import pytest
import torch

from tests import layernorm_cases as LC

pytestmark = pytest.mark.gpu

S32 = 0x7FC12345             # fp32 / fp16 NaN patterns no kernel writes
S16 = 0x7E2A
G = 2                        # guard rows on either side of the output
PAD = 8                      # guard columns behind every output row


def _out_buffer(n_rows, width, f32):
    ld = width + PAD
    buf = torch.full(((n_rows + 2 * G), ld), S32 if f32 else S16, dtype=torch.int32 if f32 else torch.int16, device="cuda")
    view = buf.view(torch.float32 if f32 else torch.float16)[G:G + n_rows, :width]
    return buf, view


def _guards_intact(buf, n_rows, width, f32):
    a = buf.cpu().numpy().view(np.uint32 if f32 else np.uint16)
    s = S32 if f32 else S16
    return (a[:G] == s).all() and (a[G + n_rows:] == s).all() and (a[:, width:] == s).all()


def _strided_input(x_np, stride_rows):
    """rows of x at a row stride of stride_rows * dim; the skipped rows hold NaN, so a wrong stride is loud"""
    n, dim = x_np.shape
    big = torch.full((n * stride_rows, dim), float("nan"), dtype=torch.float32, device="cuda")
    big[::stride_rows] = torch.from_numpy(x_np).cuda()
    return big, big[::stride_rows]


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("dim", LC.DIMS)
def test_layernorm_vs_fp64(dim, family):
    from ibloc_amd import vit as V
    w32 = w16 = w3 = 0.0
    combo = 0
    for n_rows in LC.ROWS:
        for stride_rows in (1, 7):
            for affine in LC.AFFINE:
                eps = LC.EPS[combo % 3]
                combo += 1
                x_np = LC.make_rows(family, n_rows, dim, 11)
                g_np, b_np = LC.make_affine(affine, dim, 11)
                ref, bnd = LC.reference(x_np, g_np, b_np, eps)
                big, x = _strided_input(x_np, stride_rows)
                assert x.stride(0) == stride_rows * dim or n_rows == 1
                g, b = torch.from_numpy(g_np).cuda(), torch.from_numpy(b_np).cuda()
                # fp32, out of place
                buf, out = _out_buffer(n_rows, dim, True)
                V.layernorm_f32(x, g, b, eps, V.LN_F32, out=out)
                y = out.cpu().numpy()
                assert _guards_intact(buf, n_rows, dim, True), "fp32: guard rows / columns written"
                assert np.isfinite(y).all(), "NaN from the skipped rows or a wrong stride"
                r = float((np.abs(y - ref) / bnd).max())
                w32 = max(w32, r)
                assert r <= 1.0, (dim, family, n_rows, stride_rows, affine, eps, r)
                # fp32, in place: same bits; the rows between the strides are still NaN
                big2 = big.clone()
                x2 = big2[::stride_rows]
                V.layernorm_f32(x2, g, b, eps, V.LN_F32, out=x2)
                assert np.array_equal(x2.cpu().numpy().view(np.uint32), y.view(np.uint32)), "in place != out of place"
                if stride_rows > 1:
                    skipped = torch.ones(big2.shape[0], dtype=torch.bool)
                    skipped[::stride_rows] = False
                    assert torch.isnan(big2[skipped.cuda()]).all()
                # fp16 rows of 1 / 2 / 3 terms
                first = None
                for terms, kind in ((1, V.LN_F16), (2, V.LN_F16_X2), (3, V.LN_F16_X3)):
                    buf, out = _out_buffer(n_rows, terms * dim, False)
                    V.layernorm_f32(x, g, b, eps, kind, out=out)
                    h = out.cpu().numpy()
                    assert _guards_intact(buf, n_rows, terms * dim, False), f"fp16 x{terms}: guard rows / columns written"
                    a = h[:, :dim]
                    if first is None:
                        first = a
                        r = float((np.abs(a.astype(np.float64) - ref) / (LC.ulp16(ref) / 2 + bnd)).max())
                        w16 = max(w16, r)
                        assert r <= 1.0, (dim, family, n_rows, stride_rows, affine, eps, r)
                    assert np.array_equal(a.view(np.uint16), first.view(np.uint16)), f"first block of x{terms} != x1"
                    if terms > 1:
                        want = (a.astype(np.float32) / np.float32(LC.SPLIT)).astype(np.float16)
                        assert np.array_equal(h[:, (terms - 1) * dim:].view(np.uint16), want.view(np.uint16)), f"x{terms}: a / 64 block"
                    if terms == 3:
                        two = a.astype(np.float64) + h[:, dim:2 * dim].astype(np.float64) / LC.SPLIT
                        r = float((np.abs(two - ref) / (bnd + 2.0 ** -21 * np.abs(ref))).max())
                        w3 = max(w3, r)
                        assert r <= 1.0, (dim, family, n_rows, stride_rows, affine, eps, r)
    print(f"layernorm vs fp64: dim {dim} {family}: worst error / bound fp32 {w32:.3f}, fp16 {w16:.3f}, three-term {w3:.3f}")


def test_refusals_launch_nothing():
    from ibloc_amd import _lib, vit as V
    st = torch.cuda.current_stream().cuda_stream
    for dim in (1280, 130):          # beyond the four float4 a lane holds (columns would be dropped); not a multiple of 4
        x = torch.randn(4, dim, device="cuda")
        g, b = torch.ones(dim, device="cuda"), torch.zeros(dim, device="cuda")
        buf, out = _out_buffer(4, dim, True)
        with pytest.raises(_lib.IblError):
            V.layernorm_f32(x, g, b, 1e-6, V.LN_F32, out=out)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy().view(np.uint32) == S32).all()
    x = torch.randn(4, 256, device="cuda")
    g, b = torch.ones(256, device="cuda"), torch.zeros(256, device="cuda")
    buf, out = _out_buffer(4, 512, False)
    call = _lib.lib.ibl_layernorm_f32
    p = (x.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr())
    assert call(None, 256, 4, 256, p[1], p[2], 1e-6, p[3], 520, 1, st) < 0
    assert b"null" in _lib.lib.ibl_last_error()
    assert call(p[0], 256, 4, 256, None, p[2], 1e-6, p[3], 520, 1, st) < 0
    assert call(p[0], 256, 4, 256, p[1], p[2], 1e-6, None, 520, 1, st) < 0
    assert call(p[0], 252, 4, 256, p[1], p[2], 1e-6, p[3], 520, 1, st) < 0          # input stride shorter than the row
    assert call(p[0], 256, 4, 256, p[1], p[2], 1e-6, p[3], 256, 2, st) < 0          # two terms need ld_out >= 512
    assert call(p[0], 256, 4, 256, p[1], p[2], 1e-6, p[3], 520, 4, st) < 0          # unknown out_kind
    assert call(p[0], 256, -1, 256, p[1], p[2], 1e-6, p[3], 520, 1, st) < 0
    assert call(p[0] + 4, 256, 3, 256, p[1], p[2], 1e-6, p[3], 520, 1, st) < 0      # rows not 16-byte aligned
    assert call(p[0], 256, 4, 256, p[1], p[2], 1e-6, p[0], 256, 1, st) < 0          # in place is fp32 only
    assert call(p[0], 256, 0, 256, p[1], p[2], 1e-6, p[3], 520, 1, st) == 0         # nothing to do
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint16) == S16).all()
