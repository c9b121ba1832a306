"""`ibl_attention_f16` (the encoder's attention kernel on its own: four key-tile tiers x three output layouts) against a float64
softmax(q k^T / 8) v of the same fp16 inputs -- every element, no allowed share of misses.

Bound on the first term (tests/attention_cases.py::bound): 2^-11 |ref| + 2^-11 A + 2^-14 max|v|, A = sum_i p_i |v_i|.  A CPU emulation of
the kernel's arithmetic reaches at most 0.71 of it on these inputs (tests/test_attention_model.py, which also says why 2^-14).
Measured on the MI355X, worst error / bound per family over all token counts (each case prints its own, run with -s):
    diffuse 0.47   peaked 0.68   two_level 0.21   offset 0.56 (the same rows without the offset: 0.56)   ramp 0.68   ramp_diffuse 0.34
three-term rows, a + lo / 64 against the bound with 2^-21 |ref|: 0.68 -- the kernel sits where the emulation does."""
import numpy as np
import pytest
import torch

from tests import attention_cases as AC

pytestmark = pytest.mark.gpu

SENTINEL = 0x7E2A            # an fp16 NaN pattern no kernel writes
LAYOUT_T = (1, 2, 17, 50, 64, 65, 129, 144, 197, 208, 257, 272)    # tiers and both sides of their boundaries, odd and even T


def _run(qkv_np, heads, cls_only=False, terms=1, guard=0):
    """-> (out numpy (B, T, terms * D), the whole guarded buffer as int16 numpy, G): `out` sits between G sentinel rows on either side"""
    from ibloc_amd import vit as V
    B, T, W = qkv_np.shape
    D = W // 3
    qkv = torch.from_numpy(qkv_np).cuda()
    G = guard
    buf = torch.full(((B * T + 2 * G) * terms * D,), SENTINEL, dtype=torch.int16, device="cuda")
    out = buf[G * terms * D:(G + B * T) * terms * D].view(torch.float16).view(B, T, terms * D)
    V.attention_f16(qkv, heads, cls_only=cls_only, terms=terms, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), buf.cpu().numpy().reshape(B * T + 2 * G, terms * D), G


def _ratio(a16, ref, bnd):
    return float((np.abs(a16.astype(np.float64) - ref) / bnd).max())


@pytest.mark.parametrize("family", AC.FAMILIES)
@pytest.mark.parametrize("T", AC.T_ALL)
def test_attention_vs_fp64(T, family):
    """terms = 1, every row a query: every token count x every input family"""
    H = AC.HEADS_OF_T[T]
    c = AC.case(family, T)
    ref, A, plain = AC.reference(c.get("q0", c["q"]), c.get("k0", c["k"]), c["v"])
    bnd = AC.bound(ref, A, c["v"])
    out, _, _ = _run(AC.pack(c["q"], c["k"], c["v"]), H)
    a = AC.unpack_out(out, H)[0]
    assert np.isfinite(a.astype(np.float32)).all()
    r = _ratio(a, ref, bnd)
    print(f"attention vs fp64: T {T} heads {H} {family}: worst error / bound {r:.3f}")
    assert r <= 1.0, (T, family, r)
    if family == "offset":
        # max subtraction: the rows without the common +60 give the same result within the same bound
        out0, _, _ = _run(AC.pack(c["q0"], c["k0"], c["v"]), H)
        r0 = _ratio(AC.unpack_out(out0, H)[0], ref, bnd)
        print(f"attention vs fp64: T {T} heads {H} offset removed: worst error / bound {r0:.3f}")
        assert r0 <= 1.0, (T, r0)
    if family in AC.DECISIVE and T >= 15:
        # the case is not vacuous: a kernel that ignored the logits (plain mean of v over the keys) would miss the bound >= 50-fold
        miss = np.abs(plain - ref) / bnd
        assert miss.max() >= 50.0 and np.median(miss) >= 10.0, (T, family, miss.max())


@pytest.mark.parametrize("family", ("peaked", "ramp", "two_level"))
@pytest.mark.parametrize("T", LAYOUT_T)
def test_terms_and_cls_only(T, family):
    """terms 2 / 3 and cls_only on every tier: the later column blocks derive from the first bit for bit, the first block does not depend
    on the layout, cls_only writes row 0 of every crop and nothing else"""
    H = AC.HEADS_OF_T[T]
    c = AC.case(family, T)
    qkv = AC.pack(c["q"], c["k"], c["v"])
    B, D = qkv.shape[0], H * AC.HD
    ref, A, _ = AC.reference(c["q"], c["k"], c["v"])
    bnd = AC.bound(ref, A, c["v"])
    bnd3 = AC.bound(ref, A, c["v"], out_rel=2.0 ** -21)
    full = {}
    for terms in (1, 2, 3):
        out, buf, G = _run(qkv, H, terms=terms, guard=3)
        full[terms] = out
        assert (buf[:G].view(np.uint16) == SENTINEL).all() and (buf[-G:].view(np.uint16) == SENTINEL).all(), "guard rows written"
        first = out[:, :, :D]
        assert np.array_equal(first.view(np.uint16), full[1].view(np.uint16)), f"first block of terms {terms} != terms 1"
        if terms > 1:
            want = (first.astype(np.float32) / np.float32(AC.SPLIT)).astype(np.float16)
            assert np.array_equal(out[:, :, (terms - 1) * D:].view(np.uint16), want.view(np.uint16)), f"terms {terms}: a / 64 block"
        if terms == 3:
            a, lo, _ = AC.unpack_out(out, H, 3)
            two = a.astype(np.float64) + lo.astype(np.float64) / AC.SPLIT
            r3 = float((np.abs(two - ref) / bnd3).max())
            print(f"attention three-term rows: T {T} heads {H} {family}: a + lo / 64 worst error / bound(2^-21) {r3:.3f}")
            assert r3 <= 1.0, (T, family, r3)
    assert _ratio(AC.unpack_out(full[1], H)[0], ref, bnd) <= 1.0
    for terms in (1, 2, 3):
        out, buf, G = _run(qkv, H, cls_only=True, terms=terms, guard=3)
        assert np.array_equal(out[:, 0].view(np.uint16), full[terms][:, 0].view(np.uint16)), f"cls_only row 0, terms {terms}"
        rows = buf.view(np.uint16)
        keep = np.ones(rows.shape[0], bool)
        keep[G + np.arange(B) * T] = False               # everything but the B CLS rows still holds the sentinel
        assert (rows[keep] == SENTINEL).all(), f"cls_only wrote outside the CLS rows, terms {terms}"


@pytest.mark.parametrize("T", (17, 145, 272))
def test_deterministic_and_batch_independent(T):
    H = AC.HEADS_OF_T[T]
    c = AC.case("peaked", T)
    assert c["q"].shape[0] == 3
    qkv = AC.pack(c["q"], c["k"], c["v"])
    for terms in (1, 3):
        a, _, _ = _run(qkv, H, terms=terms)
        b, _, _ = _run(qkv, H, terms=terms)
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
        for crop in range(3):
            one, _, _ = _run(np.ascontiguousarray(qkv[crop:crop + 1]), H, terms=terms)
            assert np.array_equal(one[0].view(np.uint16), a[crop].view(np.uint16)), f"crop {crop} of the batch != the crop alone"


def test_refusals_launch_nothing():
    from ibloc_amd import _lib, vit as V

    def guarded(B, T, D, terms=1):
        buf = torch.full((B * T * max(terms, 1) * D + 64,), SENTINEL, dtype=torch.int16, device="cuda")
        return buf, buf[:B * T * terms * D].view(torch.float16).view(B, T, terms * D)

    qkv = torch.zeros((1, 273, 3 * 128), dtype=torch.float16, device="cuda")
    buf, out = guarded(1, 273, 128)
    with pytest.raises(_lib.IblError):                     # one token beyond the widest tier
        V.attention_f16(qkv, 2, out=out)
    qkv = torch.zeros((2, 50, 3 * 128), dtype=torch.float16, device="cuda")
    buf2, out2 = guarded(2, 50, 128)
    with pytest.raises(_lib.IblError):                     # dim != 64 * heads
        V.attention_f16(qkv, 3, out=out2)
    st = torch.cuda.current_stream().cuda_stream
    for terms in (0, 4):
        assert _lib.lib.ibl_attention_f16(qkv.data_ptr(), out2.data_ptr(), 2, 50, 128, 2, 0, terms, st) < 0
    assert _lib.lib.ibl_attention_f16(None, out2.data_ptr(), 2, 50, 128, 2, 0, 1, st) < 0
    assert _lib.lib.ibl_attention_f16(qkv.data_ptr(), None, 2, 50, 128, 2, 0, 1, st) < 0
    assert b"null" in _lib.lib.ibl_last_error()
    assert _lib.lib.ibl_attention_f16(qkv.data_ptr(), out2.data_ptr(), -1, 50, 128, 2, 0, 1, st) < 0
    assert _lib.lib.ibl_attention_f16(qkv.data_ptr(), out2.data_ptr(), 2, 50, 128, 2, 2, 1, st) < 0            # cls_only is 0 or 1
    assert _lib.lib.ibl_attention_f16(qkv.data_ptr() + 2, out2.data_ptr(), 2, 50, 128, 2, 0, 1, st) < 0        # misaligned rows
    assert _lib.lib.ibl_attention_f16(qkv.data_ptr(), out2.data_ptr(), 0, 50, 128, 2, 0, 1, st) == 0           # nothing to do
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint16) == SENTINEL).all() and (buf2.cpu().numpy().view(np.uint16) == SENTINEL).all()
