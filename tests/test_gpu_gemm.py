"""`ibl_linear_f16_ex` (the encoder's fp16 MFMA GEMM on its own: two tile shapes x eight epilogues) against a float64 product of the same
fp16 operands -- every element, no allowed share of misses.  Inputs, reference and the per-element bounds with their derivation:
tests/gemm_cases.py.  Operands sit in NaN-padded allocations (row strides longer than the rows, NaN rows behind the last), outputs between
sentinel rows and columns, in every case.  Each case prints its worst error / bound per epilogue (run with -s); the last test prints the
worst per epilogue and family of the whole file."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gemm_cases as GC

pytestmark = pytest.mark.gpu

G = 2                                          # sentinel rows in front of and behind every output
WORST = {}                                     # (epilogue, family) -> worst error / bound seen in this run
ALL_EPIS = tuple(range(8))
# (M, N, K): the 128 x 128 form -- one row; both sides of a tile; 9 tiles (nwg % 8 = 1), nk = 3; M >= 4096 but N % 256 != 0 -- and the
# 256 x 256 form with one tile per workgroup: nk = 1 all tiles full; nk = 2, last tile one row; nk = 3, 34 tiles (nwg % 8 = 2), last 255 rows
SHAPES = [(1, 128, 64), (127, 128, 128), (128, 128, 128), (129, 128, 128), (257, 384, 192), (4100, 384, 64),
          (4096, 256, 64), (4097, 256, 128), (4351, 512, 192)]
LONG_K = (300, 128, 3072)
# persistent walks: "cus+1" = 256 * CUs + 1 rows (the issue's case: two tiles in one workgroup, the one-row tile alone in another);
# "cus+8" = 256 * (CUs + 7) + 1 rows (a workgroup walks a full tile and THEN the one-row tile); three or four tiles per workgroup
WALKS = ["cus+1", "cus+8", (66000, 768, 64)]


def _cus():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    return n // 8 * 8 if n >= 8 else 8


def _shape(s):
    if s == "cus+1":
        return 256 * _cus() + 1, 256, 64
    if s == "cus+8":
        return 256 * (_cus() + 7) + 1, 256, 64
    return s


def _assert_coverage(s, M, N, K):
    """the launch is the one the case is named for -- from the device's own CU count, so another device fails here instead of testing less"""
    w = GC.tile_walk(M, N, _cus())
    per = [len(b) for b in w["blocks"]]
    ragged_first = [b for b, blk in enumerate(w["blocks"]) if not blk[0][2]]
    if s in SHAPES[:6] or s == LONG_K:
        assert not w["t256"] and w["grid"] == w["nwg"]
    if s == (257, 384, 192):
        assert w["nwg"] == 9 and w["nwg"] % 8 == 1 and K // 64 == 3
    if s == (4100, 384, 64):
        assert M >= 4096 and N % 256 != 0
    if s in SHAPES[6:]:
        assert w["t256"] and max(per) == 1
    if s == (4096, 256, 64):
        assert K // 64 == 1 and not ragged_first
    if s == (4097, 256, 128):
        assert K // 64 == 2 and M - 256 * (w["nbm"] - 1) == 1
    if s == (4351, 512, 192):
        assert K // 64 == 3 and w["nwg"] == 34 and w["nwg"] % 8 == 2 and M - 256 * (w["nbm"] - 1) == 255
    if s == "cus+1":
        # one workgroup walks two (full) tiles; the XCD remap gives the one-row tile to the last workgroup as its only tile
        assert w["t256"] and per.count(2) == 1 and max(per) == 2 and ragged_first == [w["grid"] - 1] and not GC.full_then_ragged(w)
    if s == "cus+8":
        assert w["t256"] and GC.full_then_ragged(w) == [7] and w["blocks"][7][-1] == (w["nbm"] - 1, 0, False) and not ragged_first
    if s == (66000, 768, 64):
        assert w["t256"] and w["nwg"] == 774 and min(per) >= 3 and len(GC.full_then_ragged(w)) == 3 and not ragged_first
    return w


def _nan16(rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=torch.float16, device="cuda")


def _upload(c):
    """x, W as views into NaN-filled allocations: ldx = K + 8, ldw = K + 16, three NaN rows behind the last row of x"""
    x, W = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["W"]).cuda()
    (M, K), N = x.shape, W.shape[0]
    xb, Wb = _nan16(M + 3, K + 8), _nan16(N, K + 16)
    xb[:M, :K] = x
    Wb[:, :K] = W
    return xb[:M, :K], Wb[:, :K]


def _dev_rows(family, rows, N, tag):
    """(rows, N) fp32 on the device: what a read-modify-write epilogue finds in `out`, or position rows; integers for `exact`"""
    g = torch.Generator(device="cuda").manual_seed(GC.SEED + 1000 * tag + rows + N)
    if family == "exact":
        return torch.randint(-1000, 1001, (rows, N), generator=g, device="cuda").float()
    return torch.randn((rows, N), generator=g, device="cuda")


class Out:
    """an output of `rows` x `width` between G sentinel rows on either side and 8 sentinel columns behind every row"""

    def __init__(self, rows, width, f16, init=None, init_rows=None):
        self.rows, self.width = rows, width
        self.sent = GC.SENT16 if f16 else GC.SENT32
        self.buf = torch.full((rows + 2 * G, width + 8), self.sent, dtype=torch.int16 if f16 else torch.int32, device="cuda")
        self.win = self.buf[G:G + rows, :width].view(torch.float16 if f16 else torch.float32)
        if init is not None:
            if init_rows is None:
                self.win.copy_(init)
            else:
                self.win[init_rows] = init

    def intact(self, written_rows=None):
        """everything but the window (or its `written_rows`) still holds the sentinel"""
        chk = self.buf.clone()
        w = chk[G:G + self.rows, :self.width]
        if written_rows is None:
            w.fill_(self.sent)
        else:
            w[written_rows] = self.sent
        return bool((chk == self.sent).all())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _judge(epi, family, got, ref, bnd, what, valid=None):
    """every element of `got` within `bnd` of `ref`; on `exact`, bit-equal where gemm_cases says so"""
    assert bool(torch.isfinite(got).all()), f"{what}: NaN or infinity in the result"
    if family == "exact" and epi in GC.BIT_EXACT:
        assert torch.equal(_bits(got), _bits(ref.to(got.dtype))), f"{what}: not bit-equal to the reference on exact inputs"
    ratio = (got.double() - ref).abs() / bnd
    if valid is not None:
        ratio = torch.where(valid, ratio, torch.zeros_like(ratio))
    r = float(ratio.max())
    key = (GC.EPI_NAMES[epi] + ("" if valid is None else " h+lo/64"), family)
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f"gemm vs fp64: {what}: worst error / bound {r:.3f}")
    assert r <= 1.0, (what, r, np.unravel_index(int(ratio.argmax()), ratio.shape))


def _run_all(s, family, epis, M, N, K):
    from ibloc_amd import vit as V
    c = GC.make(family, M, N, K, resid=False)
    x, W = _upload(c)
    bias, scale = torch.from_numpy(c["bias"]).cuda(), torch.from_numpy(c["scale"]).cuda()
    b64, s64 = bias.double(), scale.double()
    y, S = GC.products(x, W)
    assert bool(torch.isfinite(y).all())
    for epi in epis:
        what = f"{M} x {N} x {K} {family} {GC.EPI_NAMES[epi]}"
        if epi in GC.F16_EPIS:
            terms = {GC.EPI_X2: 2, GC.EPI_X3: 3}.get(epi, 1)
            o = Out(M, terms * N, True)
            V.linear_f16_ex(x, W, o.win, epi, bias=bias)
            assert o.intact(), f"{what}: wrote outside its rows / columns"
            ref, bnd = GC.expected(epi, y, S, K, bias=b64)
            h = o.win[:, :N]
            _judge(epi, family, h, ref, bnd, what)
            assert bool(torch.isfinite(o.win).all()), f"{what}: NaN or infinity in a later column block"
            if terms > 1:
                assert torch.equal(_bits(o.win[:, (terms - 1) * N:]), _bits(GC.split_of(h))), f"{what}: h / 64 block"
            if terms == 3:
                ref3, bnd3, valid = GC.expected_two_term(y, S, K, bias=b64)
                two = h.double() + o.win[:, N:2 * N].double() / GC.SPLIT
                _judge(epi, family, two, ref3, bnd3, what + " h + lo / 64", valid=valid)
        elif epi in (GC.EPI_F32, GC.EPI_RESID, GC.EPI_PRE):
            r0 = _dev_rows(family, M, N, epi) if epi != GC.EPI_F32 else None
            o = Out(M, N, False, init=r0)
            V.linear_f16_ex(x, W, o.win, epi, bias=bias, scale=scale if epi == GC.EPI_RESID else None, alpha=GC.ALPHA)
            assert o.intact(), f"{what}: wrote outside its rows / columns"
            ref, bnd = GC.expected(epi, y, S, K, bias=b64, scale=s64, resid=r0.double() if r0 is not None else None, alpha=GC.ALPHA)
            _judge(epi, family, o.win, ref, bnd, what)
        else:
            # the patch scatter on this shape: one crop of M patches, M + 1 tokens (the geometry itself: test_patch_scatter)
            rows = torch.zeros(M + 1, dtype=torch.bool, device="cuda")
            rows[1:] = True
            pos = _dev_rows(family, M, N, 30)
            o = Out(M + 1, N, False)
            V.linear_f16_ex(x, W, o.win, epi, bias=bias, pos=pos, tokens_per_crop=M + 1, patches_per_crop=M)
            assert o.intact(rows), f"{what}: wrote outside the patch rows"
            ref, bnd = GC.expected(epi, y, S, K, bias=b64, pos=pos.double())
            _judge(epi, family, o.win[1:], ref, bnd, what + " (pos)")
            r0 = _dev_rows(family, M, N, 31)
            o = Out(M + 1, N, False, init=r0, init_rows=rows)
            V.linear_f16_ex(x, W, o.win, epi, bias=bias, alpha=GC.ALPHA, accumulate=True, tokens_per_crop=M + 1, patches_per_crop=M)
            assert o.intact(rows), f"{what}: wrote outside the patch rows"
            ref, bnd = GC.expected(epi, y, S, K, bias=b64, resid=r0.double(), alpha=GC.ALPHA, accumulate=True)
            _judge(epi, family, o.win[1:], ref, bnd, what + " (accumulate)")
    torch.cuda.synchronize()


@pytest.mark.parametrize("family", GC.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_epilogue_vs_fp64(shape, family):
    M, N, K = shape
    _assert_coverage(shape, M, N, K)
    _run_all(shape, family, ALL_EPIS, M, N, K)


@pytest.mark.parametrize("family", ("exact", "normal", "cancel"))
def test_long_k_vs_fp64(family):
    """48 K steps of the plain two-stage loop: the fp16 and the fp32 store epilogue"""
    M, N, K = LONG_K
    _assert_coverage(LONG_K, M, N, K)
    _run_all(LONG_K, family, (GC.EPI_F16, GC.EPI_F32), M, N, K)


@pytest.mark.parametrize("family", ("exact", "normal", "gelu_span"))
@pytest.mark.parametrize("shape", WALKS, ids=str)
def test_persistent_walk_vs_fp64(shape, family):
    """several tiles per workgroup of the 256 x 256 form: every epilogue behind the next tile's prologue"""
    M, N, K = _shape(shape)
    _assert_coverage(shape, M, N, K)
    _run_all(shape, family, ALL_EPIS, M, N, K)


@pytest.mark.parametrize("shape", WALKS, ids=str)
def test_persistent_walk_is_deterministic(shape):
    """two runs into fresh buffers, bit for bit (guards included): what a read of a stage that has not landed would break"""
    from ibloc_amd import vit as V
    M, N, K = _shape(shape)
    _assert_coverage(shape, M, N, K)
    c = GC.make("normal", M, N, K, resid=False)
    x, W = _upload(c)
    bias, scale = torch.from_numpy(c["bias"]).cuda(), torch.from_numpy(c["scale"]).cuda()
    r0 = _dev_rows("normal", M, N, 2)
    for epi in (GC.EPI_F16, GC.EPI_X3, GC.EPI_RESID, GC.EPI_PRE, GC.EPI_F32):
        outs = []
        for _ in range(2):
            f16 = epi in GC.F16_EPIS
            o = Out(M, (3 if epi == GC.EPI_X3 else 1) * N, f16, init=None if f16 or epi == GC.EPI_F32 else r0)
            V.linear_f16_ex(x, W, o.win, epi, bias=bias, scale=scale if epi == GC.EPI_RESID else None, alpha=GC.ALPHA)
            outs.append(o.buf)
        assert torch.equal(outs[0], outs[1]), f"{M} x {N} x {K} {GC.EPI_NAMES[epi]}: two runs differ"


@pytest.mark.parametrize("family", ("exact", "normal"))
def test_tile_shapes_agree(family):
    """the same rows and columns through the 256 x 256 form (the first 256 weight rows alone) and the 128 x 128 form (all 384): on exact
    inputs bit for bit, else both within the bound of the one reference (two fp16 results may legitimately differ by one ulp, which is
    twice the bound's rounding term, so the bound is held against the reference and not against each other)"""
    from ibloc_amd import vit as V
    M, N, K, NA = 4097, 384, 128, 256
    assert GC.tile_walk(M, NA, _cus())["t256"] and not GC.tile_walk(M, N, _cus())["t256"]
    c = GC.make(family, M, N, K, resid=False)
    x, W = _upload(c)
    bias, scale = torch.from_numpy(c["bias"]).cuda(), torch.from_numpy(c["scale"]).cuda()
    y, S = GC.products(x, W)
    r0 = _dev_rows(family, M, N, 4)
    for epi in (GC.EPI_F16, GC.EPI_GELU, GC.EPI_RESID, GC.EPI_F32, GC.EPI_PRE, GC.EPI_X3):
        f16, terms = epi in GC.F16_EPIS, 3 if epi == GC.EPI_X3 else 1
        rmw = epi in (GC.EPI_RESID, GC.EPI_PRE)
        got = {}
        for n in (NA, N):
            o = Out(M, terms * n, f16, init=r0[:, :n] if rmw else None)
            V.linear_f16_ex(x, W[:n], o.win, epi, bias=bias[:n].contiguous(), scale=scale[:n].contiguous() if epi == GC.EPI_RESID else None,
                            alpha=GC.ALPHA)
            assert o.intact()
            got[n] = [o.win[:, t * n:t * n + NA] for t in range(terms)]
        what = f"tile shapes, {family} {GC.EPI_NAMES[epi]}"
        ref, bnd = GC.expected(epi, y[:, :NA], S[:, :NA], K, bias=bias[:NA].double(), scale=scale[:NA].double(), resid=r0[:, :NA].double(),
                               alpha=GC.ALPHA)
        for n in (NA, N):
            _judge(epi, family, got[n][0], ref, bnd, f"{what}, n_out {n}")
        if family == "exact" and epi in GC.BIT_EXACT:
            assert torch.equal(_bits(got[NA][0]), _bits(got[N][0])), what
        if terms == 3:
            for n in (NA, N):
                assert torch.equal(_bits(got[n][2]), _bits(GC.split_of(got[n][0]))), what


@pytest.mark.parametrize("family", ("exact", "normal", "cancel"))
@pytest.mark.parametrize("shape", [(257, 384, 192), (4351, 512, 192)], ids=lambda s: "x".join(map(str, s)))
def test_resid_pre_against_resid(shape, family):
    """scale NULL, alpha 1: the preloaded-residual epilogue and the read-modify-write one compute the same thing"""
    from ibloc_amd import vit as V
    M, N, K = shape
    c = GC.make(family, M, N, K, resid=False)
    x, W = _upload(c)
    bias = torch.from_numpy(c["bias"]).cuda()
    y, S = GC.products(x, W)
    r0 = _dev_rows(family, M, N, 5)
    got = {}
    for epi in (GC.EPI_RESID, GC.EPI_PRE):
        o = Out(M, N, False, init=r0)
        V.linear_f16_ex(x, W, o.win, epi, bias=bias, alpha=1.0)
        assert o.intact()
        ref, bnd = GC.expected(epi, y, S, K, bias=bias.double(), resid=r0.double(), alpha=1.0)
        _judge(epi, family, o.win, ref, bnd, f"{M} x {N} x {K} {family} {GC.EPI_NAMES[epi]} (scale NULL, alpha 1)")
        got[epi] = o.win
    if family == "exact":
        assert torch.equal(_bits(got[GC.EPI_RESID]), _bits(got[GC.EPI_PRE]))


# (patches per crop P, tokens per crop T, crops, N, K): P + 1 and P + 5 tokens; 256 patches on both tile shapes (17 crops: 4352 rows)
@pytest.mark.parametrize("family", ("exact", "normal"))
@pytest.mark.parametrize("geo", [(3, 4, 43, 128, 64), (3, 8, 43, 128, 64), (16, 17, 17, 384, 128), (16, 21, 17, 384, 128),
                                 (256, 257, 17, 256, 64), (256, 261, 17, 256, 64), (256, 257, 17, 384, 64), (256, 261, 17, 384, 64)],
                         ids=lambda g: "P{}-T{}-B{}-N{}-K{}".format(*g))
def test_patch_scatter(geo, family):
    """row b * P + p of x lands in token row b * T + 1 + p with position row p; the CLS row of every crop and the token rows behind the
    patches keep the sentinel.  Rows that are no whole number of crops are refused (include/ibloc.h), see test_refusals."""
    from ibloc_amd import vit as V
    P, T, B, N, K = geo
    M = B * P
    assert GC.tile_walk(M, N, _cus())["t256"] == (N == 256 and P == 256)
    c = GC.make(family, M, N, K, resid=False)
    x, W = _upload(c)
    bias = torch.from_numpy(c["bias"]).cuda()
    y, S = GC.products(x, W)
    tok = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    tok[:, 1:P + 1] = True
    tok = tok.reshape(B * T)
    pos = _dev_rows(family, P, N, 6)
    pos_rows = pos.double().repeat(B, 1)                     # row b * P + p of x meets position row p
    what = f"patch scatter P {P} T {T} crops {B} n_out {N} {family}"
    o = Out(B * T, N, False)
    V.linear_f16_ex(x, W, o.win, GC.EPI_PATCH, bias=bias, pos=pos, tokens_per_crop=T, patches_per_crop=P)
    assert o.intact(tok), f"{what}: CLS or trailing token rows written"
    ref, bnd = GC.expected(GC.EPI_PATCH, y, S, K, bias=bias.double(), pos=pos_rows)
    _judge(GC.EPI_PATCH, family, o.win[tok], ref, bnd, what + " (pos)")
    r0 = _dev_rows(family, M, N, 7)
    o = Out(B * T, N, False, init=r0, init_rows=tok)
    V.linear_f16_ex(x, W, o.win, GC.EPI_PATCH, bias=bias, alpha=GC.ALPHA, accumulate=True, tokens_per_crop=T, patches_per_crop=P)
    assert o.intact(tok), f"{what}: CLS or trailing token rows written"
    ref, bnd = GC.expected(GC.EPI_PATCH, y, S, K, bias=bias.double(), resid=r0.double(), alpha=GC.ALPHA, accumulate=True)
    _judge(GC.EPI_PATCH, family, o.win[tok], ref, bnd, what + " (accumulate)")


def test_refusals_launch_nothing():
    from ibloc_amd import _lib, vit as V
    x, W = _upload(GC.make("normal", 16, 128, 64, resid=False))
    o16, o32 = Out(17, 3 * 128, True), Out(17, 128, False)
    pos = torch.zeros(16, 128, device="cuda")

    def refused(epi=0, **kw):
        out = o16 if epi in GC.F16_EPIS else o32
        f = dict(x=x.data_ptr(), ldx=x.stride(0), W=W.data_ptr(), ldw=W.stride(0), bias=None, scale=None, pos=pos.data_ptr(),
                 out=out.win.data_ptr(), ldo=out.win.stride(0), rows=16, n_out=128, n_in=64, epilogue=epi, accumulate=0,
                 tokens_per_crop=17, patches_per_crop=16, alpha=1.0)
        f.update(kw)
        d = V.LinearDesc(**f)
        with pytest.raises(_lib.IblError):
            _lib.check(_lib.lib.ibl_linear_f16_ex(C.byref(d), torch.cuda.current_stream().cuda_stream), "ibl_linear_f16_ex")

    for epi in range(8):
        for k in ("x", "W", "out"):
            refused(epi, **{k: None})                                             # a null operand
        refused(epi, n_out=100)
        refused(epi, n_in=32)
        refused(epi, ldx=56)                                                      # shorter than the row
        refused(epi, ldw=56)
        refused(epi, ldo=120)
        refused(epi, ldx=68)                                                      # no multiple of 8 elements
        refused(epi, ldw=76)
        refused(epi, ldo=388)
    refused(GC.EPI_X2, ldo=248)                                                   # ldo < terms * n_out
    refused(GC.EPI_X3, ldo=376)
    for a in (0.0, -0.015625, 3.0, 0.75, float("inf"), float("nan")):
        refused(GC.EPI_PRE, alpha=a)
        refused(GC.EPI_PATCH, alpha=a, accumulate=1)
    refused(GC.EPI_PATCH, patches_per_crop=0)
    refused(GC.EPI_PATCH, patches_per_crop=-16)
    refused(GC.EPI_PATCH, tokens_per_crop=16)                                     # no room for the CLS row
    refused(GC.EPI_PATCH, pos=None)
    refused(GC.EPI_PATCH, patches_per_crop=5, tokens_per_crop=6)                  # 16 rows: three crops and a part of one
    refused(8)
    refused(-1)
    for epi in (3, 5, 6, 7):                                                      # the older entry knows its four epilogues only
        with pytest.raises(_lib.IblError):
            _lib.check(_lib.lib.ibl_linear_f16(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), None, None, 16, 128, 64, epi,
                                               o32.win.data_ptr(), o32.win.stride(0), torch.cuda.current_stream().cuda_stream), "ibl_linear_f16")
    torch.cuda.synchronize()
    assert o16.intact(torch.zeros(17, dtype=torch.bool, device="cuda")) and o32.intact(torch.zeros(17, dtype=torch.bool, device="cuda"))
    # and rows = 0 is no error
    V.linear_f16_ex(x[:0], W, o32.win[:0], GC.EPI_F32)


def test_zz_worst_ratios():
    """not a check of its own: the table the comment block of tests/gemm_cases.py quotes (complete when the whole file ran)"""
    for (epi, family), r in sorted(WORST.items()):
        print(f"gemm worst error / bound: {epi:22s} {family:10s} {r:.3f}")
    assert all(r <= 1.0 for r in WORST.values())
