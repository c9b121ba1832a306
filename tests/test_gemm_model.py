"""CPU: what tests/test_gpu_gemm.py rests on -- C_GELU of tests/gemm_cases.py is the constant its rule gives, the input families are what
they claim, the torch fp64 reference agrees with a numpy one, the restated tile remap gives the walks the GPU cases are named for, and
`ibl_linear_f16_ex` refuses bad arguments before it touches the device."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import gemm_cases as GC


def test_c_gelu_is_the_smallest_power_of_two_under_three_quarters():
    """the emulated gelu_erf2 (its fp32 value) against the exact GELU over the gelu_span grid"""
    ratios = {}
    for e in range(-26, -19):
        ratios[e], at, two = GC.gelu_model_ratio(2.0 ** e)
        print(f"gelu_erf2 emulation vs fp64: C_GELU 2^{e}: worst error / (C_GELU |v|) {ratios[e]:.3f} at v = {at:.6g}; h + lo / 64 against "
              f"its whole bound {two:.3f}")
        assert two <= 1.0 or e < round(math.log2(GC.C_GELU))
    chosen = int(round(math.log2(GC.C_GELU)))
    assert 2.0 ** chosen == GC.C_GELU
    assert ratios[chosen] <= 0.75 < ratios[chosen - 1], (chosen, ratios)
    # and the stored first block alone (one fp16 rounding on top) stays inside the bound of IBL_LINEAR_GELU_F16
    v = GC.gelu_grid()
    h = GC.h16(GC.emulate_gelu(v)).astype(np.float64)
    v64 = torch.from_numpy(v.astype(np.float64))
    ref, bnd = GC.expected(GC.EPI_GELU, v64, torch.zeros_like(v64), 64)
    r = float(((torch.from_numpy(h) - ref).abs() / bnd).max())
    print(f"gelu_erf2 emulation, fp16 result: worst error / bound {r:.3f}")
    assert r <= 1.0


def test_emulated_gelu_details():
    v = np.array([0.0, -0.0, 1e-30, 50.0, 66000.0, -20.0], np.float32)
    g = GC.emulate_gelu(v)
    assert g[0] == 0.0 and g[1] == 0.0 and g[3] == 50.0 and g[4] == 66000.0
    assert abs(g[5]) <= GC.C_GELU * 20.0                  # the two halves cancel to a few ulp of |v|
    assert GC.h16(np.float32(1e6)) == 65504.0 and GC.h16(np.float32(-65520.0)) == -65504.0 and GC.h16(np.float32(65519.0)) == 65504.0


def test_reference_agrees_with_numpy():
    """the smallest case, every epilogue: torch.float64 against numpy float64 with math.erfc"""
    M, N, K = 1, 128, 64
    c = GC.make("normal", M, N, K)
    x, W = c["x"].astype(np.float64), c["W"].astype(np.float64)
    b, s, r = c["bias"].astype(np.float64), c["scale"].astype(np.float64), c["resid"].astype(np.float64)
    pos = GC.make_pos("normal", M, N).astype(np.float64)
    y = x @ W.T
    v = y + b
    gelu = np.array([0.5 * t * math.erfc(-t / math.sqrt(2.0)) for t in v.ravel()]).reshape(v.shape)
    want = {GC.EPI_F16: v, GC.EPI_GELU: gelu, GC.EPI_RESID: r + v * s, GC.EPI_F32: v, GC.EPI_PRE: r + b + GC.ALPHA * y, GC.EPI_X2: gelu,
            GC.EPI_X3: gelu}
    ty, tS = GC.products(torch.from_numpy(c["x"]), torch.from_numpy(c["W"]))
    assert np.abs(tS.numpy() - np.abs(x) @ np.abs(W).T).max() <= 1e-12
    t = {k: torch.from_numpy(a) for k, a in dict(bias=b, scale=s, resid=r).items()}
    for epi, w in want.items():
        ref, bnd = GC.expected(epi, ty, tS, K, bias=t["bias"], scale=t["scale"], resid=t["resid"], alpha=GC.ALPHA)
        assert np.abs(ref.numpy() - w).max() <= 1e-13 * max(1.0, np.abs(w).max()), epi
        assert float(bnd.min()) > 0.0
    ref, _ = GC.expected(GC.EPI_PATCH, ty, tS, K, bias=t["bias"], pos=torch.from_numpy(pos))
    assert np.abs(ref.numpy() - (v + pos)).max() <= 1e-13
    ref, _ = GC.expected(GC.EPI_PATCH, ty, tS, K, bias=t["bias"], resid=t["resid"], alpha=GC.ALPHA, accumulate=True)
    assert np.abs(ref.numpy() - (r + GC.ALPHA * v)).max() <= 1e-13
    ref3, _, valid = GC.expected_two_term(ty, tS, K, bias=t["bias"])
    assert np.abs(ref3.numpy() - gelu).max() <= 1e-13 and bool(valid.all())


@pytest.mark.parametrize("shape", [(257, 384, 192), (300, 128, 3072), (129, 128, 64)])
def test_exact_family_is_exact(shape):
    """every partial sum in any order is an integer of at most 2048, and the inputs are not symmetric under row / column / K swaps"""
    M, N, K = shape
    c = GC.make("exact", M, N, K)
    x, W = c["x"].astype(np.float64), c["W"].astype(np.float64)
    S = np.abs(x) @ np.abs(W).T
    assert (S + np.abs(c["bias"])[None, :]).max() <= 2048.0
    assert (x == np.round(x)).all() and np.abs(x).max() == 2 and np.abs(W).max() == 2
    y = x @ W.T
    assert (y.astype(np.float16).astype(np.float64) == y).all()
    assert len({r.tobytes() for r in c["x"][:min(M, 128)]}) == min(M, 128) and len({r.tobytes() for r in c["W"]}) == N
    for step in (8, 32, 64):                  # a K chunk swapped with its neighbour changes most results
        if 2 * step > K:
            continue
        xs = x.copy()
        xs[:, :step], xs[:, step:2 * step] = x[:, step:2 * step], x[:, :step]
        assert ((xs @ W.T) != y).mean() > 0.5 or K > 1024
    assert (np.log2(c["scale"]) == np.round(np.log2(c["scale"]))).all()
    assert (c["resid"] == np.round(c["resid"])).all() and (GC.make_pos("exact", 16, N) % 1 == 0).all()


def test_other_families_are_what_they_claim():
    M, N, K = 257, 384, 192
    c = GC.make("cancel", M, N, K)
    y, S = GC.products(torch.from_numpy(c["x"]), torch.from_numpy(c["W"]))
    ratio = float((S / y.abs().clamp_min(1e-30)).median())
    print(f"cancel: median sum|x w| / |sum x w| = {ratio:.0f}")
    assert 500.0 <= ratio <= 5000.0
    # gelu_span: every 128 x 128 tile holds pre-activations in every half-unit bin of -12 .. 12, below -6, and next to 0
    c = GC.make("gelu_span", M, N, 64)
    y, _ = GC.products(torch.from_numpy(c["x"]), torch.from_numpy(c["W"]))
    v = (y + torch.from_numpy(c["bias"]).double()).numpy()
    for r0 in (0, 128):
        for c0 in (0, 128, 256):
            t = v[r0:r0 + 128, c0:c0 + 128]
            hist, _ = np.histogram(t, bins=48, range=(-12.0, 12.0))
            assert hist.min() > 0, (r0, c0)
            assert (t < -6.0).sum() > 1000 and np.abs(t).min() < 0.01
    c = GC.make("saturate", M, N, K)
    y, _ = GC.products(torch.from_numpy(c["x"]), torch.from_numpy(c["W"]))
    v = (y + torch.from_numpy(c["bias"]).double()).numpy()
    assert (v > 65520.0).mean() > 0.2 and (v < -65520.0).mean() > 0.2 and ((np.abs(v) > 65400.0) & (np.abs(v) < 65520.0)).sum() > 1000
    assert (np.abs(v) < 10.0).mean() > 0.2


def test_tile_walks_of_the_gpu_cases():
    """with the MI355X's 256 CUs; tests/test_gpu_gemm.py asserts the same from the device's own count"""
    cus = 256
    w = GC.tile_walk(257, 384, cus)
    assert not w["t256"] and w["nwg"] == 9 and w["nwg"] % 8 == 1
    assert not GC.tile_walk(4100, 384, cus)["t256"]
    w = GC.tile_walk(4351, 512, cus)
    assert w["t256"] and w["nwg"] == 34 and w["nwg"] % 8 == 2 and all(len(b) == 1 for b in w["blocks"])
    # 256 * CUs + 1 rows: one workgroup walks two tiles, but the remap hands the one-row tile to workgroup CUs - 1 as its only tile
    w = GC.tile_walk(256 * cus + 1, 256, cus)
    assert w["nwg"] == cus + 1 and [len(b) for b in w["blocks"]].count(2) == 1 and GC.full_then_ragged(w) == []
    assert w["blocks"][cus - 1] == [(cus, 0, False)]
    # 256 * (CUs + 7) + 1 rows: workgroup 7 walks a full tile and then the one-row tile
    w = GC.tile_walk(256 * (cus + 7) + 1, 256, cus)
    assert GC.full_then_ragged(w) == [7] and w["blocks"][7][1] == (cus + 7, 0, False)
    w = GC.tile_walk(66000, 768, cus)
    assert w["nwg"] == 774 and min(len(b) for b in w["blocks"]) == 3 and len(GC.full_then_ragged(w)) == 3


def test_entry_refuses_before_touching_the_device():
    """the argument checks of ibl_linear_f16_ex come before any launch, so they run here without a GPU (the pointers are never followed)"""
    from ibloc_amd import _lib, vit as V
    P = 0x10000

    def call(**kw):
        f = dict(x=P, ldx=64, W=P, ldw=64, bias=None, scale=None, pos=None, out=P, ldo=128, rows=16, n_out=128, n_in=64, epilogue=0,
                 accumulate=0, tokens_per_crop=0, patches_per_crop=0, alpha=1.0)
        f.update(kw)
        d = V.LinearDesc(**f)
        return _lib.lib.ibl_linear_f16_ex(C.byref(d), None)

    assert _lib.lib.ibl_linear_f16_ex(None, None) < 0
    for k in ("x", "W", "out"):
        assert call(**{k: None}) < 0 and b"null" in _lib.lib.ibl_last_error()
    assert call(n_out=100) < 0 and call(n_out=0) < 0 and call(n_in=32) < 0 and call(n_in=96, ldx=96, ldw=96) < 0
    assert call(ldx=56) < 0 and call(ldw=56) < 0 and call(ldo=120) < 0              # shorter than the row
    assert call(ldx=68) < 0 and call(ldw=68) < 0 and call(ldo=132) < 0              # not a multiple of 8 elements
    assert call(epilogue=6, ldo=248) < 0 and call(epilogue=7, ldo=376) < 0 and call(epilogue=7, ldo=256) < 0
    assert call(epilogue=8) < 0 and call(epilogue=-1) < 0
    assert call(rows=-1) < 0 and call(rows=1 << 31) < 0
    for a in (0.0, -0.5, 3.0, 0.75, float("nan"), float("inf"), 1e-45):
        assert call(epilogue=5, alpha=a) < 0, a
        assert call(epilogue=3, accumulate=1, alpha=a, patches_per_crop=16, tokens_per_crop=17) < 0, a
    geo = dict(epilogue=3, pos=P, patches_per_crop=16, tokens_per_crop=17)
    assert call(**{**geo, "patches_per_crop": 0}) < 0 and call(**{**geo, "patches_per_crop": -4}) < 0
    assert call(**{**geo, "tokens_per_crop": 16}) < 0 and call(**{**geo, "tokens_per_crop": 3}) < 0
    assert call(**{**geo, "pos": None}) < 0
    assert call(**{**geo, "patches_per_crop": 5, "tokens_per_crop": 6}) < 0       # 16 rows are no whole number of crops of 5
    assert call(**{**geo, "accumulate": 2}) < 0
    for epi in range(8):
        assert call(epilogue=epi, rows=0) == 0
    assert call(rows=0, x=None) == 0
    # the older entry: its four epilogues only, the same checks
    lin = _lib.lib.ibl_linear_f16
    assert lin(P, 64, P, 64, None, None, 16, 128, 64, 3, P, 128, None) < 0 and lin(P, 64, P, 64, None, None, 16, 128, 64, 5, P, 128, None) < 0
    assert lin(P, 64, P, 64, None, None, 16, 100, 64, 0, P, 128, None) < 0 and lin(None, 64, P, 64, None, None, 16, 128, 64, 0, P, 128, None) < 0
    assert lin(P, 64, P, 64, None, None, 0, 128, 64, 0, P, 128, None) == 0
