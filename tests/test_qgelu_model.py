"""CPU: what tests/test_gpu_qgelu.py rests on -- C_QGELU and LIP_Q of tests/clip_openai_cases.py are what their rules give, the emulated
`quick_gelu2` behaves at the extremes as csrc/vit_gemm.hip says, and `ibl_linear_f16_ex` refuses a bad `activation` before it touches the
device."""
import ctypes as C
import math

import numpy as np
import torch

from tests import clip_openai_cases as QC
from tests import gemm_cases as GC


def test_c_qgelu_is_the_smallest_power_of_two_under_three_quarters():
    """the emulated quick_gelu2 (its fp32 value) against the exact QuickGELU over the grid: never NaN, within 0.75 C_QGELU max(|v|, TINY)"""
    v = QC.qgelu_grid()
    value = QC.emulate_qgelu(v)
    assert not np.isnan(value).any()
    ratios = {}
    for e in range(-26, -19):
        ratios[e], at, two = QC.qgelu_model_ratio(2.0 ** e)
        print(f"quick_gelu2 emulation vs fp64: C_QGELU 2^{e}: worst error / (C_QGELU |v|) {ratios[e]:.3f} at v = {at:.6g}; h + lo / 64 "
              f"against its whole bound {two:.3f}")
        assert two <= 1.0 or e < round(math.log2(QC.C_QGELU))
    chosen = int(round(math.log2(QC.C_QGELU)))
    assert 2.0 ** chosen == QC.C_QGELU
    assert ratios[chosen] <= 0.75 < ratios[chosen - 1], (chosen, ratios)
    # and the stored first block alone (one fp16 rounding on top) stays inside the bound of the epilogue
    v64 = torch.from_numpy(v.astype(np.float64))
    ref, bnd = QC.expected(v64, torch.zeros_like(v64), 64)
    r = float(((torch.from_numpy(GC.h16(value).astype(np.float64)) - ref).abs() / bnd).max())
    print(f"quick_gelu2 emulation, fp16 result: worst error / bound {r:.3f}")
    assert r <= 1.0


def test_lip_q_bounds_the_derivative():
    """q'(v) = s + 1.702 v s (1 - s), s = sigmoid(1.702 v): its largest magnitude, 1.0998 at v = 1.44, is what LIP_Q must cover"""
    v = np.linspace(-60.0, 60.0, 2_400_001)
    s = 1.0 / (1.0 + np.exp(-1.702 * v))
    d = np.abs(s + 1.702 * v * s * (1.0 - s))
    print(f"max |q'| = {d.max():.5f} at v = {v[d.argmax()]:.3f}")
    assert 1.0997 < d.max() <= QC.LIP_Q <= 1.11


def test_emulated_qgelu_extremes():
    f = np.float32
    v = np.array([0.0, -0.0, 1e-30, 200.0, 65504.0, 3.0e6, -200.0, -65504.0, -3.0e38, 3.0e38, -52.0, -52.25], f)
    g = QC.emulate_qgelu(v)
    assert not np.isnan(g).any()
    assert g[0] == 0.0 and g[1] == 0.0 and g[2] == f(1e-30) * f(0.5)
    assert g[3] == 200.0 and g[4] == 65504.0 and g[5] == f(3.0e6) and g[9] == f(3.0e38)          # v >> 0: v itself (f2h clamps it)
    for i in (6, 7, 8, 11):                                                                     # v << 0: exp2 overflows, rcp(inf) = 0, -0
        assert g[i] == 0.0 and np.signbit(g[i])
    assert g[10] < 0.0 and abs(g[10]) < 2.0 ** -100                                             # just before the overflow: tiny, finite
    assert (GC.h16(g[6:9]) == 0.0).all() and GC.h16(g[5]) == 65504.0
    # the reference evaluates without overflow on both sides
    r = QC.qgelu64(torch.tensor([-1.0e6, -800.0, 0.0, 800.0, 1.0e6], dtype=torch.float64))
    assert bool(torch.isfinite(r).all()) and r[0] == 0.0 and r[2] == 0.0 and r[3] == 800.0 and r[4] == 1.0e6
    x = torch.linspace(-30.0, 30.0, 6001, dtype=torch.float64)
    assert float((QC.qgelu64(x) - x * torch.sigmoid(1.702 * x)).abs().max()) <= 1e-14


def test_activation_field_lies_in_the_tail_padding():
    from ibloc_amd import vit as V
    assert C.sizeof(V.LinearDesc) == 112 and V.LinearDesc.activation.offset == 108 and V.LinearDesc.alpha.offset == 104
    assert V.LinearDesc().activation == V.ACT_GELU_ERF == 0 and V.ACT_QUICK_GELU == QC.ACT_QUICK == 1


def test_entry_refuses_a_bad_activation_before_touching_the_device():
    """the pointers are never followed: these run without a GPU"""
    from ibloc_amd import _lib, vit as V
    P = 0x10000

    def call(**kw):
        f = dict(x=P, ldx=64, W=P, ldw=64, bias=None, scale=None, pos=P, out=P, ldo=384, rows=16, n_out=128, n_in=64, epilogue=1,
                 accumulate=0, tokens_per_crop=17, patches_per_crop=16, alpha=1.0, activation=0)
        f.update(kw)
        d = V.LinearDesc(**f)
        return _lib.lib.ibl_linear_f16_ex(C.byref(d), None)

    for epi in (1, 6, 7):
        for act in (2, -1, 3, 1 << 30, -(1 << 31)):
            assert call(epilogue=epi, activation=act) < 0 and b"activation" in _lib.lib.ibl_last_error(), (epi, act)
        assert call(epilogue=epi, activation=1, rows=0) == 0
    for epi in (0, 2, 3, 4, 5):
        assert call(epilogue=epi, activation=1) < 0 and b"activation" in _lib.lib.ibl_last_error(), epi
        assert call(epilogue=epi, activation=2) < 0 and call(epilogue=epi, activation=-1) < 0
    assert call(epilogue=8) < 0 and call(epilogue=8, activation=1) < 0 and call(epilogue=9, activation=0) < 0
    assert call(epilogue=10, activation=1) < 0 and call(epilogue=-1, activation=1) < 0


def test_configurations():
    import dataclasses
    from ibloc_amd import vit as V
    want = {"clip_b32_openai": (768, 12, 12, 3072, 32, (7, 7), 512, 50), "clip_b16_openai": (768, 12, 12, 3072, 16, (14, 14), 512, 197),
            "clip_l14_openai": (1024, 24, 16, 4096, 14, (16, 16), 768, 257)}
    for name, (dim, depth, heads, mlp, patch, grid, proj, tokens) in want.items():
        c = V.CONFIGS[name]
        assert (c.name, c.dim, c.depth, c.heads, c.mlp_dim, c.patch, c.pos_grid, c.proj_dim, c.n_tokens) == \
            (name, dim, depth, heads, mlp, patch, grid, proj, tokens)
        assert c.pre_ln and c.final_ln and c.ln_eps == 1e-5 and c.recipe == "clip" and c.quick_gelu and not c.layerscale
        assert c.dim == 64 * c.heads and c.n_tokens <= 272 and c.depth <= V.MAX_LAYERS and c.dim <= 1024 and c.grid == c.pos_grid
        V.parse_precision(V.MODEL_PRECISION.get(name, V.DEFAULT_PRECISION))
    assert dataclasses.replace(V.CONFIGS["tiny_clip"], name="tiny_clip_q", quick_gelu=True) == V.CONFIGS["tiny_clip_q"]
    assert not V.CONFIGS["clip_b32"].quick_gelu and not V.VitConfig("x", 128, 1, 2, 256, 32, 224, 224, (7, 7)).quick_gelu
    assert dataclasses.replace(V.CONFIGS["clip_b32_openai"], name="clip_b32", quick_gelu=False) == V.CONFIGS["clip_b32"]
