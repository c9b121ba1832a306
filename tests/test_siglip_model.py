"""CPU: what the SigLIP GPU tests rest on -- C_TGELU and LIP_T of tests/siglip_cases.py are what their rules give, the emulated `tanh_gelu2`
behaves at the extremes as csrc/vit_gemm.hip says, the erf form breaks the tanh bound, the folded pooling head is the unfolded one, the seeded
head pools non-uniformly, the configurations are the checkpoints', and the new entries refuse bad arguments before they touch the device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import gemm_cases as GC
from tests import siglip_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_tgelu_is_the_smallest_power_of_two_under_three_quarters():
    """the emulated tanh_gelu2 (its fp32 value) against the exact tanh GELU over the grid: never NaN, within 0.75 C_TGELU max(|v|, TINY)"""
    v = SC.tgelu_grid()
    value = SC.emulate_tgelu(v)
    assert not np.isnan(value).any()
    ratios = {}
    for e in range(-26, -19):
        ratios[e], at, two = SC.tgelu_model_ratio(2.0 ** e)
        print(f"tanh_gelu2 emulation vs fp64: C_TGELU 2^{e}: worst error / (C_TGELU |v|) {ratios[e]:.3f} at v = {at:.6g}; h + lo / 64 "
              f"against its whole bound {two:.3f}")
        assert two <= 1.0 or e < round(math.log2(SC.C_TGELU))
    chosen = int(round(math.log2(SC.C_TGELU)))
    assert 2.0 ** chosen == SC.C_TGELU
    assert ratios[chosen] <= 0.75 < ratios[chosen - 1], (chosen, ratios)
    v64 = torch.from_numpy(v.astype(np.float64))
    ref, bnd = SC.expected(v64, torch.zeros_like(v64), 64)
    r = float(((torch.from_numpy(GC.h16(value).astype(np.float64)) - ref).abs() / bnd).max())
    print(f"tanh_gelu2 emulation, fp16 result: worst error / bound {r:.3f}")
    assert r <= 1.0


def test_lip_t_bounds_the_derivative():
    """g'(v) = 0.5 (1 + tanh z) + 0.5 v (1 - tanh^2 z) z'(v): its largest magnitude on a grid in fp64, 1.12899 at v = 1.42, rounded up to
    two decimals is LIP_T"""
    v = np.linspace(-60.0, 60.0, 2_400_001)
    th = np.tanh(SC.SQRT_2_PI * (v + 0.044715 * v ** 3))
    d = np.abs(0.5 * (1.0 + th) + 0.5 * v * (1.0 - th * th) * SC.SQRT_2_PI * (1.0 + 3 * 0.044715 * v * v))
    print(f"max |g'| = {d.max():.5f} at v = {v[d.argmax()]:.3f}")
    assert SC.LIP_T == math.ceil(d.max() * 100.0) / 100.0 == 1.13


def test_emulated_tgelu_extremes():
    f = np.float32
    v = np.array([0.0, -0.0, 1e-30, 200.0, 65504.0, 3.0e6, -200.0, -65504.0, -3.0e38, 3.0e38, -10.0, -10.25, 1.9e19, -1.9e19], f)
    g = SC.emulate_tgelu(v)
    assert not np.isnan(g).any()
    assert g[0] == 0.0 and g[1] == 0.0 and g[2] == f(1e-30) * f(0.5)
    assert g[3] == 200.0 and g[4] == 65504.0 and g[5] == f(3.0e6) and g[9] == f(3.0e38) and g[12] == f(1.9e19)   # v >> 0: v itself
    for i in (6, 7, 8, 11, 13):                                                    # v << 0: exp2 overflows, rcp(inf) = 0, -0 (v^2 = inf too)
        assert g[i] == 0.0 and np.signbit(g[i])
    assert g[10] < 0.0 and abs(g[10]) < 2.0 ** -100                                # just before the overflow (v = -10.07): tiny, finite
    assert (GC.h16(g[6:9]) == 0.0).all() and GC.h16(g[5]) == 65504.0
    r = SC.tgelu64(torch.tensor([-1.0e6, -800.0, 0.0, 800.0, 1.0e6], dtype=torch.float64))
    assert bool(torch.isfinite(r).all()) and r[0] == 0.0 and r[2] == 0.0 and r[3] == 800.0 and r[4] == 1.0e6
    x = torch.linspace(-8.0, 8.0, 6001, dtype=torch.float64)
    assert float((SC.tgelu64(x) - torch.nn.functional.gelu(x, approximate="tanh")).abs().max()) <= 1e-14


def test_the_erf_form_breaks_the_tanh_bound():
    """the two forms are up to 4.7e-4 apart (at v = -2.70): the exact erf GELU, rounded to fp16 like the kernel's result, lies outside
    the bound of the tanh epilogue somewhere on the grid -- the bound can see a wrong activation"""
    v64 = torch.from_numpy(SC.tgelu_grid().astype(np.float64))
    gap = (GC.gelu64(v64) - SC.tgelu64(v64)).abs()
    print(f"max |erf form - tanh form| = {float(gap.max()):.3e} at v = {float(v64[gap.argmax()]):.3f}")
    assert 4.6e-4 < float(gap.max()) < 4.8e-4
    ref, bnd = SC.expected(v64, torch.zeros_like(v64), 64)
    erf16 = torch.from_numpy(GC.h16(GC.gelu64(v64).numpy().astype(np.float32)).astype(np.float64))
    r = (erf16 - ref).abs() / bnd
    print(f"erf form against the tanh bound: worst error / bound {float(r.max()):.1f}")
    assert float(r.max()) > 2.0


def test_folded_head_is_the_unfolded_head_in_float64():
    """one constant query per head: scores through u_h and the value projection after the pooling give nn.MultiheadAttention's result.
    Measured: relative L2 difference of the head output 1.3e-15 (tiny_siglip) / 1.1e-15 (siglip_b16_224), both sides float64; asserted
    with one order of margin"""
    from ibloc_amd import siglip as S
    from ibloc_amd import vit as V
    for name in ("tiny_siglip", "siglip_b16_224"):
        cfg = V.CONFIGS[name]
        hw = S.random_head_weights(cfg, 5)
        tok = torch.from_numpy(np.random.default_rng(6).standard_normal((3, cfg.n_tokens, cfg.dim)))
        a, p = SC.head_unfolded(hw, cfg, tok, want_probs=True)
        u = S.fold_head(hw, cfg.heads, np.float64)
        b = SC.head_folded(hw, cfg, u, tok)
        d = float((a - b).norm() / a.norm())
        p2, _ = SC.stage_pool(tok, torch.from_numpy(u))
        print(f"{name}: folded vs unfolded head, float64: rel-L2 {d:.2e}, probabilities max abs {float((p - p2).abs().max()):.2e}")
        assert d <= 1.3e-14 and float((p - p2).abs().max()) <= 1e-13
        assert S.fold_head(hw, cfg.heads).dtype == np.float32 and S.fold_head(hw, cfg.heads).shape == (cfg.heads, cfg.dim)
    with pytest.raises(ValueError):
        S.fold_head(hw, 7)


def test_the_seeded_head_pools_non_uniformly():
    """a condition on the inputs: over crops like the gate's (tests/siglip_cases.gate_crops_cpu) the mean over crops and heads of
    max_t p is at least 4 / T on the fp32 restatement of tiny_siglip -- a uniform pooling would hide a wrong softmax"""
    from ibloc_amd import siglip as S
    from ibloc_amd import vit as V
    cfg = V.CONFIGS["tiny_siglip"]
    w = V.random_weights(cfg, SC.GATE_WEIGHT_SEED)
    hw = S.random_head_weights(cfg, SC.GATE_HEAD_SEED)
    crops = SC.gate_crops_cpu(np.random.default_rng(3).integers(0, 100000, size=8))
    x = ((crops.astype(np.float32) / 255.0 - 0.5) / 0.5).transpose(0, 3, 1, 2)
    _, p = SC.head_unfolded(hw, cfg, SC.trunk_tokens(w, cfg, x), want_probs=True)
    m = float(p.max(-1).values.mean())
    print(f"tiny_siglip: mean max_t p = {m:.3f} = {m * cfg.n_tokens:.1f} / T")
    assert m >= 4.0 / cfg.n_tokens
    assert set(hw) == set(S.HEAD_KEYS)


def test_configurations():
    import dataclasses
    from ibloc_amd import preprocess as pp
    from ibloc_amd import vit as V
    want = {"siglip_b16_224": (768, 12, 12, 3072, 224, 196), "siglip_b16_256": (768, 12, 12, 3072, 256, 256),
            "siglip_b16_384": (768, 12, 12, 3072, 384, 576), "siglip_l16_256": (1024, 24, 16, 4096, 256, 256),
            "siglip_l16_384": (1024, 24, 16, 4096, 384, 576), "tiny_siglip": (128, 2, 2, 256, 224, 196),
            "tiny_siglip_384": (128, 2, 2, 256, 384, 576)}
    for name, (dim, depth, heads, mlp, px, tokens) in want.items():
        c = V.CONFIGS[name]
        assert (c.name, c.dim, c.depth, c.heads, c.mlp_dim, c.patch, c.img_h, c.img_w, c.n_tokens, c.n_patches) == \
            (name, dim, depth, heads, mlp, 16, px, px, tokens, tokens)
        assert c.out_all_tokens and c.final_ln and c.ln_eps == 1e-6 and c.recipe == "siglip" and c.tanh_gelu and not c.cls_token
        assert not c.quick_gelu and not c.layerscale and not c.pre_ln and not c.proj_dim and c.n_blocks_run == -1
        assert c.dim == 64 * c.heads and c.depth <= V.MAX_LAYERS and c.dim <= 1024 and c.grid == c.pos_grid
        assert (c.n_tokens > 272) == (px == 384)                      # 196 / 256: the resident attention kernel, 576: the streaming one
        r = pp.recipe_for(c.recipe, c.img_h, c.img_w)
        assert (r.out_h, r.out_w, r.resize_mode, r.filt, r.mean, r.std) == (px, px, "exact", pp.BICUBIC, (0.5,) * 3, (0.5,) * 3)
        V.parse_precision(V.MODEL_PRECISION.get(name, V.DEFAULT_PRECISION))
        assert V.random_weights(c, 1)["pos"].shape == (tokens, dim)
    # the class-token configurations are what they were
    d = V.CONFIGS["tiny_dino"]
    assert d.cls_token and not d.tanh_gelu and d.n_tokens == 257 and d.n_patches == 256
    assert V.VitConfig("x", 128, 1, 2, 256, 32, 224, 224, (7, 7)).n_tokens == 50
    assert dataclasses.replace(V.CONFIGS["tiny_siglip"], name="tiny_siglip_384", img_h=384, img_w=384, pos_grid=(24, 24)) == V.CONFIGS["tiny_siglip_384"]
    assert pp.recipe_for("dinov2", 224, 224) is pp.RECIPES["dinov2"] and pp.recipe_for("siglip", 224, 224) is pp.RECIPES["siglip"]


def test_struct_sizes_match_the_header(tmp_path):
    from ibloc_amd import siglip as S
    pairs = [("ibl_probe_head_desc", S.ProbeHeadDesc), ("ibl_probe_head_weights", S.ProbeHeadWeights)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ibloc.h"', 'int main(void) {']
    for cname, ct in pairs:
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {fname}));')
        lines.append('  printf("\\n");')
    lines += ['  printf("%d %d %d %d\\n", IBL_VIT_NO_CLS, IBL_VIT_TANH_GELU, IBL_ACT_GELU_TANH, IBL_PROBE_WS_COUNT);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for (cname, ct), line in zip(pairs, out):
        parts = line.split()
        assert parts[0] == cname and int(parts[1]) == C.sizeof(ct)
        for (fname, _), off in zip(ct._fields_, parts[2:]):
            assert int(off) == getattr(ct, fname).offset, (cname, fname)
    from ibloc_amd import vit as V
    assert [int(t) for t in out[2].split()] == [V.FLAG_NO_CLS, V.FLAG_TANH_GELU, V.ACT_GELU_TANH, len(S.HEAD_TAPS)] == [256, 512, 2, 6]
    assert SC.ACT_TANH == V.ACT_GELU_TANH


# ---- refusals: the pointers are never followed, these run without a GPU ----------------------------------------------------------------------
P = 0x10000


def _refused(st, word=None, code=None):
    from ibloc_amd import _lib
    msg = _lib.lib.ibl_last_error()
    assert st < 0 and msg, (st, msg)
    if code is not None:
        assert st == code, (st, msg)
    if word is not None:
        assert word in msg, msg


def test_forward_refuses_the_flag_combinations_before_touching_the_device():
    from ibloc_amd import _lib, vit as V
    cfg = V.CONFIGS["tiny_siglip"]
    W = V.VitWeights()

    def call(flags):
        d = V.VitDesc(cfg.dim, cfg.depth, cfg.heads, cfg.mlp_dim, cfg.patch, cfg.img_h, cfg.img_w, cfg.n_tokens, cfg.patch_k_pad, flags,
                      cfg.depth, cfg.dim, cfg.ln_eps)
        return _lib.lib.ibl_vit_forward(C.byref(d), C.byref(W), P, 1, P, P, 1 << 40, None)

    _refused(call(V.FLAG_NO_CLS | V.FLAG_FINAL_LN), b"IBL_VIT_OUT_ALL_TOKENS", code=-4)
    _refused(call(V.FLAG_NO_CLS | V.FLAG_TANH_GELU), b"IBL_VIT_OUT_ALL_TOKENS", code=-4)
    _refused(call(V.FLAG_OUT_ALL_TOKENS | V.FLAG_QUICK_GELU | V.FLAG_TANH_GELU), b"both")
    _refused(call(V.FLAG_NO_CLS | V.FLAG_OUT_ALL_TOKENS | V.FLAG_QUICK_GELU | V.FLAG_TANH_GELU), b"both")


def test_linear_act_refuses_bad_activations_before_touching_the_device():
    from ibloc_amd import _lib, vit as V

    def call(act, **kw):
        f = dict(x=P, ldx=64, W=P, ldw=64, bias=None, scale=None, pos=P, out=P, ldo=384, rows=16, n_out=128, n_in=64, epilogue=1,
                 accumulate=0, tokens_per_crop=17, patches_per_crop=16, alpha=1.0, activation=0)
        f.update(kw)
        d = V.LinearDesc(**f)
        return _lib.lib.ibl_linear_f16_act(C.byref(d), act, None)

    for epi in (1, 6, 7):
        for act in (3, -1, 1 << 30, -(1 << 31)):
            _refused(call(act, epilogue=epi), b"activation")
        for act in (0, 1, 2):
            for field in (1, 2, -1):
                _refused(call(act, epilogue=epi, activation=field), b"activation")
            assert call(act, epilogue=epi, rows=0) == 0
    for epi in (0, 2, 3, 4, 5):
        for act in (1, 2):
            _refused(call(act, epilogue=epi), b"activation")
        _refused(call(3, epilogue=epi))
        _refused(call(-1, epilogue=epi))
    _refused(call(2, epilogue=8))
    _refused(call(2, epilogue=11))
    _refused(call(0, epilogue=-1))
    _refused(_lib.lib.ibl_linear_f16_act(None, 2, None), b"null")
    # everything ibl_linear_f16_ex refuses: a null operand, a short stride, n_out % 128
    _refused(call(2, x=None), b"null")
    _refused(call(2, ldo=64))
    _refused(call(2, n_out=64))
    # and ibl_linear_f16_ex keeps refusing the new value
    d = V.LinearDesc(x=P, ldx=64, W=P, ldw=64, out=P, ldo=384, rows=16, n_out=128, n_in=64, epilogue=1, alpha=1.0, activation=2)
    _refused(_lib.lib.ibl_linear_f16_ex(C.byref(d), None), b"activation")


def test_head_entries_refuse_bad_arguments_before_touching_the_device():
    from ibloc_amd import _lib, siglip as S
    lib = _lib.lib

    def pool(x=P, batch=2, n_tokens=196, dim=128, heads=2, u=P, pooled=P, probs=P):
        return lib.ibl_probe_pool_f32(x, batch, n_tokens, dim, heads, u, pooled, probs, None)

    for kw in (dict(x=None), dict(u=None), dict(pooled=None)):
        _refused(pool(**kw), b"null")
    for kw in (dict(batch=0), dict(batch=-3), dict(n_tokens=0), dict(n_tokens=-1), dict(dim=130), dict(dim=126), dict(dim=0), dict(heads=0),
               dict(heads=3), dict(dim=132, heads=8), dict(x=P + 4), dict(pooled=P + 8), dict(u=P + 4)):
        _refused(pool(**kw))
    _refused(pool(heads=32, dim=1024), code=-4)
    _refused(pool(dim=2048, heads=16), code=-4)
    _refused(pool(n_tokens=4000, dim=1024, heads=16), b"LDS", code=-4)

    W = S.ProbeHeadWeights(*([P] * 11))

    def head(desc=None, w=W, tokens=P, batch=2, out=P, ws=P, ws_bytes=1 << 40, **kw):
        f = dict(dim=128, heads=2, mlp_dim=256, n_tokens=196, ln_eps=1e-6)
        f.update(kw)
        d = S.ProbeHeadDesc(**f)
        return d, lib.ibl_probe_head_forward(C.byref(d) if desc is None else desc, C.byref(w) if w is not None else None, tokens, batch,
                                             out, ws, ws_bytes, None)

    for kw in (dict(w=None), dict(tokens=None), dict(out=None), dict(ws=None)):
        _refused(head(**kw)[1], b"null")
    _refused(lib.ibl_probe_head_forward(None, C.byref(W), P, 2, P, P, 1 << 40, None), b"null")
    for kw in (dict(batch=0), dict(n_tokens=0), dict(dim=130), dict(dim=126, heads=2), dict(heads=3), dict(mlp_dim=0), dict(tokens=P + 4)):
        _refused(head(**kw)[1])
    W2 = S.ProbeHeadWeights(*([P] * 11))
    W2.w_fc2 = None
    _refused(head(w=W2)[1], b"null weight")
    d = S.ProbeHeadDesc(128, 2, 256, 196, 1e-6)
    need = lib.ibl_probe_head_workspace_bytes(C.byref(d), 2)
    assert need > 0
    for n in (0, 1000, need - 257, -5):
        _refused(head(ws_bytes=n)[1], b"workspace")
    # the layout: six buffers on 256-byte boundaries, in order, inside the size the query reports
    offs = (C.c_int64 * 6)()
    assert lib.ibl_probe_head_workspace_layout(C.byref(d), 2, offs, 6) == 0
    sizes = [2 * 2 * 196, 2 * 2 * 128, 2 * 128, 2 * 128, 2 * 128, 2 * 256]
    assert offs[0] == 0 and all(o % 256 == 0 for o in offs)
    for i in range(5):
        assert offs[i + 1] >= offs[i] + 4 * sizes[i] and offs[i + 1] - (offs[i] + 4 * sizes[i]) < 256
    assert offs[5] + 4 * sizes[5] + 256 == need
    _refused(lib.ibl_probe_head_workspace_layout(C.byref(d), 2, offs, 7))
    _refused(lib.ibl_probe_head_workspace_layout(C.byref(d), 0, offs, 6))
    _refused(lib.ibl_probe_head_workspace_layout(C.byref(d), 2, None, 6))
    assert lib.ibl_probe_head_workspace_bytes(None, 2) == -1 and lib.ibl_probe_head_workspace_bytes(C.byref(d), 0) == -1


def test_encoder_classes_refuse_the_wrong_configuration_on_the_host(monkeypatch):
    from ibloc_amd import siglip as S
    from ibloc_amd import vit as V
    import dataclasses
    cfg = V.CONFIGS["tiny_siglip"]
    w = V.random_weights(cfg, 1)
    with pytest.raises(ValueError):
        S.SiglipEncoder(V.CONFIGS["tiny_dino"], w, S.random_head_weights(cfg, 1), device="cpu")
    # resampling a SigLIP position table is out of scope: a pos_grid that differs from the run grid raises (before any upload)
    bad = dataclasses.replace(cfg, img_h=256, img_w=256)
    with pytest.raises(ValueError):
        V.VitEncoder(bad, w, device="cpu")
    with pytest.raises(ValueError):
        V.VitEncoder(dataclasses.replace(cfg, out_all_tokens=False), w, device="cpu")
    with pytest.raises(ValueError):
        V.VitEncoder(dataclasses.replace(cfg, quick_gelu=True), w, device="cpu")
