"""-m gpu: `ibl_vit_forward` on trained-LIKE weight statistics (tests/vit_trained_cases.py: small LayerScale, heavy-tailed LayerNorm gains,
massive activations, peaked attention, heavy-tailed matrices, and all of them together) -- the numbers no precision plan was tuned on.

Stream families (dim 128, 3 blocks, 7 .. 20 tokens, batch 3), with the helpers and the bounds of tests/test_gpu_vit_stream.py, unchanged:
  * every all-token stage and every CLS-only stage from the device's own taps against fp64 (`block_checks`, `check32`, the 2 % cap),
    the class rows of a CLS-only block bit-identical to row 0 of the all-token run whose block is plain, the other rows untouched;
  * end to end: the device's embedding against oracle/vit_oracle.vit_forward in float64 is at most E2E_MARGIN times further off than
    the chained emulation of the same plan (tests/test_vit_trained_model.py measures the margin on the CPU).  No absolute gate.
Full size (`dinov2_vitb14`, `clip_b32_openai`, 12 blocks, batch 2 of u8-statistics crops): finite output, no fp16 tap at the clamp,
rel-L2 <= 1e-2 (ten times SURVEY 8d's gate: a broken forward, not a rounding budget); the class-row rel-L2 per (model, kind, plan) is
printed, and DESIGN (c) holds the table.  The 1e-3 gate is NOT asserted: whether it survives these statistics is what is measured.

MI355X figures (`test_zz_worst_ratios`, `test_zz_full_size_table`, run with -s).
Worst error / bound and worst share of fp16 elements not bit-equal to the emulation, per kind and stage ("cls_" = a CLS-only block):
    small_ls  qkv 0.874 / 0.50 %  att 0.513 / 0.04 %  ln2 0.989 / 0.11 %  hid 0.936 / 0.12 %  resid 0.227  patch 0.008  out_ln 0.083
              cls_ln1 0.993 / 0.04 %  cls_qkv 0.932 / 0.26 %  cls_att 0.437  cls_ln2 0.941 / 0.26 %  cls_hid 0.936 / 0.13 %  cls_resid 0.029
    ln_heavy  qkv 0.938 / 0.23 %  att 0.516 / 0.04 %  ln2 0.992 / 0.07 %  hid 0.925 / 0.06 %  resid 0.157  patch 0.027  out_ln 0.087
              cls_ln1 0.994 / 0.07 %  cls_qkv 0.957 / 0.26 %  cls_att 0.516  cls_ln2 0.992  cls_hid 0.925 / 0.13 %  cls_resid 0.113
    massive   qkv 0.786 / 1.01 %  att 0.541 / 0.05 %  ln2 0.995 / 0.07 %  hid 0.904 / 0.07 %  resid 0.248  patch 0.123  out_ln 0.079
              cls_ln1 0.996 / 0.11 %  cls_qkv 0.929 / 0.07 %  cls_att 0.477 / 0.26 %  cls_ln2 0.992 / 0.26 %  cls_hid 0.857 / 0.13 %  cls_resid 0.200
    peaked    qkv 0.910 / 0.86 %  att 0.638 / 0.07 %  ln2 0.972 / 0.07 %  hid 0.926 / 0.08 %  resid 0.037  patch 0.044  out_ln 0.089
              cls_ln1 0.994 / 0.07 %  cls_qkv 0.944 / 0.26 %  cls_att 0.460 / 0.26 %  cls_ln2 0.970 / 0.26 %  cls_hid 0.871 / 0.13 %  cls_resid 0.037
    heavy_w   qkv 0.928 / 0.61 %  att 0.482 / 0.08 %  ln2 0.987 / 0.05 %  hid 0.915 / 0.07 %  resid 0.055  patch 0.044  out_ln 0.095
              cls_ln1 0.995 / 0.04 %  cls_qkv 0.946 / 0.26 %  cls_att 0.415 / 0.52 %  cls_ln2 0.983 / 0.26 %  cls_hid 0.880 / 0.13 %  cls_resid 0.055
    all       qkv 0.872 / 0.88 %  att 0.535 / 0.07 %  ln2 0.995 / 0.07 %  hid 0.929 / 0.07 %  resid 0.274  patch 0.123  out_ln 0.069
              cls_ln1 0.995 / 0.07 %  cls_qkv 0.958 / 0.52 %  cls_att 0.485 / 0.26 %  cls_ln2 0.989 / 0.26 %  cls_hid 0.890 / 0.26 %  cls_resid 0.199
    (cls_out_ln <= 0.083, cls_proj_ln <= 0.993 / 0.26 %, cls_out_proj <= 0.034 in every kind.)
Every stage of every kind met its bound and the cap; the class rows of a CLS-only block are bit-identical to the all-token run in every
case.  One finding on the way: clip / heavy_w / p2;*:3333, CLS-only block 1 left 6.0 % of its 384 attention outputs unequal (0.28 of
the bound): one dominant softmax weight on an fp16 rounding boundary; `att_undetermined` of vit_stream_cases is the derivation for it
(0.52 % with it).
End to end, worst err_dev / err_emu per kind (margin 1.5): small_ls 1.027, ln_heavy 1.064, massive 1.010, peaked 1.048, heavy_w 1.016,
all 1.024: the device is as far from float64 as its rounding points put it, no further.  The largest err_dev is 2.98e-3 (clip, peaked,
plain; 3 blocks): the fp16 rounding of q and k under logits 11 wide, which no second weight term touches.
Full size, class-row rel-L2 mean / max over the 2 crops, default plan | p2;*:3333 (DESIGN (c) has the table with the reading):
    dinov2_vitb14    random 7.3e-4 / 7.6e-4 | 3.5e-4 / 3.5e-4   small_ls 7.3e-4 / 7.4e-4 | 3.9e-4 / 4.4e-4   ln_heavy 8.6e-4 / 8.9e-4 | 4.0e-4 / 4.6e-4
                     massive 2.7e-4 / 2.7e-4 | 9.8e-5 / 9.9e-5  peaked 1.09e-3 / 1.10e-3 | 7.6e-4 / 7.8e-4  heavy_w 7.0e-4 / 7.3e-4 | 3.4e-4 / 3.4e-4
                     all 2.3e-5 / 2.5e-5 | 9.5e-6 / 1.0e-5
    clip_b32_openai  random 7.1e-4 / 7.7e-4 | 4.2e-4 / 4.4e-4   ln_heavy 3.7e-4 / 4.1e-4 | 2.2e-4 / 2.5e-4   massive 5.4e-5 / 5.5e-5 | 1.7e-5 / 1.7e-5
                     peaked 1.27e-3 / 1.46e-3 | 8.9e-4 / 9.99e-4  heavy_w 7.4e-4 / 7.5e-4 | 4.0e-4 / 4.1e-4    all 6.4e-5 / 6.6e-5 | 1.7e-5 / 1.8e-5
No fp16 tap reached the clamp.  `peaked` misses SURVEY 8d's 1e-3 under both default plans and meets it under p2;*:3333 (clip with
0.1 % to spare); every other kind meets it under the default plan."""
import contextlib
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from ibloc_amd import _lib
from ibloc_amd import preprocess as pp
from ibloc_amd import vit as V
from oracle import vit_oracle as vo
from tests import siglip_cases as SC
from tests import test_gpu_vit_stream as TS
from tests import vit_stream_cases as SCS
from tests import vit_trained_cases as TC

pytestmark = pytest.mark.gpu
# (family, kind, plan): none and everything for every kind, all four plans of the stream tests for `all`
CASES = [(f, k, p) for f in SCS.FAMILIES for k in TC.kinds_of(f) for p in (SCS.PLANS if k == "all" else ("plain", "p2;*:3333"))]
CLS_CASES = [c for c in CASES if SCS.FAMILIES[c[0]].cls_token]
KIND_WORST = {}                # (kind, stage) -> [worst error / bound, worst unequal share]
E2E = {}                       # case -> (err_dev, err_emu)


def _id(c):
    return "-".join(c)


def cfg_of(case):
    """the configuration tuple of test_gpu_vit_stream's helpers, with the weights' kind as its fifth entry"""
    family, kind, plan = case
    return (family, plan, True, False, kind)


@contextlib.contextmanager
def noting(kind):
    """what check16 / check32 note in SCS.WORST inside the block goes to KIND_WORST[(kind, stage)] instead"""
    saved = {k: list(v) for k, v in SCS.WORST.items()}
    SCS.WORST.clear()
    try:
        yield
    finally:
        for stage, (ratio, share) in SCS.WORST.items():
            w = KIND_WORST.setdefault((kind, stage), [0.0, 0.0])
            w[0], w[1] = max(w[0], ratio), max(w[1], share)
        SCS.WORST.clear()
        SCS.WORST.update(saved)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_all_token_stages(case):
    """n_blocks_run = 0 .. 3, all tokens: patch, then qkv / att / ln2 / hid / resid of every block on every row; the final LayerNorm over
    every token at k = 3"""
    cfg = cfg_of(case)
    m = TS.model(cfg)
    with noting(case[1]):
        x0, _ = TS.x_after(cfg, 0)
        r, ok = SCS.check32("patch", x0, SCS.stage_patch(m))
        print(f"{_id(case)} patch: ratio {r:.3f}")
        assert ok
        for k in range(1, SCS.DEPTH + 1):
            x_prev, _ = TS.x_after(cfg, k - 1)
            _, taps = TS.x_after(cfg, k)
            TS._report(f"{_id(case)} block {k - 1}", SCS.block_checks(m, k - 1, x_prev, TS.dev_of(m, taps, k - 1, False)))
        out, taps = TS.run(cfg, SCS.DEPTH, True, final_ln=True)
        x3, _ = TS.x_after(cfg, SCS.DEPTH)
        assert np.array_equal(TS.flat(taps["x"], *x3.shape).view(np.uint32), x3.view(np.uint32)), "the same blocks, the same X"
        r, ok = SCS.check32("out_ln", out.reshape(x3.shape), SCS.stage_out_ln(m, x3))
        print(f"{_id(case)} out: ratio {r:.3f}")
        assert ok


@pytest.mark.parametrize("k", range(1, SCS.DEPTH + 1))
@pytest.mark.parametrize("case", CLS_CASES, ids=_id)
def test_cls_only_stages(case, k):
    """the class rows alone in block k - 1, as tests/test_gpu_vit_stream.py::test_cls_only_stages holds them: LN1 and K / V of every row,
    Q / ATT / FIN / HID / X of the class rows, the other rows of X untouched; the returned rows bit-identical to row 0 of an all-token
    run whose block k - 1 is plain; the outputs after the final LayerNorm and, for clip, the projection"""
    cfg = cfg_of(case)
    m = TS.model(cfg)
    T, D, B = m.T, m.D, SCS.BATCH
    with noting(case[1]):
        x_prev, _ = TS.x_after(cfg, k - 1)
        out, taps = TS.run(cfg, k, False)
        dev = TS.dev_of(m, taps, k - 1, True)
        TS._report(f"{_id(case)} cls block {k - 1}", SCS.block_checks(m, k - 1, x_prev, dev, cls_only=True))
        rest = np.ones(B * T, bool)
        rest[::T] = False
        assert np.array_equal(dev["x"][rest].view(np.uint32), x_prev[rest].view(np.uint32)), "a CLS-only block wrote rows other than the class rows"
        assert np.array_equal(out.view(np.uint32), dev["x"][::T].view(np.uint32)), "no final LN, no projection: the output is the class rows of X"
        full, _ = TS.run(cfg, k, True, plan=SCS.plan_without(cfg[1], k - 1))
        same = np.array_equal(full[:, 0].view(np.uint32), out.view(np.uint32))
        print(f"{_id(case)} cls block {k - 1}: rows bit-identical to the all-token run: {same}")
        assert same
        x_cls = np.ascontiguousarray(dev["x"][::T])
        out_ln, _ = TS.run(cfg, k, False, final_ln=True)
        r, ok = SCS.check32("cls_out_ln", out_ln, SCS.stage_out_ln(m, x_cls))
        print(f"{_id(case)} cls out_ln: ratio {r:.3f}")
        assert ok
        if m.cfg.proj_dim:
            out_p, taps_p = TS.run(cfg, k, False, final_ln=True, proj=True)
            ln, proj = SCS.stage_out_proj(m, x_cls)
            rows = taps_p["fin"].cpu().numpy() if ln["terms"] == 1 else TS.flat(taps_p["xn"], B, 3 * D)
            TS._report(f"{_id(case)} cls out", [("proj_ln",) + SCS.check16("cls_proj_ln", rows, ln, D)])
            r, ok = SCS.check32("cls_out_proj", out_p, proj(rows))
            print(f"{_id(case)} cls out_proj: ratio {r:.3f}")
            assert ok


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_end_to_end(case):
    """one forward of the family's own configuration (3 blocks, the last CLS-only where there is a class token, final LayerNorm,
    projection) against the float64 forward: at most E2E_MARGIN times the error of the chained emulation of the same plan"""
    family, kind, plan = case
    out, _ = TS.run(cfg_of(case), SCS.DEPTH, TC.all_tokens(family), final_ln=True, proj=True)
    assert np.isfinite(out).all()
    err_dev, err_emu = TC.rel_l2(out, TC.reference_out(family, kind)), TC.err_emu(family, kind, plan)
    E2E[case] = (err_dev, err_emu)
    print(f"{_id(case)}: err_dev {err_dev:.3e} err_emu {err_emu:.3e} ratio {err_dev / err_emu:.3f} (margin {TC.E2E_MARGIN})")
    assert err_dev <= TC.E2E_MARGIN * err_emu


def test_zz_worst_ratios():
    """prints, per kind and stage, the worst error / bound and the worst share of unequal fp16 elements, and the worst end-to-end ratio
    per kind (the figures of the module docstring)"""
    for kind in TC.KINDS:
        line = [f"{stage} {r:.3f}" + (f" / {s:.2%}" if s else "") for (k, stage), (r, s) in sorted(KIND_WORST.items()) if k == kind]
        print(f"{kind:>9}: " + "  ".join(line))
    for kind in TC.KINDS:
        rows = {c: d / e for c, (d, e) in E2E.items() if c[1] == kind}
        if rows:
            worst = max(rows, key=rows.get)
            print(f"{kind:>9}: worst err_dev / err_emu {rows[worst]:.3f} ({_id(worst)}), largest err_dev {max(E2E[c][0] for c in rows):.2e}")


# ---- full size -------------------------------------------------------------------------------------------------------------------------
FULL_MODELS = ("dinov2_vitb14", "clip_b32_openai")
FULL_WSEED, FULL_BATCH = 7501, 2
FULL_TABLE = {}                # (model, kind, plan) -> (mean, max) class-row rel-L2


def full_cfg(name):
    """the model's configuration with its position table stored at the run grid (dinov2: 16 x 16, not 37 x 37 resampled), so that a row
    of the table is a row of the run and `massive` lands in ONE patch row; the name, and with it the model's default plan, stays"""
    cfg = V.CONFIGS[name]
    return dataclasses.replace(cfg, pos_grid=cfg.grid)


@functools.lru_cache(maxsize=2)
def full_base(name):
    """-> (cfg, random weights, pixels (FULL_BATCH, 3, H, W) fp32: the synthetic u8 crops of the embedding gates, normalised by the
    model's recipe)"""
    cfg = full_cfg(name)
    rec = pp.recipe_for(cfg.recipe, cfg.img_h, cfg.img_w)
    u8 = SC.gate_crops_cpu(range(FULL_BATCH), hw=(cfg.img_h, cfg.img_w))
    px = ((u8.astype(np.float32) / np.float32(255.0) - np.asarray(rec.mean, np.float32)) / np.asarray(rec.std, np.float32))
    return cfg, V.random_weights(cfg, FULL_WSEED + FULL_MODELS.index(name)), np.ascontiguousarray(px.transpose(0, 3, 1, 2))


def full_kinds(name):
    return ("random",) + tuple(k for k in TC.KINDS if k != "small_ls" or V.CONFIGS[name].layerscale)


@pytest.mark.parametrize("name,kind", [(n, k) for n in FULL_MODELS for k in full_kinds(n)])
def test_full_size(name, kind):
    """12 blocks on the device under the model's default plan and p2;*:3333 against ONE float64 forward on the CPU"""
    cfg, w0, px = full_base(name)
    w = w0 if kind == "random" else TC.trained_like(cfg, w0, TC.SEED + 100 + FULL_MODELS.index(name), kind)
    ref = vo.vit_forward(w, cfg, px, dtype=torch.float64)
    for plan in (V.MODEL_PRECISION.get(name, V.DEFAULT_PRECISION), "p2;*:3333"):
        enc = V.VitEncoder(cfg, w, precision=plan, fold_layerscale=False, resid_kext=True)
        # the taps are views of the whole workspace, at the widest shape: what this forward does not write must not read as a finding
        enc._ws.get(0, _lib.lib.ibl_vit_workspace_bytes(C.byref(enc.desc), FULL_BATCH)).zero_()
        out, taps = enc.forward_patches(enc.patches_from_pixels(torch.from_numpy(px)), taps=True)
        torch.cuda.synchronize()
        out = out.cpu().numpy().astype(np.float64)
        assert np.isfinite(out).all(), (name, kind, plan)
        for tap in ("xn", "qkv", "att", "hid", "fin"):
            t = taps[tap].float()
            assert bool(torch.isfinite(t).all()) and not bool((t.abs() == 65504.0).any()), f"{name} {kind} {plan}: {tap} reached the fp16 clamp"
        rel = np.linalg.norm(out - ref, axis=1) / np.linalg.norm(ref, axis=1)
        FULL_TABLE[(name, kind, plan)] = (float(rel.mean()), float(rel.max()))
        print(f"{name} {kind} {plan}: class-row rel-L2 mean {rel.mean():.3e} max {rel.max():.3e}")
        assert rel.max() <= 1e-2, (name, kind, plan, rel)
        del enc, taps


def test_zz_full_size_table():
    """prints the table of DESIGN (c): class-row rel-L2 mean / max per (model, kind, plan)"""
    for (name, kind, plan), (mean, mx) in FULL_TABLE.items():
        print(f"{name:>16} {kind:>9} {plan:<28} mean {mean:.2e}  max {mx:.2e}  {'meets' if mx <= 1e-3 else 'misses'} 1e-3")
