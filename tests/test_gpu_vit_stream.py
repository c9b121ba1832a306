"""-m gpu: every stage of `ibl_vit_forward` against fp64, per family, plan and block, each stage from the DEVICE's own input to it -- the
workspace taps of `VitEncoder.forward_patches(taps=True)` (include/ibloc.h, IBL_VIT_WS_*) and the X of a run with one block less.  Cases,
references, bounds and the 2 % cap on fp16 elements that are not bit-equal to the emulation: tests/vit_stream_cases.py;
tests/test_vit_stream_model.py shows on the CPU that they refuse a chain with one operand term lost, swapped or misplaced.

Worst error / bound and worst share of fp16 elements not bit-equal to the emulation per stage, over the whole file, on an MI355X
(`test_zz_worst_ratios`, run with -s; "cls_" = the stages of a CLS-only block):
    patch 0.044            qkv 0.930 / 1.74 %     att 0.564 / 0.07 %     ln2 0.988 / 0.11 %     hid 0.908 / 0.09 %     resid 0.073
    out_ln 0.095           cls_ln1 0.995 / 0.04 % cls_qkv 0.934 / 0.26 % cls_att 0.564 / 0.26 % cls_ln2 0.977 / 0.52 % cls_hid 0.889 / 0.13 %
    cls_resid 0.044        cls_out_ln 0.070       cls_proj_ln 0.991 / 0 % cls_out_proj 0.021
The class rows of a CLS-only block are bit-identical to row 0 of an all-token run whose block is plain, in every family, plan and
block: the comment in ibl_vit_forward holds.  (att: 0.35 % before `att_undetermined` of vit_stream_cases took the outputs that one
softmax weight on an fp16 rounding boundary decides out of the share.)  Every stage of every plan met its bound and the cap: no operand
term is dead.
qkv is the one stage whose share is not a few tenths of a percent (dino, default plan, block 1: 1.74 %; dino plain, block 2: 1.34 %;
every other case under 0.8 %), and the cause is known: its operand, LayerNorm 1, is not kept by the device and is emulated here, so where
the device's LayerNorm (v_rsq_f32, the compiler's choice of fused multiply-adds) rounds ONE element of a one-term row to the other fp16
neighbour, all 384 outputs of that row move by up to an fp16 step of one product and about a tenth of them round differently: one such
element among dino's 21 rows is 0.5 % of the buffer.  `flip_allowance` of vit_stream_cases covers it in the bound; a three-term row
absorbs it in a_lo (0.1 %)."""
import functools

import numpy as np
import pytest
import torch

from ibloc_amd import vit as V
from tests import vit_stream_cases as SCS

pytestmark = pytest.mark.gpu
CONFIGS = [(f, p, True, False) for f in SCS.FAMILIES for p in SCS.PLANS] + SCS.EXTRA
CLS_CONFIGS = [c for c in CONFIGS if SCS.FAMILIES[c[0]].cls_token]


def _id(c):
    f, p, kext, fold = c
    return f"{f}-{p}" + ("" if kext else "-kext0") + ("-fold" if fold else "")


@functools.lru_cache(maxsize=None)
def model(cfg):
    return SCS.Model(*cfg)


def run(cfg, n_run, all_tokens, final_ln=False, proj=False, plan=None):
    """one forward -> (encoder's model, out numpy, taps as torch views)"""
    family, plan0, kext, fold = cfg[:4]       # (a fifth entry is the weights' kind: tests/test_gpu_vit_trained.py)
    m = model(cfg)
    c = SCS.run_cfg(family, n_run, all_tokens, final_ln=final_ln, proj=proj)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("IBL_VIT_RESID_KEXT", "1" if kext else "0")
        enc = V.VitEncoder(c, m.w, precision=plan or plan0, fold_layerscale=fold)
    out, taps = enc.forward_patches(torch.from_numpy(m.patches).cuda(), taps=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), {k: v.clone() for k, v in taps.items()}


def flat(t, rows, width):
    return t.reshape(-1)[:rows * width].reshape(rows, width).cpu().numpy()


def dev_of(m, taps, l, cls_only):
    """the taps as the numpy arrays of vit_stream_cases.block_checks, shaped by the terms block l ran with"""
    R = SCS.BATCH * m.T
    _, ot, ft, f2t = m.terms(l, cls_only)
    d = dict(x=flat(taps["x"], R, m.D), qkv=taps["qkv"].cpu().numpy(), fin=taps["fin"].cpu().numpy())
    if cls_only:
        d.update(xn=flat(taps["xn"], R, m.D), att=flat(taps["att"], R, m.D), hid=flat(taps["hid"], SCS.BATCH, m.MLP))
    else:
        d.update(xn=flat(taps["xn"], R, ft * m.D), att=flat(taps["att"], R, ot * m.D), hid=flat(taps["hid"], R, f2t * m.MLP))
    return d


@functools.lru_cache(maxsize=None)
def x_after(cfg, k):
    """X after k blocks of an all-token run without the final LayerNorm, (rows, D) fp32: x_k, every later stage's input"""
    out, taps = run(cfg, k, True)
    x = flat(taps["x"], SCS.BATCH * model(cfg).T, model(cfg).D)
    assert np.array_equal(out.reshape(x.shape).view(np.uint32), x.view(np.uint32)), "all tokens, no final LN: the output is X"
    return x, taps


def _report(tag, res):
    bad = []
    for stage, ratio, share, ok in res:
        print(f"{tag} {stage}: ratio {ratio:.3f}" + ("" if share is None else f" unequal {share:.4%}"))
        if not ok:
            bad.append((stage, ratio, share))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_all_token_stages(cfg):
    """n_blocks_run = 0 .. 3, all tokens: patch, then qkv / att / ln2 / hid / resid of every block on every row; the final LayerNorm over
    every token at k = 3"""
    m = model(cfg)
    x0, _ = x_after(cfg, 0)
    r, ok = SCS.check32("patch", x0, SCS.stage_patch(m))
    print(f"{_id(cfg)} patch: ratio {r:.3f}")
    assert ok
    for k in range(1, SCS.DEPTH + 1):
        x_prev, _ = x_after(cfg, k - 1)
        _, taps = x_after(cfg, k)
        _report(f"{_id(cfg)} block {k - 1}", SCS.block_checks(m, k - 1, x_prev, dev_of(m, taps, k - 1, False)))
    out, taps = run(cfg, SCS.DEPTH, True, final_ln=True)
    x3, _ = x_after(cfg, SCS.DEPTH)
    assert np.array_equal(flat(taps["x"], *x3.shape).view(np.uint32), x3.view(np.uint32)), "the same blocks, the same X"
    r, ok = SCS.check32("out_ln", out.reshape(x3.shape), SCS.stage_out_ln(m, x3))
    print(f"{_id(cfg)} out: ratio {r:.3f}")
    assert ok


@pytest.mark.parametrize("k", range(1, SCS.DEPTH + 1))
@pytest.mark.parametrize("cfg", CLS_CONFIGS, ids=_id)
def test_cls_only_stages(cfg, k):
    """the class rows alone in block k - 1: LN1 and K / V of every row, Q / ATT / FIN / HID / X of the class rows, the other rows of X
    untouched; the returned rows against row 0 of an all-token run whose block k - 1 is plain; the outputs after the final LayerNorm
    and, for clip, the projection"""
    m = model(cfg)
    T, D, B = m.T, m.D, SCS.BATCH
    x_prev, _ = x_after(cfg, k - 1)
    out, taps = run(cfg, k, False)
    dev = dev_of(m, taps, k - 1, True)
    _report(f"{_id(cfg)} cls block {k - 1}", SCS.block_checks(m, k - 1, x_prev, dev, cls_only=True))
    rest = np.ones(B * T, bool)
    rest[::T] = False
    assert np.array_equal(dev["x"][rest].view(np.uint32), x_prev[rest].view(np.uint32)), "a CLS-only block wrote rows other than the class rows"
    assert np.array_equal(out.view(np.uint32), dev["x"][::T].view(np.uint32)), "no final LN, no projection: the output is the class rows of X"
    # "every row of a GEMM is computed independently, so the CLS rows come out bit-identical" (ibl_vit_forward)
    full, _ = run(cfg, k, True, plan=SCS.plan_without(cfg[1], k - 1))
    same = np.array_equal(full[:, 0].view(np.uint32), out.view(np.uint32))
    print(f"{_id(cfg)} cls block {k - 1}: rows bit-identical to the all-token run: {same}")
    assert same
    # final LayerNorm of the class rows
    x_cls = np.ascontiguousarray(dev["x"][::T])
    out_ln, _ = run(cfg, k, False, final_ln=True)
    r, ok = SCS.check32("cls_out_ln", out_ln, SCS.stage_out_ln(m, x_cls))
    print(f"{_id(cfg)} cls out_ln: ratio {r:.3f}")
    assert ok
    if m.cfg.proj_dim:
        out_p, taps_p = run(cfg, k, False, final_ln=True, proj=True)
        ln, proj = SCS.stage_out_proj(m, x_cls)
        rows = taps_p["fin"].cpu().numpy() if ln["terms"] == 1 else flat(taps_p["xn"], B, 3 * D)
        _report(f"{_id(cfg)} cls out", [("proj_ln",) + SCS.check16("cls_proj_ln", rows, ln, D)])
        r, ok = SCS.check32("cls_out_proj", out_p, proj(rows))
        print(f"{_id(cfg)} cls out_proj: ratio {r:.3f}")
        assert ok


def test_zz_worst_ratios():
    """prints, over the whole file, the worst error / bound and the worst share of unequal fp16 elements per stage (the figures of the
    module docstring)"""
    for stage, (ratio, share) in sorted(SCS.WORST.items()):
        print(f"{stage:>14}: error / bound {ratio:.3f}, unequal {share:.4%}")
