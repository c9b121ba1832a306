"""CPU: the cases of tests/vit_stream_cases.py can tell a correct chain of the ViT forward from a mutated one, with the references alone.

For every family x plan x block x stage a stand-in for the device -- the same rounding points, accumulated in fp32 in numpy's order, each
stage fed the stand-in's own previous one -- stays inside the 2 % cap and the bound; with a mutant made the reference, the same stand-in
leaves at least one of them at the stages the mutant applies to.  Also: the workspace layout call (no device), and the term restatement
of vit_stream_cases against ibloc_amd.vit's."""
import ctypes as C
import functools

import numpy as np
import pytest

from ibloc_amd import _lib
from ibloc_amd import vit as V
from tests import vit_stream_cases as SCS

CONFIGS = [(f, p, True, False) for f in SCS.FAMILIES for p in SCS.PLANS] + SCS.EXTRA


def _id(c):
    f, p, kext, fold = c
    return f"{f}-{p}" + ("" if kext else "-kext0") + ("-fold" if fold else "")


@functools.lru_cache(maxsize=None)
def chain(cfg):
    """-> (model, x_0, [all-token stand-in of block l], [CLS-only stand-in of block l from the all-token x_{l-1}])"""
    m = SCS.Model(*cfg)
    x0 = SCS.stage_patch(m, np.float32)["emu"]
    xs, full, cls = [x0], [], []
    for l in range(SCS.DEPTH):
        full.append(SCS.stand_in(m, l, xs[-1]))
        if m.cfg.cls_token:
            cls.append(SCS.stand_in(m, l, xs[-1], cls_only=True))
        xs.append(full[-1]["x"])
    return m, xs, full, cls


@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_fp32_stand_in_stays_inside_cap_and_bound(cfg):
    m, xs, full, cls = chain(cfg)
    r, ok = SCS.check32("patch", xs[0], SCS.stage_patch(m))
    assert ok, f"patch: {r:.3f}"
    for l in range(SCS.DEPTH):
        for cls_only, dev in ((False, full[l]),) + (((True, cls[l]),) if cls else ()):
            for stage, ratio, share, ok in SCS.block_checks(m, l, xs[l], dev, cls_only=cls_only):
                print(f"{_id(cfg)} block {l} {'cls ' if cls_only else ''}{stage}: ratio {ratio:.3f}" + ("" if share is None else f" unequal {share:.4%}"))
                assert ok, (l, cls_only, stage, ratio, share)
    x_cls = np.ascontiguousarray(xs[-1][::m.T])
    if m.cfg.proj_dim:
        ln, proj = SCS.stage_out_proj(m, x_cls)
        assert SCS.check16("out_ln", ln["emu"], ln, m.D)[2]
        assert SCS.check32("out_proj", proj(ln["emu"])["emu"].astype(np.float32), proj(ln["emu"]))[1]
        got = SCS.stage_out_proj(m, x_cls, np.float32)[1](ln["emu"])["emu"]
        assert SCS.check32("out_proj", got, proj(ln["emu"]))[1]
    st = SCS.stage_out_ln(m, xs[-1])
    assert SCS.check32("out_ln32", st["emu"], st)[1]


def _mutant_cases():
    out = []
    for cfg in CONFIGS:
        m = SCS.Model(*cfg)
        for mutant in SCS.MUTANTS:
            if SCS.applies(mutant, m, "patch"):
                out.append((cfg, mutant, "patch", 0, False))
            if SCS.applies(mutant, m, "proj") and m.cfg.proj_dim:
                out.append((cfg, mutant, "proj", 0, False))
            for l in range(SCS.DEPTH):
                for cls_only in (False, True) if m.cfg.cls_token else (False,):
                    for stage in ("qkv", "att", "ln2", "hid", "resid"):
                        if SCS.applies(mutant, m, stage, l, cls_only):
                            out.append((cfg, mutant, stage, l, cls_only))
    return out


MUTANT_CASES = _mutant_cases()


def test_every_mutant_has_cases():
    assert {c[1] for c in MUTANT_CASES} == set(SCS.MUTANTS)


@pytest.mark.parametrize("case", MUTANT_CASES, ids=lambda c: f"{_id(c[0])}-{c[1]}-{c[2]}{c[3]}{'-cls' if c[4] else ''}")
def test_a_mutant_as_the_reference_is_refused(case):
    """the stand-in (a correct chain) against the reference with one mutation: it must leave the cap or the bound at that stage"""
    cfg, mutant, stage, l, cls_only = case
    m, xs, full, cls = chain(cfg)
    if stage == "patch":
        r, ok = SCS.check32("mutant", xs[0], SCS.stage_patch(m, mutant=mutant))
        assert not ok, f"patch {mutant}: ratio {r:.3f}"
        return
    if stage == "proj":
        x_cls = np.ascontiguousarray(xs[-1][::m.T])
        ln, _ = SCS.stage_out_proj(m, x_cls)
        got = SCS.stage_out_proj(m, x_cls, np.float32)[1](ln["emu"])["emu"]
        r, ok = SCS.check32("mutant", got, SCS.stage_out_proj(m, x_cls, mutant=mutant)[1](ln["emu"]))
        assert not ok, f"proj {mutant}: ratio {r:.3f}"
        return
    dev = (cls if cls_only else full)[l]
    saved = {k: list(v) for k, v in SCS.WORST.items()}
    res = SCS.block_checks(m, l, xs[l], dev, mutant=mutant, cls_only=cls_only, stages=(stage,))
    SCS.WORST.clear()
    SCS.WORST.update(saved)
    assert res and not all(ok for _, _, _, ok in res), f"{stage} {mutant}: {res}"


def test_operand_terms_equal_the_hosts():
    """vit_stream_cases restates the header's term definitions; ibloc_amd.vit.split_terms / weight_lo followed by the fp16 conversion of
    the upload give the same bits on the case weights"""
    for family in SCS.FAMILIES:
        cfg, w, _ = SCS.inputs(family)
        for key in ("l0.q.w", "l1.o.w", "l2.fc1.w", "l0.fc2.w", "patch.w") + (("proj.w",) if cfg.proj_dim else ()):
            a = np.asarray(w[key], np.float32).reshape(w[key].shape[0], -1)
            for terms in (2, 3):
                want = V.split_terms(a, terms).astype(np.float16)
                assert np.array_equal(SCS.w_terms(a, terms).view(np.uint16), want.view(np.uint16)), (family, key, terms)
            assert np.array_equal(SCS.w_lo(a).view(np.uint16), V.weight_lo(a).astype(np.float16).view(np.uint16)), (family, key)
            assert np.array_equal(SCS.w_terms(a, 1).view(np.uint16), a.astype(np.float16).view(np.uint16))


def _desc(family, flags_extra):
    cfg = SCS.FAMILIES[family]
    return V.VitDesc(cfg.dim, cfg.depth, cfg.heads, cfg.mlp_dim, cfg.patch, cfg.img_h, cfg.img_w, cfg.n_tokens, cfg.patch_k_pad, flags_extra,
                     cfg.depth, cfg.out_dim, cfg.ln_eps)


@pytest.mark.parametrize("flag,at", [(0, 1), (V.FLAG_ACT_TERMS2, 2), (V.FLAG_ACT_TERMS3, 3)])
def test_workspace_layout_is_ordered_aligned_and_inside_the_workspace(flag, at):
    """ibl_vit_workspace_layout (no device call): IBL_VIT_WS_COUNT buffers in the header's order, each on a 256-byte boundary, none
    overlapping, the end inside ibl_vit_workspace_bytes (less the 255 bytes the base may be rounded up by), under every ACT_TERMS flag"""
    lib = _lib.lib
    n = len(V.WS_TAPS)
    assert V.WS_TAPS == ("x", "xn", "qkv", "att", "hid", "fin") and n == 6
    for family in SCS.FAMILIES:
        cfg = SCS.FAMILIES[family]
        d = _desc(family, flag)
        for batch in (1, 3, 224):
            offs = (C.c_int64 * n)()
            assert lib.ibl_vit_workspace_layout(C.byref(d), batch, offs, n) == 0
            R = -(-batch * cfg.n_tokens // 128) * 128
            sizes = [R * cfg.dim * 4, R * cfg.dim * 2 * 3, R * 3 * cfg.dim * 2, R * cfg.dim * 2 * at, R * cfg.mlp_dim * 2 * at,
                     -(-batch // 128) * 128 * cfg.dim * 2]
            offs = list(offs)
            assert offs[0] == 0 and all(o % 256 == 0 for o in offs)
            for i in range(n - 1):
                assert offs[i] + sizes[i] <= offs[i + 1], (family, batch, i)
            total = lib.ibl_vit_workspace_bytes(C.byref(d), batch)
            assert offs[-1] + sizes[-1] + 255 <= total, (family, batch)
    d = _desc("vit", flag)
    two = (C.c_int64 * 2)()
    assert lib.ibl_vit_workspace_layout(C.byref(d), 3, two, 2) == 0 and two[1] == 128 * 128 * 4
    assert lib.ibl_vit_workspace_layout(C.byref(d), 3, two, 0) == 0
    for bad in (lib.ibl_vit_workspace_layout(C.byref(d), 0, two, 2), lib.ibl_vit_workspace_layout(C.byref(d), 3, None, 2),
                lib.ibl_vit_workspace_layout(C.byref(d), 3, two, n + 1), lib.ibl_vit_workspace_layout(C.byref(d), 3, two, -1),
                lib.ibl_vit_workspace_layout(None, 3, two, 2)):
        assert bad < 0 and lib.ibl_last_error()


def test_workspace_bytes_is_what_it_was():
    """the size callers are asked for did not change with the layout table: the sum the forward carved, fp32 final rows, nine gaps"""
    for family in SCS.FAMILIES:
        cfg = SCS.FAMILIES[family]
        for flag, at in ((0, 1), (V.FLAG_ACT_TERMS2, 2), (V.FLAG_ACT_TERMS3, 3)):
            for batch in (1, 3, 224):
                R, Rb = -(-batch * cfg.n_tokens // 128) * 128, -(-batch // 128) * 128
                want = R * cfg.dim * (4 + 6 + 6 + 2 * at) + R * cfg.mlp_dim * 2 * at + Rb * cfg.dim * 6 + 9 * 256
                assert _lib.lib.ibl_vit_workspace_bytes(C.byref(_desc(family, flag)), batch) == want
