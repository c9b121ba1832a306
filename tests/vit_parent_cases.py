"""Case table of tests/test_gpu_vit_parent.py and tools/gen_golden_vit_parent.py: the encoder forward and each of its kernels alone, on
seeded inputs, reduced to the sha256 of the output bytes.  tests/golden/vit_parent_digests.json holds the digests of the commit before the
encoder's kernels were split over csrc/vit_gemm.hip, vit_layernorm.hip, vit_attention.hip and vit.hip: that split changed no device
instruction and no launch, so anything but equality is a defect.

A group is a function that yields (case name, device tensor); `GROUPS` maps the group's name to it.  Only `out` is digested, and of it
only the window the call defines (a CLS-only attention writes row 0 of a crop, the patch scatter leaves a crop's prefix row alone): the
workspace rows a mode does not write are not defined.  Uses only the Python surface the earlier commit has.  No GEMM shape here depends
on the device's CU count."""
import contextlib
import functools
import hashlib
import os

import numpy as np
import torch

from ibloc_amd import vit as V
from tests import vit_stream_cases as SCS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_parent_digests.json")


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


# ---- the forward: every configuration tests/test_gpu_vit_stream.py runs ---------------------------------------------------------------
STREAM = [(f, p, True, False) for f in SCS.FAMILIES for p in SCS.PLANS] + SCS.EXTRA


def stream_id(c):
    f, p, kext, fold = c
    return f"{f}-{p}" + ("" if kext else "-kext0") + ("-fold" if fold else "")


@functools.lru_cache(maxsize=None)
def stream_model(cfg):
    return SCS.Model(*cfg)


def stream_group(cfg):
    """n_blocks_run 0 .. 3; all tokens and (with a class token) the class rows; with and without the final LayerNorm; clip's projection"""
    family, plan, kext, fold = cfg
    m = stream_model(cfg)
    patches = dev(m.patches)
    has_cls = SCS.FAMILIES[family].cls_token
    for k in range(SCS.DEPTH + 1):
        modes = [(True, False, False), (True, True, False)]
        if has_cls:
            modes += [(False, False, False), (False, True, False)]
            if SCS.FAMILIES[family].proj_dim:
                modes.append((False, True, True))
        for all_tokens, final_ln, proj in modes:
            c = SCS.run_cfg(family, k, all_tokens, final_ln=final_ln, proj=proj)
            with env("IBL_VIT_RESID_KEXT", "1" if kext else "0"):
                enc = V.VitEncoder(c, m.w, precision=plan, fold_layerscale=fold)
            yield f"{k}-{'all' if all_tokens else 'cls'}-{'proj' if proj else ('ln' if final_ln else 'raw')}", enc.forward_patches(patches)


# ---- the forward at V.CONFIGS: each attention tier, rotation, registers, no class token, the 256 x 256 tile inside a forward ------------
FORWARD = {"tiny_clip": 3, "tiny_dinov3": 3, "tiny_dino_reg": 3, "tiny_dinov3_384": 3, "tiny_siglip_384": 3, "tiny_dino": 17}


def forward_group(name):
    cfg = V.CONFIGS[name]
    w = V.random_weights(cfg, 41)
    x = np.random.default_rng(42).normal(size=(FORWARD[name], 3, cfg.img_h, cfg.img_w)).astype(np.float32)
    for plan in ("plain", "default"):
        enc = V.VitEncoder(cfg, w, precision=None if plan == "default" else plan)
        yield plan, enc.forward_patches(enc.patches_from_pixels(torch.from_numpy(x)))


# ---- the GEMM alone: every (epilogue, activation) that is instantiated, on both tiles, the last row tile ragged ------------------------
GEMM_SHAPES = {"128": (129, 128, 128), "256": (4351, 512, 192)}          # rows, n_out, n_in
GEMM_PAIRS = [(e, 0) for e in range(8)] + [(e, a) for e in (V.LINEAR_GELU_F16, V.LINEAR_GELU_F16_X2, V.LINEAR_GELU_F16_X3) for a in (1, 2)]
GEMM_PATCHES = {129: 43, 4351: 229}                                      # patches per crop of the scatter epilogue: whole crops


def gemm_group(shape):
    M, N, K = GEMM_SHAPES[shape]
    rng = np.random.default_rng(5100 + M)
    x = dev(rng.normal(size=(M, K)).astype(np.float16))
    W = dev((rng.normal(size=(N, K)) * 0.1).astype(np.float16))
    bias, scale = dev(rng.normal(size=N).astype(np.float32)), dev(rng.uniform(0.5, 1.5, size=N).astype(np.float32))
    P = GEMM_PATCHES[M]
    pos = dev(rng.normal(size=(P, N)).astype(np.float32))
    resid = rng.normal(size=(M, N)).astype(np.float32)
    tokens = rng.normal(size=(M // P, P + 1, N)).astype(np.float32)
    for epi, act in GEMM_PAIRS:
        call = functools.partial(V.linear_f16_act, activation=act) if act == V.ACT_GELU_TANH else functools.partial(V.linear_f16_ex, activation=act)
        name = f"e{epi}-a{act}"
        if epi in (V.LINEAR_F16, V.LINEAR_GELU_F16, V.LINEAR_GELU_F16_X2, V.LINEAR_GELU_F16_X3):
            terms = {V.LINEAR_GELU_F16_X2: 2, V.LINEAR_GELU_F16_X3: 3}.get(epi, 1)
            yield name, call(x, W, torch.empty((M, terms * N), dtype=torch.float16, device="cuda"), epi, bias=bias)
        elif epi == V.LINEAR_F32:
            yield name, call(x, W, torch.empty((M, N), dtype=torch.float32, device="cuda"), epi, bias=bias)
        elif epi == V.LINEAR_RESID_F32:
            yield name, call(x, W, dev(resid), epi, bias=bias, scale=scale)
            yield name + "-noscale", call(x, W, dev(resid), epi, bias=bias)
        elif epi == V.LINEAR_RESID_PRE_F32:
            yield name, call(x, W, dev(resid), epi, bias=bias, alpha=0.25)
        else:                                   # the scatter: rows 1 .. P of every crop are written, row 0 is the caller's
            out = dev(tokens).reshape(-1, N)
            call(x, W, out, epi, bias=bias, pos=pos, tokens_per_crop=P + 1, patches_per_crop=P)
            yield name, out.reshape(M // P, P + 1, N)[:, 1:]
            call(x, W, out, epi, accumulate=True, alpha=1.0 / 64, tokens_per_crop=P + 1, patches_per_crop=P)
            yield name + "-acc", out.reshape(M // P, P + 1, N)[:, 1:]


# ---- attention alone: one token count on each side of every tier boundary of the resident kernel; the streaming kernel ------------------
ATT_T = (64, 65, 144, 145, 208, 209, 272)
ATT_STREAM_T = (273, 300)


def _attention(fn, Ts):
    for T in Ts:
        qkv = dev(np.random.default_rng(6100 + T).normal(size=(2, T, 3 * 128)).astype(np.float16))
        for terms in (1, 2, 3):
            for cls_only in (0, 1):
                out = torch.zeros((2, T, terms * 128), dtype=torch.float16, device="cuda")
                fn(qkv, 2, cls_only=bool(cls_only), terms=terms, out=out)
                yield f"T{T}-t{terms}-c{cls_only}", out[:, :1] if cls_only else out


def attention_group():
    return _attention(V.attention_f16, ATT_T)


def attention_stream_group():
    return _attention(V.attention_stream_f16, ATT_STREAM_T)


# ---- LayerNorm and the rotation alone ------------------------------------------------------------------------------------------------------
LN_DIMS = (128, 1024, 328)            # 328: one float4 per lane and a tail


def layernorm_group():
    for dim in LN_DIMS:
        rng = np.random.default_rng(7100 + dim)
        x = dev((rng.normal(size=(37, dim)) * 3 + 1).astype(np.float32))
        g, b = dev(rng.normal(size=dim).astype(np.float32)), dev(rng.normal(size=dim).astype(np.float32))
        for kind in (V.LN_F32, V.LN_F16, V.LN_F16_X2, V.LN_F16_X3):
            yield f"d{dim}-k{kind}", V.layernorm_f32(x, g, b, 1e-6, out_kind=kind)


def rope_group():
    table = dev(V.rope_table(3, 5, 100.0).astype(np.float32))
    for k_only in (0, 1):
        qkv = dev(np.random.default_rng(8100).normal(size=(2, 20, 3 * 128)).astype(np.float16))
        yield f"k{k_only}", V.rope_f16(qkv, table, 2, 5, k_only=bool(k_only))


GROUPS = {f"stream/{stream_id(c)}": functools.partial(stream_group, c) for c in STREAM}
GROUPS.update({f"forward/{n}": functools.partial(forward_group, n) for n in FORWARD})
GROUPS.update({f"gemm/{s}": functools.partial(gemm_group, s) for s in GEMM_SHAPES})
GROUPS.update({"attention": attention_group, "attention_stream": attention_stream_group, "layernorm": layernorm_group, "rope": rope_group})


def run_group(name):
    """-> {"<group>/<case>": sha256}"""
    out = {f"{name}/{case}": digest(t) for case, t in GROUPS[name]()}
    torch.cuda.synchronize()
    return out
