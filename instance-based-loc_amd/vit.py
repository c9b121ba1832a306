"""Host side of the ViT encoders (DINOv2 / ViT-B/16 / CLIP ViT-B/32 / TransReID streams):
configuration, weight packing into the C-ABI structs of include/ibloc.h, and the batched
preprocess + forward call.  Replaces the model objects utils/embeddings.py builds at import time
(/root/reference/utils/embeddings.py:13-28) and the per-crop calls at :31-98.
"""
import ctypes as C
import dataclasses
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import preprocess as pp

FLAG_LAYERSCALE = 1
FLAG_PRE_LN = 2
FLAG_FINAL_LN = 4
FLAG_QUICK_GELU = 8
FLAG_PROJ = 16
FLAG_OUT_ALL_TOKENS = 32
FLAG_ACT_TERMS2 = 64         # IBL_VIT_ACT_TERMS2 / 3: some block takes the input of a residual GEMM as K-extended rows of 2 / 3 terms
FLAG_ACT_TERMS3 = 128
FLAG_NO_CLS = 256            # IBL_VIT_NO_CLS: the sequence is the patch tokens alone (SigLIP)
FLAG_TANH_GELU = 512         # IBL_VIT_TANH_GELU: fc1 activation gelu_pytorch_tanh (SigLIP)
MAX_LAYERS = 32
# workspace buffers of ibl_vit_forward in the order of include/ibloc.h's IBL_VIT_WS_* enum
WS_TAPS = ("x", "xn", "qkv", "att", "hid", "fin")


class VitDesc(C.Structure):
    _fields_ = [("dim", C.c_int32), ("depth", C.c_int32), ("heads", C.c_int32), ("mlp_dim", C.c_int32),
                ("patch", C.c_int32), ("img_h", C.c_int32), ("img_w", C.c_int32), ("n_tokens", C.c_int32),
                ("patch_k_pad", C.c_int32), ("flags", C.c_int32), ("n_blocks_run", C.c_int32),
                ("out_dim", C.c_int32), ("ln_eps", C.c_float), ("n_registers", C.c_int32)]


class VitLayer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ln1_g", "ln1_b", "w_qkv", "b_qkv", "w_o", "b_o", "ls1", "ln2_g", "ln2_b",
                                          "w_fc1", "b_fc1", "w_fc2", "b_fc2", "ls2",
                                          "w_qkv_x", "w_o_lo", "ls1_lo", "w_fc1_x", "w_fc2_lo", "ls2_lo")] + \
               [("qkv_terms", C.c_int32), ("fc1_terms", C.c_int32), ("o_terms", C.c_int32), ("fc2_terms", C.c_int32),
                ("w_o_x", C.c_void_p), ("w_fc2_x", C.c_void_p)]


class VitWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_patch", "b_patch", "cls_pos", "pos_patch", "ln_pre_g", "ln_pre_b",
                                          "ln_f_g", "ln_f_b", "w_proj", "w_patch_lo", "w_proj_x")] + [("layers", VitLayer * MAX_LAYERS)] + \
               [("reg_tokens", C.c_void_p), ("rope_table", C.c_void_p)]


SPLIT_SCALE = 64.0          # IBL_VIT_SPLIT_SCALE (include/ibloc.h)
F16, F32 = "fp16", "fp32"   # what `pack_top` / `pack_layer` tag an array with: both leave the host as float32, F16 is rounded on the device

# Which operands of which blocks get a second fp16 term ("p<terms>;<layer>:<qkv><o><fc1><fc2>;...", layer "*" = every other block; qkv / fc1: 1, 2 (weights) or 3
# (weights + LayerNorm output), o / fc2: 1, 2 (weights) or 3 (weights + the attention output / the GELU hidden layer in two terms: one more
# accumulating launch each, round 4), p(atch embedding): 1 or 2 (weights)).  Measured on the 12-layer ViT-B/14 with the seeded
# random-init weights (DESIGN (c), tools/sim_vit_rounding.py): the residual stream is small in the first blocks, so the patch
# embedding (18 % of the error variance at 1.3 % of the FLOPs), block 0 (46 %) and block 1 (14 %) carry most of the fp16 rounding
# error of the embedding; the default gives them exact weights where that is cheap.  "plain" = one term everywhere (rounds 1-2).
# Round 4 (3 584 crops, forward of 224 crops): round 3's "p2;0:3222;1:2211" 7.60e-4 mean / 8.97e-4 max, 15.38 ms; this default (block 0's second
# LayerNorm output and block 2's QKV weights in two terms as well -- both ride in K-extended launches, no extra launch) 7.26e-4 / 8.59e-4,
# 15.76 ms; "p2;0:3232;1:2222" 7.14e-4 / 8.49e-4 but 16.14 ms (the second-term launch of an fc2 costs a whole read-modify-write pass).
DEFAULT_PRECISION = "p2;0:3232;1:2211;2:2111"
# per-model defaults where they differ: CLIP ViT-B/32 runs 50 tokens per crop (4 ms per 224 crops), so two-term weights in every block cost
# 2 ms and take its worst crop of 896 from 9.7e-4 -- too close to SURVEY 8d's 1e-3 gate -- to 8.1e-4 (mean 7.1e-4 -> 6.1e-4)
MODEL_PRECISION = {"clip_b32": "p2;*:2222;0:3232",
                   # the OpenAI (QuickGELU) CLIP models on 896 / 896 / 224 u8 crops, mean / max (DESIGN (c) has every plan that was measured).  B/32 misses
                   # the gate under the default plan as clip_b32 does (7.0e-4 / 1.005e-3); block 1's weights and block 2's attention weights in two terms
                   # bring it to 6.9e-4 / 8.9e-4 for 4.27 instead of 3.90 ms per 224 crops (clip_b32's plan: 6.0e-4 / 8.4e-4 but 5.74 ms).  B/16 meets it
                   # under the default (6.6e-4 / 7.7e-4): no entry.  L/14's 24 blocks spread the error over more of the depth (default 8.9e-4 / 1.04e-3):
                   # two-term weights in blocks 0-3 give 8.1e-4 / 9.2e-4 for 49.8 instead of 46.5 ms
                   "clip_b32_openai": "p2;0:3232;1:2222;2:2211",
                   "clip_l14_openai": "p2;0:3232;1:2222;2:2222;3:2222;4:2211",
                   # the register / rotary models on 224 u8 crops (32 at 518 px), mean / max (DESIGN (c) has the whole ladder).  The S and B register
                   # models and dinov3_vits16 meet the gate under the default (5.7e-4 / 7.1e-4, 6.7e-4 / 7.7e-4, 6.0e-4 / 6.4e-4 at 518 px, 5.4e-4 /
                   # 6.3e-4): no entry.  dinov3_vitb16 misses it there (7.9e-4 / 1.02e-3: the rotation rounds q and k to fp16 a second time);
                   # two-term weights in blocks 0-6 give 7.1e-4 / 9.3e-4 for 17.0 instead of 13.8 ms per 224 crops.  dinov2_vitl14_reg (default
                   # 9.9e-4 / 1.23e-3) passes under the last plan of the ladder only: 6.0e-4 / 7.5e-4, but 110 instead of 48 ms -- pass
                   # precision="default" where the time matters more.  dinov3_vitl16 meets it under no plan (p2;*:3333: 1.21e-3 / 1.83e-3) and
                   # runs the default
                   "dinov3_vitb16": "p2;0:3232;1:2222;2:2222;3:2222;4:2222;5:2222;6:2211",
                   "dinov2_vitl14_reg": "p2;*:3333"}


def parse_precision(spec):
    """-> (patch_terms, {layer: (qkv, o, fc1, fc2)})"""
    if spec in (None, "", "default"):
        spec = DEFAULT_PRECISION
    if spec == "plain":
        return 1, {}
    patch, layers = 1, {}
    for part in spec.split(";"):
        part = part.strip()
        if not part:
            continue
        if part[0] == "p":
            patch = int(part[1:])
        else:
            l, t = part.split(":")
            t = tuple(int(c) for c in t)
            if len(t) != 4 or not all(1 <= v <= 3 for v in t):
                raise ValueError(f"bad precision entry {part!r}")
            layers["*" if l.strip() == "*" else int(l)] = t      # "*": every block without an entry of its own
    if patch not in (1, 2):
        raise ValueError("patch terms: 1 or 2")
    return patch, layers


def split_terms(w, terms):
    """fp32 weight (N, K) -> K-extended fp16 operand rows [W_hi | W_lo * S] (terms 2) or [W_hi | W_hi / S | W_lo * S] (terms 3)"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    hi = w.astype(np.float16).astype(np.float32)
    lo = (w - hi) * SPLIT_SCALE
    parts = [hi, lo] if terms == 2 else [hi, hi / SPLIT_SCALE, lo]
    return np.concatenate(parts, axis=1)


def weight_lo(w):
    w = np.ascontiguousarray(w, dtype=np.float32)
    return (w - w.astype(np.float16).astype(np.float32)) * SPLIT_SCALE


@dataclass
class VitConfig:
    name: str
    dim: int
    depth: int
    heads: int
    mlp_dim: int
    patch: int
    img_h: int
    img_w: int
    pos_grid: tuple            # grid of the stored position embeddings (37, 37) for DINOv2 @518
    layerscale: bool = False
    pre_ln: bool = False
    final_ln: bool = True
    proj_dim: int = 0
    ln_eps: float = 1e-6
    n_blocks_run: int = -1
    out_all_tokens: bool = False
    recipe: str = "dinov2"
    pos_interp: str = "hf-4.44"    # how stored position embeddings are resampled to the run grid ("hf-4.44" | "size" | "size-aa")
    quick_gelu: bool = False       # fc1 activation x * sigmoid(1.702 x) (OpenAI CLIP) instead of erf GELU: IBL_VIT_QUICK_GELU
    cls_token: bool = True         # False (SigLIP): no class token, `pos` is (gh * gw, D) and used as stored: IBL_VIT_NO_CLS
    tanh_gelu: bool = False        # fc1 activation 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) (SigLIP): IBL_VIT_TANH_GELU
    n_registers: int = 0           # register tokens between the class token and the patches (DINOv2-reg, DINOv3): ibl_vit_desc.n_registers
    rope_theta: float | None = None    # DINOv3: rotary position embedding of this base on q / k of the patch rows; no position table

    @property
    def grid(self):
        return self.img_h // self.patch, self.img_w // self.patch

    @property
    def n_tokens(self):
        return int(self.cls_token) + self.n_registers + self.grid[0] * self.grid[1]

    @property
    def n_prefix(self):
        return int(self.cls_token) + self.n_registers

    @property
    def n_patches(self):
        return self.grid[0] * self.grid[1]

    @property
    def patch_k(self):
        return 3 * self.patch * self.patch

    @property
    def patch_k_pad(self):
        return (self.patch_k + 63) // 64 * 64

    @property
    def out_dim(self):
        return self.proj_dim if self.proj_dim else self.dim


CONFIGS = {
    # facebook/dinov2-base, as loaded at utils/embeddings.py:18 (image_size 518 -> 37x37 stored pos-embed)
    "dinov2_vitb14": VitConfig("dinov2_vitb14", 768, 12, 12, 3072, 14, 224, 224, (37, 37), layerscale=True,
                               recipe="dinov2"),
    # facebook/dinov2-small (BASELINE config 1)
    "dinov2_vits14": VitConfig("dinov2_vits14", 384, 12, 6, 1536, 14, 224, 224, (37, 37), layerscale=True,
                               recipe="dinov2"),
    # google/vit-base-patch16-224-in21k (utils/embeddings.py:26), layer_norm_eps 1e-12
    "vit_b16": VitConfig("vit_b16", 768, 12, 12, 3072, 16, 224, 224, (14, 14), ln_eps=1e-12, recipe="vit"),
    # open_clip ViT-B-32 laion2b_s34b_b79k (utils/embeddings.py:13-16): ln_pre, ln_post, 512-d projection
    "clip_b32": VitConfig("clip_b32", 768, 12, 12, 3072, 32, 224, 224, (7, 7), pre_ln=True, proj_dim=512,
                          ln_eps=1e-5, recipe="clip"),
    # OpenAI CLIP ViT-B/32, ViT-B/16 and ViT-L/14 at 224 px (also open_clip's *-quickgelu models and what transformers builds from a
    # default CLIPVisionConfig): the architecture of clip_b32 with QuickGELU.  A state dict does not say which activation its model
    # was trained with -- the configuration does
    "clip_b32_openai": VitConfig("clip_b32_openai", 768, 12, 12, 3072, 32, 224, 224, (7, 7), pre_ln=True, proj_dim=512,
                                 ln_eps=1e-5, recipe="clip", quick_gelu=True),
    "clip_b16_openai": VitConfig("clip_b16_openai", 768, 12, 12, 3072, 16, 224, 224, (14, 14), pre_ln=True, proj_dim=512,
                                 ln_eps=1e-5, recipe="clip", quick_gelu=True),
    "clip_l14_openai": VitConfig("clip_l14_openai", 1024, 24, 16, 4096, 14, 224, 224, (16, 16), pre_ln=True, proj_dim=768,
                                 ln_eps=1e-5, recipe="clip", quick_gelu=True),
    # the same towers at their high input resolutions: more than 272 tokens per crop, so the attention streams its keys
    # (ibl_attention_stream_kernel).  OpenAI CLIP ViT-L/14@336 (577 tokens, its 24 x 24 table as stored); facebook/dinov2-base at 448 px
    # (1 025 tokens, table resampled) and at the 518 px its checkpoints are trained at (1 370 tokens, the 37 x 37 table as stored)
    "clip_l14_336_openai": VitConfig("clip_l14_336_openai", 1024, 24, 16, 4096, 14, 336, 336, (24, 24), pre_ln=True, proj_dim=768,
                                     ln_eps=1e-5, recipe="clip_336", quick_gelu=True),
    "dinov2_vitb14_448": VitConfig("dinov2_vitb14_448", 768, 12, 12, 3072, 14, 448, 448, (37, 37), layerscale=True,
                                   recipe="dinov2_448"),
    "dinov2_vitb14_518": VitConfig("dinov2_vitb14_518", 768, 12, 12, 3072, 14, 518, 518, (37, 37), layerscale=True,
                                   recipe="dinov2_518"),
    # tiny configurations used by the parity tests
    "tiny_dino": VitConfig("tiny_dino", 128, 2, 2, 256, 14, 224, 224, (37, 37), layerscale=True, recipe="dinov2"),
    "tiny_dino_518": VitConfig("tiny_dino_518", 128, 2, 2, 256, 14, 518, 518, (37, 37), layerscale=True, recipe="dinov2_518"),
    "tiny_clip": VitConfig("tiny_clip", 128, 2, 2, 256, 32, 224, 224, (7, 7), pre_ln=True, proj_dim=128,
                           ln_eps=1e-5, recipe="clip"),
    "tiny_clip_q": VitConfig("tiny_clip_q", 128, 2, 2, 256, 32, 224, 224, (7, 7), pre_ln=True, proj_dim=128,
                             ln_eps=1e-5, recipe="clip", quick_gelu=True),
}


def _siglip(name, dim, depth, heads, mlp, px):
    """a SigLIP vision tower (google/siglip-*-patch16-*, the fixed-resolution SigLIP 2 checkpoints): ViT/16 without a class token, tanh
    GELU, final LayerNorm over every token -- the trunk ibloc_amd.siglip.SiglipEncoder puts its attention-pooling head on"""
    return VitConfig(name, dim, depth, heads, mlp, 16, px, px, (px // 16, px // 16), final_ln=True, ln_eps=1e-6, out_all_tokens=True,
                     recipe="siglip", cls_token=False, tanh_gelu=True)


CONFIGS.update({
    # 196 / 256 tokens: the resident attention kernel; 576: the streaming one.  So400m (head_dim 72, mlp 4304) is not supported
    "siglip_b16_224": _siglip("siglip_b16_224", 768, 12, 12, 3072, 224),
    "siglip_b16_256": _siglip("siglip_b16_256", 768, 12, 12, 3072, 256),
    "siglip_b16_384": _siglip("siglip_b16_384", 768, 12, 12, 3072, 384),
    "siglip_l16_256": _siglip("siglip_l16_256", 1024, 24, 16, 4096, 256),
    "siglip_l16_384": _siglip("siglip_l16_384", 1024, 24, 16, 4096, 384),
    "tiny_siglip": _siglip("tiny_siglip", 128, 2, 2, 256, 224),
    "tiny_siglip_384": _siglip("tiny_siglip_384", 128, 2, 2, 256, 384),
})


def _dino_reg(name, dim, heads, depth, px, recipe="dinov2"):
    """DINOv2 with registers (dinov2_vit{s,b,l}14_reg, facebook/dinov2-with-registers-*): the DINOv2 trunk with four register rows after
    the class row; transformers resamples its 37 x 37 position table with antialiasing ("size-aa")"""
    return VitConfig(name, dim, depth, heads, 4 * dim, 14, px, px, (37, 37), layerscale=True, recipe=recipe, pos_interp="size-aa",
                     n_registers=4)


def _dinov3(name, dim, heads, depth, px=224):
    """DINOv3 ViT-S / B / L at patch 16 (facebook/dinov3-vit*16-pretrain-*): four registers, rotary position embedding (theta 100) on q / k
    of the patch rows in place of a position table, LayerScale, eps 1e-5.  The gated-MLP variants (S+, H+) are not supported"""
    return VitConfig(name, dim, depth, heads, 4 * dim, 16, px, px, (px // 16, px // 16), layerscale=True, ln_eps=1e-5, recipe="dinov3",
                     n_registers=4, rope_theta=100.0)


CONFIGS.update({
    # 261 tokens: the resident attention kernel's widest tier (272); 1 374 at 518 px: the streaming one, the table as stored
    "dinov2_vits14_reg": _dino_reg("dinov2_vits14_reg", 384, 6, 12, 224),
    "dinov2_vitb14_reg": _dino_reg("dinov2_vitb14_reg", 768, 12, 12, 224),
    "dinov2_vitl14_reg": _dino_reg("dinov2_vitl14_reg", 1024, 16, 24, 224),
    "dinov2_vitb14_reg_518": _dino_reg("dinov2_vitb14_reg_518", 768, 12, 12, 518, recipe="dinov2_518"),
    "dinov3_vits16": _dinov3("dinov3_vits16", 384, 6, 12),            # 201 tokens
    "dinov3_vitb16": _dinov3("dinov3_vitb16", 768, 12, 12),
    "dinov3_vitl16": _dinov3("dinov3_vitl16", 1024, 16, 24),
    "tiny_dino_reg": dataclasses.replace(_dino_reg("tiny_dino_reg", 128, 2, 2, 224), mlp_dim=256),
    "tiny_dino_reg_518": dataclasses.replace(_dino_reg("tiny_dino_reg_518", 128, 2, 2, 518, recipe="dinov2_518"), mlp_dim=256),
    "tiny_dinov3": dataclasses.replace(_dinov3("tiny_dinov3", 128, 2, 2), mlp_dim=256),
    "tiny_dinov3_384": dataclasses.replace(_dinov3("tiny_dinov3_384", 128, 2, 2, px=384), mlp_dim=256),      # 581 tokens: rotation in front of the streaming attention
})


def random_weights(cfg: VitConfig, seed: int):
    """Seeded synthetic weights (no pretrained checkpoints exist offline): trunc-normal-ish N(0, 0.02)
    matrices, LayerNorm gains around 1, LayerScale around 1 -- numpy fp32, keyed like the oracle expects."""
    rng = np.random.default_rng(seed)

    def mat(*shape, std=0.02):
        return np.clip(rng.normal(0, std, size=shape), -2 * std, 2 * std).astype(np.float32)

    w = {
        "patch.w": mat(cfg.dim, 3, cfg.patch, cfg.patch),
        "patch.b": mat(cfg.dim),
        "cls": mat(cfg.dim),
        "pos": mat(int(cfg.cls_token) + cfg.pos_grid[0] * cfg.pos_grid[1], cfg.dim),
        "ln_f.g": (1 + mat(cfg.dim, std=0.1)),
        "ln_f.b": mat(cfg.dim, std=0.1),
    }
    if cfg.rope_theta is not None:
        del w["pos"]                   # rotary models hold no position table
    if cfg.n_registers:
        # non-zero (transformers initialises DINOv2's registers to zero, which would hide a missing prefix row)
        w["reg"] = mat(cfg.n_registers, cfg.dim)
    if cfg.pre_ln:
        w["ln_pre.g"] = 1 + mat(cfg.dim, std=0.1)
        w["ln_pre.b"] = mat(cfg.dim, std=0.1)
    if cfg.proj_dim:
        w["proj.w"] = mat(cfg.proj_dim, cfg.dim, std=cfg.dim ** -0.5)
    for l in range(cfg.depth):
        p = f"l{l}."
        w[p + "ln1.g"] = 1 + mat(cfg.dim, std=0.1)
        w[p + "ln1.b"] = mat(cfg.dim, std=0.1)
        # larger q/k scale than 0.02 so that the attention is not uniform (exercises the softmax)
        for n in ("q", "k", "v", "o"):
            w[p + n + ".w"] = mat(cfg.dim, cfg.dim, std=0.06 if n in "qk" else 0.03)
            w[p + n + ".b"] = mat(cfg.dim, std=0.02)
        w[p + "ln2.g"] = 1 + mat(cfg.dim, std=0.1)
        w[p + "ln2.b"] = mat(cfg.dim, std=0.1)
        w[p + "fc1.w"] = mat(cfg.mlp_dim, cfg.dim, std=0.03)
        w[p + "fc1.b"] = mat(cfg.mlp_dim)
        w[p + "fc2.w"] = mat(cfg.dim, cfg.mlp_dim, std=0.02)
        w[p + "fc2.b"] = mat(cfg.dim)
        if cfg.layerscale:
            w[p + "ls1"] = 1 + mat(cfg.dim, std=0.1)
            w[p + "ls2"] = 1 + mat(cfg.dim, std=0.1)
    return w


def interpolate_pos_embed(pos: np.ndarray, cfg: VitConfig) -> np.ndarray:
    """Stored (1 + gh*gw, D) position embeddings -> (n_tokens, D) for the run grid.  One-time load step.

    "hf-4.44": transformers 4.44.0 Dinov2Embeddings.interpolate_pos_encoding (the version the reference
    pins, environment.yml:275): bicubic, align_corners=False, scale_factor = (grid + 0.1) / stored_grid.
    "size": torch's size= form (transformers >= 4.46).
    "size-aa": the size= form with antialias=True, as Dinov2WithRegistersEmbeddings.interpolate_pos_encoding resamples (37 x 37 ->
    16 x 16 at 224 px is a down-scale, so the antialiasing filter changes every row)."""
    gh, gw = cfg.pos_grid
    th, tw = cfg.grid
    if (gh, gw) == (th, tw):
        return pos.astype(np.float32)
    cls_pos, patch_pos = pos[:1], pos[1:]
    t = torch.from_numpy(patch_pos.astype(np.float32)).reshape(1, gh, gw, -1).permute(0, 3, 1, 2)
    if cfg.pos_interp == "hf-4.44":
        sf = (float((th + 0.1) / math.sqrt(gh * gw)), float((tw + 0.1) / math.sqrt(gh * gw)))
        t = torch.nn.functional.interpolate(t, scale_factor=sf, mode="bicubic", align_corners=False)
        if tuple(t.shape[-2:]) != (th, tw):
            raise ValueError("pos-embed interpolation produced an unexpected grid")
    elif cfg.pos_interp in ("size", "size-aa"):
        t = torch.nn.functional.interpolate(t, size=(th, tw), mode="bicubic", align_corners=False, antialias=cfg.pos_interp == "size-aa")
    else:
        raise ValueError(f"unknown pos_interp {cfg.pos_interp!r}")
    patch_new = t.permute(0, 2, 3, 1).reshape(th * tw, -1).numpy()
    return np.concatenate([cls_pos, patch_new], axis=0).astype(np.float32)


ATT_STREAM_MAX_TOKENS = 8192       # IBL_ATT_STREAM_MAX_TOKENS (include/ibloc.h): the longest sequence of the ragged forward, prefix rows included


def native_grid(h: int, w: int, patch: int, max_patches: int, upscale: bool = True):
    """The patch grid (gh, gw) a crop of h x w pixels runs at when it keeps its aspect ratio: the grid of (nearly) the crop's shape
    that fills a budget of max_patches patches.  Deterministic, float64:

        s  = sqrt(max_patches * patch^2 / (h * w));  if not upscale: s = min(s, 1)
        gh = min(max(1, floor(h * s / patch + 1e-9)), max_patches);  gw likewise from w
        while gh * gw > max_patches: decrement the larger of the two (gh on a tie)

    So 1 <= gh, gw and gh * gw <= max_patches always; a square crop gets the square grid of a square budget (16 x 16 of 256); with
    upscale=False a crop smaller than the budget is not blown up: gh <= max(1, h // patch), gw likewise.  The crop is then resized
    whole to (gh * patch, gw * patch): the aspect ratio is kept up to the rounding to whole patches."""
    if h < 1 or w < 1 or patch < 1 or max_patches < 1:
        raise ValueError(f"native_grid: h, w, patch and max_patches must be positive, got {h} x {w}, {patch}, {max_patches}")
    s = math.sqrt(float(max_patches) * float(patch) * float(patch) / (float(h) * float(w)))
    if not upscale:
        s = min(s, 1.0)
    gh = min(max(1, int(math.floor(h * s / patch + 1e-9))), max_patches)
    gw = min(max(1, int(math.floor(w * s / patch + 1e-9))), max_patches)
    while gh * gw > max_patches:
        if gh >= gw:
            gh -= 1
        else:
            gw -= 1
    return gh, gw


def token_chunks(tokens, max_tokens):
    """[slice] over a batch whose crop i has tokens[i] rows: consecutive crops, in order, each chunk within max_tokens rows -- except
    that a crop which alone exceeds the budget runs as a chunk of its own"""
    out, lo, acc = [], 0, 0
    for i, t in enumerate(tokens):
        if i > lo and acc + t > max_tokens:
            out.append(slice(lo, i))
            lo, acc = i, 0
        acc += t
    if len(tokens) > lo:
        out.append(slice(lo, len(tokens)))
    return out


def rope_table(grid_h: int, grid_w: int, theta: float) -> np.ndarray:
    """-> fp32 (grid_h * grid_w, 64) = [cos(32) | sin(32)] per patch: transformers' DINOv3ViTRopePositionEmbedding in eval mode (no
    shift / jitter / rescale) at head_dim 64, in its order of fp32 operations.  Patch-centre coordinates in [-1, 1], inv_freq =
    theta^-(4 j / 64), j = 0..15, angles 2 pi coord inv_freq -- the 16 of y, then the 16 of x; the model tiles these 32 twice, which is
    what `ibl_rope_kernel` does by pairing column i with i + 32."""
    inv_freq = 1 / theta ** torch.arange(0, 1, 4 / 64, dtype=torch.float32)
    ch = torch.arange(0.5, grid_h, dtype=torch.float32) / grid_h
    cw = torch.arange(0.5, grid_w, dtype=torch.float32) / grid_w
    coords = 2.0 * torch.stack(torch.meshgrid(ch, cw, indexing="ij"), dim=-1).flatten(0, 1) - 1.0
    angles = (2 * math.pi * coords[:, :, None] * inv_freq[None, None, :]).flatten(1, 2)
    return torch.cat([torch.cos(angles), torch.sin(angles)], dim=1).numpy().astype(np.float32)


class PackedCrops:
    """A list of differently sized HxWx3 uint8 crops as ONE device-resident byte string + their shapes: what `VitEncoder.preprocess`
    uploads for a list of arrays, done once (a query batch whose crops already sit in HBM).  Slices like a list."""

    def __init__(self, crops, device="cuda", _src=None, _shapes=None, _offs=None):
        if _src is not None:
            self.src, self.shapes, self.offs = _src, _shapes, _offs
            return
        self.shapes = [tuple(c.shape[:2]) for c in crops]
        self.offs = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in self.shapes])]).astype(np.int64)
        flat = np.concatenate([np.ascontiguousarray(c, dtype=np.uint8).reshape(-1) for c in crops]) if crops else np.zeros(0, np.uint8)
        self.src = torch.from_numpy(flat).to(device)

    def __len__(self):
        return len(self.shapes)

    def __getitem__(self, sl):
        if not isinstance(sl, slice):
            raise TypeError("PackedCrops supports slices only")
        lo, hi, step = sl.indices(len(self.shapes))
        assert step == 1
        return PackedCrops(None, _src=self.src[int(self.offs[lo]):int(self.offs[hi])], _shapes=self.shapes[lo:hi],
                           _offs=self.offs[lo:hi + 1] - self.offs[lo])


def resolve_options(default_plan, precision=None, fold_layerscale=None, resid_kext=None):
    """constructor arguments + environment -> (precision, fold_layerscale, resid_kext); the one place that reads $IBL_VIT_PREC,
    $IBL_VIT_FOLD_LS and $IBL_VIT_RESID_KEXT (0: second weight terms of o / fc2 as launches of their own, rounds 3-4a)"""
    return (precision if precision is not None else os.environ.get("IBL_VIT_PREC", default_plan),
            os.environ.get("IBL_VIT_FOLD_LS", "0") == "1" if fold_layerscale is None else bool(fold_layerscale),
            os.environ.get("IBL_VIT_RESID_KEXT", "1") != "0" if resid_kext is None else bool(resid_kext))


def validate(cfg: VitConfig, weights: dict):
    """what the kernels cannot run, or the weights do not fit: ValueError"""
    if cfg.depth > MAX_LAYERS:
        raise ValueError("too many layers")
    if cfg.quick_gelu and cfg.tanh_gelu:
        raise ValueError("quick_gelu and tanh_gelu are both set")
    if cfg.dim != 64 * cfg.heads:
        raise ValueError(f"head_dim {cfg.dim / cfg.heads:g} is not supported: the attention and rotation kernels run head_dim 64")
    if cfg.n_registers and not cfg.cls_token:
        raise ValueError("n_registers needs cls_token: registers follow the class row")
    if cfg.n_registers and tuple(np.shape(weights.get("reg", ()))) != (cfg.n_registers, cfg.dim):
        raise ValueError(f"the weights hold registers of shape {np.shape(weights.get('reg', ()))}, the configuration {cfg.name} "
                         f"needs ({cfg.n_registers}, {cfg.dim})")
    if not cfg.n_registers and np.size(weights.get("reg", ())):
        raise ValueError(f"the weights hold {np.shape(weights['reg'])[0]} register tokens, the configuration {cfg.name} none")
    if cfg.rope_theta is not None and "pos" in weights:
        raise ValueError("rope_theta and a position table are both given")
    if not cfg.cls_token and cfg.rope_theta is None:
        if not cfg.out_all_tokens:
            raise ValueError("cls_token=False needs out_all_tokens: there is no class row to return")
        if tuple(cfg.pos_grid) != tuple(cfg.grid) or np.shape(weights["pos"]) != (cfg.n_patches, cfg.dim):
            raise ValueError(f"cls_token=False: the position table {np.shape(weights['pos'])} of grid {cfg.pos_grid} must be that of the run grid {cfg.grid}")


def plan_terms(cfg: VitConfig, layer_terms: dict, resid_kext=True):
    """parsed plan -> ([(qkv, o, fc1, fc2) the host packs block l for], [(o, fc2): the second weight term goes as a launch of its own],
    act_terms: the widest rows a residual GEMM reads).  Without resid_kext o / fc2 are one-term rows (2 = the extra launch, 3 refused)."""
    nrun = cfg.depth if cfg.n_blocks_run < 0 else cfg.n_blocks_run
    terms, lo_launch = [], []
    for l in range(cfg.depth):
        t = layer_terms.get(l, layer_terms.get("*"))
        if t is None or (l == nrun - 1 and not cfg.out_all_tokens):     # the CLS-only last block stays plain
            t = (1, 1, 1, 1)
        for name, v in (("o", t[1]), ("fc2", t[3])):
            if not resid_kext and v > 2:
                raise ValueError(f"{name} = 3 needs the K-extended form")
        lo_launch.append((t[1] == 2, t[3] == 2) if not resid_kext else (False, False))
        terms.append(t if resid_kext else (t[0], 1, t[2], 1))
    return terms, lo_launch, max([1] + [max(t[1], t[3]) for t in terms])


def pack_top(cfg: VitConfig, weights: dict, patch_terms=1, proj_x=False) -> dict:
    """-> {ibl_vit_weights field: (F16 | F32, float32 array)} outside the layers; no device"""
    validate(cfg, weights)
    if cfg.rope_theta is not None:
        # rotary models: no position table.  The patch scatter still adds a row per patch, so it is handed zeros
        pos = np.zeros((int(cfg.cls_token) + cfg.n_patches, cfg.dim), dtype=np.float32)
    elif cfg.cls_token:
        pos = interpolate_pos_embed(weights["pos"], cfg)
    else:
        # no class token: the table is (gh * gw, D) and used as stored (resampling it is not supported)
        pos = np.ascontiguousarray(weights["pos"], dtype=np.float32)
    wp = np.zeros((cfg.dim, cfg.patch_k_pad), dtype=np.float32)
    wp[:, :cfg.patch_k] = weights["patch.w"].reshape(cfg.dim, -1)
    a = {"w_patch": (F16, wp)}
    if patch_terms == 2:
        a["w_patch_lo"] = (F16, weight_lo(wp))
    if "patch.b" in weights:
        a["b_patch"] = (F32, weights["patch.b"])
    a["pos_patch"] = (F32, pos[1:] if cfg.cls_token else pos)
    if cfg.cls_token:
        a["cls_pos"] = (F32, weights["cls"].reshape(-1) + pos[0])
    if cfg.n_registers:
        a["reg_tokens"] = (F32, weights["reg"])
    if cfg.rope_theta is not None:
        a["rope_table"] = (F32, rope_table(cfg.grid[0], cfg.grid[1], cfg.rope_theta))
    if cfg.pre_ln:
        a["ln_pre_g"], a["ln_pre_b"] = (F32, weights["ln_pre.g"]), (F32, weights["ln_pre.b"])
    if cfg.final_ln:
        a["ln_f_g"], a["ln_f_b"] = (F32, weights["ln_f.g"]), (F32, weights["ln_f.b"])
    if cfg.proj_dim:
        a["w_proj"] = (F16, weights["proj.w"])
        if proj_x:      # the last arithmetic before the output: three-term operands (free at batch x dim x out_dim)
            a["w_proj_x"] = (F16, split_terms(weights["proj.w"], 3))
    return a


def _pack_resid(cfg, weights, p, name, i, terms, lo_launch, fold):
    """one residual GEMM of a block (o: i = 1, fc2: i = 2), as `pack_layer` yields it.
    fold (lab, off by default): x += ls * (a W^T + b) = a (diag(ls) W)^T + ls * b.  Without a scale vector in the epilogue the library
    can preload the residual tile into the accumulators (EPI_RESID_PRE_F32, csrc/vit_gemm.hip).  (Without LayerScale: "folded" = no
    1 / S vectors for the second terms either)"""
    w, b = np.asarray(weights[p + name + ".w"], np.float32), np.asarray(weights[p + name + ".b"], np.float32)
    ls = np.asarray(weights[p + f"ls{i}"], np.float32) if cfg.layerscale else None
    if fold and ls is not None:
        w, b = ls[:, None] * w, ls * b
    elif ls is not None:
        yield f"ls{i}", (F32, ls)
    yield "w_" + name, (F16, w)
    yield "b_" + name, (F32, b)
    if terms > 1:
        yield f"w_{name}_x", (F16, split_terms(w, terms))
        yield name + "_terms", terms
    elif lo_launch:
        yield f"w_{name}_lo", (F16, weight_lo(w))
        if not fold:                             # (no vector: the library adds the term with the factor 1 / S, residual preloaded)
            yield f"ls{i}_lo", (F32, (ls if ls is not None else np.ones(cfg.dim, dtype=np.float32)) / SPLIT_SCALE)


def pack_layer(cfg: VitConfig, weights: dict, l: int, terms, lo_launch=(False, False), fold=False):
    """block l -> (ibl_vit_layer field, value) pairs, value = (F16 | F32, float32 array) or the int of a `*_terms` field; terms, lo_launch:
    `plan_terms`' entries for the block.  A field the block does not use is not yielded.  No device.  A generator: a consumer that uploads
    as it goes holds one operand's fp32 temporaries at a time, as the hot pages of one allocation (`dict(pack_layer(...))`: the layer's)"""
    p = f"l{l}."
    tq, to, t1, t2 = terms
    for name in ("ln1", "ln2"):
        yield name + "_g", (F32, weights[p + name + ".g"])
        yield name + "_b", (F32, weights[p + name + ".b"])
    wqkv = np.concatenate([weights[p + "q.w"], weights[p + "k.w"], weights[p + "v.w"]], axis=0)
    yield "w_qkv", (F16, wqkv)
    if tq > 1:
        yield "w_qkv_x", (F16, split_terms(wqkv, tq))
        yield "qkv_terms", tq
    yield "b_qkv", (F32, np.concatenate([weights[p + "q.b"], weights[p + "k.b"], weights[p + "v.b"]], axis=0))
    yield "w_fc1", (F16, weights[p + "fc1.w"])
    yield "b_fc1", (F32, weights[p + "fc1.b"])
    if t1 > 1:
        yield "w_fc1_x", (F16, split_terms(weights[p + "fc1.w"], t1))
        yield "fc1_terms", t1
    yield from _pack_resid(cfg, weights, p, "o", 1, to, lo_launch[0], fold)
    yield from _pack_resid(cfg, weights, p, "fc2", 2, t2, lo_launch[1], fold)


# VitConfig attribute -> descriptor flag (IBL_VIT_NO_CLS is the absence of one: `make_desc`)
CONFIG_FLAGS = (("layerscale", FLAG_LAYERSCALE), ("pre_ln", FLAG_PRE_LN), ("final_ln", FLAG_FINAL_LN), ("proj_dim", FLAG_PROJ),
                ("quick_gelu", FLAG_QUICK_GELU), ("out_all_tokens", FLAG_OUT_ALL_TOKENS), ("tanh_gelu", FLAG_TANH_GELU))


def make_desc(cfg: VitConfig, act_terms=1) -> VitDesc:
    flags = sum(flag for attr, flag in CONFIG_FLAGS if getattr(cfg, attr))
    flags |= (0 if cfg.cls_token else FLAG_NO_CLS) | {1: 0, 2: FLAG_ACT_TERMS2, 3: FLAG_ACT_TERMS3}[act_terms]
    return VitDesc(cfg.dim, cfg.depth, cfg.heads, cfg.mlp_dim, cfg.patch, cfg.img_h, cfg.img_w, cfg.n_tokens, cfg.patch_k_pad, flags,
                   cfg.depth if cfg.n_blocks_run < 0 else cfg.n_blocks_run, cfg.out_dim, cfg.ln_eps, cfg.n_registers)


class Workspace:
    """The byte buffers a C-ABI forward works in, one per lane, grown on demand; and typed views into one by the offsets of the library's
    `*_workspace_layout` call, which count from the first 256-byte boundary of the buffer."""

    def __init__(self, device):
        self.device, self._lanes = device, {}

    def get(self, lane, nbytes) -> torch.Tensor:
        ws = self._lanes.get(lane)
        if ws is None or ws.numel() < nbytes:
            ws = self._lanes[lane] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws

    def views(self, lane, offsets, specs) -> dict:
        """offsets: what the layout call filled in; specs: [(name, dtype, shape)] in the same order -> {name: view}"""
        ws = self._lanes[lane]
        base = (-ws.data_ptr()) % 256
        out = {}
        for off, (name, dtype, shape) in zip(offsets, specs):
            lo, n = base + off, math.prod(shape) * dtype.itemsize
            assert lo + n <= ws.numel()
            out[name] = ws[lo:lo + n].view(dtype).view(shape)
        return out


def embed_chunks(n, max_batch, run) -> torch.Tensor:
    """run(slice) for every chunk of at most max_batch of n crops, the results as one tensor"""
    outs = [run(slice(i, i + max_batch)) for i in range(0, n, max_batch)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


class VitEncoder:
    """Device-resident weights + batched forward through the C-ABI."""

    def __init__(self, cfg: VitConfig, weights: dict, device="cuda", precision=None, fold_layerscale=None, resid_kext=None):
        """precision: operand-term plan (see DEFAULT_PRECISION; None = $IBL_VIT_PREC or the default, "plain" = fp16 operands only);
        fold_layerscale: LayerScale multiplied into the output-projection weights at load, so that the library may run the residual GEMMs
        with the residual tile preloaded (lab: with IBL_GEMM_RESID_PRE=1; measured 2 % slower than the read-modify-write epilogue, so the
        default -- also with $IBL_VIT_FOLD_LS unset -- keeps the LayerScale vectors and round 3's arithmetic);
        resid_kext: the second and third terms of o / fc2 as K-extended rows (None = on unless $IBL_VIT_RESID_KEXT is 0)"""
        self.precision, self.fold_layerscale, resid_kext = resolve_options(MODEL_PRECISION.get(cfg.name, DEFAULT_PRECISION), precision,
                                                                           fold_layerscale, resid_kext)
        self.cfg = cfg
        self.device = torch.device(device)
        patch_terms, layer_terms = parse_precision(self.precision)
        terms, lo_launch, self.act_terms = plan_terms(cfg, layer_terms, resid_kext)
        top = pack_top(cfg, weights, patch_terms, proj_x=self.precision != "plain")
        self._keep = []                     # device tensors referenced by the structs
        self.W = VitWeights()
        self._upload(self.W, top.items())
        for l in range(cfg.depth):          # packed and uploaded operand by operand: the host never holds more than one's fp32 temporaries
            self._upload(self.W.layers[l], pack_layer(cfg, weights, l, terms[l], lo_launch[l], self.fold_layerscale))
        self._act_terms = self.act_terms    # the attribute's earlier name, which callers still read
        self.desc = make_desc(cfg, self.act_terms)
        self.recipe = pp.recipe_for(cfg.recipe, cfg.img_h, cfg.img_w)
        self._ws = Workspace(self.device)
        self._streams = []
        self._plan_cache = {}
        self._pos_stored = weights.get("pos")   # the stored table: `forward_ragged` resamples it once per distinct grid
        self._grid_pos = {}                     # (gh, gw) -> fp32 device (n_prefix + gh * gw, dim), the prefix rows zero

    def _upload(self, struct, fields):
        for name, v in fields:
            if not isinstance(v, int):
                t = torch.from_numpy(np.ascontiguousarray(v[1], dtype=np.float32)).to(self.device)
                self._keep.append(t.to(torch.float16).contiguous() if v[0] == F16 else t)
                v = self._keep[-1].data_ptr()
            setattr(struct, name, v)

    # ---- preprocessing -------------------------------------------------------------------------
    def _bytes_to_device(self, s) -> torch.Tensor:
        """a ctypes array of descriptors (anything `bytes` takes) -> uint8 device tensor"""
        return torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8).to(self.device)

    def _mean_std(self):
        """the recipe's per-channel mean and std as the float[3] arguments of the preprocessing calls"""
        return (C.c_float * 3)(*self.recipe.mean), (C.c_float * 3)(*self.recipe.std)

    def preprocess(self, crops, want_u8=False):
        """crops: list of HxWx3 uint8 numpy arrays (RGB as the detector hands them over), or a single
        uint8 device/host tensor (N, H, W, 3) of equally sized crops.  Returns fp16 patch matrix (device)."""
        r = self.recipe
        if isinstance(crops, torch.Tensor):
            n, h, w, _ = crops.shape
            shapes = [(h, w)] * n
            src = crops.to(self.device).contiguous().view(-1)
        else:
            if not isinstance(crops, PackedCrops):
                crops = PackedCrops(crops, self.device)
            shapes, src = crops.shapes, crops.src.to(self.device)
        key = tuple(shapes) if len(set(shapes)) > 1 else (shapes[0], len(shapes))
        plan = self._plan_cache.get(key)
        if plan is None:
            descs, tables, src_bytes, tmp_bytes, max_h = pp.plan_batch(r, shapes)
            d_descs = self._bytes_to_device(descs)
            d_tables = torch.from_numpy(tables).to(self.device)
            plan = (d_descs, d_tables, src_bytes, tmp_bytes, max_h)
            if len(self._plan_cache) < 64:
                self._plan_cache[key] = plan
        d_descs, d_tables, src_bytes, tmp_bytes, max_h = plan
        assert src.numel() == src_bytes
        n = len(shapes)
        P = self.cfg.n_patches
        tmp = torch.empty(max(tmp_bytes, 16), dtype=torch.uint8, device=self.device)
        patches = torch.empty((n * P, self.cfg.patch_k_pad), dtype=torch.float16, device=self.device)
        out_u8 = torch.empty((n, r.out_h, r.out_w, 3), dtype=torch.uint8, device=self.device) if want_u8 else None
        mean, std = self._mean_std()
        st = _lib.lib.ibl_preprocess_crops(src.data_ptr(), d_descs.data_ptr(), n, max_h, d_tables.data_ptr(),
                                           tmp.data_ptr(), r.out_h, r.out_w, self.cfg.patch, self.cfg.patch_k_pad,
                                           1 if r.swap_rb else 0, mean, std, patches.data_ptr(),
                                           out_u8.data_ptr() if want_u8 else None,
                                           torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "ibl_preprocess_crops")
        return (patches, out_u8) if want_u8 else patches

    # ---- forward -------------------------------------------------------------------------------
    def forward_patches(self, patches: torch.Tensor, lane: int = 0, taps: bool = False):
        """lane: which of the encoder's workspaces to use (concurrent forwards on different streams need their own).
        taps=True: -> (out, dict) with a view of every workspace buffer of this forward under its WS_TAPS name (`workspace_taps`)."""
        P = self.cfg.n_patches
        assert patches.dtype == torch.float16 and patches.is_cuda and patches.shape[1] == self.cfg.patch_k_pad
        batch = patches.shape[0] // P
        ws = self._ws.get(lane, _lib.lib.ibl_vit_workspace_bytes(C.byref(self.desc), batch))
        shape = (batch, self.cfg.n_tokens, self.cfg.dim) if self.cfg.out_all_tokens else (batch, self.cfg.out_dim)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        st = _lib.lib.ibl_vit_forward(C.byref(self.desc), C.byref(self.W), patches.data_ptr(), batch, out.data_ptr(),
                                      ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "ibl_vit_forward")
        return (out, self.workspace_taps(batch, lane)) if taps else out

    def workspace_taps(self, batch: int, lane: int = 0) -> dict:
        """Views of what the last forward of `batch` crops on `lane` left in its workspace (include/ibloc.h, IBL_VIT_WS_*), each at the
        widest shape the descriptor allows; what a run fills of it is in the header: x fp32 (B, T, dim); xn fp16 (B * T, 3 * dim) -- a row
        of `terms` column blocks is at [i * terms * dim, (i + 1) * terms * dim) of the flattened view; qkv fp16 (B, T, 3 * dim); att fp16
        (B * T, at * dim) and hid fp16 (B * T, at * mlp_dim), flat in the same way, at = the workspace's term flag; fin fp16 (B, dim).
        The next forward on the lane overwrites them."""
        c = self.cfg
        offs = (C.c_int64 * len(WS_TAPS))()
        _lib.check(_lib.lib.ibl_vit_workspace_layout(C.byref(self.desc), batch, offs, len(WS_TAPS)), "ibl_vit_workspace_layout")
        at, R, f16, f32 = self.act_terms, batch * c.n_tokens, torch.float16, torch.float32
        return self._ws.views(lane, offs, [("x", f32, (batch, c.n_tokens, c.dim)), ("xn", f16, (R, 3 * c.dim)),
                                           ("qkv", f16, (batch, c.n_tokens, 3 * c.dim)), ("att", f16, (R, at * c.dim)),
                                           ("hid", f16, (R, at * c.mlp_dim)), ("fin", f16, (batch, c.dim))])

    def patches_from_pixels(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 3, H, W) float model input (already normalised) -> fp16 patch matrix.  Data-layout plumbing
        only (used by tests and by callers that hold pre-normalised tensors)."""
        return self._patch_rows(x, self.cfg.grid, 0)

    def _patch_rows(self, x: torch.Tensor, grid, n_prefix: int) -> torch.Tensor:
        """(B, 3, gh * patch, gw * patch) at one grid -> fp16 (B * (n_prefix + gh * gw), patch_k_pad): n_prefix zero rows, then the crop's patches"""
        cfg, p, B, (gh, gw) = self.cfg, self.cfg.patch, x.shape[0], grid
        t = x.to(self.device, torch.float32).reshape(B, 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, 3 * p * p)
        out = torch.zeros((B, n_prefix + gh * gw, cfg.patch_k_pad), dtype=torch.float16, device=self.device)
        out[:, n_prefix:, :cfg.patch_k] = t.to(torch.float16)
        return out.reshape(-1, cfg.patch_k_pad)

    def embed(self, crops, max_batch=512, streams=1, min_split=128, lane=0) -> torch.Tensor:
        """crops -> (N, out_dim) fp32 device tensor (un-normalised CLS embedding, as the reference returns).

        streams > 1: a batch of >= min_split crops is embedded as that many micro-batches on their own HIP streams.  The layers of
        a ViT are a strict chain, so on one stream the MFMA-bound K loops of a GEMM never overlap its own HBM-bound epilogue
        nor the LayerNorm / attention kernels around it; two independent chains fill each other's gaps (measured: embed 20.9 ->
        20.2 ms for 224 crops).  Off by default: the kernels of the two chains share the GPU, so per-kernel timings (the bench's
        roofline line) no longer describe one kernel.  Same arithmetic per crop either way."""
        n = crops.shape[0] if isinstance(crops, torch.Tensor) else len(crops)
        if n == 0:
            return torch.empty((0, self.cfg.out_dim), dtype=torch.float32, device=self.device)
        if streams > 1 and min_split <= n <= max_batch:
            if len(self._streams) != streams:
                self._streams = [torch.cuda.Stream(device=self.device) for _ in range(streams)]
            cur = torch.cuda.current_stream(self.device)
            bounds = [n * k // streams for k in range(streams + 1)]
            outs = []
            for k, st in enumerate(self._streams):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    outs.append(self.forward_patches(self.preprocess(crops[bounds[k]:bounds[k + 1]]), lane=k))
            for st in self._streams:
                cur.wait_stream(st)
            for o in outs:
                o.record_stream(cur)
            return torch.cat(outs, dim=0)
        return embed_chunks(n, max_batch, lambda sl: self.forward_patches(self.preprocess(crops[sl]), lane=lane))

    # ---- native-aspect crops: every crop at a patch grid of its own ----------------------------
    def has_grid_tables(self) -> bool:
        """whether the model has a position table for every grid: a class token and a learned table that is resampled, nothing of CLIP's"""
        c = self.cfg
        return c.rope_theta is None and c.cls_token and not c.proj_dim and not c.pre_ln and self._pos_stored is not None

    def check_ragged(self):
        """ValueError for what `ibl_vit_forward_ragged` refuses: the models without `has_grid_tables`"""
        c = self.cfg
        if not self.has_grid_tables():
            raise ValueError(f"{c.name}: per-crop patch grids need a class-token model with a learned, resampled position table (DINOv2, "
                             "plain or with registers); rotary tables (DINOv3), SigLIP and CLIP are not supported")

    def seq_offsets(self, grids) -> np.ndarray:
        """int32 [n + 1]: crop i owns rows seq[i] .. seq[i + 1] - 1 of every per-token buffer: n_prefix rows, then gh * gw patches"""
        tokens = [self.cfg.n_prefix + gh * gw for gh, gw in grids]
        if any(gh < 1 or gw < 1 for gh, gw in grids) or max(tokens) > ATT_STREAM_MAX_TOKENS:
            raise ValueError(f"a grid is empty or has more than {ATT_STREAM_MAX_TOKENS} tokens with its prefix rows")
        return np.concatenate([[0], np.cumsum(tokens)]).astype(np.int32)

    def grid_pos_rows(self, grid) -> torch.Tensor:
        """the position rows of a crop at `grid`: the stored table resampled with the configuration's pos_interp (once per grid, kept on
        the device), under zero rows for the prefix -- the class row's position is in cls_pos, registers have none"""
        t = self._grid_pos.get(grid)
        if t is None:
            p = self.cfg.patch
            pos = interpolate_pos_embed(self._pos_stored, dataclasses.replace(self.cfg, img_h=grid[0] * p, img_w=grid[1] * p))[1:]
            t = torch.from_numpy(np.concatenate([np.zeros((self.cfg.n_prefix, self.cfg.dim), np.float32), pos])).to(self.device)
            if len(self._grid_pos) < 4096:
                self._grid_pos[grid] = t
        return t

    def preprocess_ragged(self, crops, grids, want_u8=False):
        """crops (a list of HxWx3 uint8 arrays or PackedCrops), grids [(gh, gw)] -> fp16 patch matrix (total_tokens, patch_k_pad): crop
        i resized WHOLE to (gh * patch, gw * patch) with the recipe's filter, channel swap and mean / std -- no shortest-edge step, no
        centre crop -- its patches at rows seq[i] + n_prefix + p, the prefix rows zero.  want_u8: -> (patches, [the resized u8 image
        of every crop, (gh * patch, gw * patch, 3), model channel order])."""
        r, cfg = self.recipe, self.cfg
        if not isinstance(crops, PackedCrops):
            crops = PackedCrops(crops, self.device)
        shapes, src = crops.shapes, crops.src.to(self.device)
        assert len(shapes) == len(grids) and len(shapes) > 0
        seq = self.seq_offsets(grids)
        sizes = [(gh * cfg.patch, gw * cfg.patch) for gh, gw in grids]
        descs, rdescs, tables, src_bytes, tmp_bytes, u8_bytes, max_h = pp.plan_batch_ragged(r, shapes, sizes, seq[:-1] + cfg.n_prefix)
        assert src.numel() == src_bytes
        d_descs, d_rdescs, d_tables = self._bytes_to_device(descs), self._bytes_to_device(rdescs), torch.from_numpy(tables).to(self.device)
        tmp = torch.empty(max(tmp_bytes, 16), dtype=torch.uint8, device=self.device)
        patches = torch.empty((int(seq[-1]), cfg.patch_k_pad), dtype=torch.float16, device=self.device)
        out_u8 = torch.empty(u8_bytes, dtype=torch.uint8, device=self.device) if want_u8 else None
        st = _lib.lib.ibl_preprocess_crops_ragged(src.data_ptr(), d_descs.data_ptr(), d_rdescs.data_ptr(), C.addressof(rdescs), len(shapes),
                                                  max_h, d_tables.data_ptr(), tmp.data_ptr(), cfg.patch, cfg.patch_k_pad,
                                                  1 if r.swap_rb else 0, *self._mean_std(),
                                                  patches.data_ptr(), patches.shape[0], out_u8.data_ptr() if want_u8 else None,
                                                  torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "ibl_preprocess_crops_ragged")
        if not want_u8:
            return patches
        return patches, [out_u8[rd.u8_offset:rd.u8_offset + rd.out_h * rd.out_w * 3].view(rd.out_h, rd.out_w, 3) for rd in rdescs]

    def forward_ragged(self, patches: torch.Tensor, grids, lane: int = 0) -> torch.Tensor:
        """The forward of crops at their own grids through `ibl_vit_forward_ragged`.  patches fp16 (total_tokens, patch_k_pad), one row
        per token as `preprocess_ragged` lays them out (`patches_from_pixels_ragged` for pre-normalised pixels); grids [(gh, gw)].
        -> fp32 (n, dim) class rows, or with out_all_tokens (total_tokens, dim): the crops' rows packed back to back (`seq_offsets`).
        What the library cannot run -- DINOv3, SigLIP, CLIP -- it refuses: IblError."""
        cfg = self.cfg
        seq = self.seq_offsets(grids)
        n, total = len(grids), int(seq[-1])
        assert patches.dtype == torch.float16 and patches.is_cuda and patches.is_contiguous() and patches.shape == (total, cfg.patch_k_pad)
        if self.has_grid_tables():
            pos = torch.cat([self.grid_pos_rows(tuple(g)) for g in grids], dim=0)
        else:
            pos = torch.zeros((total, cfg.dim), dtype=torch.float32, device=self.device)     # the library refuses below, in its own words
        d_seq = torch.from_numpy(seq).to(self.device)
        ws = self._ws.get(lane, _lib.lib.ibl_vit_ragged_workspace_bytes(C.byref(self.desc), total, n))
        out = torch.empty((total, cfg.dim) if cfg.out_all_tokens else (n, cfg.out_dim), dtype=torch.float32, device=self.device)
        st = _lib.lib.ibl_vit_forward_ragged(C.byref(self.desc), C.byref(self.W), patches.data_ptr(), pos.data_ptr(), d_seq.data_ptr(),
                                             seq.ctypes.data, n, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "ibl_vit_forward_ragged")
        return out

    def patches_from_pixels_ragged(self, xs) -> torch.Tensor:
        """[(3, gh * patch, gw * patch) float model input, already normalised] -> the fp16 patch matrix `forward_ragged` takes (zero
        prefix rows).  Data-layout plumbing only, as `patches_from_pixels`."""
        p = self.cfg.patch
        return torch.cat([self._patch_rows(x[None], (x.shape[1] // p, x.shape[2] // p), self.cfg.n_prefix) for x in xs], dim=0)

    def embed_native(self, crops, max_patches=None, upscale=True, max_tokens=65536, lane=0) -> torch.Tensor:
        """crops -> (N, out_dim) fp32 class embeddings, every crop at `native_grid` of its own shape (max_patches: the budget, default
        the configuration's n_patches) instead of the recipe's square window.  A batch is cut into chunks of at most max_tokens rows
        (`token_chunks`); the caller's order is kept.  These embeddings differ from `embed`'s by design: a memory and its queries must be
        embedded the same way."""
        self.check_ragged()
        if not isinstance(crops, PackedCrops):
            crops = PackedCrops(list(crops), self.device)
        if len(crops) == 0:
            return torch.empty((0, self.cfg.out_dim), dtype=torch.float32, device=self.device)
        budget = self.cfg.n_patches if max_patches is None else int(max_patches)
        grids = [native_grid(h, w, self.cfg.patch, budget, upscale) for h, w in crops.shapes]
        outs = [self.forward_ragged(self.preprocess_ragged(crops[sl], grids[sl]), grids[sl], lane=lane)
                for sl in token_chunks([self.cfg.n_prefix + gh * gw for gh, gw in grids], max_tokens)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


class NativeAspectEncoder:
    """A VitEncoder whose `embed` runs every crop at the patch grid of its own aspect ratio (`VitEncoder.embed_native`): what
    `LocaliseEngine(encoder=...)` and `utils.embeddings` take in place of the encoder itself."""

    def __init__(self, encoder: VitEncoder, max_patches=None, upscale=True):
        encoder.check_ragged()
        self.encoder, self.max_patches, self.upscale = encoder, max_patches, upscale
        self.cfg, self.device = encoder.cfg, encoder.device

    def embed(self, crops, max_batch=512, streams=1, min_split=128, lane=0) -> torch.Tensor:
        """`VitEncoder.embed`'s signature; max_batch crops at the model's own token count bound a chunk's rows (streams / min_split: one
        stream runs the ragged forward)"""
        if isinstance(crops, torch.Tensor):
            crops = list(crops.cpu().numpy())
        return self.encoder.embed_native(crops, self.max_patches, self.upscale, max_tokens=max_batch * self.cfg.n_tokens, lane=lane)


LINEAR_F16, LINEAR_GELU_F16, LINEAR_RESID_F32, LINEAR_F32 = 0, 1, 2, 4
LINEAR_PATCH_F32, LINEAR_RESID_PRE_F32, LINEAR_GELU_F16_X2, LINEAR_GELU_F16_X3 = 3, 5, 6, 7


class LinearDesc(C.Structure):              # ibl_linear_desc (include/ibloc.h)
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int64), ("W", C.c_void_p), ("ldw", C.c_int64), ("bias", C.c_void_p),
                ("scale", C.c_void_p), ("pos", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int64), ("rows", C.c_int64),
                ("n_out", C.c_int32), ("n_in", C.c_int32), ("epilogue", C.c_int32), ("accumulate", C.c_int32),
                ("tokens_per_crop", C.c_int32), ("patches_per_crop", C.c_int32), ("alpha", C.c_float), ("activation", C.c_int32)]


ACT_GELU_ERF, ACT_QUICK_GELU = 0, 1         # IBL_ACT_*: what LINEAR_GELU_F16 / _X2 / _X3 apply
ACT_GELU_TANH = 2                           # through linear_f16_act only: ibl_linear_f16_ex refuses it


def linear_f16(x: torch.Tensor, W: torch.Tensor, bias=None, epilogue=LINEAR_F16, out=None, scale=None) -> torch.Tensor:
    """out = epilogue(x W^T + bias) through `ibl_linear_f16` (the encoder's GEMM kernel on its own).
    x (rows, n_in) fp16, W (n_out, n_in) fp16 (nn.Linear layout), bias / scale fp32 (n_out).  LINEAR_RESID_F32
    accumulates into `out` (fp32), the other epilogues allocate it when it is not given."""
    assert x.dtype == torch.float16 and W.dtype == torch.float16 and x.is_cuda and W.is_cuda
    assert x.stride(-1) == 1 and W.stride(-1) == 1
    rows, n_in = x.shape
    n_out = W.shape[0]
    if out is None:
        if epilogue == LINEAR_RESID_F32:
            raise ValueError("LINEAR_RESID_F32 accumulates into `out`")
        out = torch.empty((rows, n_out), device=x.device, dtype=torch.float32 if epilogue == LINEAR_F32 else torch.float16)
    want = torch.float32 if epilogue in (LINEAR_RESID_F32, LINEAR_F32) else torch.float16
    assert out.dtype == want and out.shape == (rows, n_out) and out.stride(-1) == 1
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == n_out and bias.is_contiguous()
    if scale is not None:
        assert scale.dtype == torch.float32 and scale.numel() == n_out and scale.is_contiguous()
    st = _lib.lib.ibl_linear_f16(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), bias.data_ptr() if bias is not None else None,
                                  scale.data_ptr() if scale is not None else None, rows, n_out, n_in, epilogue, out.data_ptr(),
                                  out.stride(0), torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "ibl_linear_f16")
    return out


def linear_f16_ex(x: torch.Tensor, W: torch.Tensor, out: torch.Tensor, epilogue, bias=None, scale=None, pos=None, alpha=1.0,
                  accumulate=False, tokens_per_crop=0, patches_per_crop=0, activation=ACT_GELU_ERF, _call_activation=None) -> torch.Tensor:
    """`ibl_linear_f16_ex`: the encoder's GEMM with any of its eight epilogues, written into `out` (include/ibloc.h says what each one
    computes; `activation` = ACT_QUICK_GELU makes the three GELU epilogues apply x * sigmoid(1.702 x)).  x (rows, n_in) fp16, W (n_out, n_in) fp16, `out` fp16 (rows, terms * n_out) for LINEAR_F16 / _GELU_F16 / _GELU_F16_X2 /
    _X3, else fp32 (rows, n_out) -- for LINEAR_PATCH_F32 fp32 (rows / patches_per_crop * tokens_per_crop, n_out), the token rows.  All
    three may be row-strided views.  Only the dtypes and the devices are checked here: what the library cannot run it refuses (IblError).
    (_call_activation: `linear_f16_act`'s form of the call, which shares this body)"""
    for t in (x, W, out):
        assert t.is_cuda and t.dim() == 2 and t.stride(1) == 1
    assert x.dtype == torch.float16 and W.dtype == torch.float16
    assert out.dtype == (torch.float16 if epilogue in (LINEAR_F16, LINEAR_GELU_F16, LINEAR_GELU_F16_X2, LINEAR_GELU_F16_X3) else torch.float32)
    for t in (bias, scale, pos):
        assert t is None or (t.dtype == torch.float32 and t.is_cuda and t.is_contiguous())
    d = LinearDesc(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), bias.data_ptr() if bias is not None else None,
                   scale.data_ptr() if scale is not None else None, pos.data_ptr() if pos is not None else None, out.data_ptr(),
                   out.stride(0), x.shape[0], W.shape[0], x.shape[1], int(epilogue), int(accumulate), int(tokens_per_crop),
                   int(patches_per_crop), float(alpha), int(activation))
    stream = torch.cuda.current_stream().cuda_stream
    if _call_activation is None:
        _lib.check(_lib.lib.ibl_linear_f16_ex(C.byref(d), stream), "ibl_linear_f16_ex")
    else:
        _lib.check(_lib.lib.ibl_linear_f16_act(C.byref(d), int(_call_activation), stream), "ibl_linear_f16_act")
    return out


def linear_f16_act(x: torch.Tensor, W: torch.Tensor, out: torch.Tensor, epilogue, activation, bias=None, scale=None, pos=None, alpha=1.0,
                   accumulate=False, tokens_per_crop=0, patches_per_crop=0) -> torch.Tensor:
    """`ibl_linear_f16_act`: `linear_f16_ex` with the activation as an argument of the call -- ACT_GELU_ERF, ACT_QUICK_GELU or
    ACT_GELU_TANH (the tanh form of GELU, SigLIP's); the descriptor's own activation field stays 0.  Everything else as `linear_f16_ex`."""
    return linear_f16_ex(x, W, out, epilogue, bias, scale, pos, alpha, accumulate, tokens_per_crop, patches_per_crop, 0, activation)


def attention_f16(qkv: torch.Tensor, heads: int, cls_only: bool = False, terms: int = 1, out=None, _symbol="ibl_attention_f16") -> torch.Tensor:
    """softmax(q k^T / 8) v per (crop, head) through `ibl_attention_f16` (the encoder's attention kernel on its own).
    qkv (batch, n_tokens, 3 * dim) fp16 = [q | k | v]; returns (batch, n_tokens, terms * dim) fp16.  With `cls_only` only row 0 of
    every crop is written, so pass `out` unless the other rows may stay uninitialised.  Shapes the kernel cannot run
    (dim != 64 * heads, n_tokens > 272, terms outside 1..3) are refused by the library: IblError.
    (_symbol: `attention_stream_f16` shares this body)"""
    assert qkv.dtype == torch.float16 and qkv.is_cuda and qkv.dim() == 3 and qkv.is_contiguous() and qkv.shape[2] % 3 == 0
    batch, n_tokens, dim = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    if out is None:
        out = torch.empty((batch, n_tokens, max(int(terms), 0) * dim), device=qkv.device, dtype=torch.float16)
    assert out.dtype == torch.float16 and out.is_cuda and out.is_contiguous() and out.shape == (batch, n_tokens, terms * dim)
    st = getattr(_lib.lib, _symbol)(qkv.data_ptr(), out.data_ptr(), batch, n_tokens, dim, heads, int(cls_only), terms,
                                    torch.cuda.current_stream().cuda_stream)
    _lib.check(st, _symbol)
    return out


def attention_stream_f16(qkv: torch.Tensor, heads: int, cls_only: bool = False, terms: int = 1, out=None) -> torch.Tensor:
    """softmax(q k^T / 8) v per (crop, head) through `ibl_attention_stream_f16`: the kernel the encoder runs beyond 272 tokens (keys and
    values stream through LDS under an fp32 online softmax), on its own.  Arguments and result as for `attention_f16`; n_tokens may be
    anything up to 8192, short rows included.  Shapes the kernel cannot run are refused by the library: IblError."""
    return attention_f16(qkv, heads, cls_only, terms, out, _symbol="ibl_attention_stream_f16")


def attention_ragged_f16(qkv: torch.Tensor, seq_off, heads: int, cls_only: bool = False, terms: int = 1, out=None) -> torch.Tensor:
    """softmax(q k^T / 8) v per (crop, head) over crops of different lengths through `ibl_attention_ragged_f16`: qkv (total, 3 * dim)
    fp16, crop b in rows seq_off[b] .. seq_off[b + 1] - 1 (seq_off: int32 array of batch + 1 ascending offsets; rows outside every
    segment are left alone).  Returns (total, terms * dim) fp16; with `cls_only` only row seq_off[b] of every crop is written, so pass
    `out` unless the rest may stay uninitialised.  A crop's rows are `attention_stream_f16`'s of that crop alone, bit for bit.  What
    the kernel cannot run is refused by the library: IblError."""
    assert qkv.dtype == torch.float16 and qkv.is_cuda and qkv.dim() == 2 and qkv.is_contiguous() and qkv.shape[1] % 3 == 0
    seq = np.ascontiguousarray(seq_off, dtype=np.int32)
    assert seq.ndim == 1 and seq.size >= 1
    dim = qkv.shape[1] // 3
    if out is None:
        out = torch.empty((qkv.shape[0], max(int(terms), 0) * dim), device=qkv.device, dtype=torch.float16)
    assert out.dtype == torch.float16 and out.is_cuda and out.is_contiguous() and out.shape == (qkv.shape[0], terms * dim)
    assert int(seq.max()) <= qkv.shape[0], "a segment ends beyond the buffers"
    d_seq =torch.from_numpy(seq).to(qkv.device)
    st = _lib.lib.ibl_attention_ragged_f16(qkv.data_ptr(), out.data_ptr(), d_seq.data_ptr(), seq.ctypes.data, seq.size - 1, dim, heads,
                                           int(cls_only), terms, torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "ibl_attention_ragged_f16")
    return out


def rope_f16(qkv: torch.Tensor, table: torch.Tensor, heads: int, n_prefix: int, k_only: bool = False) -> torch.Tensor:
    """Rotary position embedding in place on q and k of the patch rows of qkv (batch, n_tokens, 3 * dim) fp16 through `ibl_rope_f16` (the
    encoder's kernel on its own); table (n_tokens - n_prefix, 64) fp32 = [cos | sin] (`rope_table`).  The first n_prefix rows of a crop
    and the v columns stay; k_only leaves q alone too.  What the kernel cannot run is refused by the library: IblError."""
    assert qkv.dtype == torch.float16 and qkv.is_cuda and qkv.dim() == 3 and qkv.is_contiguous() and qkv.shape[2] % 3 == 0
    assert table.dtype == torch.float32 and table.is_cuda and table.is_contiguous() and table.shape == (qkv.shape[1] - n_prefix, 64)
    st = _lib.lib.ibl_rope_f16(qkv.data_ptr(), table.data_ptr(), qkv.shape[0], qkv.shape[1], int(n_prefix), qkv.shape[2] // 3, heads,
                               int(k_only), torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "ibl_rope_f16")
    return qkv


LN_F32, LN_F16, LN_F16_X2, LN_F16_X3 = 0, 1, 2, 3


def layernorm_f32(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out_kind=LN_F32, out=None) -> torch.Tensor:
    """LayerNorm over the last axis of x (n_rows, dim) fp32 through `ibl_layernorm_f32` (the encoder's kernel on its own).  x and
    `out` may be row-strided views (only the last axis must be contiguous); `out=x` normalises in place (LN_F32).  LN_F16 /
    LN_F16_X2 / LN_F16_X3 give fp16 rows of 1 / 2 / 3 terms, (n_rows, terms * dim).  dim > 1024 or dim % 4 != 0 is refused
    by the library: IblError."""
    assert x.dtype == torch.float32 and x.is_cuda and x.dim() == 2 and x.stride(1) == 1
    n_rows, dim = x.shape
    width = dim * (1 if out_kind == LN_F32 else int(out_kind))
    if out is None:
        out = torch.empty((n_rows, width), device=x.device, dtype=torch.float32 if out_kind == LN_F32 else torch.float16)
    assert out.dtype == (torch.float32 if out_kind == LN_F32 else torch.float16) and out.is_cuda
    assert out.dim() == 2 and out.shape == (n_rows, width) and out.stride(1) == 1
    for t in (gamma, beta):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == dim
    st = _lib.lib.ibl_layernorm_f32(x.data_ptr(), x.stride(0), n_rows, dim, gamma.data_ptr(), beta.data_ptr(), eps, out.data_ptr(),
                                     out.stride(0), out_kind, torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "ibl_layernorm_f32")
    return out
