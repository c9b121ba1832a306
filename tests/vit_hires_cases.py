"""The golden cases of the high-resolution encoders (more than 272 tokens per crop: the attention streams its keys), shared by
tools/gen_golden_vit_hires.py (which mirrors CASES), tests/test_vit_hires_model.py and tests/test_gpu_vit_hires.py.  As in
tests/vit_cases.py only outputs are stored (tests/golden/vit_hires_golden.npz); weights and inputs are regenerated from their seeds."""
import dataclasses

import numpy as np

from ibloc_amd import vit as V

# (golden key, configuration, overrides, weight seed, input seed, batch)
CASES = [
    # transformers.Dinov2Model at 518 px: 1 370 tokens, the 37 x 37 position table as stored
    ("tiny_dino_518", "tiny_dino_518", {}, 111, 211, 2),
    # CLIPVisionModelWithProjection(hidden_act="quick_gelu") at 336 px, patch 14: 577 tokens, the 24 x 24 table as stored
    ("tiny_clip_l14_336", "clip_l14_336_openai", {"dim": 128, "depth": 2, "heads": 2, "mlp_dim": 256, "patch_bias": False}, 112, 212, 2),
]


def build(case):
    """-> (key, cfg, weights, pixels)"""
    key, name, over, wseed, iseed, batch = case
    cfg = dataclasses.replace(V.CONFIGS[name], **{k: v for k, v in over.items() if k != "patch_bias"})
    w = V.random_weights(cfg, wseed)
    if over.get("patch_bias") is False:
        w["patch.b"] = np.zeros_like(w["patch.b"])
    x = np.random.default_rng(iseed).normal(size=(batch, 3, cfg.img_h, cfg.img_w)).astype(np.float32)
    return key, cfg, w, x


def oracle_forward(w, cfg, x, device="cpu"):
    """the fp32 restatement of the forward: oracle/vit_oracle.py, or tests/clip_openai_cases.forward where the activation is QuickGELU"""
    from oracle import vit_oracle as vo
    from tests import clip_openai_cases as CQ
    if cfg.quick_gelu:
        return CQ.forward(w, cfg, x, device=device)
    return vo.vit_forward(w, cfg, x) if device == "cpu" else CQ.forward(w, cfg, x, device=device)
