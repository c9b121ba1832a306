"""Native-aspect crops (per-crop patch grids) -- what tests/test_vit_ragged_model.py (CPU), tests/test_gpu_vit_ragged.py (GPU) and
tools/gen_golden_vit_ragged.py share: the configurations, a mixed batch of grids with seeded weights and N(0, 1) pixels, transformers'
Dinov2Model / Dinov2WithRegistersModel holding those weights (both accept non-square pixel_values as they are), and the fp32
restatement of one crop at its grid -- `oracle.vit_oracle.vit_forward` (plain) and `tests.dino_reg_cases.forward` (registers) run with
dataclasses.replace(cfg, img_h=gh * patch, img_w=gw * patch)."""
import dataclasses

import numpy as np
import torch

from ibloc_amd import vit as V
from oracle import vit_oracle as vo
from tests import dino_reg_cases as DC

# 1 x 1: the smallest sequence; 3 x 7 / 7 x 3: the same token count, transposed tables; 16 x 16: the model's own grid; 20 x 9 and
# 27 x 9: budget-filling grids of 1 : 2.2 and 1 : 3 crops
GRIDS = ((1, 1), (3, 7), (7, 3), (16, 16), (20, 9), (27, 9))
# (golden key, configuration, weight seed, input seed)
CASES = (("tiny_dino", "tiny_dino", 711, 811), ("tiny_dino_reg", "tiny_dino_reg", 712, 812))
PROBE = 64                  # pixel values per crop the golden file keeps, to pin the regenerated input


def config(name):
    """V.CONFIGS[name]; the plain DINOv2 table is resampled as transformers >= 4.46 does it (size=), which is defined for any grid"""
    cfg = V.CONFIGS[name]
    return cfg if cfg.n_registers else dataclasses.replace(cfg, pos_interp="size")


def at_grid(cfg, grid):
    return dataclasses.replace(cfg, img_h=grid[0] * cfg.patch, img_w=grid[1] * cfg.patch)


def build(case, grids=GRIDS):
    """-> (key, cfg, weights, [pixels (3, gh * patch, gw * patch) fp32 per grid]), regenerated from the seeds"""
    key, name, wseed, iseed = case
    cfg = config(name)
    w = V.random_weights(cfg, wseed)
    rng = np.random.default_rng(iseed)
    return key, cfg, w, [rng.normal(size=(3, gh * cfg.patch, gw * cfg.patch)).astype(np.float32) for gh, gw in grids]


def hf_model(cfg, w):
    """transformers' model of `cfg` holding the weights `w`, in eval mode"""
    if cfg.n_registers:
        return DC.hf_model(cfg, w)
    from transformers import Dinov2Config, Dinov2Model
    c = Dinov2Config(hidden_size=cfg.dim, num_hidden_layers=cfg.depth, num_attention_heads=cfg.heads, mlp_ratio=cfg.mlp_dim // cfg.dim,
                     image_size=cfg.pos_grid[0] * cfg.patch, patch_size=cfg.patch, layer_norm_eps=cfg.ln_eps, hidden_act="gelu")
    m = Dinov2Model(c).eval()
    sd = DC.hf_dinov2_reg_state_dict(dataclasses.replace(cfg, n_registers=1), dict(w, reg=np.zeros((1, cfg.dim), np.float32)))
    del sd["embeddings.register_tokens"]
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return m


@torch.no_grad()
def hf_embed(model, x):
    """pooler_output (the class row after the final LayerNorm) of one crop (3, H, W) -> (dim,)"""
    return model(pixel_values=torch.from_numpy(x[None])).pooler_output[0].numpy()


def restate(cfg, w, x, device="cpu"):
    """the fp32 restatement of one crop (3, gh * patch, gw * patch) at its own grid -> (dim,)"""
    c = at_grid(cfg, (x.shape[1] // cfg.patch, x.shape[2] // cfg.patch))
    if cfg.n_registers:
        return DC.forward(w, c, x[None], device=device)[0]
    return vo.vit_forward(w, c, x[None], device=device)[0]
