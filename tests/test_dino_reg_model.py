"""CPU: the register / rotary configurations (DINOv2 with registers, DINOv3) without a GPU -- the fp32 restatement of
tests/dino_reg_cases.py against transformers' Dinov2WithRegistersModel and DINOv3ViTModel and against the committed golden, what a skipped
feature does to the class embedding, the rotary table and the antialiased position-table resampling against the models' own, and the
error model of `ibl_rope_kernel`."""
import functools
import os

import numpy as np
import pytest
import torch

from ibloc_amd import vit as V
from tests import dino_reg_cases as DC

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "dino_reg_golden.npz"))
IDS = [c[0] for c in DC.CASES]


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _case(i):
    key, cfg, w, x = DC.build(DC.CASES[i])
    return key, cfg, w, x, DC.forward(w, cfg, x)


def test_configurations():
    want = {"dinov2_vits14_reg": (261, 384, 6), "dinov2_vitb14_reg": (261, 768, 12), "dinov2_vitl14_reg": (261, 1024, 16),
            "dinov2_vitb14_reg_518": (1374, 768, 12), "dinov3_vits16": (201, 384, 6), "dinov3_vitb16": (201, 768, 12),
            "dinov3_vitl16": (201, 1024, 16), "tiny_dino_reg": (261, 128, 2), "tiny_dino_reg_518": (1374, 128, 2), "tiny_dinov3": (201, 128, 2),
            "tiny_dinov3_384": (581, 128, 2)}
    for name, (tokens, dim, heads) in want.items():
        c = V.CONFIGS[name]
        assert (c.n_tokens, c.dim, c.heads, c.n_registers, c.n_prefix) == (tokens, dim, heads, 4, 5) and c.dim == 64 * c.heads and c.layerscale
        if name.startswith(("dinov3", "tiny_dinov3")):
            assert c.rope_theta == 100.0 and c.ln_eps == 1e-5 and c.patch == 16 and c.recipe == "dinov3"
        else:
            assert c.rope_theta is None and c.pos_interp == "size-aa" and c.patch == 14 and c.pos_grid == (37, 37)
    # the fields default to what every earlier configuration ran
    assert V.CONFIGS["dinov2_vitb14"].n_registers == 0 and V.CONFIGS["dinov2_vitb14"].rope_theta is None and V.CONFIGS["dinov2_vitb14"].n_tokens == 257
    w = V.random_weights(V.CONFIGS["tiny_dinov3"], 1)
    assert "pos" not in w and w["reg"].shape == (4, 128) and np.count_nonzero(w["reg"]) == w["reg"].size


@pytest.mark.parametrize("i", range(len(DC.CASES)), ids=IDS)
def test_restatement_vs_transformers_and_golden(i):
    """pooler_output on seeded weights and N(0, 1) pixels, rel-L2 <= 2e-4 (what the CLIP and SigLIP restatements are held to), against
    the live model and against the committed golden; the regenerated pixels are the generator's"""
    key, cfg, w, x, got = _case(i)
    assert np.array_equal(x.reshape(-1)[:DC.PROBE], GOLD[key + ".pixels"])
    with torch.no_grad():
        hf = DC.hf_model(cfg, w)(pixel_values=torch.from_numpy(x)).pooler_output.numpy()
    r_hf, r_gold = rel_l2(got, hf), rel_l2(got, GOLD[key])
    print(f"{key}: restatement vs transformers {r_hf:.3e}, vs golden {r_gold:.3e}")
    assert got.shape == GOLD[key].shape == (x.shape[0], cfg.dim)
    assert r_hf <= 2e-4 and r_gold <= 2e-4


@pytest.mark.parametrize("i", range(len(DC.CASES)), ids=IDS)
def test_a_skipped_feature_fails_the_golden(i):
    """the restatement without the register rows, and on the rotary cases without the rotation, lies outside the 2e-3 the fp16 forward is
    held to against the golden (tests/test_gpu_dino_reg.py)"""
    key, cfg, w, x, _ = _case(i)
    r = rel_l2(DC.forward(w, cfg, x, registers=False), GOLD[key])
    print(f"{key}: without registers {r:.3e}")
    assert r > 2e-3
    if cfg.rope_theta is not None:
        r = rel_l2(DC.forward(w, cfg, x, rope=False), GOLD[key])
        print(f"{key}: without rotation {r:.3e}")
        assert r > 2e-3


@pytest.mark.parametrize("gh,gw", [(14, 14), (24, 24), (10, 17)])
def test_rope_table_is_the_models(gh, gw):
    """V.rope_table against DINOv3ViTRopePositionEmbedding in eval mode: <= 1 fp32 ulp; the model's 64 columns are the 32 tiled twice"""
    from transformers import DINOv3ViTConfig
    from transformers.models.dinov3_vit.modeling_dinov3_vit import DINOv3ViTRopePositionEmbedding
    m = DINOv3ViTRopePositionEmbedding(DINOv3ViTConfig(hidden_size=128, num_attention_heads=2, patch_size=16, rope_theta=100.0)).eval()
    with torch.no_grad():
        cos, sin = m(torch.zeros(1, 3, gh * 16, gw * 16))
    cos, sin = cos.numpy(), sin.numpy()
    assert cos.shape == (gh * gw, 64) and np.array_equal(cos[:, :32], cos[:, 32:]) and np.array_equal(sin[:, :32], sin[:, 32:])
    t = V.rope_table(gh, gw, 100.0)
    assert t.shape == (gh * gw, 64) and t.dtype == np.float32
    want = np.concatenate([cos[:, :32], sin[:, :32]], axis=1)
    ulp = np.abs(t.astype(np.float64) - want) / np.spacing(np.maximum(np.abs(want), np.float32(2.0 ** -100)))
    print(f"{gh} x {gw}: worst {ulp.max():.2f} ulp")
    assert ulp.max() <= 1.0


@pytest.mark.parametrize("px", (224, 448))
def test_size_aa_is_the_models_interpolation(px):
    """pos_interp "size-aa" equals Dinov2WithRegistersEmbeddings.interpolate_pos_encoding, and differs from the form without antialiasing"""
    import dataclasses
    from transformers import Dinov2WithRegistersConfig
    from transformers.models.dinov2_with_registers.modeling_dinov2_with_registers import Dinov2WithRegistersEmbeddings
    cfg = dataclasses.replace(V.CONFIGS["tiny_dino_reg"], img_h=px, img_w=px)
    pos = V.random_weights(cfg, 3)["pos"]
    emb = Dinov2WithRegistersEmbeddings(Dinov2WithRegistersConfig(hidden_size=cfg.dim, image_size=518, patch_size=14, num_register_tokens=4))
    with torch.no_grad():
        emb.position_embeddings.copy_(torch.from_numpy(pos).unsqueeze(0))
        want = emb.interpolate_pos_encoding(torch.zeros(1, 1 + cfg.n_patches, cfg.dim), px, px)[0].numpy()
    got = V.interpolate_pos_embed(pos, cfg)
    assert got.shape == (1 + cfg.n_patches, cfg.dim) and np.array_equal(got, want)
    plain = V.interpolate_pos_embed(pos, dataclasses.replace(cfg, pos_interp="size"))
    assert rel_l2(plain, want) > 1e-2 if px == 224 else True


def test_rotation_error_model():
    """the numpy emulation of ibl_rope_kernel stays inside the bound the GPU test holds the kernel to, on N(0, 1), near +-65504 and on
    fp16 subnormals"""
    ratio, fam = DC.rope_model_ratio()
    print(f"rotation: worst |emulation - ref| / bound = {ratio:.3f} ({fam})")
    assert ratio < 1.0
    # the emulation is a rotation: k_only leaves q alone, prefix rows and v stay
    x = DC.rope_inputs("normal", 2, 6, 2, 1)
    t = V.rope_table(1, 3, 100.0)
    full, konly = DC.emulate_rope(x, t, 3, 2), DC.emulate_rope(x, t, 3, 2, k_only=True)
    assert np.array_equal(full[:, :3], x[:, :3]) and np.array_equal(full[..., 256:], x[..., 256:])
    assert np.array_equal(konly[..., :128], x[..., :128]) and np.array_equal(konly[..., 128:], full[..., 128:])
    assert not np.array_equal(full[:, 3:, :256], x[:, 3:, :256])
