"""CPU: the fp32 restatement with QuickGELU (tests/clip_openai_cases.forward) against transformers'
CLIPVisionModelWithProjection(hidden_act="quick_gelu") (tests/golden/clip_quickgelu_golden.npz), `hf_clip_to_weights` on that model's
state dict, and the converter `load_encoder("clip", ...)` picks from the key layout."""
import os

import numpy as np
import pytest
import torch

from tests import clip_openai_cases as QC

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "clip_quickgelu_golden.npz"))


@pytest.mark.parametrize("case", QC.CASES, ids=lambda c: c[0])
def test_restatement_matches_hf_golden(case):
    """the tolerance of tests/test_oracle_vit.py"""
    key, cfg, w, x = QC.build(case)
    assert cfg.quick_gelu
    got = QC.forward(w, cfg, x)
    exp = GOLD[key]
    assert got.shape == exp.shape
    assert np.max(np.abs(got - exp)) < 2e-4 * max(1.0, np.abs(exp).max())
    # and the activation matters: the erf form on the same weights is another function (1.5e-2 away on the 12-layer model; on the
    # two-block tiny one, whose pre-activations are small, only 1.3e-3 -- what tests/test_gpu_qgelu.py's forward test takes into account)
    import dataclasses
    erf = QC.forward(w, dataclasses.replace(cfg, quick_gelu=False), x[:2])
    d = float(np.linalg.norm(erf - exp[:2]) / np.linalg.norm(exp[:2]))
    print(f"{key}: erf GELU on the same weights differs by {d:.3e}")
    assert d > (1e-2 if key == "clip_b32_openai" else 1e-3)


def test_restatement_with_erf_is_the_oracle():
    """with quick_gelu off the helper is oracle/vit_oracle.vit_forward, bit for bit"""
    import dataclasses
    from oracle import vit_oracle as vo
    key, cfg, w, x = QC.build(QC.CASES[0])
    cfg = dataclasses.replace(cfg, quick_gelu=False)
    assert np.array_equal(QC.forward(w, cfg, x[:2]), vo.vit_forward(w, cfg, x[:2]))


def test_hf_clip_converter_round_trips_the_model():
    """the state dict of the transformers model itself (its own key names, position_ids buffer included) -> the seeded weights exactly,
    and the model under those weights computes the golden"""
    from ibloc_amd.utils import embeddings as E
    key, cfg, w, x = QC.build(QC.CASES[0])
    m = QC.hf_clip_model(cfg, w)
    assert m.config.hidden_act == "quick_gelu"
    sd = m.state_dict()
    assert E.clip_converter(sd) is E.hf_clip_to_weights
    got = E.hf_clip_to_weights(sd, cfg.depth)
    assert set(got) == set(w)
    for k in w:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], w[k]), k
    with torch.no_grad():
        y = m(pixel_values=torch.from_numpy(x)).image_embeds.numpy()
    assert np.max(np.abs(y - GOLD[key])) < 2e-5 * max(1.0, np.abs(GOLD[key]).max())
    # a CLIPModel state dict carries the text tower beside the same vision keys: ignored
    sd2 = dict(sd)
    sd2["text_model.embeddings.token_embedding.weight"] = torch.zeros(4, 4)
    sd2["logit_scale"] = torch.zeros(())
    got2 = E.hf_clip_to_weights(sd2, cfg.depth)
    assert all(np.array_equal(got2[k], w[k]) for k in w)


def _open_clip_sd(w, depth):
    """the seeded weights under open_clip's / OpenAI's `model.visual` names (tests/test_converters.py does the same from a transformers model)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    sd = {"conv1.weight": t(w["patch.w"]), "class_embedding": t(w["cls"]), "positional_embedding": t(w["pos"]),
          "ln_pre.weight": t(w["ln_pre.g"]), "ln_pre.bias": t(w["ln_pre.b"]), "ln_post.weight": t(w["ln_f.g"]),
          "ln_post.bias": t(w["ln_f.b"]), "proj": t(w["proj.w"].T)}
    for l in range(depth):
        p, q = f"transformer.resblocks.{l}.", f"l{l}."
        sd[p + "ln_1.weight"], sd[p + "ln_1.bias"] = t(w[q + "ln1.g"]), t(w[q + "ln1.b"])
        sd[p + "ln_2.weight"], sd[p + "ln_2.bias"] = t(w[q + "ln2.g"]), t(w[q + "ln2.b"])
        sd[p + "attn.in_proj_weight"] = t(np.concatenate([w[q + n + ".w"] for n in "qkv"], axis=0))
        sd[p + "attn.in_proj_bias"] = t(np.concatenate([w[q + n + ".b"] for n in "qkv"], axis=0))
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = t(w[q + "o.w"]), t(w[q + "o.b"])
        sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = t(w[q + "fc1.w"]), t(w[q + "fc1.b"])
        sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = t(w[q + "fc2.w"]), t(w[q + "fc2.b"])
    return sd


def test_load_encoder_picks_the_converter_from_the_key_layout(monkeypatch):
    """both layouts reach VitEncoder with the same weights and the caller's cfg (the activation is the cfg's: a state dict has none)"""
    from ibloc_amd import vit as V
    from ibloc_amd.utils import embeddings as E
    key, cfg, w, x = QC.build(QC.CASES[0])
    seen = []

    class FakeEncoder:
        def __init__(self, cfg_, weights, device="cuda"):
            seen.append((cfg_, weights))

    monkeypatch.setattr(V, "VitEncoder", FakeEncoder)
    monkeypatch.setattr(E, "_ENCODERS", {})
    hf, oc = QC.hf_clip_state_dict(cfg, w), _open_clip_sd(w, cfg.depth)
    assert E.clip_converter(hf) is E.hf_clip_to_weights and E.clip_converter(oc) is E.open_clip_visual_to_weights
    with pytest.raises(KeyError):
        E.clip_converter({"embeddings.cls_token": 0})
    for sd in (hf, oc):
        enc = E.load_encoder("clip", sd, cfg=cfg)
        assert E._ENCODERS["clip"] is enc
    assert len(seen) == 2
    for c, got in seen:
        assert c is cfg and c.quick_gelu and set(got) == set(w)
        assert all(np.array_equal(got[k], w[k]) for k in w)
    # without a cfg the kind's default stays the laion2b model: erf GELU
    assert E._KIND_TO_CONFIG["clip"] == "clip_b32" and not V.CONFIGS["clip_b32"].quick_gelu
