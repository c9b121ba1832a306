"""CPU: the fp32 restatement of the SigLIP forward (tests/siglip_cases.forward: trunk without a class token, tanh GELU, unfolded
attention-pooling head) against transformers' SiglipVisionModel (tests/golden/siglip_golden.npz), `hf_siglip_to_weights` on that model's
state dict, and `load_encoder("siglip", ...)`."""
import os

import numpy as np
import pytest
import torch

from tests import siglip_cases as SC

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "siglip_golden.npz"))


@pytest.mark.parametrize("case", [SC.CASES[0], SC.CASES[2]], ids=lambda c: c[0])
def test_restatement_matches_hf_golden(case):
    """the tolerance of tests/test_clip_openai_converters.py for the same comparison"""
    key, cfg, w, hw, x = SC.build(case)
    assert cfg.tanh_gelu and not cfg.cls_token
    got = SC.forward(w, hw, cfg, x)
    exp = GOLD[key]
    assert got.shape == exp.shape == (x.shape[0], cfg.dim)
    assert np.max(np.abs(got - exp)) < 2e-4 * max(1.0, np.abs(exp).max())
    # the activation matters, if little: the erf form on the same weights is 6e-4 .. 1e-3 away (the forms differ by at most 4.7e-4 per
    # element, and the cases put the pre-activations where they do: siglip_cases.build)
    erf = SC.forward(w, hw, cfg, x[:2], tanh=False)
    d = float(np.linalg.norm(erf - exp[:2]) / np.linalg.norm(exp[:2]))
    print(f"{key}: erf GELU on the same weights differs by {d:.3e}")
    assert d > 4e-4 and np.max(np.abs(erf - exp[:2])) > 10 * np.max(np.abs(got - exp))


def test_golden_file_holds_the_three_cases():
    assert sorted(GOLD.files) == sorted(c[0] for c in SC.CASES)
    for key, _, _, _, batch in SC.CASES:
        assert GOLD[key].dtype == np.float32 and GOLD[key].shape[0] == batch == 5 and np.isfinite(GOLD[key]).all()


def test_hf_siglip_converter_round_trips_the_model():
    """the state dict of the transformers model itself -> the seeded weights exactly, and the model under those weights computes the
    golden; the SiglipModel layout (`vision_model.` prefix, text tower and logit scale beside it) gives the same"""
    from ibloc_amd.utils import embeddings as E
    key, cfg, w, hw, x = SC.build(SC.CASES[0])
    m = SC.hf_siglip_model(cfg, w, hw)
    assert m.config.hidden_act == "gelu_pytorch_tanh"
    sd = m.state_dict()
    got, ghw = E.hf_siglip_to_weights(sd, cfg.depth)
    assert set(got) == set(w) and set(ghw) == set(hw)
    for k in w:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], w[k]), k
    for k in hw:
        assert ghw[k].dtype == np.float32 and ghw[k].shape == hw[k].shape and np.array_equal(ghw[k], hw[k]), k
    with torch.no_grad():
        y = m(pixel_values=torch.from_numpy(x)).pooler_output.numpy()
    assert np.max(np.abs(y - GOLD[key])) < 2e-5 * max(1.0, np.abs(GOLD[key]).max())
    for prefix in ("", "vision_model."):
        sd2 = SC.hf_siglip_state_dict(cfg, w, hw, prefix=prefix)
        sd2["text_model.embeddings.token_embedding.weight"] = torch.zeros(4, 4)
        sd2["logit_scale"], sd2["logit_bias"] = torch.zeros(1), torch.zeros(1)
        got2, ghw2 = E.hf_siglip_to_weights(sd2, cfg.depth)
        assert all(np.array_equal(got2[k], w[k]) for k in w) and all(np.array_equal(ghw2[k], hw[k]) for k in hw)


def test_load_encoder_builds_the_siglip_encoder(monkeypatch):
    from ibloc_amd import siglip as S
    from ibloc_amd import vit as V
    from ibloc_amd.utils import embeddings as E
    key, cfg, w, hw, x = SC.build(SC.CASES[0])
    seen = []

    class FakeEncoder:
        def __init__(self, cfg_, trunk, head, device="cuda"):
            seen.append((cfg_, trunk, head))

        def embed(self, crops):
            return torch.arange(6.0).reshape(len(crops), -1)

    monkeypatch.setattr(S, "SiglipEncoder", FakeEncoder)
    monkeypatch.setattr(E, "_ENCODERS", {})
    enc = E.load_encoder("siglip", SC.hf_siglip_state_dict(cfg, w, hw, prefix="vision_model."), cfg="tiny_siglip")
    assert E._ENCODERS["siglip"] is enc and len(seen) == 1
    c, tw, th = seen[0]
    assert c is V.CONFIGS["tiny_siglip"] and all(np.array_equal(tw[k], w[k]) for k in w) and all(np.array_equal(th[k], hw[k]) for k in hw)
    # the facade hands the crop over as the other three do and returns the row un-normalised
    out = E.get_all_siglip_embeddings(current_obj_grounded_img=np.zeros((8, 8, 3), np.uint8))
    assert out.shape == (6,) and float(out[5]) == 5.0
    # without a cfg: the base model at 224 px (its depth is what the converter is asked for)
    with pytest.raises(KeyError):
        E.load_encoder("siglip", SC.hf_siglip_state_dict(cfg, w, hw))
