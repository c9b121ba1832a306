#!/usr/bin/env python3
"""Golden vectors for the SigLIP configurations (tiny_siglip, tiny_siglip_384, siglip_b16_224): pooler_output of transformers'
SiglipVisionModel holding the seeded random weights of ibloc_amd.vit.random_weights / ibloc_amd.siglip.random_head_weights, on seeded
N(0, 1) pixels.  Build container only (CPU).  Only outputs are stored; weights and inputs are regenerated from their seeds
(tests/siglip_cases.py: CASES, build).  Output: tests/golden/siglip_golden.npz
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tests import siglip_cases as SC  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "siglip_golden.npz")


def main():
    out = {}
    with torch.no_grad():
        for case in SC.CASES:
            key, cfg, w, hw, x = SC.build(case)
            m = SC.hf_siglip_model(cfg, w, hw)
            assert m.config.hidden_act == "gelu_pytorch_tanh"
            y = m(pixel_values=torch.from_numpy(x)).pooler_output.numpy()
            out[key] = y.astype(np.float32)
            print(key, y.shape, float(np.abs(y).mean()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
