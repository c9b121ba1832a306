#!/usr/bin/env python3
"""Golden vectors for the QuickGELU CLIP configurations (tiny_clip_q, clip_b32_openai): image_embeds of transformers'
CLIPVisionModelWithProjection(hidden_act="quick_gelu") holding the seeded random weights of ibloc_amd.vit.random_weights, on seeded
N(0, 1) pixels.  Build container only (CPU).  Only outputs are stored; weights and inputs are regenerated from their seeds
(tests/clip_openai_cases.py: CASES, build).  Output: tests/golden/clip_quickgelu_golden.npz
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tests import clip_openai_cases as QC  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "clip_quickgelu_golden.npz")


def main():
    out = {}
    with torch.no_grad():
        for case in QC.CASES:
            key, cfg, w, x = QC.build(case)
            m = QC.hf_clip_model(cfg, w)
            assert m.config.hidden_act == "quick_gelu"
            y = m(pixel_values=torch.from_numpy(x)).image_embeds.numpy()
            out[key] = y.astype(np.float32)
            print(key, y.shape, float(np.abs(y).mean()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
