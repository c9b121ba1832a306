#!/usr/bin/env python3
"""Golden vectors for the register / rotary configurations (tests/dino_reg_cases.CASES): pooler_output of transformers'
Dinov2WithRegistersModel and DINOv3ViTModel holding the seeded random weights of ibloc_amd.vit.random_weights, on seeded N(0, 1) pixels.
Build container only (CPU).  Stored per case: the output, and the first PROBE pixel values -- the inputs themselves (up to 6 MB a case)
and the weights are regenerated from their seeds, the probe pins that the regenerated pixels are the generator's.
Output: tests/golden/dino_reg_golden.npz
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tests import dino_reg_cases as DC  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "dino_reg_golden.npz")


def main():
    out = {}
    with torch.no_grad():
        for case in DC.CASES:
            key, cfg, w, x = DC.build(case)
            y = DC.hf_model(cfg, w)(pixel_values=torch.from_numpy(x)).pooler_output.numpy()
            out[key] = y.astype(np.float32)
            out[key + ".pixels"] = x.reshape(-1)[:DC.PROBE].copy()
            print(key, y.shape, float(np.abs(y).mean()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
