#!/usr/bin/env python3
"""Golden vectors of the high-resolution encoder cases (tests/vit_hires_cases.py): transformers' Dinov2Model at 518 px and
CLIPVisionModelWithProjection(hidden_act="quick_gelu") at 336 px, patch 14, built from local configs with the seeded random weights of
ibloc_amd.vit.random_weights (tools/gen_golden_vit.py says why the reference's own loader cannot run offline).  Only outputs are
stored.  Output: tests/golden/vit_hires_golden.npz"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_vit import hf_dinov2  # noqa: E402
from tests import clip_openai_cases as CQ  # noqa: E402
from tests import vit_hires_cases as HC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vit_hires_golden.npz")


def main():
    out = {}
    with torch.no_grad():
        for case in HC.CASES:
            key, cfg, w, x = HC.build(case)
            if cfg.quick_gelu:
                m = CQ.hf_clip_model(cfg, w)
                y = m(pixel_values=torch.from_numpy(x)).image_embeds.numpy()
            else:
                y = hf_dinov2(cfg, w)(torch.from_numpy(x)).numpy()
            out[key] = y.astype(np.float32)
            print(key, cfg.n_tokens, y.shape, float(np.abs(y).mean()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
