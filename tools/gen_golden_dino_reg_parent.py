#!/usr/bin/env python3
"""GPU, run on the commit BEFORE ibl_vit_desc.n_registers existed: the bytes of the tiny_dino forward through VitEncoder under the plain
and the default plan, which tests/test_gpu_dino_reg.py holds the forward with n_registers = 0 and no rotary table to.  Uses nothing the
earlier commit lacks.    python tools/gen_golden_dino_reg_parent.py OUT.npz    (committed as tests/golden/dino_reg_parent_bytes.npz)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ibloc_amd import vit as V  # noqa: E402


def main():
    cfg = V.CONFIGS["tiny_dino"]
    w = V.random_weights(cfg, 41)
    x = np.random.default_rng(42).normal(size=(3, 3, cfg.img_h, cfg.img_w)).astype(np.float32)
    out = {}
    for plan in ("plain", "default"):
        enc = V.VitEncoder(cfg, w, precision=None if plan == "default" else plan)
        out[plan] = enc.forward_patches(enc.patches_from_pixels(torch.from_numpy(x))).cpu().numpy()
        print(plan, enc.precision, out[plan].shape, float(np.abs(out[plan]).mean()))
    np.savez_compressed(sys.argv[1], **out)


if __name__ == "__main__":
    main()
