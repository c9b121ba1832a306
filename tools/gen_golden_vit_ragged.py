#!/usr/bin/env python3
"""Golden vectors for native-aspect crops (tests/vit_ragged_cases.CASES x GRIDS): pooler_output of transformers' Dinov2Model and
Dinov2WithRegistersModel holding the seeded random weights of ibloc_amd.vit.random_weights, on seeded N(0, 1) pixels of NON-SQUARE
shape -- the models resample their position table to the input's grid.  Build container only (CPU).  Stored per case: the embedding
of every grid, and the first PROBE pixel values of every crop -- inputs and weights are regenerated from their seeds, the probe pins
that the regenerated pixels are the generator's.
Output: tests/golden/vit_ragged_golden.npz
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tests import vit_ragged_cases as RC  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "vit_ragged_golden.npz")


def main():
    out = {}
    for case in RC.CASES:
        key, cfg, w, xs = RC.build(case)
        model = RC.hf_model(cfg, w)
        y = np.stack([RC.hf_embed(model, x) for x in xs]).astype(np.float32)
        out[key] = y
        out[key + ".pixels"] = np.stack([x.reshape(-1)[:RC.PROBE] for x in xs])
        print(key, y.shape, float(np.abs(y).mean()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
