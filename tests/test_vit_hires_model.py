"""CPU: the fp32 restatements of the encoder forward (oracle/vit_oracle.py; tests/clip_openai_cases.forward for QuickGELU) reproduce
transformers' Dinov2Model at 518 px (1 370 tokens) and CLIPVisionModelWithProjection(hidden_act="quick_gelu") at 336 px (577 tokens)
-- tests/golden/vit_hires_golden.npz -- to the tolerance of tests/test_oracle_vit.py."""
import os

import numpy as np
import pytest

from tests import vit_hires_cases as HC

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "vit_hires_golden.npz"))


@pytest.mark.parametrize("case", HC.CASES, ids=lambda c: c[0])
def test_forward_matches_hf_golden(case):
    key, cfg, w, x = HC.build(case)
    assert cfg.n_tokens > 272 and cfg.grid == cfg.pos_grid
    got = HC.oracle_forward(w, cfg, x)
    exp = GOLD[key]
    assert got.shape == exp.shape
    assert np.max(np.abs(got - exp)) < 2e-4 * max(1.0, np.abs(exp).max())
