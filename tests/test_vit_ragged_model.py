"""CPU: native-aspect crops without a GPU -- the grid rule `native_grid`, the position table of a non-square grid against the one
transformers' Dinov2Model / Dinov2WithRegistersModel add to their patch embeddings, the fp32 restatement of a crop at its own grid
against the live models and the committed golden, and the token-budget chunker of `VitEncoder.embed_native`."""
import functools
import os

import numpy as np
import pytest
import torch

from ibloc_amd import vit as V
from tests import vit_ragged_cases as RC

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "vit_ragged_golden.npz"))


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_native_grid_examples():
    assert V.native_grid(480, 160, 14, 256) == (27, 9)
    assert V.native_grid(40, 60, 14, 256) == (13, 19)
    assert V.native_grid(40, 60, 14, 256, upscale=False) == (2, 4)
    assert V.native_grid(10000, 10, 14, 256) == (256, 1)
    with pytest.raises(ValueError):
        V.native_grid(0, 10, 14, 256)


def test_native_grid_properties():
    """a seeded sweep of shapes from 1 px to 4 000 px, patches 14 / 16 / 32, budgets 1 .. 1 369"""
    rng = np.random.default_rng(5)
    fill = []
    for _ in range(20000):
        h, w = (int(v) for v in np.exp(rng.uniform(0, np.log(4000), size=2)))
        patch, budget = int(rng.choice([14, 16, 32])), int(rng.choice([1, 16, 49, 196, 256, 576, 1369]))
        gh, gw = V.native_grid(h, w, patch, budget)
        assert 1 <= gh and 1 <= gw and gh * gw <= budget, (h, w, patch, budget, gh, gw)
        assert (gh, gw) == V.native_grid(h, w, patch, budget), "not deterministic"
        nh, nw = V.native_grid(h, w, patch, budget, upscale=False)
        assert 1 <= nh <= max(1, h // patch) and 1 <= nw <= max(1, w // patch) and nh * nw <= budget, (h, w, patch, budget, nh, nw)
        assert nh <= gh and nw <= gw
        if budget == 256 and max(h, w) <= 8 * min(h, w):
            fill.append(gh * gw / budget)
    print(f"native_grid: median fill of a 256-patch budget {np.median(fill):.3f} over {len(fill)} shapes up to 8 : 1")
    assert np.median(fill) >= 0.9
    for budget, g in ((16, 4), (256, 16), (1369, 37)):
        for side in (1, 7, 13, 14, 100, 224, 518, 3001):
            assert V.native_grid(side, side, 14, budget) == (g, g), (side, budget)


@pytest.mark.parametrize("name", ("tiny_dino", "tiny_dino_reg"))
@pytest.mark.parametrize("grid", ((3, 7), (1, 1), (20, 9)))
def test_grid_position_table_is_the_models(name, grid):
    """the table the ragged forward adds at `grid` (plain: "size", registers: "size-aa") against the model's interpolate_pos_encoding:
    <= 1 fp32 ulp"""
    cfg = RC.config(name)
    w = V.random_weights(cfg, 3)
    gh, gw = grid
    emb = RC.hf_model(cfg, w).embeddings
    with torch.no_grad():
        want = emb.interpolate_pos_encoding(torch.zeros(1, 1 + gh * gw, cfg.dim), gh * cfg.patch, gw * cfg.patch)[0].numpy()
    got = V.interpolate_pos_embed(w["pos"], RC.at_grid(cfg, grid))
    assert got.shape == want.shape == (1 + gh * gw, cfg.dim)
    ulp = np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(np.abs(want), np.float32(2.0 ** -100)))
    print(f"{name} {gh} x {gw}: worst {ulp.max():.2f} ulp")
    assert ulp.max() <= 1.0
    if grid != (1, 1):
        assert rel_l2(V.interpolate_pos_embed(w["pos"], RC.at_grid(cfg, grid[::-1]))[1:], want[1:]) > 1e-2, "the transposed grid's table"


@functools.lru_cache(maxsize=None)
def _case(i):
    return RC.build(RC.CASES[i])


@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=[c[0] for c in RC.CASES])
def test_restatement_at_each_grid_vs_transformers_and_golden(i):
    """rel-L2 <= 2e-4 per crop (what the other restatements are held to), against the live model fed the non-square pixels as they are
    and against the committed golden; the regenerated pixels are the generator's"""
    key, cfg, w, xs = _case(i)
    model = RC.hf_model(cfg, w)
    assert GOLD[key].shape == (len(RC.GRIDS), cfg.dim)
    for j, (grid, x) in enumerate(zip(RC.GRIDS, xs)):
        assert np.array_equal(x.reshape(-1)[:RC.PROBE], GOLD[key + ".pixels"][j])
        got = RC.restate(cfg, w, x)
        r_hf, r_gold = rel_l2(got, RC.hf_embed(model, x)), rel_l2(got, GOLD[key][j])
        print(f"{key} grid {grid}: restatement vs transformers {r_hf:.3e}, vs golden {r_gold:.3e}")
        assert r_hf <= 2e-4 and r_gold <= 2e-4, (key, grid)


def test_token_chunks_keep_order_and_budget():
    rng = np.random.default_rng(9)
    for _ in range(200):
        tokens = [int(t) for t in rng.integers(2, 300, size=int(rng.integers(1, 40)))]
        budget = int(rng.integers(100, 2000))
        chunks = V.token_chunks(tokens, budget)
        assert [i for sl in chunks for i in range(sl.start, sl.stop)] == list(range(len(tokens))), "order or coverage"
        for sl in chunks:
            n = sum(tokens[sl])
            assert sl.stop > sl.start and (n <= budget or sl.stop - sl.start == 1), (tokens, budget, sl)
        for a, b in zip(chunks, chunks[1:]):        # greedy: the next crop did not fit
            assert sum(tokens[a]) + tokens[b.start] > budget
    assert V.token_chunks([], 10) == []
    assert V.token_chunks([50, 3, 3, 50, 2], 10) == [slice(0, 1), slice(1, 3), slice(3, 4), slice(4, 5)]
