"""CPU: the bound tests/test_gpu_attention_long.py holds `ibl_attention_stream_kernel` to is reachable by its arithmetic -- a numpy
emulation of the online softmax (tests/attention_long_cases.py::emulate_stream, chunks of 128 keys as the kernel's) stays within 0.8 of
the project's attention bound (tests/attention_cases.py::bound, unchanged) against the float64 reference on every case and family; the
remaining fifth is for what the emulation does not reproduce, the device's exp2 and the MFMA accumulation order.

Worst ratio error / bound of the emulation over all cases: the six families of the resident kernel 0.73 (ramp, T = 1025), the
staircases 0.39 (0.26 beyond 272 tokens); three-term rows (a + lo / 64 against the bound with
2^-21 |ref|) 0.70.  Also here, because they are decided before any launch: the argument checks of `ibl_attention_stream_f16`; and
the new high-resolution configurations."""
import numpy as np
import pytest

from tests import attention_long_cases as LC


@pytest.mark.parametrize("family", LC.LONG_FAMILIES)
def test_stream_emulation_within_bound(family):
    worst, worst3, at = 0.0, 0.0, None
    for (T, H, B) in LC.CASES:
        c, ref, A, plain, bnd, bnd3 = LC.case(family, T, H, B)
        a, value = LC.emulate_stream(c["q"], c["k"], c["v"], LC.KV)
        assert np.isfinite(value).all()
        r = float((np.abs(a.astype(np.float64) - ref) / bnd).max()) if T > 1 else 0.0
        if r > worst:
            worst, at = r, (T, H, B)
        _, lo = LC.split_terms(a, value)
        worst3 = max(worst3, float((np.abs(a.astype(np.float64) + lo.astype(np.float64) / LC.SPLIT - ref) / bnd3).max()))
        if T == 1:       # one key: the result is v itself, exactly
            assert np.array_equal(a, c["v"])
        if family in LC.LONG_DECISIVE and T > 272:
            # not vacuous: the plain mean of v (a kernel that ignored the logits) misses the bound at least 50-fold somewhere, and on
            # most elements by a wide margin
            miss = np.abs(plain - ref) / bnd
            assert miss.max() >= 50.0 and np.median(miss) >= 10.0, (T, miss.max(), np.median(miss))
    print(f"streaming attention emulation vs fp64, {family}: worst error / bound {worst:.3f} at {at}, three-term {worst3:.3f}")
    assert worst <= 0.8, (family, at, worst)
    assert worst3 <= 0.8, (family, worst3)


@pytest.mark.parametrize("chunk", (32, 64))
def test_bound_does_not_hinge_on_the_chunk(chunk):
    """other chunk sizes of the same arithmetic stay within the same 0.8 at the longest row"""
    for family in ("ramp", "stair_up"):
        c, ref, A, _, bnd, _ = LC.case(family, 1025, 2, 1)
        a, _ = LC.emulate_stream(c["q"], c["k"], c["v"], chunk)
        assert float((np.abs(a.astype(np.float64) - ref) / bnd).max()) <= 0.8


def test_staircases_rescale_at_every_chunk():
    for family, rising in (("stair_up", True), ("stair_down", False)):
        c = LC.make_long(family, 577, 2, 1)
        s = np.einsum("bhqd,bhkd->bhqk", c["q"].astype(np.float64), c["k"].astype(np.float64)) / 8.0
        cm = np.stack([s[..., k0:k0 + LC.KV].max(axis=-1) for k0 in range(0, 577, LC.KV)], axis=-1)      # maximum of every chunk
        d = np.diff(cm, axis=-1)
        # (the last chunk of 577 keys holds one key, a single half-logit step above the chunk before it)
        assert (d > 0.25).all() if rising else (d < -0.25).all()


def test_entry_refuses_before_touching_the_device():
    """the argument checks of ibl_attention_stream_f16 come before any launch: no GPU needed, the pointers are never followed"""
    from ibloc_amd import _lib
    call, P = _lib.lib.ibl_attention_stream_f16, 0x10000
    assert call(P, P, 1, LC.MAX_TOKENS + 1, 128, 2, 0, 1, None) < 0 and b"8192" in _lib.lib.ibl_last_error()
    assert call(P, P, 2, 577, 128, 3, 0, 1, None) < 0            # dim != 64 * heads
    assert call(P, P, 2, 577, 128, 2, 0, 0, None) < 0 and call(P, P, 2, 577, 128, 2, 0, 4, None) < 0
    assert call(P, P, 2, 577, 128, 2, 2, 1, None) < 0            # cls_only is 0 or 1
    assert call(None, P, 2, 577, 128, 2, 0, 1, None) < 0 and b"null" in _lib.lib.ibl_last_error()
    assert call(P, None, 2, 577, 128, 2, 0, 1, None) < 0
    assert call(P, P, -1, 577, 128, 2, 0, 1, None) < 0 and call(P, P, 2, -1, 128, 2, 0, 1, None) < 0
    assert call(P + 2, P, 2, 577, 128, 2, 0, 1, None) < 0 and call(P, P + 4, 2, 577, 128, 2, 0, 1, None) < 0
    assert call(P, P, 0, 577, 128, 2, 0, 1, None) == 0 and call(P, P, 2, 0, 128, 2, 0, 1, None) == 0


def test_resident_entry_keeps_its_limit():
    from ibloc_amd import _lib
    assert _lib.lib.ibl_attention_f16(0x10000, 0x10000, 1, 273, 128, 2, 0, 1, None) < 0


@pytest.mark.parametrize("name,tokens,pos_grid", (("clip_l14_336_openai", 577, (24, 24)), ("dinov2_vitb14_448", 1025, (37, 37)),
                                                  ("dinov2_vitb14_518", 1370, (37, 37)), ("tiny_dino_518", 1370, (37, 37))))
def test_high_resolution_configurations(name, tokens, pos_grid):
    from ibloc_amd import preprocess as pp, vit as V
    cfg = V.CONFIGS[name]
    assert cfg.name == name and cfg.n_tokens == tokens and cfg.pos_grid == pos_grid
    assert cfg.dim == 64 * cfg.heads and cfg.depth <= V.MAX_LAYERS
    patch, layers = V.parse_precision(V.MODEL_PRECISION.get(name, V.DEFAULT_PRECISION))
    assert patch in (1, 2) and all(l == "*" or 0 <= l < V.MAX_LAYERS for l in layers)
    r = pp.RECIPES[cfg.recipe]
    assert (r.out_h, r.out_w) == (cfg.img_h, cfg.img_w) and r.resize_mode == "shortest" and r.shortest >= cfg.img_h
    if name.startswith("dinov2") or name == "tiny_dino_518":
        assert r.shortest * 224 == r.out_h * 256 and r.crop_rounding == "floor"       # the HF processor's 256 / 224
    else:
        assert r.shortest == 336 and r.crop_rounding == "round"
    if name in ("clip_l14_336_openai", "dinov2_vitb14_518"):
        pos = np.arange(tokens * 4, dtype=np.float32).reshape(tokens, 4)
        assert cfg.grid == cfg.pos_grid and V.interpolate_pos_embed(pos, cfg) is not None
        assert np.array_equal(V.interpolate_pos_embed(pos, cfg), pos)                 # the stored table, as stored
