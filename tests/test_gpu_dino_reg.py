"""-m gpu: the register / rotary encoders end to end (csrc/vit.hip with ibl_vit_desc.n_registers and ibl_vit_weights.rope_table).

1. The prefix rows: with n_blocks_run = 0 the residual stream holds cls_pos and the registers bit for bit, and the patch rows of the same
   model without registers, shifted by R rows; n_registers = 0 without a table gives the bytes the forward gave before the field existed
   (tests/golden/dino_reg_parent_bytes.npz, recorded on the parent build by tools/gen_golden_dino_reg_parent.py).
2. The forward of every golden case of tests/dino_reg_cases.py against transformers (tests/golden/dino_reg_golden.npz) under the plain,
   the default and the p2;*:3333 plan; the class rows of an all-token run are those of the class-only run bit for bit.
3. SURVEY 8d's 1e-3 gate on u8 crops for the checkpoint configurations under the plan each is given (all but dinov3_vitl16, which no plan
   brings under it).
4. load_encoder / embed_batch / get_all_dinov3_embeddings against the encoder itself; the recipe `dinov3` bit-exact against PIL."""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from tests import dino_reg_cases as DC
from tests.test_gpu_flip_rate import GpuCrops

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
GOLD = np.load(os.path.join(HERE, "golden", "dino_reg_golden.npz"))
PARENT = np.load(os.path.join(HERE, "golden", "dino_reg_parent_bytes.npz"))
IDS = [c[0] for c in DC.CASES]
PLANS = [("plain", "plain"), (None, "default"), ("p2;*:3333", "p2-3333")]


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def cosine(a, b):
    return float(np.min(np.sum(a * b, -1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))))


@functools.lru_cache(maxsize=None)
def _case(i):
    return DC.build(DC.CASES[i])


# ---- 1. prefix rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_dino_reg", "tiny_dinov3"])
def test_prefix_rows_and_shifted_patch_rows(name):
    from ibloc_amd import vit as V
    cfg = dataclasses.replace(V.CONFIGS[name], n_blocks_run=0)
    w = DC.seeded_weights(cfg, 9)
    x = np.random.default_rng(10).normal(size=(3, 3, cfg.img_h, cfg.img_w)).astype(np.float32)
    enc = V.VitEncoder(cfg, w)
    assert enc.desc.n_registers == 4 and bool(enc.W.reg_tokens) and bool(enc.W.rope_table) == (cfg.rope_theta is not None)
    _, taps = enc.forward_patches(enc.patches_from_pixels(torch.from_numpy(x)), taps=True)
    X = taps["x"].cpu().numpy()
    assert X.shape == (3, cfg.n_tokens, cfg.dim)
    pos0 = V.interpolate_pos_embed(w["pos"], cfg)[0] if cfg.rope_theta is None else np.zeros(cfg.dim, np.float32)
    for b in range(3):
        assert np.array_equal(X[b, 0].view(np.int32), (w["cls"] + pos0).astype(np.float32).view(np.int32))
        assert np.array_equal(X[b, 1:5].view(np.int32), w["reg"].view(np.int32))
    plain_cfg = dataclasses.replace(cfg, n_registers=0)
    plain = V.VitEncoder(plain_cfg, {k: v for k, v in w.items() if k != "reg"})
    assert plain.desc.n_registers == 0 and plain.desc.n_tokens == cfg.n_tokens - 4 and not plain.W.reg_tokens
    _, taps0 = plain.forward_patches(plain.patches_from_pixels(torch.from_numpy(x)), taps=True)
    X0 = taps0["x"].cpu().numpy()
    assert np.array_equal(X0[:, 0].view(np.int32), X[:, 0].view(np.int32)) and np.array_equal(X0[:, 1:].view(np.int32), X[:, 5:].view(np.int32))


def test_registers_with_no_cls_and_bad_counts_are_refused():
    import ctypes as C
    from ibloc_amd import _lib
    from ibloc_amd import vit as V
    cfg = V.CONFIGS["tiny_dino_reg"]
    enc = V.VitEncoder(cfg, DC.seeded_weights(cfg, 9))
    patches = torch.zeros((cfg.n_patches, cfg.patch_k_pad), dtype=torch.float16, device="cuda")
    out = torch.full((1, cfg.dim), 7.0, device="cuda")
    ws = torch.zeros(_lib.lib.ibl_vit_workspace_bytes(C.byref(enc.desc), 1), dtype=torch.uint8, device="cuda")
    for field, value in (("flags", enc.desc.flags | V.FLAG_NO_CLS | V.FLAG_OUT_ALL_TOKENS), ("n_registers", -1), ("n_registers", cfg.n_tokens - 1)):
        d = V.VitDesc.from_buffer_copy(enc.desc)
        setattr(d, field, value)
        st = _lib.lib.ibl_vit_forward(C.byref(d), C.byref(enc.W), patches.data_ptr(), 1, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream)
        assert st < 0, (field, value)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(ws.any()), "a refused forward launched something"


@pytest.mark.parametrize("plan", ["plain", "default"])
def test_no_registers_no_table_is_the_parents_forward(plan):
    """tiny_dino through VitEncoder: the bytes recorded on the build before ibl_vit_desc.n_registers existed"""
    from ibloc_amd import vit as V
    cfg = V.CONFIGS["tiny_dino"]
    enc = V.VitEncoder(cfg, V.random_weights(cfg, 41), precision=None if plan == "default" else plan)
    assert enc.desc.n_registers == 0 and not enc.W.reg_tokens and not enc.W.rope_table
    x = np.random.default_rng(42).normal(size=(3, 3, cfg.img_h, cfg.img_w)).astype(np.float32)
    got = enc.forward_patches(enc.patches_from_pixels(torch.from_numpy(x))).cpu().numpy()
    assert np.array_equal(got.view(np.int32), PARENT[plan].view(np.int32))


# ---- 2. forward against the golden ------------------------------------------------------------------------------------------------------------
def _plan_without_last_block(plan, depth):
    """the plan the class-only run executes: its last block stays plain (ibloc_amd.vit), so an all-token run is given the same plan with
    that block's entry taken out, "*" spelled out for the blocks before it"""
    from ibloc_amd import vit as V
    if plan == "plain":
        return plan
    patch, layers = V.parse_precision(plan)
    out = [f"p{patch}"]
    for l in range(depth - 1):
        t = layers.get(l, layers.get("*"))
        if t:
            out.append(f"{l}:" + "".join(str(v) for v in t))
    return ";".join(out)


@pytest.mark.parametrize("plan", [p for p, _ in PLANS], ids=[n for _, n in PLANS])
@pytest.mark.parametrize("i", range(len(DC.CASES)), ids=IDS)
def test_forward_vs_hf_golden(i, plan):
    """the gate of tests/test_gpu_vit.py: rel-L2 <= 2e-3 and cosine >= 0.99999, batches 1 and all.  tests/test_dino_reg_model.py shows that
    a forward without the register rows or without the rotation is 5e-3 .. 1e-1 from the golden"""
    from ibloc_amd import vit as V
    key, cfg, w, x = _case(i)
    enc = V.VitEncoder(cfg, w, precision=plan)
    assert enc.desc.n_registers == 4 and bool(enc.W.rope_table) == (cfg.rope_theta is not None)
    exp = GOLD[key]
    for batch in (1, x.shape[0]):
        got = enc.forward_patches(enc.patches_from_pixels(torch.from_numpy(x[:batch]))).cpu().numpy()
        r, c = rel_l2(got, exp[:batch]), cosine(got, exp[:batch])
        print(f"{key} plan {enc.precision} batch {batch}: rel_l2={r:.3e} cos={c:.6f}")
        assert np.isfinite(got).all() and got.shape == (batch, cfg.dim)
        assert r <= 2e-3 and c >= 0.99999
    # every token asked for: the class rows are the class-only run's, bit for bit (same plan in the blocks both run on every row)
    all_cfg = dataclasses.replace(cfg, out_all_tokens=True)
    all_enc = V.VitEncoder(all_cfg, w, precision=_plan_without_last_block(enc.precision, cfg.depth))
    tok = all_enc.forward_patches(all_enc.patches_from_pixels(torch.from_numpy(x))).cpu().numpy()
    assert tok.shape == (x.shape[0], cfg.n_tokens, cfg.dim) and np.isfinite(tok).all()
    assert np.array_equal(tok[:, 0].view(np.int32), got.view(np.int32))
    if key.startswith("tiny"):
        ref = DC.forward(w, cfg, x, all_tokens=True)
        r = rel_l2(tok, ref)
        print(f"{key} plan {enc.precision}: every token vs the fp32 restatement rel_l2={r:.3e}")
        assert r <= 2e-3


def test_the_long_cases_stream_their_keys():
    from ibloc_amd import vit as V
    assert V.CONFIGS["tiny_dino_reg_518"].n_tokens == 1374 > 272 and V.CONFIGS["tiny_dinov3_384"].n_tokens == 581 > 272
    assert {"tiny_dino_reg_518", "tiny_dinov3_384"} <= set(IDS)


# ---- 3. the 1e-3 gate -------------------------------------------------------------------------------------------------------------------------
def embed_both(enc, wt, cfg, crops_u8, batch):
    """both sides start from the same resized u8 image; the restatement runs in torch fp32 on the device"""
    mean = torch.tensor(enc.recipe.mean, dtype=torch.float32, device="cuda")
    std = torch.tensor(enc.recipe.std, dtype=torch.float32, device="cuda")
    hip, ora = [], []
    for i in range(0, len(crops_u8), batch):
        patches, img = enc.preprocess(crops_u8[i:i + batch], want_u8=True)
        hip.append(enc.forward_patches(patches).cpu().numpy())
        x = (((img.to(torch.float64) * (1 / 255)).to(torch.float32) - mean) / std).permute(0, 3, 1, 2).contiguous()
        ora.append(DC.forward(wt, cfg, x, device="cuda"))
    return np.concatenate(hip), np.concatenate(ora)


def gate_weights(cfg):
    w = DC.seeded_weights(cfg, DC.GATE_WEIGHT_SEED)
    return w, {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).cuda() for k, v in w.items()}


GATE = {"dinov2_vits14_reg": (224, 224), "dinov2_vitb14_reg": (224, 224), "dinov2_vitl14_reg": (224, 224), "dinov2_vitb14_reg_518": (32, 16),
        "dinov3_vits16": (224, 224), "dinov3_vitb16": (224, 224)}      # model -> (crops, batch)
# dinov3_vitl16 meets the gate under no plan up to p2;*:3333 (default 1.57e-3 mean / 2.06e-3 max, p2;*:3333 1.21e-3 / 1.83e-3 over these 224
# crops: DESIGN.md (c)), so it ships without the assertion; tools/perf_dino_reg.py measures it with the others
UNGATED = {"dinov3_vitl16": (224, 224)}


@pytest.mark.parametrize("name", list(GATE))
def test_embedding_gate_on_u8_crops(name):
    """every crop < 1e-3 and the mean < 0.85e-3 against the fp32 restatement on the device, under the plan MODEL_PRECISION gives the
    configuration (DESIGN.md (c) lists every plan that was measured)"""
    from ibloc_amd import vit as V
    cfg = V.CONFIGS[name]
    n_crops, batch = GATE[name]
    w, wt = gate_weights(cfg)
    enc = V.VitEncoder(cfg, w)
    assert enc.precision == V.MODEL_PRECISION.get(name, V.DEFAULT_PRECISION) or "IBL_VIT_PREC" in os.environ
    ids = np.random.default_rng(3).integers(0, 100000, size=n_crops)
    hip, ora = embed_both(enc, wt, cfg, GpuCrops(21).variants(ids), batch)
    rel = np.linalg.norm(hip - ora, axis=1) / np.linalg.norm(ora, axis=1)
    print(f"[gate {name}] precision plan {enc.precision}: embedding rel-L2 mean {rel.mean():.2e} max {rel.max():.2e} over {rel.size} crops")
    assert rel.max() < 1e-3 and rel.mean() < 0.85e-3


# ---- 4. facades and the recipe ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name,getter", [("dinov3", "tiny_dinov3", "get_all_dinov3_embeddings"), ("dino", "tiny_dino_reg", "get_all_dino_embeddings")])
def test_load_encoder_and_embed_batch_are_the_encoder(kind, name, getter):
    from ibloc_amd import vit as V
    from ibloc_amd.utils import embeddings as E
    cfg = V.CONFIGS[name]
    w = DC.seeded_weights(cfg, 12)
    enc = V.VitEncoder(cfg, w)
    rng = np.random.default_rng(5)
    crops = [rng.integers(0, 256, size=(h, ww, 3), dtype=np.uint8) for h, ww in [(120, 90), (224, 224), (60, 200), (300, 310), (50, 50)]]
    direct = enc.embed(crops)
    assert direct.shape == (5, cfg.dim) and bool(torch.isfinite(direct).all())
    old = dict(E._ENCODERS)
    try:
        loaded = E.load_encoder(kind, DC.hf_state_dict(cfg, w), cfg=name)
        assert isinstance(loaded, V.VitEncoder) and loaded.desc.n_registers == 4
        assert torch.equal(E.embed_batch(kind, crops), direct)
        assert torch.equal(getattr(E, getter)(current_obj_grounded_img=crops[2]), enc.embed(crops[2:3])[0])
    finally:
        E._ENCODERS.clear()
        E._ENCODERS.update(old)
    assert torch.equal(enc.embed(crops, max_batch=2), direct)


@pytest.mark.parametrize("px", (224, 384))
def test_dinov3_recipe_is_bit_exact_against_pil(px):
    """exact resize to the model size with PIL's bilinear tables, no crop, ImageNet mean / std"""
    from PIL import Image
    from ibloc_amd import preprocess as pp
    from ibloc_amd import vit as V
    cfg = V.CONFIGS["tiny_dinov3" if px == 224 else "tiny_dinov3_384"]
    enc = V.VitEncoder(cfg, DC.seeded_weights(cfg, 1))
    r = enc.recipe
    assert (r.out_h, r.out_w, r.resize_mode, r.filt, r.mean, r.std) == (px, px, "exact", pp.BILINEAR, pp.IMAGENET_MEAN, pp.IMAGENET_STD)
    rng = np.random.default_rng(px)
    crops = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in [(120, 90), (px, px), (60, 500), (700, 333), (px + 1, px - 1), (17, 23)]]
    patches, img = enc.preprocess(crops, want_u8=True)
    img = img.cpu().numpy()
    for k, c in enumerate(crops):
        ref = np.asarray(Image.fromarray(c[:, :, ::-1].copy()).resize((px, px), Image.BILINEAR))     # the swap the other recipes apply
        assert np.array_equal(img[k], ref), (px, c.shape)
    mean, std = torch.tensor(r.mean), torch.tensor(r.std)
    t = ((torch.from_numpy(img[:1].astype(np.float32) / 255.0) - mean) / std).permute(0, 3, 1, 2)
    want = enc.patches_from_pixels(t)
    assert float((patches[:cfg.n_patches].float() - want.float()).abs().max()) <= 4e-3
