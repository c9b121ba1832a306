"""-m gpu: `ibl_vit_forward_ragged` -- the ViT forward over crops with different patch grids (native-aspect crops).

  1. equal grids beyond 272 tokens (where the fixed forward runs the streaming attention too): the ragged forward equals
     `forward_patches` bit for bit, class rows and every token, under three precision plans;
  2. a crop's embedding does not depend on the batch it runs in;
  3. every crop of a mixed batch against the fp32 restatement at its grid and against transformers' Dinov2Model /
     Dinov2WithRegistersModel on the non-square pixels (tests/golden/vit_ragged_golden.npz): rel-L2 <= 2e-3, cosine >= 0.99999 -- the
     tolerances of the golden cases on N(0, 1) pixels (tests/test_gpu_vit.py);
  4. SURVEY 8d's 1e-3 gate on u8 crops of 12 shapes at full size;
  5. the engine takes a NativeAspectEncoder as it takes an encoder;
  6. what has no position table for every grid is refused."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from tests import vit_ragged_cases as RC

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "vit_ragged_golden.npz"))


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def cosine(a, b):
    return float(np.sum(a * b) / (np.linalg.norm(a) * np.linalg.norm(b)))


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- 1. equal grids are the fixed forward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ("plain", None, "p2;*:3333"), ids=("plain", "default", "p2-3333"))
@pytest.mark.parametrize("all_tokens", (False, True), ids=("class-rows", "all-tokens"))
@pytest.mark.parametrize("name", ("tiny_dino_reg_518", "tiny_dino_518"))
def test_equal_grids_are_the_fixed_forward(name, all_tokens, plan):
    from ibloc_amd import vit as V
    cfg = dataclasses.replace(V.CONFIGS[name], out_all_tokens=all_tokens)
    assert cfg.n_tokens > 272
    enc = V.VitEncoder(cfg, V.random_weights(cfg, 31), precision=plan)
    x = np.random.default_rng(32).normal(size=(2, 3, cfg.img_h, cfg.img_w)).astype(np.float32)
    fixed = enc.forward_patches(enc.patches_from_pixels(torch.from_numpy(x))).cpu().numpy()
    ragged = enc.forward_ragged(enc.patches_from_pixels_ragged(list(torch.from_numpy(x))), [cfg.grid] * 2).cpu().numpy()
    assert np.isfinite(fixed).all()
    assert _same(ragged, fixed.reshape(ragged.shape)), f"{name} plan {enc.precision}: max |diff| {np.abs(ragged - fixed.reshape(ragged.shape)).max():.3e}"


# ---- 2. / 3. a mixed batch ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=range(len(RC.CASES)), ids=[c[0] for c in RC.CASES])
def mixed(request):
    from ibloc_amd import vit as V
    key, cfg, w, xs = RC.build(RC.CASES[request.param])
    enc = V.VitEncoder(cfg, w)
    xt = [torch.from_numpy(x) for x in xs]
    got = enc.forward_ragged(enc.patches_from_pixels_ragged(xt), list(RC.GRIDS)).cpu().numpy()
    return key, cfg, w, xs, xt, enc, got


def test_a_crop_does_not_depend_on_its_batch(mixed):
    key, cfg, w, xs, xt, enc, got = mixed
    assert got.shape == (len(RC.GRIDS), cfg.dim) and np.isfinite(got).all()
    for j, grid in enumerate(RC.GRIDS):
        alone = enc.forward_ragged(enc.patches_from_pixels_ragged([xt[j]]), [grid]).cpu().numpy()
        assert _same(alone[0], got[j]), f"{key}: crop {j} at grid {grid} alone != in the batch"
    back = enc.forward_ragged(enc.patches_from_pixels_ragged(xt[::-1]), list(RC.GRIDS)[::-1]).cpu().numpy()
    assert _same(back[::-1].copy(), got), "the reversed batch"
    # every token: a crop's rows are packed at its offsets, the class rows are the class-row run's
    all_cfg = dataclasses.replace(cfg, out_all_tokens=True)
    from ibloc_amd import vit as V
    all_enc = V.VitEncoder(all_cfg, w, precision="plain")
    tok = all_enc.forward_ragged(all_enc.patches_from_pixels_ragged(xt), list(RC.GRIDS)).cpu().numpy()
    seq = all_enc.seq_offsets(RC.GRIDS)
    assert tok.shape == (int(seq[-1]), cfg.dim) and np.isfinite(tok).all()
    plain = V.VitEncoder(cfg, w, precision="plain").forward_ragged(enc.patches_from_pixels_ragged(xt), list(RC.GRIDS)).cpu().numpy()
    assert _same(tok[seq[:-1]], plain), "class rows of the all-token run != the class-row run (plain plan)"


def test_mixed_batch_vs_restatement_and_golden(mixed):
    key, cfg, w, xs, xt, enc, got = mixed
    for j, (grid, x) in enumerate(zip(RC.GRIDS, xs)):
        assert np.array_equal(x.reshape(-1)[:RC.PROBE], GOLD[key + ".pixels"][j])
        ref = RC.restate(cfg, w, x)
        r, c, rg, cg = rel_l2(got[j], ref), cosine(got[j], ref), rel_l2(got[j], GOLD[key][j]), cosine(got[j], GOLD[key][j])
        print(f"{key} grid {grid} plan {enc.precision}: vs restatement rel_l2={r:.3e} cos={c:.7f}; vs transformers rel_l2={rg:.3e} cos={cg:.7f}")
        assert r <= 2e-3 and c >= 0.99999 and rg <= 2e-3 and cg >= 0.99999, (key, grid)


def test_a_forward_that_ignored_the_grid_fails_the_golden(mixed):
    """the same crop resized to the model's square input and run through the fixed forward lies far outside the tolerance"""
    key, cfg, w, xs, xt, enc, got = mixed
    for grid in ((3, 7), (27, 9)):
        j = RC.GRIDS.index(grid)
        sq = torch.nn.functional.interpolate(xt[j][None], size=(cfg.img_h, cfg.img_w), mode="bilinear", align_corners=False)
        at_square = enc.forward_patches(enc.patches_from_pixels(sq)).cpu().numpy()[0]
        r = rel_l2(at_square, GOLD[key][j])
        print(f"{key} grid {grid}: the crop at the square model grid is {r:.3e} from its native-aspect golden")
        assert r > 1e-2


# ---- 4. the 1e-3 gate at full size ----------------------------------------------------------------------------------------------------------
# 12 shapes cut from 224 x 224 crops, aspect ratios 1 : 4 .. 4 : 1
SHAPES = ((56, 224), (224, 56), (75, 224), (224, 75), (112, 224), (224, 112), (150, 224), (224, 150), (224, 224), (64, 128), (128, 64), (180, 200))


@pytest.mark.parametrize("name", ("dinov2_vitb14", "dinov2_vitb14_reg"))
def test_embedding_gate_on_u8_crops_of_12_shapes(name):
    """every crop < 1e-3 and the mean < 0.85e-3 against the fp32 restatement evaluated on the device per grid, both sides from the same
    resized u8 image, under the plan the encoder runs"""
    from ibloc_amd import vit as V
    from tests import dino_reg_cases as DC
    from tests.test_gpu_flip_rate import GpuCrops
    from oracle import vit_oracle as vo
    cfg = RC.config(name)
    w = DC.seeded_weights(cfg, DC.GATE_WEIGHT_SEED)
    wt = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).cuda() for k, v in w.items()}
    enc = V.VitEncoder(cfg, w)
    u8 = GpuCrops(21).variants(np.random.default_rng(3).integers(0, 100000, size=224)).cpu().numpy()
    crops = [np.ascontiguousarray(c[:SHAPES[i % 12][0], :SHAPES[i % 12][1]]) for i, c in enumerate(u8)]
    grids = [V.native_grid(c.shape[0], c.shape[1], cfg.patch, cfg.n_patches) for c in crops]
    assert len(set(grids)) >= 10
    patches, imgs = enc.preprocess_ragged(crops, grids, want_u8=True)
    hip = enc.forward_ragged(patches, grids).cpu().numpy()
    mean = torch.tensor(enc.recipe.mean, dtype=torch.float32, device="cuda")
    std = torch.tensor(enc.recipe.std, dtype=torch.float32, device="cuda")
    ora = np.zeros_like(hip)
    for grid in sorted(set(grids)):
        idx = [i for i, g in enumerate(grids) if g == grid]
        img = torch.stack([imgs[i] for i in idx])
        x = (((img.to(torch.float64) * (1 / 255)).to(torch.float32) - mean) / std).permute(0, 3, 1, 2).contiguous()
        c = RC.at_grid(cfg, grid)
        ora[idx] = DC.forward(wt, c, x, device="cuda") if cfg.n_registers else vo.vit_forward(wt, c, x, device="cuda")
    rel = np.linalg.norm(hip - ora, axis=1) / np.linalg.norm(ora, axis=1)
    print(f"[gate {name} native-aspect] precision plan {enc.precision}: embedding rel-L2 mean {rel.mean():.2e} max {rel.max():.2e} over "
          f"{rel.size} crops, {len(set(grids))} grids, {sum(gh * gw for gh, gw in grids)} patches")
    assert rel.max() < 1e-3 and rel.mean() < 0.85e-3


# ---- 5. the engine ------------------------------------------------------------------------------------------------------------------------------
def test_engine_takes_a_native_aspect_encoder():
    """localise_batch(crops=PackedCrops) with a NativeAspectEncoder returns, record for record, what det_emb = embed_native gives"""
    import bench
    from ibloc_amd import vit as V
    from ibloc_amd.engine import LocaliseEngine, MemoryShard, intensity_from_colors
    from ibloc_amd.registration import CloudBatch, RegContext
    from ibloc_amd.synth import SynthWorld
    M, E, Q = 6, 2, 2
    cfg = RC.config("tiny_dino")
    enc = V.VitEncoder(cfg, V.random_weights(cfg, 20))
    nat = V.NativeAspectEncoder(enc)
    world = SynthWorld(M, pts_per_object=4000, E=E, D=cfg.out_dim, seed=11)
    gen, rng = bench.VarCrops(21), np.random.default_rng(10)
    mem = nat.embed([gen.make(k, rng) for k in range(M) for _ in range(E)]).cpu().numpy()
    frames = [world.make_frame(rng, q=Q, pts_per_object=4000) for _ in range(2)]
    det_crops = [gen.make(k, rng) for f in frames for k in f["ids"]]
    assert len({c.shape[:2] for c in det_crops}) > 1
    qs = [len(f["ids"]) for f in frames]
    ctx = RegContext(2 << 30)
    shard = MemoryShard(ctx, list(mem.reshape(M, E, -1)), world.points, colors=world.colors)
    det = lambda: CloudBatch.from_numpy([c[0] for f in frames for c in f["clouds"]], [intensity_from_colors(c[1]) for f in frames for c in f["clouds"]])
    kw = dict(fpfh_voxel_size=0.05, fpfh_global_dist_factor=1.5, fpfh_local_dist_factor=1.5, seed=10)
    emb = enc.embed_native(V.PackedCrops(det_crops))
    assert _same(emb.cpu().numpy(), nat.embed(det_crops).cpu().numpy())
    eng = LocaliseEngine(shard, nat)
    a = eng.localise_batch(det(), qs, crops=V.PackedCrops(det_crops), **kw)
    b = eng.localise_batch(det(), qs, det_emb=emb, **kw)
    assert len(a) == len(b) == len(frames)
    for ra, rb in zip(a, b):
        assert ra.assignments == rb.assignments and ra.best == rb.best and ra.n_clean == rb.n_clean
        assert np.array_equal(ra.pose, rb.pose) and np.array_equal(ra.pose_corrected, rb.pose_corrected)
        assert len(ra.records) == len(rb.records) > 0
        for x, y in zip(ra.records, rb.records):
            assert x.keys() == y.keys() and all(np.array_equal(np.asarray(x[k]), np.asarray(y[k])) for k in x), "a record differs"
    # the square recipe embeds the same crops elsewhere: the two paths are not interchangeable
    assert rel_l2(enc.embed(det_crops).cpu().numpy(), emb.cpu().numpy()) > 1e-2
    ctx.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,word", [("tiny_dinov3", b"rotary"), ("tiny_siglip", b"NO_CLS"), ("tiny_clip", b"CLIP")])
def test_models_without_a_table_for_every_grid_are_refused(name, word):
    from ibloc_amd import _lib
    from ibloc_amd import vit as V
    from tests import dino_reg_cases as DC
    cfg = V.CONFIGS[name]
    enc = V.VitEncoder(cfg, DC.seeded_weights(cfg, 5))
    grids = [(3, 7), (2, 2)]
    total = int(enc.seq_offsets(grids)[-1])
    patches = torch.zeros((total, cfg.patch_k_pad), dtype=torch.float16, device="cuda")
    import ctypes
    ws = enc._ws.get(0, _lib.lib.ibl_vit_ragged_workspace_bytes(ctypes.byref(enc.desc), total, len(grids)))      # the buffer the call will be given
    ws.fill_(0x5A)
    with pytest.raises(_lib.IblError) as e:
        enc.forward_ragged(patches, grids)
    assert word in str(e.value).encode() and "ibl_vit_forward_ragged" in str(e.value)
    torch.cuda.synchronize()
    assert bool((enc._ws.get(0, 1) == 0x5A).all()), "a refused forward wrote to the workspace"
    with pytest.raises(ValueError):
        V.NativeAspectEncoder(enc)
    with pytest.raises(ValueError):
        enc.embed_native([np.zeros((30, 40, 3), np.uint8)])


@pytest.mark.parametrize("kind,cfg", [("dinov3", "tiny_dinov3"), ("siglip", "tiny_siglip"), ("clip", "tiny_clip")])
def test_load_encoder_refuses_native_aspect_before_any_upload(kind, cfg, monkeypatch):
    from ibloc_amd import vit as V
    from ibloc_amd.utils import embeddings as E

    def no_upload(*a, **k):
        raise AssertionError("an encoder was built before the refusal")

    monkeypatch.setattr(V.VitEncoder, "__init__", no_upload)
    registered = E._ENCODERS.get(kind)
    with pytest.raises(ValueError, match="native_aspect"):
        E.load_encoder(kind, {}, cfg=cfg, native_aspect=True)       # an empty state dict: refused before it is read
    assert E._ENCODERS.get(kind) is registered


def test_load_encoder_native_aspect_registers_the_wrapper():
    from ibloc_amd import vit as V
    from ibloc_amd.utils import embeddings as E
    from tests import dino_reg_cases as DC
    cfg = V.CONFIGS["tiny_dino_reg"]
    w = DC.seeded_weights(cfg, 12)
    sd = DC.hf_dinov2_reg_state_dict(cfg, w)
    old = E._ENCODERS.get("dino")
    try:
        nat = E.load_encoder("dino", sd, cfg=cfg, native_aspect=True, max_patches=100, upscale=False)
        assert isinstance(nat, V.NativeAspectEncoder) and E._ENCODERS["dino"] is nat
        crop = np.random.default_rng(1).integers(0, 256, size=(90, 300, 3), dtype=np.uint8)
        got = E.get_all_dino_embeddings(current_obj_grounded_img=crop).cpu().numpy()
        want = nat.encoder.embed_native([crop], max_patches=100, upscale=False).cpu().numpy()[0]
        assert _same(got, want) and got.shape == (cfg.dim,)
        assert V.native_grid(90, 300, cfg.patch, 100, upscale=False) == (5, 18)
        plain = E.load_encoder("dino", sd, cfg=cfg)
        assert isinstance(plain, V.VitEncoder)
    finally:
        if old is None:
            E._ENCODERS.pop("dino", None)
        else:
            E._ENCODERS["dino"] = old
