"""Drop-in for the reference's `utils/embeddings.py` on the MI355X build.

The reference loads four encoders at import time by fetching checkpoints by name
(/root/reference/utils/embeddings.py:13-28, 101-103) and embeds ONE crop per call.  Here the encoders are
`ibloc_amd.vit.VitEncoder` objects (HIP kernels behind the C-ABI) registered once with `set_encoder(kind, encoder)`
or built from a converted checkpoint with `load_encoder(kind, state_dict)` (kinds "dino" | "dinov3" | "vit" | "clip" | "dator" | "siglip"); the four reference entry points keep
their names and `(**kwargs) -> torch.Tensor` signature:

    get_all_clip_embeddings   :31-50   L2-normalised 512-d
    get_all_dino_embeddings   :53-71   CLS after the final LayerNorm, 768-d, un-normalised
    get_all_vit_embeddings    :74-98   CLS, 768-d
    get_dator_embeddings      :105-121 RGB-D 128-d (ibloc_amd.dator.DatorEncoder registered as kind "dator")

`embed_batch(kind, crops)` is the batched form the localisation engine uses (one launch sequence for many crops).
"""
import numpy as np
import torch

from ibloc_amd import match
from ibloc_amd import vit as V

_ENCODERS = {}
_KIND_TO_CONFIG = {"dino": "dinov2_vitb14", "dinov3": "dinov3_vitb16", "vit": "vit_b16", "clip": "clip_b32"}


def set_encoder(kind: str, encoder: V.VitEncoder) -> None:
    _ENCODERS[kind] = encoder


def _refuse_gated_mlp(sd: dict, what: str) -> None:
    gated = [k for k in sd if ".mlp.gate_proj." in k or ".mlp.weights_in." in k or ".mlp.w12." in k]
    if gated:
        raise ValueError(f"{what}: a gated MLP ({gated[0]}; use_gated_mlp / SwiGLU checkpoints: DINOv3 ViT-S+ / H+, DINOv2-g) is not supported")


def hf_dinov2_to_weights(sd: dict, depth: int) -> dict:
    """transformers Dinov2Model.state_dict() (4.44 naming) or Dinov2WithRegistersModel.state_dict() -> the weight dict VitEncoder takes.
    Register tokens (`embeddings.register_tokens`, or `register_tokens` as the hub checkpoints name them) become "reg" (R, dim); a SwiGLU
    checkpoint is refused."""
    g = lambda k: np.asarray(sd[k].float().cpu() if hasattr(sd[k], "float") else sd[k], dtype=np.float32)
    _refuse_gated_mlp(sd, "hf_dinov2_to_weights")
    w = {"patch.w": g("embeddings.patch_embeddings.projection.weight"), "patch.b": g("embeddings.patch_embeddings.projection.bias"),
         "cls": g("embeddings.cls_token").reshape(-1), "pos": g("embeddings.position_embeddings")[0],
         "ln_f.g": g("layernorm.weight"), "ln_f.b": g("layernorm.bias")}
    for l in range(depth):
        p, q = f"encoder.layer.{l}.", f"l{l}."
        w[q + "ln1.g"], w[q + "ln1.b"] = g(p + "norm1.weight"), g(p + "norm1.bias")
        w[q + "ln2.g"], w[q + "ln2.b"] = g(p + "norm2.weight"), g(p + "norm2.bias")
        for hf, mine in (("query", "q"), ("key", "k"), ("value", "v")):
            w[q + mine + ".w"], w[q + mine + ".b"] = g(p + f"attention.attention.{hf}.weight"), g(p + f"attention.attention.{hf}.bias")
        w[q + "o.w"], w[q + "o.b"] = g(p + "attention.output.dense.weight"), g(p + "attention.output.dense.bias")
        w[q + "fc1.w"], w[q + "fc1.b"] = g(p + "mlp.fc1.weight"), g(p + "mlp.fc1.bias")
        w[q + "fc2.w"], w[q + "fc2.b"] = g(p + "mlp.fc2.weight"), g(p + "mlp.fc2.bias")
        w[q + "ls1"], w[q + "ls2"] = g(p + "layer_scale1.lambda1"), g(p + "layer_scale2.lambda1")
    for k in ("embeddings.register_tokens", "register_tokens"):
        if k in sd and g(k).size:
            w["reg"] = g(k).reshape(-1, w["cls"].shape[0])
    return w


def hf_dinov3_to_weights(sd: dict, depth: int) -> dict:
    """transformers DINOv3ViTModel.state_dict() -> the weight dict VitEncoder takes.  The separate q_proj / k_proj / v_proj become the
    "q" / "k" / "v" entries VitEncoder packs into w_qkv; k_proj has no bias (key_bias False), so its slice of b_qkv is zeros.  There is no
    position table (rotary embedding: the configuration's rope_theta); mask_token is ignored; a gated-MLP checkpoint is refused."""
    g = lambda k: np.asarray(sd[k].float().cpu() if hasattr(sd[k], "float") else sd[k], dtype=np.float32)
    _refuse_gated_mlp(sd, "hf_dinov3_to_weights")
    w = {"patch.w": g("embeddings.patch_embeddings.weight"), "patch.b": g("embeddings.patch_embeddings.bias"),
         "cls": g("embeddings.cls_token").reshape(-1), "ln_f.g": g("norm.weight"), "ln_f.b": g("norm.bias")}
    D = w["cls"].shape[0]
    if g("embeddings.register_tokens").size:
        w["reg"] = g("embeddings.register_tokens").reshape(-1, D)
    for l in range(depth):
        p, q = f"model.layer.{l}.", f"l{l}."
        w[q + "ln1.g"], w[q + "ln1.b"] = g(p + "norm1.weight"), g(p + "norm1.bias")
        w[q + "ln2.g"], w[q + "ln2.b"] = g(p + "norm2.weight"), g(p + "norm2.bias")
        for hf, mine in (("q_proj", "q"), ("k_proj", "k"), ("v_proj", "v"), ("o_proj", "o")):
            w[q + mine + ".w"] = g(p + f"attention.{hf}.weight")
            w[q + mine + ".b"] = g(p + f"attention.{hf}.bias") if p + f"attention.{hf}.bias" in sd else np.zeros(w[q + mine + ".w"].shape[0], np.float32)
        w[q + "fc1.w"], w[q + "fc1.b"] = g(p + "mlp.up_proj.weight"), g(p + "mlp.up_proj.bias")
        w[q + "fc2.w"], w[q + "fc2.b"] = g(p + "mlp.down_proj.weight"), g(p + "mlp.down_proj.bias")
        w[q + "ls1"], w[q + "ls2"] = g(p + "layer_scale1.lambda1"), g(p + "layer_scale2.lambda1")
    return w


def check_dino_weights(w: dict, cfg: V.VitConfig) -> None:
    """what load_encoder refuses for the DINO kinds before anything is uploaded: a head_dim other than 64, and a register count that is
    not the configuration's"""
    if cfg.dim != 64 * cfg.heads:
        raise ValueError(f"{cfg.name}: head_dim {cfg.dim / cfg.heads:g} is not supported (the attention and rotation kernels run head_dim 64)")
    have = int(np.shape(w["reg"])[0]) if "reg" in w else 0
    if have != cfg.n_registers:
        raise ValueError(f"the state dict holds {have} register tokens, the configuration {cfg.name} {cfg.n_registers}: pick the "
                         "configuration of the checkpoint (dinov2_*_reg have 4, the plain DINOv2 ones none)")


def hf_vit_to_weights(sd: dict, depth: int) -> dict:
    """transformers ViTModel.state_dict() -> weight dict.  Both parameter namings are read: transformers 4.44 (the version the reference
    pins, environment.yml:275: `encoder.layer.N.attention.attention.query`, `intermediate.dense`, `output.dense`) and 5.x
    (`layers.N.attention.q_proj`, `mlp.fc1`, `mlp.fc2`)."""
    g = lambda k: np.asarray(sd[k].float().cpu() if hasattr(sd[k], "float") else sd[k], dtype=np.float32)
    w = {"patch.w": g("embeddings.patch_embeddings.projection.weight"), "patch.b": g("embeddings.patch_embeddings.projection.bias"),
         "cls": g("embeddings.cls_token").reshape(-1), "pos": g("embeddings.position_embeddings")[0],
         "ln_f.g": g("layernorm.weight"), "ln_f.b": g("layernorm.bias")}
    new_names = "layers.0.attention.q_proj.weight" in sd
    for l in range(depth):
        p, q = (f"layers.{l}." if new_names else f"encoder.layer.{l}."), f"l{l}."
        w[q + "ln1.g"], w[q + "ln1.b"] = g(p + "layernorm_before.weight"), g(p + "layernorm_before.bias")
        w[q + "ln2.g"], w[q + "ln2.b"] = g(p + "layernorm_after.weight"), g(p + "layernorm_after.bias")
        if new_names:
            for hf, mine in (("q_proj", "q"), ("k_proj", "k"), ("v_proj", "v"), ("o_proj", "o")):
                w[q + mine + ".w"], w[q + mine + ".b"] = g(p + f"attention.{hf}.weight"), g(p + f"attention.{hf}.bias")
            w[q + "fc1.w"], w[q + "fc1.b"] = g(p + "mlp.fc1.weight"), g(p + "mlp.fc1.bias")
            w[q + "fc2.w"], w[q + "fc2.b"] = g(p + "mlp.fc2.weight"), g(p + "mlp.fc2.bias")
        else:
            for hf, mine in (("query", "q"), ("key", "k"), ("value", "v")):
                w[q + mine + ".w"], w[q + mine + ".b"] = g(p + f"attention.attention.{hf}.weight"), g(p + f"attention.attention.{hf}.bias")
            w[q + "o.w"], w[q + "o.b"] = g(p + "attention.output.dense.weight"), g(p + "attention.output.dense.bias")
            w[q + "fc1.w"], w[q + "fc1.b"] = g(p + "intermediate.dense.weight"), g(p + "intermediate.dense.bias")
            w[q + "fc2.w"], w[q + "fc2.b"] = g(p + "output.dense.weight"), g(p + "output.dense.bias")
    return w


def open_clip_visual_to_weights(sd: dict, depth: int) -> dict:
    """open_clip `model.visual.state_dict()` (VisionTransformer) -> weight dict (fused in_proj split into q/k/v)."""
    g = lambda k: np.asarray(sd[k].float().cpu() if hasattr(sd[k], "float") else sd[k], dtype=np.float32)
    D = g("class_embedding").shape[0]
    w = {"patch.w": g("conv1.weight"), "patch.b": np.zeros(D, np.float32), "cls": g("class_embedding"),
         "pos": g("positional_embedding"), "ln_pre.g": g("ln_pre.weight"), "ln_pre.b": g("ln_pre.bias"),
         "ln_f.g": g("ln_post.weight"), "ln_f.b": g("ln_post.bias"), "proj.w": g("proj").T.copy()}
    for l in range(depth):
        p, q = f"transformer.resblocks.{l}.", f"l{l}."
        w[q + "ln1.g"], w[q + "ln1.b"] = g(p + "ln_1.weight"), g(p + "ln_1.bias")
        w[q + "ln2.g"], w[q + "ln2.b"] = g(p + "ln_2.weight"), g(p + "ln_2.bias")
        wi, bi = g(p + "attn.in_proj_weight"), g(p + "attn.in_proj_bias")
        for i, mine in enumerate("qkv"):
            w[q + mine + ".w"], w[q + mine + ".b"] = wi[i * D:(i + 1) * D], bi[i * D:(i + 1) * D]
        w[q + "o.w"], w[q + "o.b"] = g(p + "attn.out_proj.weight"), g(p + "attn.out_proj.bias")
        w[q + "fc1.w"], w[q + "fc1.b"] = g(p + "mlp.c_fc.weight"), g(p + "mlp.c_fc.bias")
        w[q + "fc2.w"], w[q + "fc2.b"] = g(p + "mlp.c_proj.weight"), g(p + "mlp.c_proj.bias")
    return w


def hf_clip_to_weights(sd: dict, depth: int) -> dict:
    """transformers `CLIPVisionModelWithProjection.state_dict()` or `CLIPModel.state_dict()` (the text tower's keys are ignored) -> weight
    dict.  `pre_layrnorm` is transformers' own spelling."""
    g = lambda k: np.asarray(sd[k].float().cpu() if hasattr(sd[k], "float") else sd[k], dtype=np.float32)
    v = "vision_model."
    D = g(v + "embeddings.class_embedding").shape[0]
    w = {"patch.w": g(v + "embeddings.patch_embedding.weight"), "patch.b": np.zeros(D, np.float32),
         "cls": g(v + "embeddings.class_embedding"), "pos": g(v + "embeddings.position_embedding.weight"),
         "ln_pre.g": g(v + "pre_layrnorm.weight"), "ln_pre.b": g(v + "pre_layrnorm.bias"),
         "ln_f.g": g(v + "post_layernorm.weight"), "ln_f.b": g(v + "post_layernorm.bias"), "proj.w": g("visual_projection.weight")}
    for l in range(depth):
        p, q = v + f"encoder.layers.{l}.", f"l{l}."
        w[q + "ln1.g"], w[q + "ln1.b"] = g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias")
        w[q + "ln2.g"], w[q + "ln2.b"] = g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias")
        for hf, mine in (("q_proj", "q"), ("k_proj", "k"), ("v_proj", "v"), ("out_proj", "o")):
            w[q + mine + ".w"], w[q + mine + ".b"] = g(p + f"self_attn.{hf}.weight"), g(p + f"self_attn.{hf}.bias")
        w[q + "fc1.w"], w[q + "fc1.b"] = g(p + "mlp.fc1.weight"), g(p + "mlp.fc1.bias")
        w[q + "fc2.w"], w[q + "fc2.b"] = g(p + "mlp.fc2.weight"), g(p + "mlp.fc2.bias")
    return w


def hf_siglip_to_weights(sd: dict, depth: int):
    """transformers `SiglipVisionModel.state_dict()` or `SiglipModel.state_dict()` (the text tower's keys and the logit scale / bias are
    ignored), with or without the `vision_model.` prefix -> (trunk weights, head weights): the dicts `ibloc_amd.siglip.SiglipEncoder` takes.
    The pooling head's fused `in_proj_weight` / `in_proj_bias` are split into q / k / v."""
    v = "vision_model." if any(k.startswith("vision_model.") for k in sd) else ""
    g = lambda k: np.asarray(sd[v + k].float().cpu() if hasattr(sd[v + k], "float") else sd[v + k], dtype=np.float32)
    w = {"patch.w": g("embeddings.patch_embedding.weight"), "patch.b": g("embeddings.patch_embedding.bias"),
         "pos": g("embeddings.position_embedding.weight"), "ln_f.g": g("post_layernorm.weight"), "ln_f.b": g("post_layernorm.bias")}
    for l in range(depth):
        p, q = f"encoder.layers.{l}.", f"l{l}."
        w[q + "ln1.g"], w[q + "ln1.b"] = g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias")
        w[q + "ln2.g"], w[q + "ln2.b"] = g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias")
        for hf, mine in (("q_proj", "q"), ("k_proj", "k"), ("v_proj", "v"), ("out_proj", "o")):
            w[q + mine + ".w"], w[q + mine + ".b"] = g(p + f"self_attn.{hf}.weight"), g(p + f"self_attn.{hf}.bias")
        w[q + "fc1.w"], w[q + "fc1.b"] = g(p + "mlp.fc1.weight"), g(p + "mlp.fc1.bias")
        w[q + "fc2.w"], w[q + "fc2.b"] = g(p + "mlp.fc2.weight"), g(p + "mlp.fc2.bias")
    D = w["pos"].shape[1]
    wi, bi = g("head.attention.in_proj_weight"), g("head.attention.in_proj_bias")
    hw = {"probe": g("head.probe").reshape(-1), "o.w": g("head.attention.out_proj.weight"), "o.b": g("head.attention.out_proj.bias"),
          "ln.g": g("head.layernorm.weight"), "ln.b": g("head.layernorm.bias"), "fc1.w": g("head.mlp.fc1.weight"),
          "fc1.b": g("head.mlp.fc1.bias"), "fc2.w": g("head.mlp.fc2.weight"), "fc2.b": g("head.mlp.fc2.bias")}
    for i, mine in enumerate("qkv"):
        hw[mine + ".w"], hw[mine + ".b"] = wi[i * D:(i + 1) * D].copy(), bi[i * D:(i + 1) * D].copy()
    return w, hw


def clip_converter(state_dict):
    """the converter of a CLIP vision state dict, from its key layout: `vision_model.*` is transformers', `conv1.weight` open_clip's
    `model.visual` (OpenAI's released checkpoints use the same names)"""
    if any(k.startswith("vision_model.") for k in state_dict):
        return hf_clip_to_weights
    if "conv1.weight" in state_dict:
        return open_clip_visual_to_weights
    raise KeyError("neither a transformers CLIP state dict (vision_model.*) nor an open_clip / OpenAI visual one (conv1.weight)")


def load_encoder(kind: str, state_dict, device="cuda", cfg: V.VitConfig = None, native_aspect=False, max_patches=None, upscale=True):
    """Build + register the encoder of `kind` ("dino" | "vit" | "clip" | "dator") from a checkpoint state dict.  cfg: another
    architecture / position-embedding rule than the checkpoint the reference loads (default: V.CONFIGS of the kind).

    "clip": the state dict may be open_clip's / OpenAI's `model.visual.state_dict()` or transformers' CLIPVisionModelWithProjection /
    CLIPModel one; the key layout picks the converter.  A state dict does not carry the activation: it is `cfg.quick_gelu`, the caller's
    -- the default cfg (clip_b32, laion2b) runs erf GELU; OpenAI's checkpoints, open_clip's *-quickgelu models and transformers models
    with hidden_act "quick_gelu" need V.CONFIGS["clip_b32_openai"] / "clip_b16_openai" / "clip_l14_openai" / "clip_l14_336_openai".
    cfg may also be the name of a configuration: "clip_l14_336_openai" (577 tokens, its 24 x 24 position table as stored),
    "dinov2_vitb14_448" or "dinov2_vitb14_518" (the 37 x 37 table as stored) run the same checkpoints' towers at their high resolutions.

    "dator": `state_dict` is a `build_FourDNet` checkpoint as the reference's `load_model('.../dator_best_tum.pth')` reads it
    (utils/embeddings.py:101-103, make_model.py:620-626) -- the dict itself or the path of the `.pth` file (loaded with
    `weights_only=True`: a checkpoint is data) -> `ibloc_amd.dator.DatorEncoder` (`module.` prefix stripped, `classifier*` skipped, LoRA
    folded into the QKV weights).

    "dino" also takes the register checkpoints (Dinov2WithRegistersModel) with cfg "dinov2_vits14_reg" / "dinov2_vitb14_reg" /
    "dinov2_vitl14_reg" / "dinov2_vitb14_reg_518"; "dinov3" a transformers `DINOv3ViTModel` state dict, cfg "dinov3_vits16" /
    "dinov3_vitb16" (default) / "dinov3_vitl16".  Gated-MLP checkpoints, head_dim != 64 and a register count that is not the
    configuration's are refused (ValueError) before anything is uploaded.

    "siglip": a transformers `SiglipVisionModel` / `SiglipModel` state dict -> `ibloc_amd.siglip.SiglipEncoder` (trunk + attention-pooling
    head); cfg defaults to "siglip_b16_224", the other towers are "siglip_b16_256" / "_384" and "siglip_l16_256" / "_384".

    native_aspect=True ("dino" only, plain or with registers): the registered and returned encoder is a `V.NativeAspectEncoder` -- every
    crop runs at the patch grid of its own aspect ratio (`V.native_grid` with `max_patches`, default the configuration's, and `upscale`)
    instead of the recipe's centre-cropped square, so `embed_batch` / `get_all_dino_embeddings` take the ragged forward.  Such
    embeddings differ from the reference's by design: embed a memory and its queries the same way.  Any other kind, and a configuration
    without a resampled position table, is refused (ValueError) before anything is uploaded.  False: today's objects, unchanged."""
    if native_aspect:
        c = V.CONFIGS[cfg] if isinstance(cfg, str) else (cfg or V.CONFIGS.get(_KIND_TO_CONFIG.get(kind)))
        if kind != "dino" or c.rope_theta is not None or not c.cls_token or c.proj_dim or c.pre_ln:
            raise ValueError(f"native_aspect: kind {kind!r} is not supported: per-crop patch grids need a DINOv2 encoder (plain or with "
                             "registers), whose position table is defined for every grid")
    if kind == "dator":
        from ibloc_amd import dator as D
        if isinstance(state_dict, (str, bytes)) or hasattr(state_dict, "__fspath__"):
            state_dict = torch.load(state_dict, map_location="cpu", weights_only=True)
        rw, dw, hw = D.fourdnet_state_dict_to_weights(state_dict)
        enc = D.DatorEncoder(rw, dw, hw, device=device)
        set_encoder(kind, enc)
        return enc
    if isinstance(cfg, str):
        cfg = V.CONFIGS[cfg]
    if kind == "siglip":
        from ibloc_amd import siglip as S
        cfg = cfg or V.CONFIGS["siglip_b16_224"]
        tw, hw = hf_siglip_to_weights(state_dict, cfg.depth)
        enc = S.SiglipEncoder(cfg, tw, hw, device=device)
        set_encoder(kind, enc)
        return enc
    cfg = cfg or V.CONFIGS[_KIND_TO_CONFIG[kind]]
    conv = clip_converter(state_dict) if kind == "clip" else {"dino": hf_dinov2_to_weights, "dinov3": hf_dinov3_to_weights,
                                                              "vit": hf_vit_to_weights}[kind]
    weights = conv(state_dict, cfg.depth)
    if kind in ("dino", "dinov3"):
        check_dino_weights(weights, cfg)
    enc = V.VitEncoder(cfg, weights, device=device)
    if native_aspect:
        enc = V.NativeAspectEncoder(enc, max_patches, upscale)
    set_encoder(kind, enc)
    return enc


def _encoder(kind):
    if kind not in _ENCODERS:
        raise RuntimeError(
            f"no '{kind}' encoder registered: call utils.embeddings.load_encoder('{kind}', state_dict) with the checkpoint the "
            "reference loads at import time (utils/embeddings.py:13-28), or set_encoder(kind, VitEncoder) -- checkpoints cannot be "
            "fetched by name on an offline MI355X box")
    return _ENCODERS[kind]


def embed_batch(kind: str, crops) -> torch.Tensor:
    """crops: list of HxWx3 uint8 arrays (or a uint8 tensor N x H x W x 3) -> (N, D) device tensor."""
    out = _encoder(kind).embed(crops)
    if kind == "clip":
        out = match.normalize_rows(out)          # clip_features /= clip_features.norm(dim=-1, keepdim=True), :48
    return out


def get_all_clip_embeddings(**kwargs) -> torch.Tensor:
    return embed_batch("clip", [kwargs["current_obj_grounded_img"]])[0]


def get_all_dino_embeddings(**kwargs) -> torch.Tensor:
    return embed_batch("dino", [kwargs["current_obj_grounded_img"]])[0]


def get_all_dinov3_embeddings(**kwargs) -> torch.Tensor:
    """DINOv3 pooler_output of the crop (the class row after the final LayerNorm), un-normalised, as get_all_dino_embeddings returns it"""
    return embed_batch("dinov3", [kwargs["current_obj_grounded_img"]])[0]


def get_all_vit_embeddings(**kwargs) -> torch.Tensor:
    return embed_batch("vit", [kwargs["current_obj_grounded_img"]])[0]


def get_all_siglip_embeddings(**kwargs) -> torch.Tensor:
    """SigLIP pooler_output of the crop, un-normalised (no counterpart in the reference: the crop is treated as the other three do)"""
    return embed_batch("siglip", [kwargs["current_obj_grounded_img"]])[0]


def get_dator_embeddings(**kwargs) -> torch.Tensor:
    """utils/embeddings.py:105-121: crop the full depth image with the bounding box (xyxy), embed (RGB crop, depth crop)."""
    enc = _encoder("dator")
    bb = kwargs["current_obj_bounding_box"]
    depth = kwargs["full_depth_image"][int(bb[1]):int(bb[3]), int(bb[0]):int(bb[2])]
    return enc.embed([kwargs["current_obj_grounded_img"]], [np.asarray(depth, dtype=np.float32)])[0]
