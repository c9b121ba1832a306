"""DINOv2 with registers and DINOv3 (register tokens, rotary position embedding) -- what the tests of `ibl_rope_kernel`, of the prefix rows and
of the new configurations share:

  * `rope64` / `emulate_rope` / `rope_bound`: the rotation of `ibl_rope_kernel` (csrc/vit_attention.hip) in float64, in numpy fp32 operation for
    operation (one rounded product, then one fma, then f2h_pk's round-to-nearest-even and clamp), and its per-element bound
        2^-11 |ref| + 2^-22 (|a cos| + |b sin|) + 2^-25
    -- one fp16 rounding of the result, three fp32 roundings of the two terms (the kernel spends two: the product and the fma) and the
    half-spacing of the fp16 subnormals.  ref is the fp64 rotation of the same fp16 inputs and fp32 table, clamped to +-65504 as the
    kernel's conversion clamps;
  * `forward`: the fp32 restatement of both forwards in torch (oracle/vit_oracle.py knows neither a register nor a rotation), pinned
    against transformers' Dinov2WithRegistersModel and DINOv3ViTModel in tests/test_dino_reg_model.py; `registers=False` leaves the
    register rows out of the sequence, `rope=False` switches the rotation off -- the two ways a build could skip a feature;
  * the golden cases of tests/golden/dino_reg_golden.npz (generator: tools/gen_golden_dino_reg.py walks CASES)."""
import numpy as np
import torch

from ibloc_amd import vit as V
from tests import gemm_cases as GC

F16_MAX = 65504.0


# ---- the rotation -------------------------------------------------------------------------------------------------------------------------
def _split(qkv, table, n_prefix, heads):
    """qkv (B, T, 3 D) any float dtype -> views a, b (B, P, 2, heads, 32) of columns i / i + 32 of q and k of the patch rows, and cos, sin
    (1, P, 1, 1, 32)"""
    B, T, D3 = qkv.shape
    D = D3 // 3
    x = qkv[:, n_prefix:, :2 * D].reshape(B, T - n_prefix, 2, heads, 64)
    cos, sin = table[:, :32], table[:, 32:]
    return x[..., :32], x[..., 32:], cos[None, :, None, None, :], sin[None, :, None, None, :]


def rope64(qkv16, table32, n_prefix, heads, k_only=False):
    """-> (ref, bound) float64 arrays of qkv's shape: the rotated buffer (everything the kernel leaves alone is the input, bound 0 there)"""
    q = np.asarray(qkv16, np.float16).astype(np.float64)
    t = np.asarray(table32, np.float32).astype(np.float64)
    a, b, c, s = _split(q, t, n_prefix, heads)
    lo, hi = a * c - b * s, b * c + a * s
    mag_lo, mag_hi = np.abs(a * c) + np.abs(b * s), np.abs(b * c) + np.abs(a * s)
    ref, bound = q.copy(), np.zeros_like(q)
    B, T, D3 = q.shape
    D = D3 // 3
    rv = ref[:, n_prefix:, :2 * D].reshape(B, T - n_prefix, 2, heads, 64)
    bv = bound[:, n_prefix:, :2 * D].reshape(B, T - n_prefix, 2, heads, 64)
    x0 = 1 if k_only else 0
    for val, mag, sl in ((lo, mag_lo, slice(0, 32)), (hi, mag_hi, slice(32, 64))):
        val = np.clip(val, -F16_MAX, F16_MAX)
        rv[:, :, x0:, :, sl] = val[:, :, x0:]
        bv[:, :, x0:, :, sl] = (2.0 ** -11 * np.abs(val) + 2.0 ** -22 * mag + 2.0 ** -25)[:, :, x0:]
    return ref, bound


def emulate_rope(qkv16, table32, n_prefix, heads, k_only=False):
    """ibl_rope_kernel in numpy: fp16 in -> fp16 out, ra = fma(a, cos, -(b * sin)), rb = fma(b, cos, a * sin) in fp32, then f2h_pk"""
    f = np.float32
    q = np.asarray(qkv16, np.float16)
    out = q.copy()
    a, b, c, s = _split(q.astype(f), np.asarray(table32, f), n_prefix, heads)
    with np.errstate(over="ignore", invalid="ignore"):
        ra = GC._fma(a, c, -(b * s).astype(f))
        rb = GC._fma(b, c, (a * s).astype(f))
    B, T, D3 = q.shape
    D = D3 // 3
    ov = out[:, n_prefix:, :2 * D].reshape(B, T - n_prefix, 2, heads, 64)
    x0 = 1 if k_only else 0
    ov[:, :, x0:, :, :32] = GC.h16(ra)[:, :, x0:]
    ov[:, :, x0:, :, 32:] = GC.h16(rb)[:, :, x0:]
    return out


FAMILIES = ("normal", "saturate", "subnormal")


def rope_inputs(family, batch, n_tokens, heads, seed):
    """fp16 (batch, n_tokens, 3 * 64 * heads): N(0, 1); magnitudes around 65504 / sqrt(2) .. 65504, where a rotation's result crosses the
    clamp; fp16 subnormals and the smallest normals (|x| < 2^-13)"""
    rng = np.random.default_rng([seed, FAMILIES.index(family)])
    shape = (batch, n_tokens, 3 * 64 * heads)
    if family == "normal":
        x = rng.normal(size=shape)
    elif family == "saturate":
        x = rng.uniform(40000.0, 65504.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    else:
        x = rng.integers(-2048, 2049, size=shape) * 2.0 ** -24
    return x.astype(np.float16)


def rope_model_ratio(shapes=((2, 1, 5, 49), (16, 1, 1, 196)), seed=7):
    """worst |emulation - ref| / bound over the three input families on two of the GPU test's shapes (heads, batch, prefix, patches), a
    14 x 14 and a 7 x 7 table -> (ratio, family)"""
    worst = (0.0, None)
    for heads, batch, prefix, patches in shapes:
        g = int(round(patches ** 0.5))
        table = V.rope_table(g, g, 100.0)
        for fam in FAMILIES:
            x = rope_inputs(fam, batch, prefix + patches, heads, seed)
            ref, bound = rope64(x, table, prefix, heads)
            got = emulate_rope(x, table, prefix, heads).astype(np.float64)
            live = bound > 0
            r = float((np.abs(got - ref)[live] / bound[live]).max())
            assert np.array_equal(got[~live], x.astype(np.float64)[~live])
            if r > worst[0]:
                worst = (r, fam)
    return worst


# ---- the forward in torch, any dtype --------------------------------------------------------------------------------------------------------
def _t(a, device, dtype):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(device=device, dtype=dtype)


def _rotate(x, cos, sin, n_prefix):
    """transformers' apply_rotary_pos_emb: x (B, heads, T, 64), cos / sin (P, 64) (the 32 angles tiled twice); the prefix rows stay"""
    pre, pat = x[:, :, :n_prefix], x[:, :, n_prefix:]
    half = torch.cat((-pat[..., 32:], pat[..., :32]), dim=-1)
    return torch.cat((pre, pat * cos + half * sin), dim=2)


@torch.no_grad()
def forward(weights: dict, cfg, pixel_values, device="cpu", dtype=torch.float32, registers=True, rope=True, all_tokens=False) -> np.ndarray:
    """pixel_values (B, 3, H, W) -> (B, dim): pooler_output (the class row after the final LayerNorm) of Dinov2WithRegistersModel /
    DINOv3ViTModel restated in torch.  registers=False: the sequence without its register rows; rope=False: q and k as projected.
    all_tokens: -> (B, T, dim), every row after the final LayerNorm"""
    F = torch.nn.functional
    w = {k: _t(v, device, dtype) for k, v in weights.items() if k != "pos"}
    x = _t(pixel_values, device, dtype)
    B = x.shape[0]
    x = F.conv2d(x, w["patch.w"], w["patch.b"], stride=cfg.patch).flatten(2).transpose(1, 2)
    cls = w["cls"].reshape(1, 1, -1).expand(B, -1, -1)
    if cfg.rope_theta is None:
        stored = weights["pos"]
        stored = stored.detach().cpu().numpy() if isinstance(stored, torch.Tensor) else np.asarray(stored)
        pos = _t(V.interpolate_pos_embed(stored.astype(np.float32), cfg), device, dtype)
        x, cls = x + pos[1:], cls + pos[0]
    n_reg = cfg.n_registers if registers else 0
    x = torch.cat([cls] + ([w["reg"].unsqueeze(0).expand(B, -1, -1)] if n_reg else []) + [x], dim=1)
    n_prefix = 1 + n_reg
    cos = sin = None
    if cfg.rope_theta is not None and rope:
        t = _t(V.rope_table(cfg.grid[0], cfg.grid[1], cfg.rope_theta), device, dtype)
        cos, sin = torch.cat([t[:, :32]] * 2, dim=1), torch.cat([t[:, 32:]] * 2, dim=1)
    hd = cfg.dim // cfg.heads
    for l in range(cfg.depth):
        p = f"l{l}."
        h = F.layer_norm(x, (cfg.dim,), w[p + "ln1.g"], w[p + "ln1.b"], cfg.ln_eps)
        q, k, v = (F.linear(h, w[p + n + ".w"], w[p + n + ".b"]).view(B, -1, cfg.heads, hd).transpose(1, 2) for n in "qkv")
        if cos is not None:
            q, k = _rotate(q, cos, sin, n_prefix), _rotate(k, cos, sin, n_prefix)
        a = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1) @ v
        x = x + w[p + "ls1"] * F.linear(a.transpose(1, 2).reshape(B, -1, cfg.dim), w[p + "o.w"], w[p + "o.b"])
        h = F.layer_norm(x, (cfg.dim,), w[p + "ln2.g"], w[p + "ln2.b"], cfg.ln_eps)
        x = x + w[p + "ls2"] * F.linear(F.gelu(F.linear(h, w[p + "fc1.w"], w[p + "fc1.b"])), w[p + "fc2.w"], w[p + "fc2.b"])
    x = F.layer_norm(x, (cfg.dim,), w["ln_f.g"], w["ln_f.b"], cfg.ln_eps)
    return (x if all_tokens else x[:, 0]).cpu().numpy()


GATE_WEIGHT_SEED = 30


# ---- golden cases: (configuration name = golden key, weight seed, input seed, batch) ----------------------------------------------------------
CASES = [("tiny_dino_reg", 511, 611, 5), ("tiny_dino_reg_518", 512, 612, 2), ("tiny_dinov3", 513, 613, 5), ("tiny_dinov3_384", 514, 614, 3),
         ("dinov2_vitb14_reg", 515, 615, 2), ("dinov3_vitb16", 516, 616, 2)]
PROBE = 64                 # pixel values per case the golden file keeps, to pin the regenerated input


def seeded_weights(cfg, seed):
    """V.random_weights in the form a checkpoint of the family can hold: DINOv3's key projection has no bias"""
    w = V.random_weights(cfg, seed)
    if cfg.rope_theta is not None:
        for l in range(cfg.depth):
            w[f"l{l}.k.b"] = np.zeros_like(w[f"l{l}.k.b"])
    return w


def build(case):
    """-> (key, cfg, weights, pixels): seeded weights and N(0, 1) pixels, regenerated from the seeds.  random_weights as drawn (registers
    of the class token's size, q / k weights of standard deviation 0.06) already puts a skipped feature far outside the 2e-3 the fp16
    forward is held to, so nothing is scaled: the class embedding without the register rows is 5e-3 (tiny_dino_reg_518, four rows of
    1 374) to 3e-2 away, without the rotation 1e-1 (tests/test_dino_reg_model.py asserts and prints the separations)."""
    key, wseed, iseed, batch = case
    cfg = V.CONFIGS[key]
    w = seeded_weights(cfg, wseed)
    x = np.random.default_rng(iseed).normal(size=(batch, 3, cfg.img_h, cfg.img_w)).astype(np.float32)
    return key, cfg, w, x


# ---- transformers models holding the seeded weights ---------------------------------------------------------------------------------------
def _tt(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _hf_layers(sd, cfg, w, prefix, names):
    for l in range(cfg.depth):
        p, q = f"{prefix}{l}.", f"l{l}."
        sd[p + "norm1.weight"], sd[p + "norm1.bias"] = _tt(w[q + "ln1.g"]), _tt(w[q + "ln1.b"])
        sd[p + "norm2.weight"], sd[p + "norm2.bias"] = _tt(w[q + "ln2.g"]), _tt(w[q + "ln2.b"])
        sd[p + "layer_scale1.lambda1"], sd[p + "layer_scale2.lambda1"] = _tt(w[q + "ls1"]), _tt(w[q + "ls2"])
        for hf, mine in names:
            sd[p + hf + ".weight"] = _tt(w[q + mine + ".w"])
            if not (cfg.rope_theta is not None and mine == "k"):
                sd[p + hf + ".bias"] = _tt(w[q + mine + ".b"])


def hf_dinov2_reg_state_dict(cfg, w):
    """the weights under the names of transformers' Dinov2WithRegistersModel"""
    sd = {"embeddings.cls_token": _tt(w["cls"]).reshape(1, 1, -1), "embeddings.mask_token": torch.zeros(1, cfg.dim),
          "embeddings.register_tokens": _tt(w["reg"]).unsqueeze(0), "embeddings.position_embeddings": _tt(w["pos"]).unsqueeze(0),
          "embeddings.patch_embeddings.projection.weight": _tt(w["patch.w"]), "embeddings.patch_embeddings.projection.bias": _tt(w["patch.b"]),
          "layernorm.weight": _tt(w["ln_f.g"]), "layernorm.bias": _tt(w["ln_f.b"])}
    _hf_layers(sd, cfg, w, "encoder.layer.", (("attention.attention.query", "q"), ("attention.attention.key", "k"),
                                              ("attention.attention.value", "v"), ("attention.output.dense", "o"), ("mlp.fc1", "fc1"),
                                              ("mlp.fc2", "fc2")))
    return sd


def hf_dinov3_state_dict(cfg, w):
    """the weights under the names of transformers' DINOv3ViTModel (k_proj has no bias)"""
    sd = {"embeddings.cls_token": _tt(w["cls"]).reshape(1, 1, -1), "embeddings.mask_token": torch.zeros(1, 1, cfg.dim),
          "embeddings.register_tokens": _tt(w["reg"]).unsqueeze(0),
          "embeddings.patch_embeddings.weight": _tt(w["patch.w"]), "embeddings.patch_embeddings.bias": _tt(w["patch.b"]),
          "norm.weight": _tt(w["ln_f.g"]), "norm.bias": _tt(w["ln_f.b"])}
    _hf_layers(sd, cfg, w, "model.layer.", (("attention.q_proj", "q"), ("attention.k_proj", "k"), ("attention.v_proj", "v"),
                                            ("attention.o_proj", "o"), ("mlp.up_proj", "fc1"), ("mlp.down_proj", "fc2")))
    return sd


def hf_state_dict(cfg, w):
    return hf_dinov3_state_dict(cfg, w) if cfg.rope_theta is not None else hf_dinov2_reg_state_dict(cfg, w)


def hf_model(cfg, w):
    """transformers' model of `cfg` holding the weights `w`, in eval mode"""
    if cfg.rope_theta is not None:
        from transformers import DINOv3ViTConfig, DINOv3ViTModel
        c = DINOv3ViTConfig(hidden_size=cfg.dim, intermediate_size=cfg.mlp_dim, num_hidden_layers=cfg.depth, num_attention_heads=cfg.heads,
                            image_size=cfg.img_h, patch_size=cfg.patch, num_register_tokens=cfg.n_registers, rope_theta=cfg.rope_theta,
                            layer_norm_eps=cfg.ln_eps, hidden_act="gelu")
        m = DINOv3ViTModel(c).eval()
    else:
        from transformers import Dinov2WithRegistersConfig, Dinov2WithRegistersModel
        c = Dinov2WithRegistersConfig(hidden_size=cfg.dim, num_hidden_layers=cfg.depth, num_attention_heads=cfg.heads,
                                      mlp_ratio=cfg.mlp_dim // cfg.dim, image_size=cfg.pos_grid[0] * cfg.patch, patch_size=cfg.patch,
                                      num_register_tokens=cfg.n_registers, layer_norm_eps=cfg.ln_eps, hidden_act="gelu")
        m = Dinov2WithRegistersModel(c).eval()
    missing, unexpected = m.load_state_dict(hf_state_dict(cfg, w), strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return m
