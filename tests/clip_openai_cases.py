"""QuickGELU (OpenAI CLIP: v * sigmoid(1.702 v)) -- what the tests of the QuickGELU epilogue of `ibl_gemm_f16_tn` and of the OpenAI CLIP
configurations share:

  * `emulate_qgelu`: `quick_gelu2` (csrc/vit_gemm.hip) in numpy fp32, operation for operation, and the fp64 reference `qgelu64`;
  * the per-element bound of IBL_LINEAR_GELU_F16 / _X2 / _X3 with IBL_ACT_QUICK_GELU.  It is the bound of tests/gemm_cases.py with two
    constants exchanged:  LIP_Q e1 + C_QGELU max(|v|, TINY) + 2^-11 |ref| + 2^-25  (e1, TINY, SLACK: gemm_cases).
      LIP_Q = 1.10 >= max |q'| = 1.0998 (at v = 1.44) carries the accumulation error through the activation.
      C_QGELU |v| is the error of the kernel's form: four fp32 roundings (c v, 1 + e, rcp, v r) and the exp2 of an argument that carries
      half an ulp of c v -- |c v| 2^-24 ln 2 relative in e, weighted with e / (1 + e).  The sum is largest where |c v| e / (1 + e) is, at
      v ~ 4.3, and it is relative to the result, which is at most |v|.
    C_QGELU is the smallest power of two for which the emulation stays at or under 0.75 of C_QGELU max(|v|, TINY) on `qgelu_grid` -- the
    rule C_GELU was chosen by; tests/test_qgelu_model.py asserts it and prints the ratios: 2^-23 gives 1.18, 2^-22 0.59 (at v = 4.29).
    As there, the emulation uses the exact reciprocal and exp2 where the kernel runs v_rcp_f32 and v_exp_f32 (one ulp).
  * `forward`: the fp32 restatement of the encoder forward with the activation of `cfg.quick_gelu` (oracle/vit_oracle.py knows erf GELU
    only), pinned against transformers' CLIPVisionModelWithProjection(hidden_act="quick_gelu") in tests/test_clip_openai_converters.py;
  * the golden cases of tests/golden/clip_quickgelu_golden.npz (generator: tools/gen_golden_clip_quickgelu.py mirrors CASES)."""
import numpy as np
import torch

from ibloc_amd import vit as V
from oracle import vit_oracle as vo
from tests import gemm_cases as GC

ACT_QUICK = 1                                  # IBL_ACT_QUICK_GELU
LIP_Q = 1.10
C_QGELU = 2.0 ** -22
C_EXP = np.float32(-1.702 * 1.4426950408889634)      # c of quick_gelu2: -1.702 log2(e), rounded to fp32


def qgelu64(v):
    """v / (1 + exp(-1.702 v)) in float64 (torch), evaluated without overflow: for v < 0 as v exp(1.702 v) / (1 + exp(1.702 v))"""
    e = torch.exp(-1.702 * v.abs())
    return torch.where(v >= 0, v / (1.0 + e), v * e / (1.0 + e))


def emulate_qgelu(v):
    """quick_gelu2 (csrc/vit_gemm.hip) in numpy fp32, operation for operation; v fp32 -> value fp32"""
    f = np.float32
    v = np.asarray(v, f)
    with np.errstate(over="ignore"):
        a = v * C_EXP
        e = np.exp2(a.astype(np.float64)).astype(f)           # +inf from a >= 128 on, as v_exp_f32
        d = e + f(1.0)
        r = (1.0 / d.astype(np.float64)).astype(f)            # 1 / inf = 0
        return v * r


def qgelu_grid():
    """gemm_cases.gelu_grid (what `gelu_span` covers) and the extremes: +-200, +-65504 and both sides of the v where exp2(c v) overflows
    (c v = 128 at v = -52.13, i.e. exp(-1.702 v) at -88.7 / 1.702) in steps of 2^-10"""
    edge = np.arange(-54.0, -50.0, 2.0 ** -10)
    return np.concatenate([GC.gelu_grid(), [200.0, -200.0, 65504.0, -65504.0], edge]).astype(np.float32)


def qgelu_model_ratio(c_q):
    """-> (worst |value - q(v)| / (c_q max(|v|, TINY)), where, worst error / bound of h + lo / 64) of the emulation over `qgelu_grid`
    (see gemm_cases.gelu_model_ratio)"""
    v = qgelu_grid()
    value = emulate_qgelu(v)
    h = GC.h16(value)
    lo = GC.h16((value - h.astype(np.float32)) * np.float32(GC.SPLIT))
    two = h.astype(np.float64) + lo.astype(np.float64) / GC.SPLIT
    ref = qgelu64(torch.from_numpy(v.astype(np.float64))).numpy()
    poly = c_q * np.maximum(np.abs(v.astype(np.float64)), GC.TINY)
    lo_round = 2.0 ** -11 * (2.0 ** -11 * np.abs(ref) + 2.0 ** -25) + 2.0 ** -31
    r = np.abs(value.astype(np.float64) - ref) / poly
    ok = np.abs(ref) <= GC.F16_MAX                            # h + lo / 64 is the value only where h is not saturated
    r2 = np.where(ok, np.abs(two - ref) / ((poly + lo_round) * GC.SLACK), 0.0)
    return float(r.max()), float(v[r.argmax()]), float(r2.max())


def expected(y, S, K, bias=None):
    """-> (ref, bound) float64 (M, N) of the first column block of the GELU epilogues with IBL_ACT_QUICK_GELU"""
    b = bias if bias is not None else torch.zeros((), dtype=torch.float64, device=y.device)
    v = y + b
    ref = qgelu64(v).clamp(-GC.F16_MAX, GC.F16_MAX)
    bnd = LIP_Q * GC._e1(S, bias, K) + C_QGELU * v.abs().clamp_min(GC.TINY) + GC._f16_round(ref)
    return ref, bnd * GC.SLACK


def expected_two_term(y, S, K, bias=None):
    """IBL_LINEAR_GELU_F16_X3 with IBL_ACT_QUICK_GELU: -> (ref, bound, valid) for h + lo / 64; valid = h is not saturated"""
    b = bias if bias is not None else torch.zeros((), dtype=torch.float64, device=y.device)
    v = y + b
    ref = qgelu64(v)
    lo_round = 2.0 ** -11 * (2.0 ** -11 * ref.abs() + 2.0 ** -25) + 2.0 ** -31
    bnd = LIP_Q * GC._e1(S, bias, K) + C_QGELU * v.abs().clamp_min(GC.TINY) + lo_round
    return ref, bnd * GC.SLACK, ref.abs() <= GC.F16_MAX


# ---- the encoder forward in fp32 with the configuration's activation --------------------------------------------------------------------
@torch.no_grad()
def forward(weights: dict, cfg, pixel_values, device="cpu") -> np.ndarray:
    """pixel_values (B, 3, H, W) float32 -> (B, out_dim) float32: oracle/vit_oracle.vit_forward's CLS path with
    x * sigmoid(1.702 x) where cfg.quick_gelu is set."""
    F = torch.nn.functional
    act = (lambda t: t * torch.sigmoid(1.702 * t)) if cfg.quick_gelu else F.gelu
    w = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v, dtype=np.float32))).to(device) for k, v in weights.items()}
    x = pixel_values if isinstance(pixel_values, torch.Tensor) else torch.from_numpy(np.asarray(pixel_values, dtype=np.float32))
    x = x.to(device=device, dtype=torch.float32)
    B = x.shape[0]
    x = F.conv2d(x, w["patch.w"], w.get("patch.b"), stride=cfg.patch).flatten(2).transpose(1, 2)
    x = torch.cat([w["cls"].reshape(1, 1, -1).expand(B, -1, -1), x], dim=1)
    x = x + vo.interpolate_pos(w["pos"], cfg.pos_grid, cfg.grid, cfg.pos_interp).unsqueeze(0)
    if cfg.pre_ln:
        x = F.layer_norm(x, (cfg.dim,), w["ln_pre.g"], w["ln_pre.b"], cfg.ln_eps)
    hd = cfg.dim // cfg.heads
    for l in range(cfg.depth if cfg.n_blocks_run < 0 else cfg.n_blocks_run):
        p = f"l{l}."
        h = F.layer_norm(x, (cfg.dim,), w[p + "ln1.g"], w[p + "ln1.b"], cfg.ln_eps)
        q, k, v = (F.linear(h, w[p + n + ".w"], w[p + n + ".b"]).view(B, -1, cfg.heads, hd).transpose(1, 2) for n in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1) @ v
        a = F.linear(a.transpose(1, 2).reshape(B, -1, cfg.dim), w[p + "o.w"], w[p + "o.b"])
        x = x + (a * w[p + "ls1"] if cfg.layerscale else a)
        h = F.layer_norm(x, (cfg.dim,), w[p + "ln2.g"], w[p + "ln2.b"], cfg.ln_eps)
        h = F.linear(act(F.linear(h, w[p + "fc1.w"], w[p + "fc1.b"])), w[p + "fc2.w"], w[p + "fc2.b"])
        x = x + (h * w[p + "ls2"] if cfg.layerscale else h)
    c = x[:, 0]
    if cfg.final_ln:
        c = F.layer_norm(c, (cfg.dim,), w["ln_f.g"], w["ln_f.b"], cfg.ln_eps)
    if cfg.proj_dim:
        c = c @ w["proj.w"].t()
    return c.cpu().numpy()


# ---- golden cases: (golden key = configuration name, weight seed, input seed, batch) -----------------------------------------------------
CASES = [("tiny_clip_q", 301, 401, 5), ("clip_b32_openai", 302, 402, 5)]


def build(case):
    """-> (key, cfg, weights, pixels): seeded weights (no patch bias, as CLIP) and N(0, 1) pixels, regenerated from the seeds"""
    key, wseed, iseed, batch = case
    cfg = V.CONFIGS[key]
    w = V.random_weights(cfg, wseed)
    w["patch.b"] = np.zeros_like(w["patch.b"])
    x = np.random.default_rng(iseed).normal(size=(batch, 3, cfg.img_h, cfg.img_w)).astype(np.float32)
    return key, cfg, w, x


def hf_clip_state_dict(cfg, w):
    """the seeded weights under the names of transformers' CLIPVisionModelWithProjection"""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    sd = {"vision_model.embeddings.class_embedding": t(w["cls"]),
          "vision_model.embeddings.position_embedding.weight": t(w["pos"]),
          "vision_model.embeddings.patch_embedding.weight": t(w["patch.w"]),
          "vision_model.pre_layrnorm.weight": t(w["ln_pre.g"]), "vision_model.pre_layrnorm.bias": t(w["ln_pre.b"]),
          "vision_model.post_layernorm.weight": t(w["ln_f.g"]), "vision_model.post_layernorm.bias": t(w["ln_f.b"]),
          "visual_projection.weight": t(w["proj.w"])}
    for l in range(cfg.depth):
        p, q = f"vision_model.encoder.layers.{l}.", f"l{l}."
        sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"] = t(w[q + "ln1.g"]), t(w[q + "ln1.b"])
        sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"] = t(w[q + "ln2.g"]), t(w[q + "ln2.b"])
        for hf, mine in (("q_proj", "q"), ("k_proj", "k"), ("v_proj", "v"), ("out_proj", "o")):
            sd[p + f"self_attn.{hf}.weight"], sd[p + f"self_attn.{hf}.bias"] = t(w[q + mine + ".w"]), t(w[q + mine + ".b"])
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = t(w[q + "fc1.w"]), t(w[q + "fc1.b"])
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = t(w[q + "fc2.w"]), t(w[q + "fc2.b"])
    return sd


def hf_clip_model(cfg, w):
    """transformers' CLIPVisionModelWithProjection of `cfg` (hidden_act from cfg.quick_gelu) holding the weights `w`"""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    c = CLIPVisionConfig(hidden_size=cfg.dim, num_hidden_layers=cfg.depth, num_attention_heads=cfg.heads, intermediate_size=cfg.mlp_dim,
                         image_size=cfg.img_h, patch_size=cfg.patch, layer_norm_eps=cfg.ln_eps,
                         hidden_act="quick_gelu" if cfg.quick_gelu else "gelu", projection_dim=cfg.proj_dim)
    m = CLIPVisionModelWithProjection(c).eval()
    missing, unexpected = m.load_state_dict(hf_clip_state_dict(cfg, w), strict=False)
    missing = [k for k in missing if "position_ids" not in k]
    assert not unexpected and not missing, (missing, unexpected)
    return m
