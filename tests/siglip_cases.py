"""SigLIP (tanh GELU, no class token, attention-pooling head) -- what the tests of the tanh-GELU epilogue of `ibl_gemm_f16_tn`, of the pooling
head (csrc/siglip.hip) and of the SigLIP configurations share:

  * `emulate_tgelu`: `tanh_gelu2` (csrc/vit_gemm.hip) in numpy fp32, operation for operation, and the fp64 reference `tgelu64`;
  * the per-element bound of IBL_LINEAR_GELU_F16 / _X2 / _X3 with IBL_ACT_GELU_TANH (through ibl_linear_f16_act).  It is the bound of
    tests/gemm_cases.py with two constants exchanged:  LIP_T e1 + C_TGELU max(|v|, TINY) + 2^-11 |ref| + 2^-25  (e1, TINY, SLACK: gemm_cases).
      LIP_T = 1.13 >= max |g'| = 1.12899 (at v = 1.42) carries the accumulation error through the activation.
      C_TGELU |v| is the error of the kernel's form v * rcp(1 + exp2(c v (1 + 0.044715 v^2))): the roundings of v^2, of the fma, of the two
      products in front of the exp2, of 1 + e, the rcp and the final product, and the exp2 of an argument that carries up to two ulp --
      |a| 2^-23 ln 2 relative in e, weighted with e / (1 + e).  It is relative to the result, which is at most |v|.
    C_TGELU is the smallest power of two for which the emulation stays at or under 0.75 of C_TGELU max(|v|, TINY) on `tgelu_grid` -- the
    rule C_GELU and C_QGELU were chosen by; tests/test_siglip_model.py asserts it and prints the ratios: 2^-23 gives 1.14, 2^-22 0.57
    (at v = 1.22).  As there, the emulation uses the exact reciprocal and exp2 where the kernel runs v_rcp_f32 and v_exp_f32 (one ulp).
  * `forward`: the fp32 restatement of the SigLIP forward (trunk without a class token, tanh GELU, then the UNFOLDED attention-pooling
    head as nn.MultiheadAttention computes it; oracle/vit_oracle.py knows neither), pinned against transformers' SiglipVisionModel in
    tests/test_siglip_converters.py; `head_stages` restates the FOLDED head stage by stage in any dtype;
  * the golden cases of tests/golden/siglip_golden.npz (generator: tools/gen_golden_siglip.py mirrors CASES)."""
import numpy as np
import torch

from ibloc_amd import siglip as S
from ibloc_amd import vit as V
from tests import gemm_cases as GC

ACT_TANH = 2                                   # IBL_ACT_GELU_TANH
LIP_T = 1.13
C_TGELU = 2.0 ** -22
K_CUBE = np.float32(0.044715)
C_EXP = np.float32(-2.0 * 1.4426950408889634 * 0.7978845608028654)      # c of tanh_gelu2: -2 log2(e) sqrt(2 / pi), rounded to fp32
SQRT_2_PI = 0.7978845608028654


def tgelu64(v):
    """0.5 v (1 + tanh(z)) = v / (1 + exp(-2 z)), z = sqrt(2 / pi) (v + 0.044715 v^3), in float64 (torch) without overflow or
    cancellation: for z < 0 as v exp(2 z) / (1 + exp(2 z))"""
    z = SQRT_2_PI * (v + 0.044715 * v * v * v)
    e = torch.exp(-2.0 * z.abs())
    return torch.where(z >= 0, v / (1.0 + e), v * e / (1.0 + e))


def emulate_tgelu(v):
    """tanh_gelu2 (csrc/vit_gemm.hip) in numpy fp32, operation for operation (the fma is the one -ffp-contract fuses); v fp32 -> value fp32"""
    f = np.float32
    v = np.asarray(v, f)
    with np.errstate(over="ignore", invalid="ignore"):
        u = v * v
        k = np.where(np.isinf(u), u, GC._fma(u, K_CUBE, f(1.0)))
        w = v * k
        a = w * C_EXP
        e = np.exp2(a.astype(np.float64)).astype(f)           # +inf from a >= 128 on, 0 far below, as v_exp_f32
        d = e + f(1.0)
        r = (1.0 / d.astype(np.float64)).astype(f)            # 1 / inf = 0
        return v * r


def tgelu_grid():
    """tests/clip_openai_cases.qgelu_grid with the overflow edge of this form: exp2(c v (1 + 0.044715 v^2)) overflows from c w = 128 on,
    i.e. at v = -10.07 (inside gelu_grid's -12 .. 12 already); both sides of it in steps of 2^-12 as well"""
    edge = np.arange(-10.5, -9.5, 2.0 ** -12)
    return np.concatenate([GC.gelu_grid(), [200.0, -200.0, 65504.0, -65504.0], np.arange(-54.0, -50.0, 2.0 ** -10), edge]).astype(np.float32)


def tgelu_model_ratio(c_t):
    """-> (worst |value - g(v)| / (c_t max(|v|, TINY)), where, worst error / bound of h + lo / 64) of the emulation over `tgelu_grid`
    (see gemm_cases.gelu_model_ratio)"""
    v = tgelu_grid()
    value = emulate_tgelu(v)
    h = GC.h16(value)
    lo = GC.h16((value - h.astype(np.float32)) * np.float32(GC.SPLIT))
    two = h.astype(np.float64) + lo.astype(np.float64) / GC.SPLIT
    ref = tgelu64(torch.from_numpy(v.astype(np.float64))).numpy()
    poly = c_t * np.maximum(np.abs(v.astype(np.float64)), GC.TINY)
    lo_round = 2.0 ** -11 * (2.0 ** -11 * np.abs(ref) + 2.0 ** -25) + 2.0 ** -31
    r = np.abs(value.astype(np.float64) - ref) / poly
    ok = np.abs(ref) <= GC.F16_MAX
    r2 = np.where(ok, np.abs(two - ref) / ((poly + lo_round) * GC.SLACK), 0.0)
    return float(r.max()), float(v[r.argmax()]), float(r2.max())


def bound_terms(y, S_, K, bias, act64, lip, c_act):
    b = bias if bias is not None else torch.zeros((), dtype=torch.float64, device=y.device)
    v = y + b
    return v, act64(v), lip * GC._e1(S_, bias, K) + c_act * v.abs().clamp_min(GC.TINY)


def expected(y, S_, K, bias=None):
    """-> (ref, bound) float64 (M, N) of the first column block of the GELU epilogues with IBL_ACT_GELU_TANH"""
    v, ref, core = bound_terms(y, S_, K, bias, tgelu64, LIP_T, C_TGELU)
    ref = ref.clamp(-GC.F16_MAX, GC.F16_MAX)
    return ref, (core + GC._f16_round(ref)) * GC.SLACK


def expected_two_term(y, S_, K, bias=None):
    """IBL_LINEAR_GELU_F16_X3 with IBL_ACT_GELU_TANH: -> (ref, bound, valid) for h + lo / 64; valid = h is not saturated"""
    v, ref, core = bound_terms(y, S_, K, bias, tgelu64, LIP_T, C_TGELU)
    lo_round = 2.0 ** -11 * (2.0 ** -11 * ref.abs() + 2.0 ** -25) + 2.0 ** -31
    return ref, (core + lo_round) * GC.SLACK, ref.abs() <= GC.F16_MAX


# ---- the forward in torch, any dtype --------------------------------------------------------------------------------------------------------
def _t(a, device, dtype):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(device=device, dtype=dtype)


@torch.no_grad()
def trunk_tokens(weights: dict, cfg, pixel_values, device="cpu", dtype=torch.float32, tanh=None) -> torch.Tensor:
    """(B, 3, H, W) -> (B, T, D): the trunk without a class token, every token through the final LayerNorm.  tanh: the activation
    (default cfg.tanh_gelu; False = erf GELU on the same weights)"""
    F = torch.nn.functional
    tanh = cfg.tanh_gelu if tanh is None else tanh
    w = {k: _t(v, device, dtype) for k, v in weights.items()}
    x = _t(pixel_values, device, dtype)
    B = x.shape[0]
    assert not cfg.cls_token and tuple(cfg.pos_grid) == tuple(cfg.grid)
    x = F.conv2d(x, w["patch.w"], w.get("patch.b"), stride=cfg.patch).flatten(2).transpose(1, 2) + w["pos"].unsqueeze(0)
    hd = cfg.dim // cfg.heads
    for l in range(cfg.depth):
        p = f"l{l}."
        h = F.layer_norm(x, (cfg.dim,), w[p + "ln1.g"], w[p + "ln1.b"], cfg.ln_eps)
        q, k, v = (F.linear(h, w[p + n + ".w"], w[p + n + ".b"]).view(B, -1, cfg.heads, hd).transpose(1, 2) for n in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1) @ v
        x = x + F.linear(a.transpose(1, 2).reshape(B, -1, cfg.dim), w[p + "o.w"], w[p + "o.b"])
        h = F.layer_norm(x, (cfg.dim,), w[p + "ln2.g"], w[p + "ln2.b"], cfg.ln_eps)
        h = F.gelu(F.linear(h, w[p + "fc1.w"], w[p + "fc1.b"]), approximate="tanh" if tanh else "none")
        x = x + F.linear(h, w[p + "fc2.w"], w[p + "fc2.b"])
    return F.layer_norm(x, (cfg.dim,), w["ln_f.g"], w["ln_f.b"], cfg.ln_eps)


@torch.no_grad()
def head_unfolded(hw: dict, cfg, tokens: torch.Tensor, want_probs=False):
    """the pooling head as nn.MultiheadAttention computes it: keys and values of every token projected, one query.  tokens (B, T, D) in
    the dtype and on the device to compute in -> (B, D) (and the probabilities (B, heads, T))"""
    F = torch.nn.functional
    w = {k: _t(v, tokens.device, tokens.dtype) for k, v in hw.items()}
    B, T, D = tokens.shape
    H, hd = cfg.heads, cfg.dim // cfg.heads
    q = (w["q.w"] @ w["probe"].reshape(-1) + w["q.b"]).view(H, hd)
    k = F.linear(tokens, w["k.w"], w["k.b"]).view(B, T, H, hd)
    v = F.linear(tokens, w["v.w"], w["v.b"]).view(B, T, H, hd)
    p = torch.softmax(torch.einsum("hd,bthd->bht", q, k) * hd ** -0.5, dim=-1)
    a = F.linear(torch.einsum("bht,bthd->bhd", p, v).reshape(B, D), w["o.w"], w["o.b"])
    h = F.layer_norm(a, (D,), w["ln.g"], w["ln.b"], cfg.ln_eps)
    out = a + F.linear(F.gelu(F.linear(h, w["fc1.w"], w["fc1.b"]), approximate="tanh"), w["fc2.w"], w["fc2.b"])
    return (out, p) if want_probs else out


def stage_pool(x: torch.Tensor, u: torch.Tensor):
    """x (B, T, D), u (H, D) in one dtype -> (probs (B, H, T), pooled (B, H, D)): what ibl_probe_pool_f32 computes"""
    p = torch.softmax(torch.einsum("btd,hd->bht", x, u), dim=-1)
    return p, torch.einsum("bht,btd->bhd", p, x)


@torch.no_grad()
def head_stages(hw: dict, cfg, u, tokens, taps: dict, dtype) -> dict:
    """every stage of the FOLDED head in `dtype`, each from the inputs the device had for it: the tokens (probs, pooled) or the tap in
    front of it (vcat < pooled, att < vcat, ln < att, hid < ln, out < att and hid).  u: the folded (heads, dim) fp32 array the device holds."""
    F = torch.nn.functional
    w = {k: _t(v, "cpu", dtype) for k, v in hw.items()}
    t = {k: v.detach().cpu().to(dtype) for k, v in taps.items()}
    B, D, H = tokens.shape[0], cfg.dim, cfg.heads
    hd = D // H
    r = {}
    r["probs"], r["pooled"] = stage_pool(_t(tokens, "cpu", dtype), _t(u, "cpu", dtype))
    r["vcat"] = (torch.einsum("bhd,hid->bhi", t["pooled"], w["v.w"].view(H, hd, D)) + w["v.b"].view(H, hd)).reshape(B, D)
    r["att"] = F.linear(t["vcat"], w["o.w"], w["o.b"])
    r["ln"] = F.layer_norm(t["att"], (D,), w["ln.g"], w["ln.b"], cfg.ln_eps)
    z = F.linear(t["ln"], w["fc1.w"], w["fc1.b"])
    r["hid"] = tgelu64(z) if dtype == torch.float64 else F.gelu(z, approximate="tanh")
    r["out"] = t["att"] + F.linear(t["hid"], w["fc2.w"], w["fc2.b"])
    return r


@torch.no_grad()
def head_folded(hw: dict, cfg, u, tokens: torch.Tensor):
    """the head in the folded form the device runs (include/ibloc.h), in the dtype of `tokens`; u (heads, dim)"""
    F = torch.nn.functional
    w = {k: _t(v, tokens.device, tokens.dtype) for k, v in hw.items()}
    B, T, D = tokens.shape
    H, hd = cfg.heads, cfg.dim // cfg.heads
    _, pooled = stage_pool(tokens, _t(u, tokens.device, tokens.dtype))
    vcat = (torch.einsum("bhd,hid->bhi", pooled, w["v.w"].view(H, hd, D)) + w["v.b"].view(H, hd)).reshape(B, D)
    a = F.linear(vcat, w["o.w"], w["o.b"])
    h = F.layer_norm(a, (D,), w["ln.g"], w["ln.b"], cfg.ln_eps)
    return a + F.linear(F.gelu(F.linear(h, w["fc1.w"], w["fc1.b"]), approximate="tanh"), w["fc2.w"], w["fc2.b"])


GATE_WEIGHT_SEED, GATE_HEAD_SEED, GATE_CROP_SEED = 20, 22, 21


def gate_crops_cpu(ids, hw=(224, 224), seed=GATE_CROP_SEED):
    """tests/test_gpu_flip_rate.GpuCrops in numpy: the synthetic crops of the embedding gates (a low-frequency pattern per id + pixel
    noise), (len(ids), h, w, 3) u8.  Same statistics, not the same noise values"""
    h, w = hw
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    rng = np.random.default_rng([seed, 7])
    out = []
    for k in ids:
        par = np.random.default_rng([seed, int(k)]).uniform(size=(3, 4, 4))
        fx, fy, ph, amp = 0.5 + 5.5 * par[..., 0], 0.5 + 5.5 * par[..., 1], 2 * np.pi * par[..., 2], 0.3 + 0.7 * par[..., 3]
        arg = 2 * np.pi * (fx[..., None, None] * xx + fy[..., None, None] * yy) + ph[..., None, None]
        img = (amp[..., None, None] * np.sin(arg)).sum(1)
        img = ((img - img.min()) / (img.max() - img.min() + 1e-9)).transpose(1, 2, 0)
        out.append(np.clip((img + 0.03 * rng.standard_normal(img.shape)) * 255.0, 0, 255).astype(np.uint8))
    return np.stack(out)


@torch.no_grad()
def forward(weights: dict, head_weights: dict, cfg, pixel_values, device="cpu", tanh=None) -> np.ndarray:
    """pixel_values (B, 3, H, W) float32 -> (B, dim) float32: SiglipVisionModel's pooler_output restated in torch fp32"""
    tok = trunk_tokens(weights, cfg, pixel_values, device=device, tanh=tanh)
    return head_unfolded(head_weights, cfg, tok).cpu().numpy()


# ---- golden cases: (golden key = configuration name, weight seed, head seed, input seed, batch) ---------------------------------------------
CASES = [("tiny_siglip", 311, 321, 411, 5), ("tiny_siglip_384", 312, 322, 412, 5), ("siglip_b16_224", 313, 323, 413, 5)]


def build(case):
    """-> (key, cfg, trunk weights, head weights, pixels): seeded weights and N(0, 1) pixels, regenerated from the seeds.  The fc1
    layers are set so that the activation can be told from the erf form: weights of standard deviation 0.5 / sqrt(dim) and biases around
    -2.7 put the pre-activations at -2.7 +- 0.5, where the two forms of GELU differ most (4.7e-4, 5 % of the value there).  The embeddings
    of the two activations are then 1.0e-3 (tiny_siglip) and 6e-4 (tiny_siglip_384) apart.  With random_weights' own fc1 (pre-activations
    of +-0.3) they are 4e-5 apart, and with any spread around zero at most 2e-4 -- the size of ONE fp16 rounding of the hidden layer, below
    the 3e-4 .. 7e-4 the fp16 forward is from the fp32 one on these two-block models, so that which of the two restatements a result
    lies nearer to would be decided by the direction of its rounding error"""
    key, wseed, hseed, iseed, batch = case
    cfg = V.CONFIGS[key]
    w = V.random_weights(cfg, wseed)
    del w["cls"]
    for l in range(cfg.depth):
        w[f"l{l}.fc1.w"] = w[f"l{l}.fc1.w"] * np.float32(0.5 / cfg.dim ** 0.5 / 0.03)
        w[f"l{l}.fc1.b"] = w[f"l{l}.fc1.b"] + np.float32(-2.7)
    hw = S.random_head_weights(cfg, hseed)
    x = np.random.default_rng(iseed).normal(size=(batch, 3, cfg.img_h, cfg.img_w)).astype(np.float32)
    return key, cfg, w, hw, x


def hf_siglip_state_dict(cfg, w, hw, prefix=""):
    """the seeded weights under the names of transformers' SiglipVisionModel (prefix "vision_model." for the SiglipModel layout)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    sd = {"embeddings.patch_embedding.weight": t(w["patch.w"]), "embeddings.patch_embedding.bias": t(w["patch.b"]),
          "embeddings.position_embedding.weight": t(w["pos"]),
          "post_layernorm.weight": t(w["ln_f.g"]), "post_layernorm.bias": t(w["ln_f.b"]),
          "head.probe": t(hw["probe"]).reshape(1, 1, -1),
          "head.attention.in_proj_weight": t(np.concatenate([hw[n + ".w"] for n in "qkv"], axis=0)),
          "head.attention.in_proj_bias": t(np.concatenate([hw[n + ".b"] for n in "qkv"], axis=0)),
          "head.attention.out_proj.weight": t(hw["o.w"]), "head.attention.out_proj.bias": t(hw["o.b"]),
          "head.layernorm.weight": t(hw["ln.g"]), "head.layernorm.bias": t(hw["ln.b"]),
          "head.mlp.fc1.weight": t(hw["fc1.w"]), "head.mlp.fc1.bias": t(hw["fc1.b"]),
          "head.mlp.fc2.weight": t(hw["fc2.w"]), "head.mlp.fc2.bias": t(hw["fc2.b"])}
    for l in range(cfg.depth):
        p, q = f"encoder.layers.{l}.", f"l{l}."
        sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"] = t(w[q + "ln1.g"]), t(w[q + "ln1.b"])
        sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"] = t(w[q + "ln2.g"]), t(w[q + "ln2.b"])
        for hf, mine in (("q_proj", "q"), ("k_proj", "k"), ("v_proj", "v"), ("out_proj", "o")):
            sd[p + f"self_attn.{hf}.weight"], sd[p + f"self_attn.{hf}.bias"] = t(w[q + mine + ".w"]), t(w[q + mine + ".b"])
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = t(w[q + "fc1.w"]), t(w[q + "fc1.b"])
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = t(w[q + "fc2.w"]), t(w[q + "fc2.b"])
    return {prefix + k: v for k, v in sd.items()}


def hf_siglip_model(cfg, w, hw):
    """transformers' SiglipVisionModel of `cfg` holding the weights `w`, `hw`"""
    from transformers import SiglipVisionConfig, SiglipVisionModel
    c = SiglipVisionConfig(hidden_size=cfg.dim, num_hidden_layers=cfg.depth, num_attention_heads=cfg.heads, intermediate_size=cfg.mlp_dim,
                           image_size=cfg.img_h, patch_size=cfg.patch, layer_norm_eps=cfg.ln_eps, hidden_act="gelu_pytorch_tanh")
    m = SiglipVisionModel(c).eval()
    sd = hf_siglip_state_dict(cfg, w, hw, prefix="vision_model." if any(k.startswith("vision_model.") for k in m.state_dict()) else "")
    missing, unexpected = m.load_state_dict(sd, strict=False)
    missing = [k for k in missing if "position_ids" not in k]
    assert not unexpected and not missing, (missing, unexpected)
    return m
