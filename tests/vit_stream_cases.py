"""Cases, per-stage fp64 references and reference mutants for the chain `ibl_vit_forward` (csrc/vit.hip) and `VitEncoder.__init__`
(ibloc_amd/vit.py) build out of the encoder's kernels; no device.  Shared by tests/test_vit_stream_model.py (CPU: the cases can tell a
correct chain from a mutated one) and tests/test_gpu_vit_stream.py (GPU: the device's chain meets them).

Every stage is fed the DEVICE's own input to it (a workspace tap, include/ibloc.h IBL_VIT_WS_*, or the X of a run with one block less),
so that nothing drifts: what is compared is one kernel launch (two for `resid`) with the operands this file says it should have had.
The operands are restated here from the header's term definitions:
    W_hi = fp16(W), W_lo = fp16((W - W_hi) * S), S = 64
    terms 2: A' = [a | a / S],             W' = [W_hi | W_lo]
    terms 3: A' = [a | a_lo * S | a / S],  W' = [W_hi | W_hi / S | W_lo]
The arithmetic of each stage is composed from what the kernel tests define (layernorm_cases, gemm_cases, clip_openai_cases, siglip_cases,
attention_cases): their emulations give the value every fp16 element is expected to EQUAL, their bounds what it may differ by.

Measures (`check16`, `check32`):
  * fp16 buffers: every element within the kernel test's bound for that epilogue / kernel, and at most CAP = 2 % of the elements not
    bit-equal to the emulation.  The second and third column block of a multi-term row are held as the kernel tests hold them: a / S
    bit for bit from the a that was written, a + a_lo within the bound without the first block's fp16 rounding.
  * fp32 rows (X, outputs): every element within the sum of the gemm_cases bounds of the GEMMs it passed through plus one fp32 ulp per
    addition.
Two allowances that the kernel tests do not need, both first order and derived, not measured:
  * `flip_allowance`: where a stage's GEMM operand is itself emulated here (LayerNorm 1 is not kept by the device), an element of it whose
    fp32 value lies within the LayerNorm's own fp32 bound of an fp16 rounding boundary may have been rounded the other way by the device;
    the GEMM bound grows by |W'| times one fp16 step of exactly those elements.
  * `att_undetermined`: the attention kernel rounds every softmax weight p to fp16 before the PV product.  A p whose fp32 value lies
    within what a correct fp32 implementation may differ by -- one ulp of exp2, the order of the 64-term score sums of p and of the
    row's maximum, in the root mean square as in `check32` -- of an fp16 rounding boundary may be rounded the other way by the device;
    the 64 outputs of that (crop, head, query) row then move by one fp16 step of that p times |v| / sum p, and those of them that lie
    within that distance of their own rounding boundary need not EQUAL the emulation.  They stay out of the unequal share (the bound
    holds them as it holds every element).  The score sums of numpy in three orders measure 0.2 .. 0.5 of 2^-24 sum |q_i k_i| in the
    root mean square and 3.9 of it at most, against the sqrt(66) assumed.  1 .. 7 % of an all-token buffer are excused on these cases
    (up to 25 % of one CLS-only buffer of 384), so the cap asks what it asked of the other 93 % and more.  Why it is needed: ONE dominant
    p rounded the other way moves its row's 64 outputs by a third of a step, and among the 3 x 2 x 17 weights of a CLS-only block that
    is 6 % of its 384 outputs (met on the MI355X: clip, heavy-tailed matrices, block 1; within 0.28 of the bound), which a cap of 2 % of
    so small a buffer cannot hold.
  * `ln_lipschitz`: where a LayerNorm's input is itself a reference value with a bound d (the residual after the output projection is
    overwritten before the call returns), the output moves by at most rstd |g_i| (d_i + mean d + |xhat_i| sqrt(mean d^2)).

One deviation from the issue that asked for this: it names proj_dim 64 for the clip family, which the GEMM refuses (n_out must be a
multiple of 128, launch_gemm); the family runs proj_dim 128, the smallest the library takes."""
import dataclasses
import functools

import numpy as np
import torch

from ibloc_amd import vit as V
from tests import attention_cases as AC
from tests import clip_openai_cases as CQ
from tests import gemm_cases as GC
from tests import layernorm_cases as LC
from tests import siglip_cases as SC

S = 64.0                       # IBL_VIT_SPLIT_SCALE
CAP = 0.02                     # largest share of fp16 elements that may differ from the emulation
BATCH = 3
DEPTH = 3
WSEED, ISEED = 7301, 7401

FAMILIES = {
    # class token, LayerScale, patch 14 (588 -> 640 padded), final LN, erf GELU: 7 tokens
    "dino": V.VitConfig("stream_dino", 128, DEPTH, 2, 256, 14, 28, 42, (2, 3), layerscale=True, recipe="dinov2"),
    # patch 16, no LayerScale: 17 tokens
    "vit": V.VitConfig("stream_vit", 128, DEPTH, 2, 256, 16, 64, 64, (4, 4), ln_eps=1e-12, recipe="vit"),
    # pre-LN, projection, QuickGELU, no patch bias: 17 tokens
    "clip": V.VitConfig("stream_clip", 128, DEPTH, 2, 256, 16, 64, 64, (4, 4), pre_ln=True, proj_dim=128, ln_eps=1e-5, recipe="clip",
                        quick_gelu=True),
    # no class token, tanh GELU, all tokens, final LN: 20 tokens (4 x 5 patches, so that the rows still cross a 16-wide tile)
    "siglip": V.VitConfig("stream_siglip", 128, DEPTH, 2, 256, 16, 64, 80, (4, 5), out_all_tokens=True, recipe="siglip", cls_token=False,
                          tanh_gelu=True),
}
PLANS = ("plain", "p2;*:2222", "p2;*:3333", "p2;0:3232;1:2211;2:2111")
# (family, plan, kext, fold): the launch-per-term form and LayerScale folded into the weights
EXTRA = [(f, "p2;*:2222", kext, fold) for f in ("dino", "vit") for kext, fold in ((False, False), (True, True), (False, True))]


@functools.lru_cache(maxsize=None)
def inputs(family, kind="random"):
    """-> (cfg, weights, pixels (BATCH, 3, H, W) fp32).  kind: "random" = `random_weights` as they are, else those weights with the
    trained-like statistics of that name (tests/vit_trained_cases.py)"""
    cfg = FAMILIES[family]
    w = V.random_weights(cfg, WSEED + list(FAMILIES).index(family))
    if family == "clip":
        del w["patch.b"]                 # the null-bias path of the patch GEMM
    if kind != "random":
        from tests import vit_trained_cases as TC
        w = TC.trained_like(cfg, w, TC.SEED + list(FAMILIES).index(family), kind)
    px = np.random.default_rng(ISEED + list(FAMILIES).index(family)).normal(size=(BATCH, 3, cfg.img_h, cfg.img_w)).astype(np.float32)
    return cfg, w, px


def run_cfg(family, n_run, all_tokens, final_ln=None, proj=True):
    """the family's configuration for one run: n_blocks_run, all tokens or the class rows, final LN on or off, projection kept or not"""
    cfg = FAMILIES[family]
    return dataclasses.replace(cfg, n_blocks_run=n_run, out_all_tokens=all_tokens, final_ln=cfg.final_ln if final_ln is None else final_ln,
                               proj_dim=cfg.proj_dim if proj else 0)


def plan_without(plan, block):
    """the plan with every block's entry spelled out and `block` left plain"""
    patch, layers = V.parse_precision(plan)
    parts = [f"p{patch}"]
    for l in range(DEPTH):
        t = layers.get(l, layers.get("*"))
        if t is not None and l != block:
            parts.append(f"{l}:" + "".join(str(v) for v in t))
    return ";".join(parts)


# ---- operands, restated from include/ibloc.h -------------------------------------------------------------------------------------------
def f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float32).astype(np.float16)


def w_terms(w, terms):
    """fp32 (N, K) -> fp16 (N, terms * K) operand rows"""
    w = np.asarray(w, np.float32)
    hi = f16(w)
    if terms == 1:
        return hi
    lo = f16((w - hi.astype(np.float32)) * np.float32(S))
    if terms == 2:
        return np.concatenate([hi, lo], axis=1)
    return np.concatenate([hi, f16(hi.astype(np.float32) / np.float32(S)), lo], axis=1)


def w_lo(w):
    w = np.asarray(w, np.float32)
    return f16((w - f16(w).astype(np.float32)) * np.float32(S))


def a_terms(a16, value32, terms, split):
    """first block a16 (fp16) and the fp32 value it was rounded from -> (rows, terms * K) fp16, by the kernel test's `split_terms`"""
    if terms == 1:
        return a16
    over, lo = split(a16, value32)
    return np.concatenate([a16, over] if terms == 2 else [a16, lo, over], axis=1)


class Model:
    """What one encoder (family, plan, kext, fold) should hand its kernels.  mutant: a name of MUTANTS, applied where it says."""

    def __init__(self, family, plan, kext=True, fold=False, kind="random"):
        self.family, self.plan, self.kext, self.fold, self.kind = family, plan, kext, fold, kind
        self.cfg, self.w, self.px = inputs(family, kind)
        c = self.cfg
        self.patch_terms, self.layer_terms = V.parse_precision(plan)
        self.D, self.T, self.P, self.H, self.MLP = c.dim, c.n_tokens, c.n_patches, c.heads, c.mlp_dim
        self.eps = np.float32(c.ln_eps)
        gh, gw = c.grid
        p = c.patch
        t = self.px.reshape(BATCH, 3, gh, p, gw, p).transpose(0, 2, 4, 1, 3, 5).reshape(BATCH * gh * gw, 3 * p * p)
        self.patches = np.zeros((BATCH * self.P, c.patch_k_pad), np.float16)
        self.patches[:, :c.patch_k] = f16(t)

    def terms(self, l, cls_only, mutant=None):
        """(qt, ot, ft, f2t) block l runs with: the plan's, one everywhere in a CLS-only block"""
        t = self.layer_terms.get(l, self.layer_terms.get("*"))
        if t is None or (cls_only and mutant != "cls_block_terms"):
            return (1, 1, 1, 1)
        # IBL_VIT_RESID_KEXT=0: the residual GEMMs take one-term rows and their second weight term as a launch of its own (`lo_launch`)
        return t if self.kext else (t[0], 1, t[2], 1)

    def lo_launch(self, l, cls_only):
        """(o, fc2): the second weight term of the residual GEMM runs as its own launch (the older form; never in a CLS-only block)"""
        t = self.layer_terms.get(l, self.layer_terms.get("*"))
        if t is None or cls_only or self.kext:
            return (False, False)
        return (t[1] == 2, t[3] == 2)

    def layer(self, l):
        """fp32 weights of block l as the host prepares them: qkv stacked, LayerScale folded or as vectors (ones without)"""
        w, c, p = self.w, self.cfg, f"l{l}."
        f32 = np.float32
        d = dict(g1=w[p + "ln1.g"], b1=w[p + "ln1.b"], g2=w[p + "ln2.g"], b2=w[p + "ln2.b"],
                 wqkv=np.concatenate([w[p + "q.w"], w[p + "k.w"], w[p + "v.w"]], axis=0),
                 bqkv=np.concatenate([w[p + "q.b"], w[p + "k.b"], w[p + "v.b"]], axis=0),
                 wo=w[p + "o.w"], bo=w[p + "o.b"], w1=w[p + "fc1.w"], bb1=w[p + "fc1.b"], w2=w[p + "fc2.w"], bb2=w[p + "fc2.b"],
                 ls1=None, ls2=None)
        if c.layerscale:
            ls1, ls2 = np.asarray(w[p + "ls1"], f32), np.asarray(w[p + "ls2"], f32)
            if self.fold:
                d["wo"], d["bo"] = ls1[:, None] * np.asarray(d["wo"], f32), ls1 * np.asarray(d["bo"], f32)
                d["w2"], d["bb2"] = ls2[:, None] * np.asarray(d["w2"], f32), ls2 * np.asarray(d["bb2"], f32)
            else:
                d["ls1"], d["ls2"] = ls1, ls2
        return {k: (None if v is None else np.asarray(v, f32)) for k, v in d.items()}


MUTANTS = ("w_term2", "a_term2", "swap23", "ls_not_bias", "kv_bias0", "cls_block_terms")
# w_term2: the second weight term dropped; a_term2: the activation's second term dropped; swap23: column blocks 2 and 3 of a three-term row
# swapped; ls_not_bias: LayerScale applied to the product but not to the bias; kv_bias0: the K / V bias of a CLS-only block read from offset
# 0; cls_block_terms: the plan's terms applied to the CLS-only block


def applies(mutant, m, stage, l=None, cls_only=False):
    """does `mutant` change what `stage` of block l should compute?  (stages: patch qkv att ln2 hid resid proj)"""
    if stage == "patch":
        return mutant == "w_term2" and m.patch_terms == 2
    if stage == "proj":
        return mutant in ("w_term2", "a_term2", "swap23") and m.plan != "plain"
    if mutant == "kv_bias0":
        return cls_only and stage == "qkv"
    qt, ot, ft, f2t = m.terms(l, cls_only)
    lo_o, lo_f = m.lo_launch(l, cls_only)
    if mutant == "cls_block_terms":
        pt = m.terms(l, True, "cls_block_terms")
        return cls_only and {"qkv": pt[0] > 1, "att": pt[1] > 1, "ln2": pt[2] > 1, "hid": pt[2] > 1 or pt[3] > 1,
                             "resid": pt[1] > 1 or pt[3] > 1}[stage]
    if mutant == "ls_not_bias":
        return stage in ("ln2", "resid") and m.cfg.layerscale and not m.fold
    if mutant == "w_term2":
        # (the output projection's terms are seen at `resid`: after LN2 and its fp16 rounding they move a few elements of XN only)
        return {"qkv": qt > 1, "att": False, "ln2": False, "hid": ft > 1, "resid": ot > 1 or f2t > 1 or lo_o or lo_f}[stage]
    if mutant == "a_term2":
        return {"qkv": qt == 3, "att": False, "ln2": False, "hid": ft == 3, "resid": ot == 3 or f2t == 3}[stage]
    if mutant == "swap23":          # (at the stage that WRITES a three-term row the swap shows in the a / S block: `att`, and `ln2` for ft)
        return {"qkv": qt == 3, "att": ot == 3, "ln2": ft == 3, "hid": ft == 3, "resid": ot == 3 or f2t == 3}[stage]
    raise KeyError(mutant)


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------------
def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def mm(a16, w16, acc):
    """x W^T of fp16 operands: acc = np.float64 (the reference's and the emulation's) or np.float32 (the stand-in for a device)"""
    return np.asarray(a16, acc) @ np.asarray(w16, acc).T


def drop_w2(w16, terms, K):
    """mutant w_term2: the W_lo block zeroed"""
    w = w16.copy()
    if terms >= 2:
        w[:, (terms - 1) * K:] = 0
    return w


def drop_a2(a16, terms, K):
    """mutant a_term2: the a_lo block zeroed"""
    a = a16.copy()
    if terms == 3:
        a[:, K:2 * K] = 0
    return a


def swap23(a16, terms, K):
    """mutant swap23: column blocks 2 and 3 of a three-term row exchanged"""
    if terms != 3:
        return a16
    return np.concatenate([a16[:, :K], a16[:, 2 * K:], a16[:, K:2 * K]], axis=1)


def widen(a16, terms, K):
    """one-term rows as rows of `terms` blocks (what a reference that applies the plan to a CLS-only block would multiply)"""
    if a16.shape[1] == terms * K:
        return a16
    return a_terms(a16[:, :K], a16[:, :K].astype(np.float32), terms, LC.split_terms)


def flip_allowance(value32, ln_bnd, w16):
    """see the module docstring -> (rows, N) float64"""
    v = value32.astype(np.float64)
    a = f16(value32).astype(np.float64)
    step = LC.ulp16(v)
    dist = step / 2 - np.abs(v - a)                       # distance of the value from the nearest rounding boundary
    may = (dist <= 2 * ln_bnd) * step
    return may @ np.abs(w16.astype(np.float64)).T


def att_undetermined(q, k, v, value32):
    """see the module docstring: q (B, H, Tq, 64), k, v (B, H, T, 64) fp16, value32 (B, H, Tq, 64) the emulation's fp32 outputs ->
    bool (B, H, Tq, 64), True where the device's fp16 output need not equal the emulation's"""
    q64, k64, v64 = (a.astype(np.float64) for a in (q, k, v))
    c2 = 0.125 * 1.4426950408889634
    s = np.einsum("bhqd,bhkd->bhqk", q64, k64)
    s_abs = np.einsum("bhqd,bhkd->bhqk", np.abs(q64), np.abs(k64))
    top = np.take_along_axis(s_abs, s.argmax(axis=-1)[..., None], axis=-1)             # the sum of |products| of the row's maximum
    ds = np.sqrt(AC.HD + 2.0) * 2.0 ** -24 * (s_abs + top)
    p = np.exp2((s - s.max(axis=-1, keepdims=True)) * c2)
    dp = p * (2.0 ** -23 + np.log(2.0) * c2 * ds)
    p16 = f16(p.astype(np.float32)).astype(np.float64)
    step = LC.ulp16(p)
    flag = (step / 2 - np.abs(p - p16) <= dp) * step                                   # one fp16 step of exactly those p
    move = np.einsum("bhqk,bhkd->bhqd", flag, np.abs(v64)) / p.sum(axis=-1, keepdims=True)
    val = value32.astype(np.float64)
    ostep = LC.ulp16(val)
    dist = ostep / 2 - np.abs(val - f16(value32).astype(np.float64))
    return (move > 0) & (dist <= move + 4 * 2.0 ** -24 * np.abs(val))


def ln_lipschitz(x64, g, eps, d):
    mean = x64.mean(axis=1, keepdims=True)
    var = ((x64 - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + np.float64(eps))
    xhat = (x64 - mean) * rstd
    return rstd * np.abs(g.astype(np.float64)) * (d + d.mean(axis=1, keepdims=True) + np.abs(xhat) * np.sqrt((d * d).mean(axis=1, keepdims=True)))


def ln_stage(x32, g, b, eps, terms, in_bnd=None, x64=None):
    """LayerNorm of fp32 rows to fp16 rows of `terms` blocks -> dict emu (fp16), value (fp32), ref, bnd (first block, float64)"""
    value = LC.emulate(x32, g, b, eps)
    a16 = f16(np.clip(value, -65504.0, 65504.0))
    ref, bnd = LC.reference(x32, g, b, eps)
    if in_bnd is not None:
        ref, _ = _ln64(x64, g, b, eps)
        bnd = (bnd + ln_lipschitz(x64, g, eps, in_bnd)) * GC.SLACK
    return dict(emu=a_terms(a16, value, terms, LC.split_terms), value=value, ref=ref, bnd32=bnd, bnd=bnd + LC.ulp16(ref) / 2, terms=terms,
                lo_rel=2.0 ** -21)


def _ln64(x64, g, b, eps):
    mean = x64.mean(axis=1, keepdims=True)
    var = ((x64 - mean) ** 2).mean(axis=1, keepdims=True)
    xhat = (x64 - mean) / np.sqrt(var + np.float64(np.float32(eps)))
    return xhat * g.astype(np.float64) + b.astype(np.float64), xhat


def k_rms(K):
    """the K at which gemm_cases' accumulation term (K + 2) u (S + |bias|) becomes sqrt(K + 2) u (S + |bias|): see `check32`"""
    return float(np.sqrt(K + 2.0) - 2.0)


def resid_step(x, a16, w16, bias, scale, acc, alpha=None, x_emu=None):
    """one residual GEMM -> (emu fp32, ref, bnd, rms): EPI_RESID_F32 x + scale * (a W^T + bias), or with alpha EPI_RESID_PRE_F32
    x + alpha * (a W^T) (the launch-per-term form without a scale vector); ref and the bounds start from x, the emulation from x_emu
    (fp32; x itself where none is given)"""
    f32 = np.float32
    K = a16.shape[1]
    y = mm(a16, w16, acc)
    yt, St = GC.products(torch.from_numpy(a16), torch.from_numpy(w16))
    x32 = np.asarray(x if x_emu is None else x_emu, f32)
    kw = dict(bias=None if bias is None else t64(bias), scale=None if scale is None else t64(scale), resid=t64(x))
    if alpha is None:
        ref, bnd = GC.expected(GC.EPI_RESID, yt, St, K, **kw)
        rms = GC.expected(GC.EPI_RESID, yt, St, k_rms(K), **kw)[1]
        v = y.astype(f32) + (f32(0) if bias is None else bias)
        emu = x32 + (v * scale if scale is not None else v)
    else:
        ref, bnd = GC.expected(GC.EPI_PRE, yt, St, K, bias=None, resid=t64(x), alpha=alpha)
        rms = GC.expected(GC.EPI_PRE, yt, St, k_rms(K), bias=None, resid=t64(x), alpha=alpha)[1]
        emu = ((x32 * f32(1.0 / alpha)).astype(np.float64) + y).astype(f32) * f32(alpha)
    return emu.astype(f32), ref.numpy(), bnd.numpy(), rms.numpy()


# ---- stages ----------------------------------------------------------------------------------------------------------------------------
def stage_patch(m, acc=np.float64, mutant=None):
    """patches -> x_0 (BATCH * T, D) fp32 (for clip: after the in-place pre-LN) -> dict emu, ref, bnd"""
    c, w, f32 = m.cfg, m.w, np.float32
    wp = np.zeros((m.D, c.patch_k_pad), f32)
    wp[:, :c.patch_k] = w["patch.w"].reshape(m.D, -1)
    pos = np.asarray(w["pos"], f32)
    bias = np.asarray(w["patch.b"], f32) if "patch.b" in w else None
    pos_patch = pos[1:] if c.cls_token else pos
    K = c.patch_k_pad
    pos_rows = np.tile(pos_patch, (BATCH, 1))
    a = m.patches
    hi = f16(wp)
    yt, St = GC.products(torch.from_numpy(a), torch.from_numpy(hi))
    ref, bnd = GC.expected(GC.EPI_PATCH, yt, St, K, bias=None if bias is None else t64(bias), pos=t64(pos_rows))
    rms = GC.expected(GC.EPI_PATCH, yt, St, k_rms(K), bias=None if bias is None else t64(bias), pos=t64(pos_rows))[1]
    emu = (mm(a, hi, acc).astype(f32) + (f32(0) if bias is None else bias)) + pos_rows
    if m.patch_terms == 2 and mutant != "w_term2":
        lo = w_lo(wp)
        y2, S2 = GC.products(torch.from_numpy(a), torch.from_numpy(lo))
        ref2, bnd2 = GC.expected(GC.EPI_PATCH, y2, S2, K, resid=ref, alpha=1.0 / S, accumulate=True)
        rms = rms + GC.expected(GC.EPI_PATCH, y2, S2, k_rms(K), resid=ref, alpha=1.0 / S, accumulate=True)[1]
        ref, bnd = ref2, bnd + bnd2
        emu = (mm(a, lo, acc).astype(f32).astype(np.float64) / S + emu.astype(np.float64)).astype(f32)      # fmaf(v, 1 / S, x)
    ref, bnd, rms = ref.numpy(), bnd.numpy(), rms.numpy()
    if c.cls_token:
        cls = (np.asarray(w["cls"], f32).reshape(-1) + pos[0]).astype(f32)          # the host's fp32 sum, stored as is
        full = lambda rows, crow: np.concatenate([np.broadcast_to(crow, (BATCH, 1, m.D)), rows.reshape(BATCH, m.P, m.D)], axis=1).reshape(-1, m.D)
        emu, ref, bnd, rms = full(emu, cls), full(ref, cls.astype(np.float64)), full(bnd, np.zeros(m.D)), full(rms, np.zeros(m.D))
    if c.pre_ln:
        g, b = np.asarray(w["ln_pre.g"], f32), np.asarray(w["ln_pre.b"], f32)
        _, lb = LC.reference(emu, g, b, m.eps)
        r64, _ = _ln64(ref, g, b, m.eps)
        bnd, rms = (lb + ln_lipschitz(ref, g, m.eps, bnd)) * GC.SLACK, (lb + ln_lipschitz(ref, g, m.eps, rms)) * GC.SLACK
        emu, ref = LC.emulate(emu, g, b, m.eps), r64
    return dict(emu=emu.astype(f32), ref=ref, bnd=bnd, rms=rms)


def gemm16(a16, w16, bias, acc, act=None, terms=1, extra=None):
    """fp16-output GEMM (EPI_BIAS_H16, or a GELU epilogue of `terms` column blocks) -> dict emu, ref, bnd (first block), two = (ref, bnd,
    valid) of h + lo / S for three terms"""
    f32 = np.float32
    K = a16.shape[1]
    yt, St = GC.products(torch.from_numpy(a16), torch.from_numpy(w16))
    bt = None if bias is None else t64(bias)
    v = mm(a16, w16, acc).astype(f32) + (f32(0) if bias is None else bias)
    two = None
    if act is None:
        ref, bnd = GC.expected(GC.EPI_F16, yt, St, K, bias=bt)
        value = v
    else:
        exp, exp2, emulate = {"erf": (lambda *a, **k: GC.expected(GC.EPI_GELU, *a, **k), GC.expected_two_term, GC.emulate_gelu),
                              "quick": (CQ.expected, CQ.expected_two_term, CQ.emulate_qgelu),
                              "tanh": (SC.expected, SC.expected_two_term, SC.emulate_tgelu)}[act]
        ref, bnd = exp(yt, St, K, bias=bt)
        value = emulate(v)
        if terms == 3:
            two = tuple(t.numpy() for t in exp2(yt, St, K, bias=bt))
    h = GC.h16(value)
    bnd = bnd.numpy()
    if extra is not None:
        bnd = bnd + extra * GC.SLACK
        if two is not None:
            two = (two[0], two[1] + extra * GC.SLACK, two[2])
    return dict(emu=a_terms(h, np.asarray(value, f32), terms, LC.split_terms), ref=ref.numpy(), bnd=bnd, terms=terms, two=two)


def act_of(cfg):
    return "quick" if cfg.quick_gelu else ("tanh" if cfg.tanh_gelu else "erf")


def stage_qkv(m, l, x_prev, acc=np.float64, mutant=None, cls_only=False):
    """x_{l-1} (rows, D) fp32 -> LN1 in qt terms -> QKV.  cls_only: -> also `xn` (LN1 in one term, which the device keeps)"""
    L = m.layer(l)
    qt = m.terms(l, cls_only, mutant)[0]
    ln = ln_stage(x_prev, L["g1"], L["b1"], m.eps, qt)
    a, w16 = ln["emu"], w_terms(L["wqkv"], qt)
    if mutant == "w_term2":
        w16 = drop_w2(w16, qt, m.D)
    if mutant == "a_term2":
        a = drop_a2(a, qt, m.D)
    if mutant == "swap23":
        a = swap23(a, qt, m.D)
    return gemm16(a, w16, L["bqkv"], acc, extra=flip_allowance(ln["value"], ln["bnd32"], w16[:, :m.D]))


def stage_qkv_cls(m, l, xn, acc=np.float64, mutant=None):
    """CLS-only block: the device's LN1 rows xn (rows, D) fp16 -> (kv: k | v of every row (rows, 2 D), q: of the class rows (BATCH, D))"""
    L = m.layer(l)
    qt = m.terms(l, True, mutant)[0]
    w16 = w_terms(L["wqkv"], qt)
    a = xn if qt == 1 else a_terms(xn, xn.astype(np.float32), qt, LC.split_terms)
    bkv = L["bqkv"][:2 * m.D] if mutant == "kv_bias0" else L["bqkv"][m.D:]
    kv = gemm16(a, w16[m.D:], bkv, acc)
    q = gemm16(a[::m.T], w16[:m.D], L["bqkv"][:m.D], acc)
    return kv, q


def stage_att(m, l, qkv, acc=np.float64, mutant=None, cls_only=False):
    """QKV (BATCH, T, 3 D) fp16 -> ATT rows (BATCH * T or BATCH, ot * D)"""
    ot = m.terms(l, cls_only, mutant)[1]
    B, T, D, H = qkv.shape[0], m.T, m.D, m.H
    q, k, v = (qkv[:, :, i * D:(i + 1) * D].reshape(B, T, H, AC.HD).transpose(0, 2, 1, 3) for i in range(3))
    if cls_only:
        q = q[:, :, :1]
    ref, A, _ = AC.reference(q, k, v)
    bnd = AC.bound(ref, A, v)
    if acc == np.float32:                       # the stand-in for a device: the same arithmetic, keys summed in the other order
        a16, value = AC.emulate(q, k[:, :, ::-1], v[:, :, ::-1])
    else:
        a16, value = AC.emulate(q, k, v)
    rows = lambda x: np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(-1, D)
    may = rows(att_undetermined(q, k, v, value))
    a16, value = rows(a16), rows(value)
    emu = a_terms(a16, value, ot, AC.split_terms)
    if mutant == "swap23":
        emu = swap23(emu, ot, D)
    return dict(emu=emu, ref=rows(ref), bnd=rows(bnd), terms=ot, lo_bnd=rows(AC.bound(ref, A, v, out_rel=2.0 ** -21)), may=may)


def resid_o(m, l, x_prev, att, acc, mutant=None, cls_only=False):
    """x_mid = x_{l-1} + ls1 * (ATT W_o'^T + b_o) -> (emu fp32, ref, bnd, rms); att: the device's rows (rows, ot * D)"""
    L = m.layer(l)
    ot = m.terms(l, cls_only, mutant)[1]
    return _resid(m, x_prev, att, L["wo"], L["bo"], L["ls1"], ot, m.D, acc, mutant, m.lo_launch(l, cls_only)[0])


def _resid(m, x, a16, w, bias, ls, terms, K, acc, mutant, lo_launch, x_emu=None):
    w16 = w_terms(w, terms)
    if mutant == "w_term2":
        w16 = drop_w2(w16, terms, K)
    a = widen(a16, terms, K)
    if mutant == "swap23":
        a = swap23(a, terms, K)
    if mutant == "a_term2":
        a = drop_a2(a, terms, K)
    if mutant == "ls_not_bias" and ls is not None:
        emu, ref, bnd, rms = resid_step(x, a, w16, None, ls, acc, x_emu=x_emu)
        emu, ref = (emu + bias).astype(np.float32), ref + bias.astype(np.float64)
    else:
        emu, ref, bnd, rms = resid_step(x, a, w16, bias, ls, acc, x_emu=x_emu)
    if lo_launch and mutant != "w_term2":          # the launch-per-term form: + (ls / S) * (a W_lo^T), or alpha = 1 / S without a vector
        lo = w_lo(w)
        if m.fold:
            emu, ref2, b2, r2 = resid_step(ref, a, lo, None, None, acc, alpha=1.0 / S, x_emu=emu)
        else:
            sc = ((ls if ls is not None else np.ones(m.D, np.float32)) / np.float32(S)).astype(np.float32)
            emu, ref2, b2, r2 = resid_step(ref, a, lo, None, sc, acc, x_emu=emu)
        ref, bnd, rms = ref2, bnd + b2, rms + r2
    return emu, ref, bnd, rms


def stage_ln2(m, l, x_prev, att, acc=np.float64, mutant=None, cls_only=False):
    """(x_{l-1}, ATT) -> x_mid -> LN2 in ft terms: XN rows, or FIN (one term) for the class rows of a CLS-only block"""
    L = m.layer(l)
    ft = m.terms(l, cls_only, mutant)[2]
    emu, ref, bnd, _ = resid_o(m, l, x_prev, att, acc, mutant, cls_only)
    out = ln_stage(emu, L["g2"], L["b2"], m.eps, ft, in_bnd=bnd, x64=ref)
    if mutant == "swap23":
        out["emu"] = swap23(out["emu"], ft, m.D)
    return out


def stage_hid(m, l, xn, acc=np.float64, mutant=None, cls_only=False):
    """XN rows (rows, ft * D) fp16 (the device's) -> HID rows (rows, f2t * MLP)"""
    L = m.layer(l)
    _, _, ft, f2t = m.terms(l, cls_only, mutant)
    w16 = w_terms(L["w1"], ft)
    if mutant == "w_term2":
        w16 = drop_w2(w16, ft, m.D)
    a = widen(xn, ft, m.D)
    if mutant == "a_term2":
        a = drop_a2(a, ft, m.D)
    if mutant == "swap23":
        a = swap23(a, ft, m.D)
    return gemm16(a, w16, L["bb1"], acc, act=act_of(m.cfg), terms=f2t)


def stage_resid(m, l, x_prev, att, hid, acc=np.float64, mutant=None, cls_only=False):
    """(x_{l-1}, ATT, HID) -> X = x_{l-1} + ls1 * (ATT W_o'^T + b_o) + ls2 * (HID W_fc2'^T + b_fc2) -> dict emu, ref, bnd"""
    L = m.layer(l)
    f2t = m.terms(l, cls_only, mutant)[3]
    emu, ref, bnd, rms = resid_o(m, l, x_prev, att, acc, mutant, cls_only)
    lo2 = m.lo_launch(l, cls_only)[1]
    emu2, ref2, bnd2, rms2 = _resid(m, ref, hid, L["w2"], L["bb2"], L["ls2"], f2t, m.MLP, acc, mutant, lo2, x_emu=emu)
    ulps = 2 * 2.0 ** -23 * np.abs(ref2)
    return dict(emu=emu2, ref=ref2, bnd=bnd + bnd2 + ulps, rms=rms + rms2 + ulps)


def stage_out_ln(m, x, acc=np.float64):
    """final LayerNorm to fp32 rows (all tokens, or the class rows without a projection) -> dict emu, ref, bnd"""
    g, b = np.asarray(m.w["ln_f.g"], np.float32), np.asarray(m.w["ln_f.b"], np.float32)
    ref, bnd = LC.reference(x, g, b, m.eps)
    return dict(emu=LC.emulate(x, g, b, m.eps), ref=ref, bnd=bnd)


def stage_out_proj(m, x_cls, acc=np.float64, mutant=None):
    """class rows (BATCH, D) fp32 -> (ln: the final LayerNorm as the projection's operand rows -- one term in FIN under `plain`, three in
    XN under a plan --, proj(a16): those rows (the device's) -> out (BATCH, out_dim) fp32)"""
    terms = 1 if m.plan == "plain" else 3
    g, b = np.asarray(m.w["ln_f.g"], np.float32), np.asarray(m.w["ln_f.b"], np.float32)
    ln = ln_stage(x_cls, g, b, m.eps, terms)
    w16 = w_terms(m.w["proj.w"], terms)
    if mutant == "w_term2":
        w16 = drop_w2(w16, terms, m.D)

    def proj(a16):
        if mutant == "a_term2":
            a16 = drop_a2(a16, terms, m.D)
        if mutant == "swap23":
            a16 = swap23(a16, terms, m.D)
        yt, St = GC.products(torch.from_numpy(a16), torch.from_numpy(w16))
        ref, bnd = GC.expected(GC.EPI_F32, yt, St, a16.shape[1])
        rms = GC.expected(GC.EPI_F32, yt, St, k_rms(a16.shape[1]))[1]
        return dict(emu=mm(a16, w16, acc).astype(np.float32), ref=ref.numpy(), bnd=bnd.numpy(), rms=rms.numpy())
    return ln, proj


def stage_ln1_cls(m, l, x_prev):
    """CLS-only block: x_{l-1} -> LN1 in one term, which stays in XN (the second LayerNorm of such a block goes to FIN)"""
    L = m.layer(l)
    return ln_stage(x_prev, L["g1"], L["b1"], m.eps, 1)


def block_checks(m, l, x_prev, dev, mutant=None, cls_only=False, acc=np.float64, stages=None):
    """Every stage of block l against what a device left: x_prev (rows, D) fp32 and dev = dict of numpy arrays qkv (BATCH, T, 3 D), att,
    xn, hid (rows, terms * width), x (rows, D), fin (BATCH, D) -> list of (stage, ratio, share or None, ok)"""
    D, T = m.D, m.T
    out = []

    def want(s):
        return stages is None or s in stages

    def c16(name, got, st, K):
        r, sh, ok = check16(("cls_" if cls_only else "") + name, got, st, K)
        out.append((name, r, sh, ok))

    def c32(name, got, st):
        r, ok = check32(("cls_" if cls_only else "") + name, got, st)
        out.append((name, r, None, ok))

    if not cls_only:
        if want("qkv"):
            c16("qkv", dev["qkv"].reshape(-1, 3 * D), stage_qkv(m, l, x_prev, acc, mutant), 3 * D)
        if want("att"):
            c16("att", dev["att"], stage_att(m, l, dev["qkv"], acc, mutant), D)
        if want("ln2"):
            c16("ln2", dev["xn"], stage_ln2(m, l, x_prev, dev["att"], acc, mutant), D)
        if want("hid"):
            c16("hid", dev["hid"], stage_hid(m, l, dev["xn"], acc, mutant), m.MLP)
        if want("resid"):
            c32("resid", dev["x"], stage_resid(m, l, x_prev, dev["att"], dev["hid"], acc, mutant))
        return out
    xc, att_c = np.ascontiguousarray(x_prev[::T]), np.ascontiguousarray(dev["att"][::T, :D])
    if want("ln1"):
        c16("ln1", dev["xn"], stage_ln1_cls(m, l, x_prev), D)
    if want("qkv"):
        kv, q = stage_qkv_cls(m, l, dev["xn"], acc, mutant)
        qkv2 = dev["qkv"].reshape(-1, 3 * D)
        c16("qkv", np.ascontiguousarray(qkv2[:, D:]), kv, 2 * D)
        c16("qkv", np.ascontiguousarray(qkv2[::T, :D]), q, D)
    if want("att"):
        c16("att", att_c, stage_att(m, l, dev["qkv"], acc, mutant, cls_only=True), D)
    if want("ln2"):
        c16("ln2", dev["fin"], stage_ln2(m, l, xc, att_c, acc, mutant, cls_only=True), D)
    if want("hid"):
        c16("hid", dev["hid"][:BATCH, :m.MLP], stage_hid(m, l, dev["fin"], acc, mutant, cls_only=True), m.MLP)
    if want("resid"):
        c32("resid", dev["x"][::T], stage_resid(m, l, xc, att_c, np.ascontiguousarray(dev["hid"][:BATCH, :m.MLP]), acc, mutant, cls_only=True))
    return out


def stand_in(m, l, x_prev, cls_only=False, acc=np.float32):
    """What a device that accumulates in fp32, in numpy's order, would leave of block l: the `dev` of `block_checks`, each stage from the
    stand-in's own previous one.  (acc = np.float64: the emulation itself chained, what the design gives without accumulation error)"""
    D, T = m.D, m.T
    dev = {}
    if not cls_only:
        dev["qkv"] = stage_qkv(m, l, x_prev, acc)["emu"].reshape(BATCH, T, 3 * D)
        dev["att"] = stage_att(m, l, dev["qkv"], acc)["emu"]
        dev["xn"] = stage_ln2(m, l, x_prev, dev["att"], acc)["emu"]
        dev["hid"] = stage_hid(m, l, dev["xn"], acc)["emu"]
        dev["x"] = stage_resid(m, l, x_prev, dev["att"], dev["hid"], acc)["emu"]
        return dev
    dev["xn"] = stage_ln1_cls(m, l, x_prev)["emu"]
    kv, q = stage_qkv_cls(m, l, dev["xn"], acc)
    qkv = np.zeros((BATCH * T, 3 * D), np.float16)
    qkv[:, D:], qkv[::T, :D] = kv["emu"], q["emu"]
    dev["qkv"] = qkv.reshape(BATCH, T, 3 * D)
    att = np.zeros((BATCH * T, D), np.float16)
    att[::T] = stage_att(m, l, dev["qkv"], acc, cls_only=True)["emu"]
    dev["att"] = att
    xc = np.ascontiguousarray(x_prev[::T])
    dev["fin"] = stage_ln2(m, l, xc, att[::T], acc, cls_only=True)["emu"]
    dev["hid"] = stage_hid(m, l, dev["fin"], acc, cls_only=True)["emu"]
    x = x_prev.copy()
    x[::T] = stage_resid(m, l, xc, att[::T], dev["hid"], acc, cls_only=True)["emu"]
    dev["x"] = x
    return dev


# ---- measures --------------------------------------------------------------------------------------------------------------------------
WORST = {}                     # stage -> [worst error / bound, worst unequal share]: what the GPU test prints at its end


def _note(stage, ratio, share=0.0):
    w = WORST.setdefault(stage, [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], share)


def check16(stage, got, st, K):
    """got (rows, terms * K) fp16 against a stage dict -> (worst error / bound, unequal share, ok)"""
    terms = st.get("terms", 1)
    got = np.ascontiguousarray(got)
    emu = st["emu"]
    if got.shape != emu.shape:              # (a mutated reference may expect another number of column blocks)
        return float("inf"), 1.0, False
    # the a_lo block of a three-term row is the fp32 remainder of the first block's rounding, scaled: ANY difference in the fp32 value (the
    # order of a sum) changes its bits, so it is held by the bound on a + a_lo below and stays out of the share
    cols = np.ones(got.shape[1], bool)
    if terms == 3:
        cols[K:2 * K] = False
    neq = got.view(np.uint16) != emu.view(np.uint16)
    if "may" in st:                         # `att_undetermined`: elements that need not equal the emulation (and their a / S)
        neq &= ~np.tile(st["may"], (1, got.shape[1] // K))
    share = float(neq[:, cols].mean())
    g64 = got.astype(np.float64)
    ok = bool(np.isfinite(g64).all())
    ratio = float((np.abs(g64[:, :K] - st["ref"]) / st["bnd"]).max())
    if terms > 1:                           # a / S from the a that was written, bit for bit
        over, _ = LC.split_terms(got[:, :K], got[:, :K].astype(np.float32))
        ok = ok and np.array_equal(got[:, (terms - 1) * K:].view(np.uint16), over.view(np.uint16))
    if terms == 3:
        sum2 = g64[:, :K] + g64[:, K:2 * K] / S
        if st.get("two") is not None:
            ref2, bnd2, valid = st["two"]
            r2 = float(np.where(valid, np.abs(sum2 - ref2) / bnd2, 0.0).max())
        elif "lo_bnd" in st:
            r2 = float((np.abs(sum2 - st["ref"]) / st["lo_bnd"]).max())
        else:
            r2 = float((np.abs(sum2 - st["ref"]) / (st["bnd32"] + st["lo_rel"] * np.abs(st["ref"]))).max())
        ratio = max(ratio, r2)
    _note(stage, ratio, share)
    return ratio, share, ok and ratio <= 1.0 and share <= CAP


def check32(stage, got, st):
    """got fp32 rows against a stage dict -> (worst error / bound, ok)"""
    g64 = np.asarray(got, np.float64)
    assert g64.shape == st["ref"].shape, (stage, g64.shape, st["ref"].shape)
    err = np.abs(g64 - st["ref"])
    ratio = float(np.where(err == 0, 0.0, err / np.maximum(st["bnd"], 1e-300)).max())
    if "rms" in st:
        # Second condition on a GEMM's fp32 rows, because the element bound is a worst case over every summation order -- K + 2 roundings,
        # all of one sign, each of a partial sum as large as S -- and at K = 768 (the patch GEMM) a dropped second weight term moves an
        # element by a fifth of it.  Roundings are not of one sign: K + 2 independent ones of at most u (S + |bias|) each add up to
        # sqrt(K + 2) u (S + |bias|) in the root mean square, the other terms of the bound unchanged (`k_rms`).  Held per ROW in the
        # 2-norm, where 128 elements average: an fp32 sum in numpy's order measures at most 0.05 of it on these cases
        # (the MI355X: 0.07), a dropped second weight term of the patch GEMM 8 times it.
        num, den = np.sqrt((err * err).sum(axis=1)), np.sqrt((st["rms"] ** 2).sum(axis=1))
        ratio = max(ratio, float(np.where(num == 0, 0.0, num / np.maximum(den, 1e-300)).max()))
    _note(stage, ratio)
    return ratio, bool(np.isfinite(g64).all()) and ratio <= 1.0
