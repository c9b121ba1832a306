"""ORACLE (test infrastructure; never imported by the product path).

Torch-fp32 restatement of DATOR's forward:
  * TransReID stream with local_feature=True: 11 of 12 blocks, no final norm, LoRA added to the QKV projection of
    the last two blocks (dator/model/backbones/vit_pytorch.py:182-185, 381-391, 422-443);
  * fusion head build_FourDNet.forward (dator/model/make_model.py:629-843): global/local projections and merge,
    hyper-network gates, Q/V, four deformable-sampling attentions (grid_sample, align_corners=True, bilinear, zero
    padding; x = first 24 selector channels, y = last 24), residual + LayerNorm (eps 1e-5), gated mean.
Pinned against the reference's own build_FourDNet run in the build container with the same seeded weights
(tests/golden/dator_golden.npz, tools/gen_golden_dator.py).  Trained weights (dator_best_tum.pth) and the reference's
`dator_wrapper.get_model_input` are not in its repository: preprocessing follows dator/get_embeds.py:80-87,129-136
and pretrained-weight parity is unpinned.

`head_stages` and the `stage_*` functions restate the same head stage by stage in fp64 or fp32 (the stage-alone tests of the
product's head recompute each stage from its inputs); `preprocess_depth_f64` is the float64 value reference of the depth resize."""
import numpy as np
import torch
from PIL import Image

from . import vit_oracle as vo

F = torch.nn.functional


def stream_tokens(w: dict, cfg, pixels: np.ndarray) -> np.ndarray:
    """(B, 3, 256, 128) -> (B, 129, 768): vit_oracle forward with the LoRA term folded exactly as F.linear(x, (A@B).T)."""
    w2 = dict(w)
    for l in range(cfg.depth):
        if f"l{l}.lora_down" in w:
            delta = (torch.from_numpy(w[f"l{l}.lora_down"]) @ torch.from_numpy(w[f"l{l}.lora_up"])).T.numpy()
            for i, n in enumerate("qkv"):
                w2[f"l{l}.{n}.w"] = w[f"l{l}.{n}.w"] + delta[i * cfg.dim:(i + 1) * cfg.dim]
    return vo.vit_forward(w2, cfg, pixels, all_tokens=True)


@torch.no_grad()
def head_forward(hw: dict, rgb_tokens: np.ndarray, depth_tokens: np.ndarray) -> np.ndarray:
    h = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in hw.items()}
    xr, xd = torch.from_numpy(rgb_tokens), torch.from_numpy(depth_tokens)
    B, N = xr.shape[0], xr.shape[1] - 1

    def lin(name, x):
        return F.linear(x, h[name + ".w"], h[name + ".b"])

    def merged(x, side):
        g = lin(f"proj_global_{side}", x[:, 0])
        loc = lin(f"proj_local_{side}", x[:, 1:])
        return lin(f"merge_{side}", torch.cat((g.unsqueeze(1).repeat(1, N, 1), loc), -1))

    fr, fd = merged(xr, "rgb"), merged(xd, "depth")
    dsp = fd.reshape(B, 16, 8, 128).permute(0, 3, 1, 2)
    rsp = fr.reshape(B, 16, 8, 128).permute(0, 3, 1, 2)
    x = torch.cat((dsp, rsp), dim=1)
    for i in range(4):
        x = F.conv2d(x, h[f"hyper.{i}.w"], h[f"hyper.{i}.b"], padding=1)
        if i < 3:
            x = F.relu(x)
    filt = F.softmax(x.permute(0, 2, 3, 1), dim=-1)
    rgb_f, depth_f = filt[..., 0].reshape(B, 128, 1), filt[..., 1].reshape(B, 128, 1)
    q_r, v_r, q_d, v_d = lin("Q_r", fr), lin("V_r", fr), lin("Q_d", fd), lin("V_d", fd)

    def deform(op, q, v):
        sel = torch.sigmoid(lin(op + ".sel", q))
        aw = F.softmax(lin(op + ".aw", q), dim=-1)
        grid = torch.stack((sel[:, :, :24], sel[:, :, 24:]), -1) * 2 - 1
        vm = v.permute(0, 2, 1).reshape(B, 128, 16, 8)
        samp = F.grid_sample(vm, grid, align_corners=True).permute(0, 2, 3, 1)
        return lin(op + ".ffn", torch.sum(samp * aw.unsqueeze(-1), dim=-2))

    def ln(op, x):
        return F.layer_norm(x, (128,), h[op + ".norm.g"], h[op + ".norm.b"], 1e-5)

    fr = ln("r2r", fr + deform("r2r", q_r, v_r))
    fd = ln("d2d", fd + deform("d2d", q_d, v_d))
    fr = ln("d2r", fr + deform("d2r", q_d, v_r) * rgb_f)
    fd = ln("r2d", fd + deform("r2d", q_r, v_d) * depth_f)
    return torch.mean(fd * depth_f + fr * rgb_f, dim=-2).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# The same head, stage by stage, in a chosen precision.  Every stage function takes its INPUTS as arguments (token-major rows
# [B*128, C], torch tensors of the dtype of `h`), so a test can recompute one stage from another implementation's own intermediates
# without chaining rounding through the stages in front of it.  `head_forward` above stays the fp32 statement the golden pins.
# ---------------------------------------------------------------------------------------------------------------------------------
def head_weights_as(hw: dict, dtype) -> dict:
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dtype) for k, v in hw.items()}


def stage_linear(h, name, x):
    return F.linear(x, h[name + ".w"], h[name + ".b"])


def stage_project(h, side, tokens):
    """tokens [B, 129, 768] -> (global projection of the CLS row [B, 128], local projection of the patch rows [B*128, 128])"""
    return stage_linear(h, f"proj_global_{side}", tokens[:, 0]), stage_linear(h, f"proj_local_{side}", tokens[:, 1:].reshape(-1, tokens.shape[-1]))


def stage_merge(h, side, gl, lp):
    n = lp.shape[0] // gl.shape[0]
    return stage_linear(h, f"merge_{side}", torch.cat((gl.repeat_interleave(n, dim=0), lp), -1))


def stage_hyper(h, i, x):
    """layer i of the hyper-network on token-major rows [B*128, Cin] of the 16 x 8 grid -> [B*128, Cout] (ReLU after layers 0-2)"""
    y = F.conv2d(x.reshape(-1, 16, 8, x.shape[-1]).permute(0, 3, 1, 2), h[f"hyper.{i}.w"], h[f"hyper.{i}.b"], padding=1)
    y = F.relu(y) if i < 3 else y
    return y.permute(0, 2, 3, 1).reshape(x.shape[0], -1)


def stage_gates(h4):
    """[B*128, 2] -> (rgb_f, depth_f), each [B, 128]"""
    filt = F.softmax(h4, dim=-1)
    return filt[:, 0].reshape(-1, 128), filt[:, 1].reshape(-1, 128)


def stage_sel(h, op, q):
    return torch.sigmoid(stage_linear(h, op + ".sel", q))


def stage_aw_logits(h, op, q):
    return stage_linear(h, op + ".aw", q)


def stage_sample(sel, aw_logits, v):
    """selectors [R, 48] (x = first 24, y = last 24, in [0, 1]), attention logits [R, 24], values [R, 128] -> weighted samples [R, 128]"""
    B = v.shape[0] // 128
    grid = torch.stack((sel[:, :24], sel[:, 24:]), -1).reshape(B, 128, 24, 2) * 2 - 1
    vm = v.reshape(B, 128, 128).permute(0, 2, 1).reshape(B, 128, 16, 8)
    samp = F.grid_sample(vm, grid, mode="bilinear", padding_mode="zeros", align_corners=True).permute(0, 2, 3, 1)     # [B, 128, 24, C]
    aw = F.softmax(aw_logits, dim=-1).reshape(B, 128, 24, 1)
    return torch.sum(samp * aw, dim=-2).reshape(-1, 128)


def stage_ffn(h, op, samp):
    return stage_linear(h, op + ".ffn", samp)


def stage_add_ln(h, op, f, feat, gate=None):
    """LayerNorm(f + feat * gate) over the 128 channels; gate [B, 128] or None"""
    x = f + (feat if gate is None else feat * gate.reshape(-1, 1))
    return F.layer_norm(x, (128,), h[op + ".norm.g"], h[op + ".norm.b"], 1e-5)


def stage_deform(h, op, q, v):
    sel, awl = stage_sel(h, op, q), stage_aw_logits(h, op, q)
    samp = stage_sample(sel, awl, v)
    return {"sel": sel, "aw_logits": awl, "aw": F.softmax(awl, dim=-1), "samp": samp, "feat": stage_ffn(h, op, samp)}


def stage_final(h, cat, q_r, v_r, q_d, v_d, rgb_f, depth_f):
    """the four attentions from the merged features cat = [fd | fr], the queries / values and the gates -> dict with the per-operation
    intermediates ('r2r.sel', ...), the features after the two ungated attentions ('fr_r2r', 'fd_d2d') and the final 'fr', 'fd'"""
    s = {}
    fd, fr = cat[:, :128], cat[:, 128:]
    for op, q, v in (("r2r", q_r, v_r), ("d2d", q_d, v_d), ("d2r", q_d, v_r), ("r2d", q_r, v_d)):
        s.update({f"{op}.{k}": t for k, t in stage_deform(h, op, q, v).items()})
    s["fr_r2r"] = stage_add_ln(h, "r2r", fr, s["r2r.feat"])
    s["fd_d2d"] = stage_add_ln(h, "d2d", fd, s["d2d.feat"])
    s["fr"] = stage_add_ln(h, "d2r", s["fr_r2r"], s["d2r.feat"], rgb_f)
    s["fd"] = stage_add_ln(h, "r2d", s["fd_d2d"], s["r2d.feat"], depth_f)
    return s


def stage_pool(fr, fd, rgb_f, depth_f):
    B = rgb_f.shape[0]
    return torch.mean(fd.reshape(B, 128, 128) * depth_f.unsqueeze(-1) + fr.reshape(B, 128, 128) * rgb_f.unsqueeze(-1), dim=1)


@torch.no_grad()
def head_stages(hw: dict, rgb_tokens, depth_tokens, dtype=torch.float64, swap_gates=False) -> dict:
    """Every intermediate of the head under the names of the product's workspace taps (include/ibloc.h, IBL_DATOR_WS_*): 'gl', 'lp'
    (depth side; 'gl_rgb', 'lp_rgb' the other), 'cat' = [fd | fr] merged, 'h1'..'h4', 'rgb_f', 'depth_f', 'q_r', 'v_r', 'q_d', 'v_d',
    '<op>.sel' / '.aw_logits' / '.aw' / '.samp' / '.feat' for op in r2r, d2d, d2r, r2d, 'fr_r2r', 'fd_d2d', 'fr', 'fd', 'out'; torch
    tensors of `dtype` (float64 or float32) on the CPU.  swap_gates exchanges rgb_f and depth_f after the hyper-network (a deliberately
    wrong head, for tests that show a case would notice)."""
    h = head_weights_as(hw, dtype)
    xr, xd = torch.as_tensor(np.asarray(rgb_tokens)).to(dtype), torch.as_tensor(np.asarray(depth_tokens)).to(dtype)
    s = {}
    s["gl_rgb"], s["lp_rgb"] = stage_project(h, "rgb", xr)
    s["gl"], s["lp"] = stage_project(h, "depth", xd)
    s["cat"] = torch.cat((stage_merge(h, "depth", s["gl"], s["lp"]), stage_merge(h, "rgb", s["gl_rgb"], s["lp_rgb"])), -1)
    x = s["cat"]
    for i in range(4):
        x = s[f"h{i + 1}"] = stage_hyper(h, i, x)
    s["rgb_f"], s["depth_f"] = stage_gates(s["h4"])
    if swap_gates:
        s["rgb_f"], s["depth_f"] = s["depth_f"], s["rgb_f"]
    fd, fr = s["cat"][:, :128], s["cat"][:, 128:]
    s["q_r"], s["v_r"] = stage_linear(h, "Q_r", fr), stage_linear(h, "V_r", fr)
    s["q_d"], s["v_d"] = stage_linear(h, "Q_d", fd), stage_linear(h, "V_d", fd)
    s.update(stage_final(h, s["cat"], s["q_r"], s["v_r"], s["q_d"], s["v_d"], s["rgb_f"], s["depth_f"]))
    s["out"] = stage_pool(s["fr"], s["fd"], s["rgb_f"], s["depth_f"])
    return s


def forward(rgb_w, depth_w, head_w, cfg, rgb_pixels, depth_pixels):
    return head_forward(head_w, stream_tokens(rgb_w, cfg, rgb_pixels), stream_tokens(depth_w, cfg, depth_pixels))


def preprocess_rgb(crop: np.ndarray) -> np.ndarray:
    """dator/get_embeds.py:80-87: ToPILImage, Resize([256, 128]) (bilinear), ToTensor, Normalize(0.5, 0.5)."""
    res = np.asarray(Image.fromarray(np.ascontiguousarray(crop, dtype=np.uint8)).resize((128, 256), resample=Image.BILINEAR))
    x = (res.astype(np.float64) * (1 / 255)).astype(np.float32)
    return np.ascontiguousarray(((x - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1))


def resize_coords(o: int, n: int):
    """The fp32 coordinate rule of the bilinear resize of n source samples to o outputs (cv2.INTER_LINEAR: half-pixel centres, edge
    clamp): source position f = (i + 0.5) * (n / o) - 0.5 in float32 -> (i0, i1, weight of i1) per output sample."""
    f = (np.arange(o, dtype=np.float32) + np.float32(0.5)) * np.float32(n / o) - np.float32(0.5)
    i0 = np.floor(f).astype(np.int64)
    fr = f - i0.astype(np.float32)
    lo = i0 < 0
    hi = i0 >= n - 1
    i0 = np.clip(i0, 0, n - 1)
    i1 = np.clip(i0 + 1, 0, n - 1)
    fr = np.where(lo | hi, np.float32(0), fr).astype(np.float32)
    i1 = np.where(hi, i0, i1)
    return i0, i1, fr


def preprocess_depth_f64(depth_crop: np.ndarray, dmin=0.0, dmax=50.0, oh=256, ow=128) -> np.ndarray:
    """One channel (oh, ow) of `preprocess_depth` with the taps and weights of the fp32 coordinate rule, and the interpolation, the
    clip and the normalisation in float64: what the fp32 arithmetic behind the rule should round to."""
    d = np.ascontiguousarray(depth_crop, dtype=np.float32).astype(np.float64)
    y0, y1, fy = resize_coords(oh, d.shape[0])
    x0, x1, fx = resize_coords(ow, d.shape[1])
    fy, fx = fy.astype(np.float64)[:, None], fx.astype(np.float64)[None, :]
    top = d[y0][:, x0] * (1 - fx) + d[y0][:, x1] * fx
    bot = d[y1][:, x0] * (1 - fx) + d[y1][:, x1] * fx
    r = np.clip(top * (1 - fy) + bot * fy, float(dmin), float(dmax))
    return ((r - dmin) / (dmax - dmin) - 0.5) / 0.5


def preprocess_depth(depth_crop: np.ndarray, dmin=0.0, dmax=50.0) -> np.ndarray:
    """dator/get_embeds.py:129-136: cv2.resize(depth, (128, 256)) (INTER_LINEAR: half-pixel centres, edge clamp, no
    antialiasing), tile to 3 channels, clip, (d - min) / (max - min), (x - 0.5) / 0.5."""
    d = np.ascontiguousarray(depth_crop, dtype=np.float32)
    h, w = d.shape
    oh, ow = 256, 128
    y0, y1, fy = resize_coords(oh, h)
    x0, x1, fx = resize_coords(ow, w)
    top = d[y0][:, x0] * (1 - fx)[None, :] + d[y0][:, x1] * fx[None, :]
    bot = d[y1][:, x0] * (1 - fx)[None, :] + d[y1][:, x1] * fx[None, :]
    r = (top * (1 - fy)[:, None] + bot * fy[:, None]).astype(np.float32)
    r = np.clip(r, np.float32(dmin), np.float32(dmax))
    r = (r - np.float32(dmin)) / np.float32(dmax - dmin)
    r = (r - np.float32(0.5)) / np.float32(0.5)
    return np.repeat(r[None], 3, axis=0).astype(np.float32)


def embed(rgb_w, depth_w, head_w, rgb_crops, depth_crops):
    """RGB crops (HxWx3 u8) + depth crops (h x w float, metres) -> (n, 128): preprocessing of dator/get_embeds.py:80-87,129-136,
    then build_FourDNet.forward.  Stream weights with the LoRA factors already folded (ibloc_amd.dator.fold_lora)."""
    from ibloc_amd.dator import STREAM_CFG
    rgb = np.stack([preprocess_rgb(c) for c in rgb_crops])
    dep = np.stack([preprocess_depth(c) for c in depth_crops])
    return forward(rgb_w, depth_w, head_w, STREAM_CFG, rgb, dep)
