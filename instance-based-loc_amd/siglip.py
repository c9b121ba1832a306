"""SigLIP image encoder (google/siglip-base-patch16-224 / -256 / -384, siglip-large-patch16-256 / -384 and the fixed-resolution SigLIP 2
checkpoints with the same vision tower): a ViT/16 trunk on the shared ViT kernels -- no class token, tanh GELU, final LayerNorm over every
token (ibloc_amd.vit with cls_token=False, tanh_gelu=True) -- and the attention-pooling head (transformers'
SiglipMultiheadAttentionPoolingHead) as fp32 HIP kernels behind `ibl_probe_head_forward` (csrc/siglip.hip).

The head's single query is a constant, so its key and value projections over all tokens are folded at load (`fold_head`, float64):
    q = W_q probe + b_q;   u_h = W_k,h^T q_h / sqrt(head_dim);   score[b, h, t] = x[b, t] . u_h     (q_h . b_k,h cancels in the softmax)
    sum_t p (W_v,h x_t + b_v,h) = W_v,h (sum_t p x_t) + b_v,h
The embedding is the model's `pooler_output`, un-normalised (the match stage normalises)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import vit as V


class ProbeHeadDesc(C.Structure):           # ibl_probe_head_desc (include/ibloc.h)
    _fields_ = [("dim", C.c_int32), ("heads", C.c_int32), ("mlp_dim", C.c_int32), ("n_tokens", C.c_int32), ("ln_eps", C.c_float)]


class ProbeHeadWeights(C.Structure):        # ibl_probe_head_weights
    _fields_ = [(n, C.c_void_p) for n in ("u", "w_v", "b_v", "w_o", "b_o", "ln_g", "ln_b", "w_fc1", "b_fc1", "w_fc2", "b_fc2")]


HEAD_KEYS = ("probe", "q.w", "q.b", "k.w", "k.b", "v.w", "v.b", "o.w", "o.b", "ln.g", "ln.b", "fc1.w", "fc1.b", "fc2.w", "fc2.b")


def random_head_weights(cfg: V.VitConfig, seed: int) -> dict:
    """Seeded synthetic head weights, keyed like HEAD_KEYS.  The probe and the query / key matrices are scaled so that the pooling is not
    uniform: the post-LayerNorm tokens have entries of order 1, so u_h . x_t has a spread of several logits over the tokens of a crop
    (tests/test_siglip_model.py holds the mean of max_t p to at least 4 / T on tiny_siglip)."""
    rng = np.random.default_rng(seed)
    D, M = cfg.dim, cfg.mlp_dim

    def mat(*shape, std=0.02):
        return np.clip(rng.normal(0, std, size=shape), -2 * std, 2 * std).astype(np.float32)

    s = D ** -0.5
    return {"probe": mat(D, std=1.0), "q.w": mat(D, D, std=2.0 * s), "q.b": mat(D, std=0.02), "k.w": mat(D, D, std=2.0 * s), "k.b": mat(D, std=0.02),
            "v.w": mat(D, D, std=s), "v.b": mat(D, std=0.02), "o.w": mat(D, D, std=s), "o.b": mat(D, std=0.02),
            "ln.g": 1 + mat(D, std=0.1), "ln.b": mat(D, std=0.1),
            "fc1.w": mat(M, D, std=s), "fc1.b": mat(M), "fc2.w": mat(D, M, std=M ** -0.5), "fc2.b": mat(D)}


def fold_head(hw: dict, heads: int, dtype=np.float32) -> np.ndarray:
    """-> U (heads, dim): u_h = W_k,h^T (W_q probe + b_q)_h / sqrt(head_dim), computed in float64 and rounded once to `dtype`"""
    f = lambda k: np.asarray(hw[k], dtype=np.float64)
    D = f("probe").size
    if D % heads:
        raise ValueError(f"dim {D} is not a multiple of heads {heads}")
    hd = D // heads
    q = f("q.w") @ f("probe").reshape(-1) + f("q.b")
    wk = f("k.w")
    U = np.stack([wk[h * hd:(h + 1) * hd].T @ q[h * hd:(h + 1) * hd] for h in range(heads)]) / np.sqrt(hd)
    return U.astype(dtype)


# workspace buffers of ibl_probe_head_forward in the order of include/ibloc.h's IBL_PROBE_WS_* enum
HEAD_TAPS = ("probs", "pooled", "vcat", "att", "ln", "hid")


def probe_pool(x: torch.Tensor, u: torch.Tensor, want_probs=True, pooled=None, probs=None):
    """`ibl_probe_pool_f32`, the pooling kernel alone: x (B, T, D) fp32, u (heads, D) fp32 -> (pooled (B, heads, D), probs (B, heads, T)
    or None).  `pooled` / `probs` may be given (contiguous views of larger buffers)."""
    assert x.dtype == torch.float32 and u.dtype == torch.float32 and x.is_cuda and u.is_cuda and x.is_contiguous() and u.is_contiguous()
    B, T, D = x.shape
    H = u.shape[0]
    if pooled is None:
        pooled = torch.empty((B, H, D), dtype=torch.float32, device=x.device)
    if probs is None and want_probs:
        probs = torch.empty((B, H, T), dtype=torch.float32, device=x.device)
    assert pooled.is_contiguous() and pooled.shape == (B, H, D) and (probs is None or (probs.is_contiguous() and probs.shape == (B, H, T)))
    st = _lib.lib.ibl_probe_pool_f32(x.data_ptr(), B, T, D, H, u.data_ptr(), pooled.data_ptr(), probs.data_ptr() if probs is not None else None,
                                     torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "ibl_probe_pool_f32")
    return pooled, probs


class ProbeHead:
    """The attention-pooling head alone: folds and packs the head weights for `ibl_probe_head_forward` and owns a workspace per lane."""

    def __init__(self, cfg: V.VitConfig, head_weights: dict, device="cuda"):
        self.cfg = cfg
        self.device = torch.device(device)
        self._keep = {}
        D, M = cfg.dim, cfg.mlp_dim
        hw = head_weights
        # struct field -> (array, shape it must have); `u` is folded from the probe, the query and the key projection
        fields = {"u": (fold_head(hw, cfg.heads), (cfg.heads, D)), "w_v": (hw["v.w"], (D, D)), "b_v": (hw["v.b"], (D,)), "w_o": (hw["o.w"], (D, D)),
                  "b_o": (hw["o.b"], (D,)), "ln_g": (hw["ln.g"], (D,)), "ln_b": (hw["ln.b"], (D,)), "w_fc1": (hw["fc1.w"], (M, D)),
                  "b_fc1": (hw["fc1.b"], (M,)), "w_fc2": (hw["fc2.w"], (D, M)), "b_fc2": (hw["fc2.b"], (D,))}
        W = ProbeHeadWeights()
        for name, (a, shape) in fields.items():
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"head weight {name}: shape {a.shape}, expected {shape}")
            t = torch.from_numpy(a).to(self.device)
            self._keep[name] = t
            setattr(W, name, t.data_ptr())
        self.W = W
        self.desc = ProbeHeadDesc(D, cfg.heads, M, cfg.n_tokens, cfg.ln_eps)
        self._ws = V.Workspace(self.device)

    @property
    def u(self) -> torch.Tensor:
        return self._keep["u"]

    def forward(self, tokens: torch.Tensor, lane: int = 0) -> torch.Tensor:
        """fp32 tokens (B, n_tokens, dim) after the trunk's final LayerNorm -> (B, dim).  lane: workspace index for concurrent forwards."""
        assert tokens.dtype == torch.float32 and tokens.is_cuda and tokens.is_contiguous()
        assert tuple(tokens.shape[1:]) == (self.cfg.n_tokens, self.cfg.dim)
        B = tokens.shape[0]
        ws_bytes = _lib.lib.ibl_probe_head_workspace_bytes(C.byref(self.desc), B)
        if ws_bytes < 0:
            _lib.check(-1, "ibl_probe_head_workspace_bytes")
        ws = self._ws.get(lane, ws_bytes)
        out = torch.empty((B, self.cfg.dim), dtype=torch.float32, device=self.device)
        st = _lib.lib.ibl_probe_head_forward(C.byref(self.desc), C.byref(self.W), tokens.data_ptr(), B, out.data_ptr(), ws.data_ptr(),
                                             ws.numel(), torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "ibl_probe_head_forward")
        return out

    def taps(self, batch: int, lane: int = 0) -> dict:
        """Views of what the last `forward` of `batch` crops on `lane` left in its workspace (include/ibloc.h, IBL_PROBE_WS_*):
        probs (B, heads, T), pooled (B, heads, dim), vcat / att / ln (B, dim), hid (B, mlp_dim).  The next forward overwrites them."""
        c = self.cfg
        offs = (C.c_int64 * len(HEAD_TAPS))()
        _lib.check(_lib.lib.ibl_probe_head_workspace_layout(C.byref(self.desc), batch, offs, len(HEAD_TAPS)), "ibl_probe_head_workspace_layout")
        shapes = {"probs": (batch, c.heads, c.n_tokens), "pooled": (batch, c.heads, c.dim), "vcat": (batch, c.dim), "att": (batch, c.dim),
                  "ln": (batch, c.dim), "hid": (batch, c.mlp_dim)}
        return self._ws.views(lane, offs, [(name, torch.float32, shapes[name]) for name in HEAD_TAPS])


class SiglipEncoder:
    """Trunk + head.  `embed` has the signature of `VitEncoder.embed`, so `LocaliseEngine` takes the encoder unchanged."""

    def __init__(self, cfg: V.VitConfig, trunk_weights: dict, head_weights: dict, device="cuda", precision=None):
        if cfg.cls_token or not cfg.tanh_gelu or not cfg.out_all_tokens or not cfg.final_ln:
            raise ValueError(f"{cfg.name} is not a SigLIP trunk (cls_token=False, tanh_gelu, out_all_tokens, final_ln)")
        self.cfg = cfg
        self.device = torch.device(device)
        self.trunk = V.VitEncoder(cfg, trunk_weights, device=device, precision=precision)
        self.precision = self.trunk.precision
        self.recipe = self.trunk.recipe
        self.head = ProbeHead(cfg, head_weights, device=device)

    def preprocess(self, crops, want_u8=False):
        return self.trunk.preprocess(crops, want_u8=want_u8)

    def forward_patches(self, patches: torch.Tensor, lane: int = 0) -> torch.Tensor:
        return self.head.forward(self.trunk.forward_patches(patches, lane=lane), lane=lane)

    def forward_pixels(self, x: torch.Tensor, lane: int = 0) -> torch.Tensor:
        """(B, 3, H, W) pre-normalised float tensor -> (B, dim): the model's pooler_output"""
        return self.forward_patches(self.trunk.patches_from_pixels(x), lane=lane)

    def embed(self, crops, max_batch=512, lane=0) -> torch.Tensor:
        """crops (list of HxWx3 uint8 arrays, a uint8 tensor (N, H, W, 3) or PackedCrops) -> (N, dim) fp32 device tensor, un-normalised"""
        n = crops.shape[0] if isinstance(crops, torch.Tensor) else len(crops)
        if n == 0:
            return torch.empty((0, self.cfg.dim), dtype=torch.float32, device=self.device)
        return V.embed_chunks(n, max_batch, lambda sl: self.forward_patches(self.preprocess(crops[sl]), lane=lane))
