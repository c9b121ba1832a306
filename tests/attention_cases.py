"""Inputs, fp64 reference, error bound and a CPU emulation of the arithmetic of `ibl_attention_kernel` (csrc/vit_attention.hip), shared by
tests/test_attention_model.py (CPU: the bound is reachable) and tests/test_gpu_attention.py (GPU: the kernel meets it).

Arrays are (batch, heads, n_tokens, 64); `pack` lays them out as the kernel's qkv rows [q | k | v], each [heads][64]."""
import numpy as np

HD = 64                       # head_dim of every encoder here
SPLIT = 64.0                  # IBL_VIT_SPLIT_SCALE
# Bound on the first term (see `bound`):  2^-11 |ref| + 2^-11 A + C_REST max|v|.  C_REST is the smallest power of two for which the
# emulation below stays at or under 0.75 of the bound on every case of `case` (tests/test_attention_model.py prints the ratios):
# 2^-16 gives 0.81, 2^-15 0.77, 2^-14 0.71.  What drives the ratio is not the exp2 or the subnormal p but the first two terms being
# sharp: a peaked row with a second key one logit below the winner has p2 ~ 0.57, which rounds to fp16 with a relative error near
# 2^-11, and where the result lands just above a power of two its own rounding is 2^-11 |ref| as well -- two legitimate roundings that
# together reach 0.8 of the bound among ~10^6 elements.
C_REST = 2.0 ** -14
T_ALL = (1, 2, 15, 16, 17, 50, 63, 64, 65, 129, 144, 145, 197, 208, 209, 257, 271, 272)
FAMILIES = ("diffuse", "peaked", "two_level", "offset", "ramp", "ramp_diffuse")
# families in which the softmax decides the answer: a kernel that ignored the logits (plain mean of v) must miss the bound 50-fold
DECISIVE = ("peaked", "two_level", "ramp")


def winners(T):
    """key indices that win a query in the peaked families: in the first tile, the first and a middle key of the last (partial) tile,
    the very last key, the middle of the row and key 0"""
    last0 = 16 * ((T - 1) // 16)
    cand = [3, last0, last0 + (T - 1 - last0) // 2, T - 1, T // 2, 0]
    out = []
    for c in cand:
        c = min(max(c, 0), T - 1)
        if c not in out:
            out.append(c)
    return out


def _noise(rng, shape, lo, scale=0.55):
    """N(0, scale) in head dimensions lo .. 63, zero below: scaled logits of two such rows are O(scale^2) ~ 0.3"""
    a = np.zeros(shape, np.float64)
    a[..., lo:] = rng.normal(size=shape[:-1] + (HD - lo,)) * scale
    return a


def _ramp(B, H, T):
    """v[key][d] = +-(key + 1) * {1, 1.25, 1.5, 1.75}: a distinct magnitude per key (exact in fp16 up to 272 * 1.75), signs alternating
    with the key so that a dropped, doubled or permuted key moves the result by whole units instead of averaging away"""
    j = np.arange(T, dtype=np.float64)[:, None]
    d = np.arange(HD)[None, :]
    v = (j + 1.0) * (1.0 + (d % 4) / 4.0) * np.where((j.astype(np.int64) + d // 7) % 2 == 0, 1.0, -1.0)
    return np.broadcast_to(v, (B, H, T, HD)).copy()


def _peaked_qk(rng, B, H, T):
    """every query has one winning key 10 .. 38 (scaled logit, noise included) above the rest, every third query a second key 1 below the first.  Key
    w_m carries 8 in head dimension m, the query a gap g in the dimension of the key it picks; the noise lives in dimensions 8 .. 63"""
    W = winners(T)
    q = _noise(rng, (B, H, T, HD), 8)
    k = _noise(rng, (B, H, T, HD), 8)
    for m, w in enumerate(W):
        k[:, :, w, m] = 8.0
    for i in range(T):
        m = (i + i // len(W)) % len(W)
        g = 12.0 + 2.5 * ((7 * i) % 11)
        q[:, :, i, m] = g
        if i % 3 == 0 and len(W) > 1:
            q[:, :, i, (m + 1) % len(W)] = g - 1.0
    return q, k


def make(family, T, heads, batch, seed):
    """-> dict q, k, v (fp16); for "offset" also q0, k0: the same rows without the common logit offset (the fp64 reference and a second
    kernel run use those)"""
    rng = np.random.default_rng([seed, T, heads, batch, FAMILIES.index(family)])
    B, H = batch, heads
    shape = (B, H, T, HD)
    extra = {}
    if family == "diffuse":
        q, k, v = _noise(rng, shape, 0), _noise(rng, shape, 0), rng.normal(size=shape)
    elif family == "peaked":
        q, k = _peaked_qk(rng, B, H, T)
        v = rng.normal(size=shape)
    elif family == "two_level":
        # half of the keys at scaled logit 12, the others at 0 (+ noise): p of the low half ~ e^-12 = 6e-6 < 2^-14, fp16 subnormals
        q, k = _noise(rng, shape, 1), _noise(rng, shape, 1)
        high = np.zeros(T, bool)
        high[rng.permutation(T)[:(T + 1) // 2]] = True
        q[..., 0] = 16.0
        k[..., 0] = np.where(high, 6.0, 0.0)
        v = rng.normal(size=shape) * np.where(high, 1.0, 8.0)[:, None]
    elif family == "offset":
        # logits O(1) in dimensions 0 .. 62; dimension 63 adds 32 * 15 / 8 = 60 to EVERY scaled logit of a row
        q0, k0 = _noise(rng, shape, 0, 1.0), _noise(rng, shape, 0, 1.0)
        q0[..., 63] = 0.0
        k0[..., 63] = 0.0
        q, k = q0.copy(), k0.copy()
        q[..., 63] = 32.0
        k[..., 63] = 15.0
        v = rng.normal(size=shape)
        extra = {"q0": q0.astype(np.float16), "k0": k0.astype(np.float16)}
    elif family == "ramp":
        q, k = _peaked_qk(rng, B, H, T)
        v = _ramp(B, H, T)
    elif family == "ramp_diffuse":
        q, k, v = _noise(rng, shape, 0), _noise(rng, shape, 0), _ramp(B, H, T)
    else:
        raise KeyError(family)
    return dict(q=q.astype(np.float16), k=k.astype(np.float16), v=v.astype(np.float16), **extra)


def pack(q, k, v):
    """(B, H, T, 64) x 3 -> qkv (B, T, 3 * H * 64) fp16"""
    B, H, T, _ = q.shape
    rows = [a.transpose(0, 2, 1, 3).reshape(B, T, H * HD) for a in (q, k, v)]
    return np.ascontiguousarray(np.concatenate(rows, axis=2))


def unpack_out(out, heads, terms=1):
    """kernel output (B, T, terms * D) -> list of `terms` arrays (B, H, T, 64)"""
    B, T, W = out.shape
    D = W // terms
    return [out[:, :, t * D:(t + 1) * D].reshape(B, T, heads, HD).transpose(0, 2, 1, 3) for t in range(terms)]


def reference(q, k, v):
    """float64 softmax(q k^T / 8) v from the fp16 inputs (which therefore carry no error) -> ref, A = sum_i p_i |v_i| (the softmax-
    weighted mean of |v|), plain = mean of v over the keys (what a kernel that ignored the logits would return)"""
    q64, k64, v64 = (a.astype(np.float64) for a in (q, k, v))
    s = np.einsum("bhqd,bhkd->bhqk", q64, k64) / 8.0
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    ref = np.einsum("bhqk,bhkd->bhqd", p, v64)
    A = np.einsum("bhqk,bhkd->bhqd", p, np.abs(v64))
    plain = np.broadcast_to(v64.mean(axis=2, keepdims=True), ref.shape)
    return ref, A, plain


def bound(ref, A, v, c=C_REST, out_rel=2.0 ** -11):
    """|out - ref| <= out_rel |ref| + 2^-11 A + c max|v|: the output's own fp16 rounding; the fp16 rounding of every p (worst case, all
    of one sign); the rest -- p below 2^-14 kept as fp16 subnormals or flushed, the exp2 approximation, fp32 accumulation order.
    max|v| is taken per (crop, head)."""
    vmax = np.abs(v.astype(np.float64)).max(axis=(2, 3), keepdims=True)
    return out_rel * np.abs(ref) + 2.0 ** -11 * A + c * vmax


def _h16(x32):
    """the kernel's f2h: clamp to the finite range, round to nearest even"""
    return np.clip(x32, -65504.0, 65504.0).astype(np.float16)


def emulate(q, k, v):
    """The kernel's arithmetic on the CPU: fp32 scores from fp16 products, p = exp2 in fp32 of fma(s, 0.125 log2 e, -max * that), fp32
    row sum of the UNROUNDED p, p rounded to fp16 for the PV product, fp32 accumulation, times 1 / sum in fp32, one fp16 rounding.
    -> (a fp16, value fp32): the stored first term and the fp32 number it was rounded from"""
    f32 = np.float32
    s = np.matmul(q.astype(f32), np.swapaxes(k.astype(f32), -1, -2))
    c2 = f32(0.125) * f32(1.4426950408889634)
    mc = -s.max(axis=-1, keepdims=True) * c2
    arg = (s.astype(np.float64) * np.float64(c2) + mc.astype(np.float64)).astype(f32)     # one rounding: the fma
    p = np.exp2(arg)
    assert p.dtype == f32
    rowsum = p.sum(axis=-1, keepdims=True, dtype=f32)
    o = np.matmul(p.astype(np.float16).astype(f32), v.astype(f32))
    value = (o * (f32(1.0) / rowsum)).astype(f32)
    return _h16(value), value


def split_terms(a16, value32):
    """the second / third column block the kernel derives from its first: (a / S in fp16, (value - a) * S in fp16)"""
    a32 = a16.astype(np.float32)
    return _h16(a32 * np.float32(1.0 / SPLIT)), _h16((value32 - a32) * np.float32(SPLIT))


# heads (dim = 64 * heads: 128 .. 1024) and batch each token count runs with; every T runs every family with terms = 1 and all queries
HEADS_OF_T = {1: 2, 2: 6, 15: 12, 16: 16, 17: 2, 50: 6, 63: 12, 64: 16, 65: 2, 129: 12, 144: 6, 145: 16, 197: 12, 208: 2, 209: 6, 257: 12,
              271: 16, 272: 16}
BATCH_OF_T = {2: 3, 17: 3, 50: 3, 145: 3, 257: 3, 272: 3}
SEED = 20250


def case(family, T):
    return make(family, T, HEADS_OF_T[T], BATCH_OF_T.get(T, 1), SEED)
