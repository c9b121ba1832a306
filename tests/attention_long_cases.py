"""Case table of the streaming attention kernel `ibl_attention_stream_kernel` (csrc/vit_attention.hip): the input families, fp64 reference and
error bound of tests/attention_cases.py at token counts beyond the resident kernel's 272, two families that force the online softmax
to rescale at every key chunk, and a CPU emulation of the kernel's arithmetic.  Shared by tests/test_attention_long_model.py (CPU:
the bound is reachable) and tests/test_gpu_attention_long.py (GPU: the kernel meets it)."""
import functools

import numpy as np

from tests.attention_cases import (C_REST, DECISIVE, FAMILIES, HD, SEED, SPLIT, _h16, _noise, bound, emulate, make, pack,  # noqa: F401
                                   reference, split_terms, unpack_out)

KV = 128                      # ATT_S_KV: keys per chunk of the kernel
QB = 64                       # ATT_S_QB: queries per workgroup
MAX_TOKENS = 8192             # IBL_ATT_STREAM_MAX_TOKENS
STAIRS = ("stair_up", "stair_down")
LONG_FAMILIES = FAMILIES + STAIRS
# a kernel that ignored the logits must miss the bound 50-fold on these (asserted at the token counts beyond 272)
LONG_DECISIVE = ("peaked", "ramp") + STAIRS

# (T, heads, batch)
LONG = ((273, 2, 1), (289, 2, 3), (577, 2, 1), (1025, 2, 1), (1370, 2, 1))
CASES = LONG + (
    (273, 16, 1),                                              # the head stride at dim 1024
    (1, 2, 1), (17, 2, 3), (272, 2, 1),                        # short rows: the entry takes them too
    (KV - 1, 2, 1), (KV, 2, 1), (KV + 1, 2, 1), (2 * KV + 1, 2, 1), (QB + 1, 2, 1))
# terms 2 / 3 and cls_only run on these
LAYOUT_CASES = ((273, 2, 1), (289, 2, 3), (577, 2, 1), (1370, 2, 1), (2 * KV + 1, 2, 1))


def make_long(family, T, heads, batch, seed=SEED):
    """`attention_cases.make` plus the staircases: q[..., 0] = 8 and k[key][0] = 0.5 * (key // 16) (stair_up) give the scaled logit
    0.5 * (key // 16) + O(0.3) noise -- the row maximum rises by half a logit with every 16 keys, so every chunk raises the running
    maximum and rescales; stair_down is the mirror image, every later chunk lies below the maximum of the first."""
    if family not in STAIRS:
        return make(family, T, heads, batch, seed)
    rng = np.random.default_rng([seed, T, heads, batch, 100 + STAIRS.index(family)])
    shape = (batch, heads, T, HD)
    q, k = _noise(rng, shape, 1), _noise(rng, shape, 1)
    v = rng.normal(size=shape)
    step = np.arange(T) // 16
    if family == "stair_down":
        step = (T - 1) // 16 - step
    q[..., 0] = 8.0
    k[..., 0] = 0.5 * step
    return dict(q=q.astype(np.float16), k=k.astype(np.float16), v=v.astype(np.float16))


@functools.lru_cache(maxsize=None)
def case(family, T, heads, batch):
    """-> (inputs, ref, A, plain, bound, three-term bound); computed once per process and shared: do not modify"""
    c = make_long(family, T, heads, batch)
    ref, A, plain = reference(c.get("q0", c["q"]), c.get("k0", c["k"]), c["v"])
    return c, ref, A, plain, bound(ref, A, c["v"]), bound(ref, A, c["v"], out_rel=2.0 ** -21)


def emulate_stream(q, k, v, chunk=KV):
    """The streaming kernel's arithmetic on the CPU, as `emulate` is for the resident kernel: fp32 scores; per chunk of keys the
    running maximum m, alpha = exp2((m_old - m_new) c2), p = exp2(fma(s, c2, -m_new c2)) in fp32, l = fma(l, alpha, sum of the unrounded
    p), O = O * alpha + fp16(p) V with fp32 accumulation; 1 / l once at the end in fp32, one fp16 rounding.
    -> (a fp16, value fp32)"""
    f32 = np.float32
    s = np.matmul(q.astype(f32), np.swapaxes(k.astype(f32), -1, -2))
    v32 = v.astype(f32)
    T = s.shape[-1]
    c2 = f32(0.125) * f32(1.4426950408889634)
    m = np.full(s.shape[:-1] + (1,), -np.inf, f32)
    l = np.zeros_like(m)
    o = np.zeros(s.shape[:-1] + (HD,), f32)
    for k0 in range(0, T, chunk):
        sc = s[..., k0:k0 + chunk]
        mn = np.maximum(m, sc.max(axis=-1, keepdims=True))
        alpha = np.exp2(((m - mn) * c2).astype(f32))
        mc = (-mn * c2).astype(f32)
        arg = (sc.astype(np.float64) * np.float64(c2) + mc.astype(np.float64)).astype(f32)     # one rounding: the fma
        p = np.exp2(arg)
        assert p.dtype == f32 and alpha.dtype == f32
        psum = p.sum(axis=-1, keepdims=True, dtype=f32)
        l = (l.astype(np.float64) * alpha.astype(np.float64) + psum.astype(np.float64)).astype(f32)
        o = (o * alpha).astype(f32) + np.matmul(p.astype(np.float16).astype(f32), v32[..., k0:k0 + chunk, :])
        m = mn
    value = (o * (f32(1.0) / l)).astype(f32)
    return _h16(value), value
