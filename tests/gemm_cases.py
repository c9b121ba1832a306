"""Inputs, fp64 reference, per-element error bounds and a CPU emulation of `gelu_erf2` for `ibl_gemm_f16_tn` (csrc/vit_gemm.hip), shared by
tests/test_gemm_model.py (CPU: the families are what they claim, C_GELU is chosen by rule) and tests/test_gpu_gemm.py (GPU: every element of
every epilogue on both tile shapes meets the bound).

y = x W^T from the exact fp16 operands in float64, then each epilogue's operation in float64 (GELU with the exact erfc).  The reference and
the bound are torch.float64 tensors on whatever device the operands are on, so the large cases never leave the GPU.

Bounds (u = 2^-24, half an ulp of fp32; S = sum_k |x_k w_k|, e1 = (K + 2) u (S + |bias|)):
  * fp32 accumulation of K products, each exact in fp32 (11 x 11 significand bits), plus the bias, in ANY order: every partial sum is at
    most S + |bias| and there are at most K + 1 roundings, so the error is at most e1.  It needs no knowledge of the order inside the MFMA;
    it still fails an fp16 accumulation (2^-11 per addition) at every K >= 64.
  * IBL_LINEAR_F32 (4): e1.
  * IBL_LINEAR_F16 (0): e1 + 2^-11 |ref| + 2^-25 -- the output's rounding (half an ulp of fp16; 2^-25 is half a subnormal step).  The
    reference clamps to +-65504 before rounding, as f2h documents; clamping does not grow an error.
  * IBL_LINEAR_RESID_F32 (2): t = (acc + b) * scale and out = x + t are one fp32 rounding each: |scale| e1 + u |t| + u |ref|.
  * IBL_LINEAR_RESID_PRE_F32 (5): c0 = x + b is rounded once (u |c0|); c0 / alpha is exact; the chain then sums K products and c0 / alpha,
    (K + 2) u (S + |c0| / alpha); the final * alpha is exact: u |c0| + (K + 2) u (alpha S + |c0|).
  * IBL_LINEAR_PATCH_F32 (3): e1 + u |ref| for v + pos; alpha e1 + u |ref| for fma(v, alpha, x).
  * IBL_LINEAR_GELU_F16 (1): LIP e1 + C_GELU max(|v|, TINY) + 2^-11 |ref| + 2^-25.  LIP = 1.13 >= max |gelu'| = 1.1290 carries the
    accumulation error through the activation; C_GELU |v| is the error of the kernel's polynomial erf form, which is proportional to |v|
    everywhere (for v << 0 the two halves of 0.5 v + z erf(z) / sqrt 2 cancel to a few ulp of |v|, not of the result).
  * IBL_LINEAR_GELU_F16_X2 / _X3 (6 / 7): the first block as (1); the last block is fp16(h / 64) of the h the kernel wrote, bit for bit;
    for _X3, h + lo / 64 meets the fp32-level bound: LIP e1 + C_GELU max(|v|, TINY) + the rounding of lo, which is 2^-11 |value - h| +
    2^-31 (half a subnormal step of lo, over 64) with |value - h| <= 2^-11 |ref| + 2^-25 -- wherever h is not saturated (|ref| <= 65504).
Second-order terms (an error of an error) are covered by the factor 1 + 2^-10 on every bound.

C_GELU is the smallest power of two for which `emulate_gelu` (numpy fp32, the kernel's operations in the kernel's order with fused
multiply-adds where -ffp-contract fuses them) stays at or under 0.75 of C_GELU max(|v|, TINY) on `gelu_grid` -- the rule C_REST of
attention_cases.py was chosen by, applied to the one term of the bound that is an estimate (`gelu_model_ratio` says why the derived
rounding terms stay out of it); tests/test_gemm_model.py asserts it and prints the ratios: 2^-22 gives 1.07, 2^-21 0.54, 2^-20 0.27 (worst at v = 0.068:
the 1.5e-7 absolute error of the Abramowitz-Stegun erf, times 0.5 |v|, plus the cancellation in 1 - erfc).
The emulation's one known difference from the hardware: it uses the exact reciprocal and exp2 (correctly rounded) where the kernel runs
v_rcp_f32 and v_exp_f32, which are good to one ulp.

Worst error / bound per epilogue and family: tests/test_gpu_gemm.py prints it per case and, in its last test, for the whole file (run
with -s).  The table has not been recorded from an MI355X run yet -- when it is, it belongs here, measured against this fp64 reference
and never against the kernel's own earlier output.  For orientation only, a torch fp32 stand-in for the kernel on the CPU (exact GELU,
sequential fp32 sums) gives: f16 0.99 and gelu_f16 0.99 (the fp16 rounding term is sharp), f32 0.10, resid_f32 0.90 and patch_f32 0.87
(the final fp32 addition is sharp), resid_pre_f32 0.09, h + lo / 64 of gelu_f16_x3 0.08; `exact` bit-equal throughout."""
import numpy as np
import torch

SPLIT = 64.0                                  # IBL_VIT_SPLIT_SCALE
U32 = 2.0 ** -24
F16_MAX = 65504.0
LIP = 1.13
TINY = 2.0 ** -24                             # only guards v == 0, where the kernel's result is exactly 0 as well
C_GELU = 2.0 ** -21
SLACK = 1.0 + 2.0 ** -10
EPI_F16, EPI_GELU, EPI_RESID, EPI_PATCH, EPI_F32, EPI_PRE, EPI_X2, EPI_X3 = range(8)
EPI_NAMES = ("f16", "gelu_f16", "resid_f32", "patch_f32", "f32", "resid_pre_f32", "gelu_f16_x2", "gelu_f16_x3")
F16_EPIS = (EPI_F16, EPI_GELU, EPI_X2, EPI_X3)
BIT_EXACT = (EPI_F16, EPI_RESID, EPI_PATCH, EPI_F32, EPI_PRE)     # on the `exact` family
FAMILIES = ("exact", "normal", "cancel", "gelu_span", "saturate")
SENT16 = 0x7E2A                               # an fp16 NaN pattern and an fp32 NaN pattern no kernel writes
SENT32 = 0x7FC5A3E1
SEED = 20251
ALPHA = 1.0 / 64.0                            # what the encoder passes for a second weight term
# biases of `saturate`: both sides of 65504 (65519.99 still rounds to 65504, 65520 is the first value that rounds to infinity) and far out
BIG = (65440.0, 65472.0, 65504.0, 65519.0, 65520.0, 65536.0, 65600.0, 70000.0, 1.0e5, 3.0e6)


def make(family, M, N, K, seed=SEED, resid=True):
    """-> dict x (M, K) fp16, W (N, K) fp16, bias / scale (N) fp32, resid (M, N) fp32 (what a read-modify-write epilogue finds in `out`;
    None with resid=False).  Independent draws per (row, k) and (col, k), seeded from the shape."""
    rng = np.random.default_rng([seed, M, N, K, FAMILIES.index(family)])
    f32 = np.float32
    if family == "exact":
        # integers -2 .. 2; x sparse enough that 2 sum_k |x_k| + max |bias| <= 2048: every partial sum in any order, and y + bias, is an
        # integer of at most 2048 in magnitude -- exact in fp32 and in fp16
        d = min(0.6, 300.0 / K)
        x = rng.integers(-2, 3, size=(M, K)) * (rng.random((M, K)) < d)
        W = rng.integers(-2, 3, size=(N, K)) * (rng.random((N, K)) < 0.6)
        assert 2 * int(np.abs(x).sum(axis=1).max()) + 40 <= 2048, "exact: a row of x is too dense"
        bias = rng.integers(-40, 41, size=N).astype(f32)
        scale = (2.0 ** rng.integers(-2, 3, size=N)).astype(f32)
        r = rng.integers(-1000, 1001, size=(M, N)).astype(f32) if resid else None
    elif family in ("normal", "saturate"):
        x = rng.standard_normal((M, K), dtype=f32)
        W = rng.standard_normal((N, K), dtype=f32) / f32(np.sqrt(K))
        bias = rng.standard_normal(N, dtype=f32)
        if family == "saturate":
            n = np.arange(N)
            big = np.asarray(BIG, f32)[(n // 2) % len(BIG)] * np.where(n % 2 == 0, 1.0, -1.0).astype(f32)
            bias = np.where(n % 32 < 24, big, bias).astype(f32)
        scale = rng.random(N, dtype=f32)
        r = rng.standard_normal((M, N), dtype=f32) if resid else None
    elif family == "cancel":
        # columns 2 i and 2 i + 1 carry products of opposite sign that agree to ~2^-7: sum |x w| ~ 10^3 |sum x w|
        a = 4.0 * rng.standard_normal((M, K // 2), dtype=f32)
        c = 4.0 * rng.standard_normal((N, K // 2), dtype=f32) / f32(np.sqrt(K))
        x = np.empty((M, K), f32)
        W = np.empty((N, K), f32)
        x[:, 0::2], x[:, 1::2] = a, a * (1.0 + 2.0 ** -7 * rng.standard_normal((M, K // 2), dtype=f32))
        W[:, 0::2], W[:, 1::2] = c, -c * (1.0 + 2.0 ** -7 * rng.standard_normal((N, K // 2), dtype=f32))
        bias = 0.01 * rng.standard_normal(N, dtype=f32)
        scale = rng.random(N, dtype=f32)
        r = rng.standard_normal((M, N), dtype=f32) if resid else None
    elif family == "gelu_span":
        # v = bias[n] + x[m][0] + noise: the bias steps through -12 .. 12 in 128 steps of 0.189 within every 128 columns (in a scrambled
        # order, so every lane's columns span the range), x[m][0] fills the step in 64 sub-steps every 64 rows, the noise (sigma 0.05)
        # makes it a continuum
        x = rng.standard_normal((M, K), dtype=f32)
        W = rng.standard_normal((N, K), dtype=f32) * f32(0.05 / np.sqrt(K))
        x[:, 0] = ((np.arange(M) * 29) % 64) / 64.0 * 0.1875
        W[:, 0] = 1.0
        bias = (-12.0 + 24.0 * (((np.arange(N) % 128) * 37) % 128) / 127.0).astype(f32)
        scale = rng.random(N, dtype=f32)
        r = rng.standard_normal((M, N), dtype=f32) if resid else None
    else:
        raise KeyError(family)
    return dict(x=x.astype(np.float16), W=W.astype(np.float16), bias=bias, scale=scale, resid=r)


def make_pos(family, P, N, seed=SEED):
    """position rows (P, N) fp32 of the patch epilogue: integers for `exact`"""
    rng = np.random.default_rng([seed, P, N, 77, FAMILIES.index(family)])
    if family == "exact":
        return rng.integers(-1000, 1001, size=(P, N)).astype(np.float32)
    return rng.standard_normal((P, N), dtype=np.float32)


def products(x, W):
    """x (M, K), W (N, K) fp16 tensors -> y = x W^T and S = |x| |W|^T in float64 on their device"""
    x64, W64 = x.double(), W.double()
    return x64 @ W64.t(), x64.abs() @ W64.abs().t()


def gelu64(v):
    """0.5 v (1 + erf(v / sqrt 2)) as 0.5 v erfc(-v / sqrt 2): no cancellation for v << 0"""
    return 0.5 * v * torch.special.erfc(v * (-0.70710678118654752440))


def _e1(S, bias, K):
    return (K + 2) * U32 * (S + (bias.abs() if bias is not None else 0.0))


def _f16_round(ref):
    return 2.0 ** -11 * ref.abs() + 2.0 ** -25


def expected(epi, y, S, K, bias=None, scale=None, resid=None, pos=None, alpha=1.0, accumulate=False):
    """-> (ref, bound) float64 (M, N) of the FIRST column block of epilogue `epi`.  bias / scale (N), resid / pos (M, N): float64 or None
    (pos already expanded to one row per row of x).  For the GELU epilogues also see `expected_two_term`."""
    b = bias if bias is not None else torch.zeros((), dtype=torch.float64, device=y.device)
    v = y + b
    e1 = _e1(S, bias, K)
    if epi == EPI_F32:
        ref, bnd = v, e1
    elif epi == EPI_F16:
        ref = v.clamp(-F16_MAX, F16_MAX)
        bnd = e1 + _f16_round(ref)
    elif epi in (EPI_GELU, EPI_X2, EPI_X3):
        ref = gelu64(v).clamp(-F16_MAX, F16_MAX)
        bnd = LIP * e1 + C_GELU * v.abs().clamp_min(TINY) + _f16_round(ref)
    elif epi == EPI_RESID:
        t = v * scale if scale is not None else v
        ref = resid + t
        bnd = (scale.abs() if scale is not None else 1.0) * e1 + U32 * t.abs() + U32 * ref.abs()
    elif epi == EPI_PRE:
        c0 = resid + b
        ref = c0 + alpha * y
        bnd = U32 * c0.abs() + (K + 2) * U32 * (alpha * S + c0.abs())
    elif epi == EPI_PATCH:
        if accumulate:
            ref = resid + alpha * v
            bnd = alpha * e1 + U32 * ref.abs()
        else:
            ref = v + pos
            bnd = e1 + U32 * ref.abs()
    else:
        raise KeyError(epi)
    return ref, bnd * SLACK


def expected_two_term(y, S, K, bias=None):
    """IBL_LINEAR_GELU_F16_X3: -> (ref, bound, valid) for h + lo / 64; valid = h is not saturated"""
    b = bias if bias is not None else torch.zeros((), dtype=torch.float64, device=y.device)
    v = y + b
    ref = gelu64(v)
    lo_round = 2.0 ** -11 * (2.0 ** -11 * ref.abs() + 2.0 ** -25) + 2.0 ** -31
    bnd = LIP * _e1(S, bias, K) + C_GELU * v.abs().clamp_min(TINY) + lo_round
    return ref, bnd * SLACK, ref.abs() <= F16_MAX


def split_of(h):
    """the last column block the kernel derives from the h it wrote: fp16(h / 64), from the fp32 value of h"""
    return (h.float() * (1.0 / SPLIT)).to(torch.float16)


# ---- the kernel's GELU on the CPU -------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    f64 = np.float64
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(np.float32)     # the product of two fp32 is exact in fp64


def emulate_gelu(v):
    """gelu_erf2 (csrc/vit_gemm.hip) in numpy fp32, operation for operation; v fp32 -> value fp32"""
    f = np.float32
    v = np.asarray(v, f)
    c = f(0.70710678118654752)
    z = np.abs(v) * c
    t = (1.0 / _fma(z, f(0.3275911), f(1.0)).astype(np.float64)).astype(f)
    p = _fma(t, f(1.061405429), f(-1.453152027))
    p = _fma(p, t, f(1.421413741))
    p = _fma(p, t, f(-0.284496736))
    p = _fma(p, t, f(0.254829592))
    a = (z * f(-1.4426950408889634)) * z
    e = np.exp2(a.astype(np.float64)).astype(f)
    u = _fma(-(p * t), e, f(1.0))
    return _fma(z * u, c, v * f(0.5))


def h16(x32):
    """f2h / f2h_pk: round to nearest even, clamped to the finite range"""
    with np.errstate(over="ignore"):
        return np.clip(np.asarray(x32, np.float32).astype(np.float16), -F16_MAX, F16_MAX)


def gelu_grid():
    """the pre-activations `gelu_span` covers, as a grid: -12 .. 12 in steps of 2^-15 * 1.5 and +-2^e for e = -20 .. 3.58 in 4096 steps"""
    lin = np.linspace(-12.0, 12.0, (1 << 19) + 1)
    geo = 2.0 ** np.linspace(-20.0, np.log2(12.0), 4096)
    return np.concatenate([lin, geo, -geo]).astype(np.float32)


def gelu_model_ratio(c_gelu):
    """-> (worst |value - gelu(v)| / (c_gelu max(|v|, TINY)), where, worst error / bound of h + lo / 64) of the emulation over `gelu_grid`
    for a candidate C_GELU (e1 = 0: the grid is the pre-activation itself).  The first is what the 0.75 rule is about: the fp32 value
    against the one term of the bound that is an estimate.  The roundings of h and lo are derived and sharp -- a legitimate rounding
    reaches them (an fp16 subnormal lo is off by half a step, 2^-31 after the division by 64, whenever value - h falls midway) -- so the
    two-term sum may come as close to its whole bound as it likes, and is only required to stay inside it."""
    v = gelu_grid()
    value = emulate_gelu(v)
    h = h16(value)
    lo = h16((value - h.astype(np.float32)) * np.float32(SPLIT))
    two = h.astype(np.float64) + lo.astype(np.float64) / SPLIT
    v64 = torch.from_numpy(v.astype(np.float64))
    ref = gelu64(v64).numpy()
    poly = c_gelu * np.maximum(np.abs(v.astype(np.float64)), TINY)
    lo_round = 2.0 ** -11 * (2.0 ** -11 * np.abs(ref) + 2.0 ** -25) + 2.0 ** -31
    r = np.abs(value.astype(np.float64) - ref) / poly
    r2 = np.abs(two - ref) / ((poly + lo_round) * SLACK)
    return float(r.max()), float(v[r.argmax()]), float(r2.max())


# ---- which tiles a workgroup walks: GEMM_SET_TILE and launch_gemm restated ---------------------------------------------------------------
def tile_walk(M, N, cus):
    """-> dict: t256, BM, nbn, nbm, nwg, grid, blocks = per workgroup the list of (row tile, column tile, full) it computes, in order.
    `cus`: the device's CU count rounded down to a multiple of 8 (at least 8), as launch_gemm_cfg does."""
    t256 = N % 256 == 0 and M >= 4096
    BM = 256 if t256 else 128
    nbn, nbm = N // BM, -(-M // BM)
    nwg = nbn * nbm
    grid = min(nwg, cus) if t256 else nwg
    q, r = nwg // 8, nwg % 8

    def place(t):
        xcd = t % 8
        bid = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + t // 8
        return bid // nbn, bid % nbn, (bid // nbn + 1) * BM <= M

    blocks = [[place(t) for t in range(b, nwg, grid)] for b in range(grid)]
    seen = sorted((rt, ct) for blk in blocks for rt, ct, _ in blk)
    assert seen == [(i, j) for i in range(nbm) for j in range(nbn)], "the remap must visit every tile once"
    return dict(t256=t256, BM=BM, nbn=nbn, nbm=nbm, nwg=nwg, grid=grid, blocks=blocks)


def full_then_ragged(walk):
    """workgroups whose walk contains a ragged tile directly after a full one (where the fp16 epilogues' tile-top wait changes from the
    counted vmcnt to vmcnt(0))"""
    return [b for b, blk in enumerate(walk["blocks"]) if any(f0 and not f1 for (_, _, f0), (_, _, f1) in zip(blk, blk[1:]))]
