"""-m gpu: the SigLIP attention-pooling head (csrc/siglip.hip) alone.

1. `ibl_probe_pool_f32`, the pooling kernel: probabilities and pooled tokens against float64 computed from the same fp32 inputs, for
   every token count at which the kernel's loops change shape (1, 2, one wave of tokens +- 1, the 196 / 256 / 576 of the configurations,
   729) times every (dim, heads) the token interleave of its weighted sum differs for, on five input families:
     uniform   scores within +-0.15: the softmax is nearly flat, every token carries weight
     peak0     token 0 lies 10 .. 40 logits above the rest (per crop and head): one probability is ~1, the others down to e^-40
     peakT     the same at token T - 1 (the last, partial round of the token loops)
     offset    +60 on every score: without the max subtraction exp overflows to infinity
     ramp      x grows with the token index: a token taken twice, skipped or weighted with a neighbour's probability shows in pooled
   The batch of 3 crops is held to the project's stage rule; batch 1 (every crop alone) and batch 65 (the three crops cycled: crop i is
   crop i % 3, so a wrong crop offset shows) must reproduce those bits -- a crop's result does not depend on its batch -- and so does a
   second run and a run without the probabilities.  Outputs lie between NaN guard rows.
2. `ibl_probe_head_forward` stage by stage: every stage recomputed in float64 from the DEVICE's own inputs to it (the workspace taps of
   `ProbeHead.taps`), on tiny_siglip and siglip_b16_224 head weights.

Tolerance, per (case, stage), as tests/test_gpu_dator_head.py: with e32 = max|stage_fp32 - stage_fp64| of the torch fp32 CPU
restatement fed the same inputs,

    max|device - stage_fp64| <= max(16 * e32, 2^-22 * max|stage_fp64|)

The yardstick is the fp32 restatement's own distance to float64, never the kernel's.

Worst device error / e32, measured on an MI355X (the bound is 16; the tests print one line per case and stage, run with -s).

The pooling kernel alone, over the 45 shapes, per family (450 lines):

family    worst ratio   at                         stage    device error   e32
uniform   1.88          T=729 D=768  H=12          pooled   5.1e-09        2.7e-09
peak0     5.16          T=256 D=128  H=1           probs    1.5e-07        2.9e-08
peakT     2.95          T=256 D=128  H=1           probs    1.6e-07        5.3e-08
offset    1.85          T=729 D=1024 H=16          pooled   1.5e-05        8.3e-06
ramp      1.60          T=729 D=768  H=12          pooled   8.9e-07        5.6e-07

(on the peaked families e32 is little more than the rounding of one probability of ~1, 3e-8 .. 5e-8, and the device's IEEE division
and expf land within 1.6e-7 of float64.)

The head, over the five runs:

stage    recomputed from                         worst ratio   run                     device error   e32
probs    tokens, u                               1.05          tiny_siglip B=1         7.9e-08        7.5e-08
pooled   tokens, u                               1.00          tiny_siglip B=1         4.1e-07        4.1e-07
vcat     tapped pooled (per-head W_v, K = dim)   3.96          siglip_b16_224 B=3      3.5e-06        8.7e-07
att      tapped vcat (out_proj)                  3.53          siglip_b16_224 B=3      2.2e-06        6.2e-07
ln       tapped att                              1.60          tiny_siglip B=3         5.3e-07        3.3e-07
hid      tapped ln (fc1 + tanh GELU)             3.22          tiny_siglip B=3         1.7e-06        5.2e-07
out      tapped att, hid (fc2 + residual)        6.06          siglip_b16_224 B=65     5.2e-06        8.5e-07

The linears are one k-ordered fmaf chain per output (K = 768 .. 3 072) against torch's blocked fp32 sums, as in the DATOR head (worst
6.3 there).  The whole head is 5e-7 (tiny_siglip) / 1.2e-6 (siglip_b16_224) from the unfolded float64 head.
"""
import numpy as np
import pytest
import torch

from tests import siglip_cases as SC

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 16.0, 2.0 ** -22
TOKENS = (1, 2, 63, 64, 65, 196, 256, 576, 729)
DIMS = ((128, 1), (128, 2), (384, 6), (768, 12), (1024, 16))
FAMILIES = ("uniform", "peak0", "peakT", "offset", "ramp")
NAN32 = 0x7FC5A3E1


def make_inputs(family, B, T, D, H):
    """-> x (B, T, D), u (H, D) fp32 numpy, seeded from the shape"""
    rng = np.random.default_rng([77, T, D, H, FAMILIES.index(family)])
    u = (rng.standard_normal((H, D)) / np.sqrt(D)).astype(np.float32)
    un = np.linalg.pinv(u.astype(np.float64)).T                  # u un^T = 1: x += c un[h] raises score h by c and no other score
    x = rng.standard_normal((B, T, D))
    if family == "uniform":
        x *= 0.05
    elif family in ("peak0", "peakT"):
        c = rng.uniform(10.0, 40.0, size=(B, H))
        x[:, 0 if family == "peak0" else T - 1] += c @ un
    elif family == "offset":
        x += 60.0 * un.sum(0)
    elif family == "ramp":
        x = 0.3 * x + (np.arange(1, T + 1)[None, :, None] / T) * rng.standard_normal((B, 1, D))
    return x.astype(np.float32), u


def guarded(shape):
    """an fp32 device buffer of `shape` between one NaN guard row (of shape[1:]) on either side -> (buffer as int32, the window)"""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), NAN32, dtype=torch.int32, device="cuda")
    return buf, buf[1:-1].view(torch.float32)


def guards_intact(buf):
    return bool((buf[0] == NAN32).all()) and bool((buf[-1] == NAN32).all())


def run_pool(x, u, want_probs=True):
    from ibloc_amd import siglip as S
    B, T, D = x.shape
    H = u.shape[0]
    pb, pooled = guarded((B, H, D))
    qb, probs = guarded((B, H, T))
    S.probe_pool(x, u, want_probs=want_probs, pooled=pooled, probs=probs if want_probs else None)
    torch.cuda.synchronize()
    assert guards_intact(pb) and guards_intact(qb), "wrote outside its rows"
    if not want_probs:
        assert bool((qb == NAN32).all()), "probs = NULL wrote probabilities somewhere"
    return pooled, probs


def judge(what, stage, dev, r64, r32, missed):
    got = dev.detach().cpu().to(torch.float64)
    assert got.shape == r64.shape, (what, stage, got.shape, r64.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values in {stage}"
    err = float((got - r64).abs().max())
    e32 = float((r32.to(torch.float64) - r64).abs().max())
    tol = max(FACTOR * e32, FLOOR * float(r64.abs().max()))
    print(f"[probe head] {what:34s} {stage:7s} device err {err:.3e}  e32 {e32:.3e}  ratio {err / e32 if e32 else float('inf'):8.2f}  tol {tol:.3e}"
          f"  max|ref| {float(r64.abs().max()):.3e}")
    if not err <= tol:
        missed.append((what, stage, err, e32, tol))


@pytest.mark.parametrize("dim,heads", DIMS, ids=[f"D{d}H{h}" for d, h in DIMS])
@pytest.mark.parametrize("T", TOKENS)
def test_pool_kernel_vs_fp64(T, dim, heads):
    missed = []
    for family in FAMILIES:
        what = f"T={T} D={dim} H={heads} {family}"
        xn, un = make_inputs(family, 3, T, dim, heads)
        x, u = torch.from_numpy(xn).cuda(), torch.from_numpy(un).cuda()
        pooled, probs = run_pool(x, u)
        # the condition the family is there for, on the float64 reference
        p64, o64 = SC.stage_pool(torch.from_numpy(xn).double(), torch.from_numpy(un).double())
        p32, o32 = SC.stage_pool(torch.from_numpy(xn), torch.from_numpy(un))
        s64 = torch.einsum("btd,hd->bht", torch.from_numpy(xn).double(), torch.from_numpy(un).double())
        if family == "offset":
            assert float(s64.min()) > 45.0
        if family in ("peak0", "peakT") and T > 1:
            t = 0 if family == "peak0" else T - 1
            assert bool((p64.argmax(-1) == t).all()) and float(p64[:, :, t].min()) > 0.9
        if family == "uniform" and T > 1:
            assert float(p64.max()) * T < 2.0
        judge(what, "probs", probs, p64, p32, missed)
        judge(what, "pooled", pooled, o64, o32, missed)
        assert float((probs.sum(-1) - 1.0).abs().max()) < 1e-5
        # the same bits: a second run, a run without the probabilities, every crop alone, the crops cycled through a batch of 65
        pooled2, probs2 = run_pool(x, u)
        assert torch.equal(pooled2, pooled) and torch.equal(probs2, probs), f"{what}: two runs differ"
        pooled3, _ = run_pool(x, u, want_probs=False)
        assert torch.equal(pooled3, pooled), f"{what}: probs = NULL changes pooled"
        for b in range(3):
            p1, q1 = run_pool(x[b:b + 1].contiguous(), u)
            assert torch.equal(p1[0], pooled[b]) and torch.equal(q1[0], probs[b]), f"{what}: crop {b} alone differs from the crop in the batch"
        if family in ("peakT", "ramp"):
            idx = torch.arange(65, device="cuda") % 3
            p65, q65 = run_pool(x[idx].contiguous(), u)
            assert torch.equal(p65, pooled[idx]) and torch.equal(q65, probs[idx]), f"{what}: batch 65 differs from the same crops in a batch of 3"
    assert not missed, missed


def _head_case(name, batch):
    from ibloc_amd import siglip as S
    from ibloc_amd import vit as V
    cfg = V.CONFIGS[name]
    hw = S.random_head_weights(cfg, SC.GATE_HEAD_SEED)
    # post-LayerNorm tokens: unit-variance rows with a gain and a shift per column
    rng = np.random.default_rng([88, cfg.dim, batch])
    tok = rng.standard_normal((batch, cfg.n_tokens, cfg.dim))
    tok = (tok - tok.mean(-1, keepdims=True)) / tok.std(-1, keepdims=True) * (1 + 0.1 * rng.standard_normal(cfg.dim)) + 0.1 * rng.standard_normal(cfg.dim)
    return cfg, hw, tok.astype(np.float32)


@pytest.mark.parametrize("name,batch", [("tiny_siglip", 1), ("tiny_siglip", 3), ("tiny_siglip", 65), ("siglip_b16_224", 3), ("siglip_b16_224", 65)],
                         ids=lambda v: str(v))
def test_every_stage_of_the_head_against_fp64_from_the_devices_own_inputs(name, batch):
    from ibloc_amd import siglip as S
    cfg, hw, tok = _head_case(name, batch)
    head = S.ProbeHead(cfg, hw)
    t = torch.from_numpy(tok).cuda()
    out = head.forward(t)
    torch.cuda.synchronize()
    tap = {k: v.cpu() for k, v in head.taps(batch).items()}
    dev = dict(tap, out=out.cpu())
    u = head.u.cpu().numpy()
    r64 = SC.head_stages(hw, cfg, u, tok, tap, torch.float64)
    r32 = SC.head_stages(hw, cfg, u, tok, tap, torch.float32)
    missed = []
    for stage in ("probs", "pooled", "vcat", "att", "ln", "hid", "out"):
        judge(f"{name} B={batch}", stage, dev[stage], r64[stage], r32[stage], missed)
    assert not missed, missed
    # the seeded head does not pool uniformly on these tokens either, and the whole head agrees with the unfolded float64 head
    assert float(r64["probs"].max(-1).values.mean()) >= 4.0 / cfg.n_tokens
    full = SC.head_unfolded(hw, cfg, torch.from_numpy(tok).double())
    rel = float((out.cpu().double() - full).norm() / full.norm())
    print(f"[probe head] {name} B={batch}: whole head vs the unfolded float64 head: rel-L2 {rel:.2e}")
    assert rel < 1e-5
    # a crop alone gives the bits it has in the batch, on another lane, and leaves the first lane's taps alone
    out1 = head.forward(t[batch - 1:].contiguous(), lane=1)
    assert torch.equal(out1[0], out[batch - 1])
    for k, v in head.taps(batch).items():
        assert torch.equal(v.cpu(), tap[k]), k
    # the pooling kernel on its own is the head's first stage, bit for bit
    pooled, probs = S.probe_pool(t, head.u)
    assert torch.equal(pooled.cpu(), tap["pooled"]) and torch.equal(probs.cpu(), tap["probs"])
