"""-m gpu: every stage of the DATOR fusion head (csrc/dator.hip) alone, per token and per channel, against an fp64 recomputation of that
stage from the DEVICE's own inputs to it -- the workspace taps of `DatorHead.taps` (include/ibloc.h, IBL_DATOR_WS_*) cast to fp64 and
put through the stage functions of oracle/dator_oracle.py.  Queries and values come from the un-updated features, so every quantity is
one operation behind a tap (the final fr / fd: the four attentions behind cat, q_*, v_* and the gates); nothing is chained through
sigmoid logits.  Cases: tests/dator_head_cases.py (tests/test_dator_head_model.py shows on the CPU what each is there for).

Tolerance, per (case, stage): with e32 = max|stage_fp32 - stage_fp64|, both restatements fed the same tapped inputs,

    max|device - stage_fp64| <= max(16 * e32, 2^-22 * max|stage_fp64|)

The yardstick is the fp32 restatement's own distance to fp64, never the kernel's.  16 covers the sequential 768-term fmaf chain of
ibl_linear_f32_kernel against torch's blocked sums (about 3x under random rounding) and the device's expf; the floor covers stages
where fp32 torch happens to be exact.  A wrong tap, border, tile, gate or channel half lands four or more orders above it.

Worst device error / e32 per stage over all seven runs, measured on an MI355X (the bound is 16; `offset` samp has e32 = 0 -- saturated
selectors and one-hot attention pick single corner values -- and the device is exact there too, so the floor is never needed):

stage          recomputed from                                     worst ratio   run            device error   e32
gl             depth tokens (CLS rows, K = 768)                    3.73          random B=65    4.7e-06        1.3e-06
lp             depth tokens (patch rows, K = 768)                  2.87          random B=65    6.3e-06        2.2e-06
cat            both sides' tokens (projections + merge)            1.82          random B=2     3.0e-06        1.6e-06
cat[fd]<gl,lp  tapped gl, lp (the depth merge alone)               1.97          random B=1     3.0e-06        1.5e-06
h1             tapped cat                                          1.00          random B=2     7.1e-06        7.1e-06
h2             tapped h1                                           3.44          random B=1     1.6e-06        4.7e-07
h3             tapped h2                                           2.08          random B=1     3.0e-07        1.5e-07
h4             tapped h3                                           1.24          random B=1     6.1e-08        4.9e-08
rgb_f          tapped h4                                           1.00          random B=1     5.0e-08        5.0e-08
depth_f        tapped h4                                           1.03          random B=1     5.6e-08        5.5e-08
q_r, v_r       tapped cat (rgb half)                               1.00          offset B=2     1.3e-04        1.3e-04
q_d, v_d       tapped cat (depth half)                             1.00          random B=1     1.9e-06        1.9e-06
sel  (r2d)     tapped q_r                                          1.00          offset B=2     1.1e-06        1.1e-06
aw   (r2d)     tapped q_r (logits; the softmax is in the sampler)  1.10          borders B=2    8.7e-07        7.9e-07
samp (r2d)     tapped sel, aw, v_d                                 1.86          borders B=2    8.1e-07        4.4e-07
feat (r2d)     tapped samp                                         1.00          borders B=2    1.1e-06        1.1e-06
fr             tapped cat, q_*, v_*, rgb_f (r2r then d2r)          1.06          sharp B=2      2.6e-05        2.5e-05
fd             tapped cat, q_*, v_*, depth_f (d2d then r2d)        1.09          random B=1     5.6e-06        5.2e-06
out            tapped fr, fd, rgb_f, depth_f                       6.31          random B=2     5.4e-07        8.6e-08

A ratio of 1.00 means that the device's worst element is as far from fp64 as the fp32 restatement's worst element: on the K = 128
linears a k-ordered fmaf chain with the bias added last rounds like torch's fp32 CPU GEMM does.  The rows q_r, v_r / q_d, v_d show the
worse of the two stages.
"""
import numpy as np
import pytest
import torch

from oracle import dator_oracle as do
from tests import dator_head_cases as hc

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 16.0, 2.0 ** -22
RUNS = [("random", 1), ("random", 2), ("random", 65), ("borders", 2), ("gates", 2), ("offset", 2), ("sharp", 2)]
FULL_BATCH = 2          # above it only the projection, merge and pooled stages are recomputed


@pytest.fixture(scope="module")
def heads():
    from ibloc_amd import dator as D
    cache = {}

    def get(name):
        if name not in cache:
            hw = hc.case_weights(name)
            cache[name] = (hw, D.DatorHead(hw))
        return cache[name]
    return get


def recompute(hw, rt, dt, tap, dtype, full):
    """stage name -> that stage in `dtype`, from the tokens (gl, lp, cat) or from the taps in front of it (everything else)"""
    h = do.head_weights_as(hw, dtype)
    t = {k: v.to(dtype) for k, v in tap.items()}
    xr, xd = torch.from_numpy(rt).to(dtype), torch.from_numpy(dt).to(dtype)
    r = {}
    r["gl"], r["lp"] = do.stage_project(h, "depth", xd)
    r["cat"] = torch.cat((do.stage_merge(h, "depth", r["gl"], r["lp"]), do.stage_merge(h, "rgb", *do.stage_project(h, "rgb", xr))), -1)
    r["cat[fd]<gl,lp"] = do.stage_merge(h, "depth", t["gl"], t["lp"])
    r["out"] = do.stage_pool(t["fr"], t["fd"], t["rgb_f"], t["depth_f"])
    if not full:
        return r
    prev = t["cat"]
    for i in range(4):
        r[f"h{i + 1}"] = do.stage_hyper(h, i, prev)
        prev = t[f"h{i + 1}"]
    r["rgb_f"], r["depth_f"] = do.stage_gates(t["h4"])
    fd, fr = t["cat"][:, :128], t["cat"][:, 128:]
    r["q_r"], r["v_r"] = do.stage_linear(h, "Q_r", fr), do.stage_linear(h, "V_r", fr)
    r["q_d"], r["v_d"] = do.stage_linear(h, "Q_d", fd), do.stage_linear(h, "V_d", fd)
    r["sel"], r["aw"] = do.stage_sel(h, "r2d", t["q_r"]), do.stage_aw_logits(h, "r2d", t["q_r"])
    r["samp"] = do.stage_sample(t["sel"], t["aw"], t["v_d"])
    r["feat"] = do.stage_ffn(h, "r2d", t["samp"])
    fin = do.stage_final(h, t["cat"], t["q_r"], t["v_r"], t["q_d"], t["v_d"], t["rgb_f"], t["depth_f"])
    r["fr"], r["fd"] = fin["fr"], fin["fd"]
    return r


@pytest.mark.parametrize("name,batch", RUNS, ids=[f"{n}-B{b}" for n, b in RUNS])
def test_every_stage_against_fp64_from_the_devices_own_inputs(heads, name, batch):
    hw, head = heads(name)
    rt, dt = hc.tokens(batch)
    out = head.forward(torch.from_numpy(rt).cuda(), torch.from_numpy(dt).cuda())
    tap = {k: v.cpu() for k, v in head.taps(batch).items()}
    dev = dict(tap, out=out.cpu())
    dev["cat[fd]<gl,lp"] = tap["cat"][:, :128]
    for k, v in dev.items():
        assert bool(torch.isfinite(v).all()), f"{name} B={batch}: non-finite values in {k}"
    full = batch <= FULL_BATCH
    with torch.no_grad():
        r64, r32 = recompute(hw, rt, dt, tap, torch.float64, full), recompute(hw, rt, dt, tap, torch.float32, full)
    missed = []
    for stage, ref in r64.items():
        got = dev[stage].to(torch.float64)
        assert got.shape == ref.shape, (stage, got.shape, ref.shape)
        err = float((got - ref).abs().max())
        e32 = float((r32[stage].to(torch.float64) - ref).abs().max())
        tol = max(FACTOR * e32, FLOOR * float(ref.abs().max()))
        at = np.unravel_index(int((got - ref).abs().argmax()), ref.shape)
        print(f"[dator head] {name:8s} B={batch:<3d} {stage:14s} device err {err:.3e}  e32 {e32:.3e}  ratio {err / e32 if e32 else float('inf'):8.2f}"
              f"  tol {tol:.3e}  max|ref| {float(ref.abs().max()):.3e}  worst at {tuple(int(i) for i in at)}")
        if not err <= tol:
            missed.append((stage, err, e32, tol, tuple(int(i) for i in at)))
    assert not missed, missed


def test_taps_are_views_of_the_workspace_the_forward_used(heads):
    """`taps` reads the layout the library reports: after a forward the final features it shows pool to the returned embedding (checked
    above to rounding), and a second forward on another lane leaves the first lane's taps untouched"""
    hw, head = heads("random")
    rt, dt = hc.tokens(2)
    out0 = head.forward(torch.from_numpy(rt).cuda(), torch.from_numpy(dt).cuda(), lane=0)
    before = {k: v.clone() for k, v in head.taps(2, lane=0).items()}
    out1 = head.forward(torch.from_numpy(rt[:1]).cuda(), torch.from_numpy(dt[:1]).cuda(), lane=1)
    after = head.taps(2, lane=0)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert torch.equal(out0[:1], out1)                 # crops are independent: the same crop alone gives the same bits
    for k, v in head.taps(1, lane=1).items():
        assert torch.equal(v, before[k][:v.shape[0]]), k
