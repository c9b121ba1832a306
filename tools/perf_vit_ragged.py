#!/usr/bin/env python3
"""GPU: the ragged ViT forward (ibl_vit_forward_ragged, native-aspect crops) on dinov2_vitb14 beside the fixed forward.

    python tools/perf_vit_ragged.py [--out FILE] [step ...]

steps (default: all, each in a child process of its own under a time limit; the first failure ends the run).  Medians of device-event
timings after a warm-up; none is a condition:
    forward         224 crops at the model's own 16 x 16 grid: forward_ragged beside forward_patches of the same crops -- the price of the
                    streaming attention below 272 tokens and of the gather / scatter kernels
    crops           224 variable-size crops of the bench generator (H, W ~ U{64..400}) under upscale=True and upscale=False: total tokens,
                    and preprocessing + forward in ms beside the fixed path's on the same crops
    kernel          the ragged attention alone on those two segment lists beside the resident kernel at T = 257, 12 heads
    gate:<model>    embedding rel-L2 per crop against the fp32 restatement on the device at every crop's grid, 224 u8 crops of 12 shapes,
                    over the ladder of operand-term plans: plan, mean, max, forward in ms"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.perf_attention_long import LADDER, median_ms  # noqa: E402

N, MODEL = 224, "dinov2_vitb14"
GATE_MODELS = ("dinov2_vitb14", "dinov2_vitb14_reg")
LIMITS = {"forward": 240, "crops": 300, "kernel": 240, "gate": 540}


def _encoder(name=MODEL, plan=None):
    from ibloc_amd import vit as V
    from tests import vit_ragged_cases as RC
    cfg = RC.config(name)
    return V.VitEncoder(cfg, V.random_weights(cfg, 20), precision=plan)


def _var_crops():
    import bench
    gen, rng = bench.VarCrops(21), np.random.default_rng(10)
    return [gen.make(k % 50, rng) for k in range(N)]


def _grids(enc, crops, upscale):
    from ibloc_amd import vit as V
    return [V.native_grid(c.shape[0], c.shape[1], enc.cfg.patch, enc.cfg.n_patches, upscale) for c in crops]


def step_forward(say):
    import torch
    enc = _encoder()
    cfg = enc.cfg
    x = torch.randn((N, 3, cfg.img_h, cfg.img_w), device="cuda")
    fixed, ragged, grids = enc.patches_from_pixels(x), enc.patches_from_pixels_ragged(list(x)), [cfg.grid] * N
    a = median_ms(lambda: enc.forward_patches(fixed), reps=10, warm=3)
    b = median_ms(lambda: enc.forward_ragged(ragged, grids), reps=10, warm=3)
    say(f"  {MODEL} (plan {enc.precision}), {N} crops at 16 x 16: forward_patches {a:.2f} ms, forward_ragged {b:.2f} ms ({b / a:.2f}x; includes "
        "the host's offset and position-row assembly)")
    return 0


def step_crops(say):
    from ibloc_amd import vit as V
    enc = _encoder()
    crops = V.PackedCrops(_var_crops())
    fixed = median_ms(lambda: enc.forward_patches(enc.preprocess(crops)), reps=10, warm=3)
    say(f"  {MODEL}, {N} variable-size crops: fixed path (centre crop, {N * enc.cfg.n_tokens} tokens) preprocess + forward {fixed:.2f} ms")
    for upscale in (True, False):
        grids = _grids(enc, [np.empty(s) for s in crops.shapes], upscale)
        tokens = int(enc.seq_offsets(grids)[-1])
        ms = median_ms(lambda: enc.forward_ragged(enc.preprocess_ragged(crops, grids), grids), reps=10, warm=3)
        say(f"    native aspect, upscale={upscale}: {tokens} tokens, preprocess + forward {ms:.2f} ms ({ms / fixed:.2f}x the fixed path)")
    return 0


def step_kernel(say):
    import torch
    from ibloc_amd import vit as V
    enc = _encoder()
    H, D = enc.cfg.heads, enc.cfg.dim
    crops = _var_crops()
    qkv = torch.randn((N, 257, 3 * D), device="cuda").to(torch.float16)
    out = torch.zeros((N, 257, D), dtype=torch.float16, device="cuda")
    res = median_ms(lambda: V.attention_f16(qkv, H, out=out))
    say(f"  attention alone, {N} crops, {H} heads: resident kernel at T = 257 ({N * 257} rows) {res:.4f} ms")
    for label, grids in (("16 x 16 each", [(16, 16)] * N), ("upscale=True", _grids(enc, crops, True)), ("upscale=False", _grids(enc, crops, False))):
        seq = enc.seq_offsets(grids)
        q = torch.randn((int(seq[-1]), 3 * D), device="cuda").to(torch.float16)
        o = torch.zeros((int(seq[-1]), D), dtype=torch.float16, device="cuda")
        ms = median_ms(lambda: V.attention_ragged_f16(q, seq, H, out=o))
        say(f"    ragged kernel, {label}: {int(seq[-1])} rows, longest {int(np.diff(seq).max())}: {ms:.4f} ms (includes the upload of the offsets)")
    return 0


def step_gate(say, name):
    import torch
    from ibloc_amd import vit as V
    from oracle import vit_oracle as vo
    from tests import dino_reg_cases as DC
    from tests import vit_ragged_cases as RC
    from tests.test_gpu_flip_rate import GpuCrops
    from tests.test_gpu_vit_ragged import SHAPES
    cfg = RC.config(name)
    w = DC.seeded_weights(cfg, DC.GATE_WEIGHT_SEED)
    wt = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).cuda() for k, v in w.items()}
    u8 = GpuCrops(21).variants(np.random.default_rng(3).integers(0, 100000, size=N)).cpu().numpy()
    crops = [np.ascontiguousarray(c[:SHAPES[i % 12][0], :SHAPES[i % 12][1]]) for i, c in enumerate(u8)]
    grids = [V.native_grid(c.shape[0], c.shape[1], cfg.patch, cfg.n_patches) for c in crops]
    ref = None
    say(f"  {name}, {N} u8 crops of 12 shapes at their native grids: plan, rel-L2 mean, max, forward_ragged")
    for plan in LADDER:
        enc = V.VitEncoder(cfg, w, precision=V.DEFAULT_PRECISION if plan == "default" else plan)
        patches, imgs = enc.preprocess_ragged(crops, grids, want_u8=True)
        out = enc.forward_ragged(patches, grids).clone()
        if ref is None:
            mean = torch.tensor(enc.recipe.mean, dtype=torch.float32, device="cuda")
            std = torch.tensor(enc.recipe.std, dtype=torch.float32, device="cuda")
            ref = torch.zeros_like(out)
            for grid in sorted(set(grids)):
                idx = [i for i, g in enumerate(grids) if g == grid]
                x = (((torch.stack([imgs[i] for i in idx]).to(torch.float64) * (1 / 255)).to(torch.float32) - mean) / std).permute(0, 3, 1, 2).contiguous()
                c = RC.at_grid(cfg, grid)
                r = DC.forward(wt, c, x, device="cuda") if cfg.n_registers else vo.vit_forward(wt, c, x, device="cuda")
                ref[idx] = torch.from_numpy(r).cuda()
        rel = (torch.linalg.norm(out - ref, dim=1) / torch.linalg.norm(ref, dim=1)).cpu().numpy()
        ms = median_ms(lambda: enc.forward_ragged(patches, grids), reps=5, warm=2)
        say(f"    {plan:52s} {rel.mean():.3e}  {rel.max():.3e}  {ms:8.2f} ms{'   (inside the gate)' if rel.max() < 1e-3 and rel.mean() < 0.85e-3 else ''}")
        del enc
    return 0


def main():
    argv = sys.argv[1:]
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    child = "--step" in argv
    if child:
        argv.remove("--step")

    def say(line):
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")

    if child:
        import torch
        if not torch.cuda.is_available():
            sys.exit("perf_vit_ragged: no GPU (nothing here is measured without one)")
        step = argv[0]
        fn = {"forward": step_forward, "crops": step_crops, "kernel": step_kernel}.get(step)
        sys.exit(fn(say) if fn else step_gate(say, step.split(":", 1)[1]))
    steps = argv or ["forward", "crops", "kernel"] + [f"gate:{m}" for m in GATE_MODELS]
    for step in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + (["--out", out] if out else [])
        try:
            rc = subprocess.run(cmd, timeout=LIMITS[step.split(":")[0]]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            say(f"step {step} ended with status {rc}: stopping")
            sys.exit(rc)


if __name__ == "__main__":
    main()
