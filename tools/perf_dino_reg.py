#!/usr/bin/env python3
"""GPU: the register / rotary encoders (DINOv2 with registers, DINOv3) -- what the rotation kernel costs, what each model's forward
costs next to its plain sibling, and which operand-term plan each configuration needs.

    python tools/perf_dino_reg.py [--out FILE] [step ...]

steps (default: all, each in a child process of its own under a time limit; the first failure ends the run):
    rope            ibl_rope_kernel beside the QKV GEMM of the same block (ibl_linear_f16, one term) on the dinov3_vitb16 and
                    dinov3_vitl16 shapes (224 crops x 201 tokens) and on a 581-token shape (ViT-B at 384 px, 64 crops): median of 20
                    windows of 8 calls (device events), round robin over four QKV buffers so that no call finds its rows in the caches
                    (one buffer: 207 MB at ViT-B); bytes = the q and k columns of the patch rows read and written once
    forward         forward of 224 crops (32 at 518 px) of every new model and of its plain sibling, default plan of each, median of 10
    gate:<model>[:<plan>,<plan>...]
                    embedding rel-L2 per crop against the fp32 restatement on the device over the ladder of operand-term plans
                    (or over the plans given) on the crops of tests/test_gpu_dino_reg.py's gate: plan, mean, max, forward time of the gate's batch"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LADDER = ("plain", "default", "p2;0:3232;1:2222;2:2211", "p2;0:3232;1:2222;2:2222;3:2211", "p2;0:3232;1:2222;2:2222;3:2222;4:2211",
          "p2;0:3232;1:2222;2:2222;3:2222;4:2222;5:2222;6:2211", "p2;*:2222;0:3232", "p2;*:3333")
LIMITS = {"rope": 240, "forward": 300, "gate": 420}
SIBLINGS = [("dinov2_vits14_reg", "dinov2_vits14"), ("dinov2_vitb14_reg", "dinov2_vitb14"), ("dinov2_vitl14_reg", None),
            ("dinov2_vitb14_reg_518", "dinov2_vitb14_518"), ("dinov3_vits16", None), ("dinov3_vitb16", "vit_b16"), ("dinov3_vitl16", None)]
ROPE_SHAPES = [("dinov3_vitb16", 224, 201, 12), ("dinov3_vitl16", 224, 201, 16), ("vitb16 at 384 px", 64, 581, 12)]


def median_ms(fn, reps=20, warm=5, inner=1):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return float(np.median(ts))


def step_rope(say):
    import torch
    from ibloc_amd import vit as V
    say("ibl_rope_kernel beside the block's QKV GEMM: ms per call, bytes of q and k of the patch rows read + written, achieved rate")
    for name, batch, T, heads in ROPE_SHAPES:
        D, prefix = 64 * heads, 5
        g = int(round((T - prefix) ** 0.5))
        table = torch.from_numpy(V.rope_table(g, g, 100.0)).cuda()
        gen = torch.Generator(device="cuda").manual_seed(3)
        bufs = [torch.randn((batch, T, 3 * D), device="cuda", generator=gen).to(torch.float16) for _ in range(4)]
        xn = torch.randn((batch * T, D), device="cuda", generator=gen).to(torch.float16)
        w = (0.03 * torch.randn((3 * D, D), device="cuda", generator=gen)).to(torch.float16)
        bias = torch.zeros(3 * D, device="cuda")
        k = [0]

        def rope(k_only=False):
            k[0] += 1
            V.rope_f16(bufs[k[0] % 4], table, heads, prefix, k_only=k_only)

        def gemm():
            k[0] += 1
            V.linear_f16(xn, w, bias, out=bufs[k[0] % 4].view(batch * T, 3 * D))

        t_rope, t_k, t_gemm = median_ms(rope, inner=8), median_ms(lambda: rope(True), inner=8), median_ms(gemm, inner=8)
        nbytes = 2 * batch * (T - prefix) * 2 * D * 2
        say(f"  {name:18s} {batch} x {T} tokens, {heads} heads: rope {t_rope:.4f} ms = {nbytes / 1e6:.1f} MB at {nbytes / t_rope / 1e9:.2f} TB/s"
            f" ({100 * nbytes / t_rope / 1e9 / 6.29:.0f} % of the 6.29 TB/s a float4 copy reaches); k_only {t_k:.4f} ms at "
            f"{nbytes / 2 / t_k / 1e9:.2f} TB/s; QKV GEMM {t_gemm:.4f} ms; rope / GEMM {100 * t_rope / t_gemm:.1f} %")
    return 0


def step_forward(say):
    import torch
    from ibloc_amd import vit as V
    say("forward of one batch, default plan of each model, median of 10 (ms): model | its plain sibling")
    gen = torch.Generator(device="cuda").manual_seed(7)
    for name, sib in SIBLINGS:
        row = []
        for n in (name, sib):
            if n is None:
                row.append("-")
                continue
            cfg = V.CONFIGS[n]
            batch = 224 if cfg.n_tokens <= 272 else 32
            enc = V.VitEncoder(cfg, V.random_weights(cfg, 30))
            patches = torch.randn((batch * cfg.n_patches, cfg.patch_k_pad), device="cuda", generator=gen).to(torch.float16)
            row.append(f"{n} ({batch} x {cfg.n_tokens} tokens, plan {enc.precision}) {median_ms(lambda: enc.forward_patches(patches), reps=10, warm=3):.3f}")
            del enc
            torch.cuda.empty_cache()
        say("  " + "  |  ".join(row))
    return 0


def step_gate(say, name, plans=LADDER):
    import torch
    from ibloc_amd import vit as V
    from tests.test_gpu_dino_reg import GATE, UNGATED, embed_both, gate_weights
    from tests.test_gpu_flip_rate import GpuCrops
    n_crops, batch = {**GATE, **UNGATED}[name]
    cfg = V.CONFIGS[name]
    ids = np.random.default_rng(3).integers(0, 100000, size=n_crops)
    crops = GpuCrops(21).variants(ids)
    w, wt = gate_weights(cfg)
    say(f"[gate {name}] {n_crops} crops, batch {batch}: plan, mean, max, forward of {batch} crops (ms)")
    ora = None
    for plan in plans:
        enc = V.VitEncoder(cfg, w, precision=None if plan == "default" else plan)
        if ora is None:
            hip, ora = embed_both(enc, wt, cfg, crops, batch)
        else:
            hip = np.concatenate([enc.forward_patches(enc.preprocess(crops[i:i + batch])).cpu().numpy() for i in range(0, n_crops, batch)])
        rel = np.linalg.norm(hip - ora, axis=1) / np.linalg.norm(ora, axis=1)
        patches = enc.preprocess(crops[:batch])
        ms = median_ms(lambda: enc.forward_patches(patches), reps=10, warm=2)
        ok = rel.max() < 1e-3 and rel.mean() < 0.85e-3
        say(f"  {plan:58s} {rel.mean():.3e} {rel.max():.3e} {ms:9.3f}  {'meets the gate' if ok else 'misses'}")
        del enc
        torch.cuda.empty_cache()
    return 0


def _gate_args(step):
    parts = step.split(":", 2)
    return (parts[1],) if len(parts) == 2 else (parts[1], tuple(parts[2].split(",")))


def main():
    args = sys.argv[1:]
    out = None
    if args[:1] == ["--out"]:
        out, args = args[1], args[2:]
    if args[:1] == ["--child"]:
        import torch
        assert torch.cuda.is_available(), "perf_dino_reg.py needs a GPU"
        step = args[1]
        f = open(out, "a") if out else None

        def say(s):
            print(s, flush=True)
            if f:
                f.write(s + "\n")
                f.flush()
        return {"rope": step_rope, "forward": step_forward}[step](say) if ":" not in step else step_gate(say, *_gate_args(step))
    from tests.test_gpu_dino_reg import GATE, UNGATED
    steps = args or ["rope", "forward"] + [f"gate:{m}" for m in {**GATE, **UNGATED}]
    for step in steps:
        limit = LIMITS[step.split(":")[0]]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + (["--out", out] if out else []) + ["--child", step]
        rc = subprocess.call(cmd, cwd=ROOT)
        if rc != 0:
            print(f"step {step} ended with status {rc}: nothing more is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
