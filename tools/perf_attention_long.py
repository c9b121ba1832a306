#!/usr/bin/env python3
"""GPU: the streaming attention kernel (ibl_attention_stream_f16, rows beyond 272 tokens) and the high-resolution encoders that run it.

    python tools/perf_attention_long.py [--out FILE] [step ...]

steps (default: all, each in a child process of its own under a time limit; the first failure ends the run):
    kernel          median of 20 launches (device events, after a warm-up) at B = 32, heads 12, T = 577 / 1025 / 1370: terms 1 and 3 with
                    all rows as queries, and cls_only; in the same process ibl_attention_f16 at T = 272 and
                    torch.nn.functional.scaled_dot_product_attention on the same fp16 tensors.  Condition (exit status 1 if missed): the
                    time per query x key pair of the streaming kernel at T = 577 and 1370 is at most 2x the resident kernel's at T = 272.
    forward         clip_l14_336_openai and dinov2_vitb14_518: forward of 32 crops under the model's plan, and the attention launches' share
    gate:<model>    embedding rel-L2 per crop against the fp32 restatement on the device, 32 u8 crops of the bench generator, over the ladder
                    of operand-term plans: plan, mean, max, forward time of 32 crops"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, HEADS, T_LONG, T_RES = 32, 12, (577, 1025, 1370), 272
GATE_MODELS = ("dinov2_vitb14_518", "dinov2_vitb14_448", "clip_l14_336_openai")
LADDER = ("plain", "default", "p2;0:3232;1:2222;2:2211", "p2;0:3232;1:2222;2:2222;3:2211", "p2;0:3232;1:2222;2:2222;3:2222;4:2211",
          "p2;0:3232;1:2222;2:2222;3:2222;4:2222;5:2222;6:2211", "p2;*:2222;0:3232", "p2;*:3333")
LIMITS = {"kernel": 240, "forward": 300, "gate": 420}


def median_ms(fn, reps=20, warm=5):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def step_kernel(say):
    import torch
    from ibloc_amd import vit as V
    D = 64 * HEADS
    gen = torch.Generator(device="cuda").manual_seed(7)
    per_pair = {}
    say(f"attention kernels, B = {B}, heads = {HEADS} (dim {D}), median of 20 launches, ms  [ns per query x key pair of one head]")
    for T in (T_RES,) + T_LONG:
        qkv = torch.randn((B, T, 3 * D), device="cuda", generator=gen).to(torch.float16)
        entry, name = (V.attention_f16, "resident") if T <= 272 else (V.attention_stream_f16, "stream")
        row = []
        for terms, cls in ((1, False), (3, False), (1, True)):
            out = torch.zeros((B, T, terms * D), dtype=torch.float16, device="cuda")
            ms = median_ms(lambda: entry(qkv, HEADS, cls_only=cls, terms=terms, out=out))
            row.append(ms)
            if terms == 1 and not cls:
                per_pair[T] = ms * 1e6 / (B * HEADS * T * T)
        q, k, v = (qkv[:, :, i * D:(i + 1) * D].reshape(B, T, HEADS, 64).transpose(1, 2) for i in range(3))
        sd = median_ms(lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v))
        say(f"  T {T:5d} {name:8s} terms 1 {row[0]:8.4f}  terms 3 {row[1]:8.4f}  cls_only {row[2]:8.4f}   [{per_pair[T]:.4f}]   "
            f"SDPA {sd:8.4f}  (kernel / SDPA {row[0] / sd:.2f})")
    ok = True
    for T in (577, 1370):
        ratio = per_pair[T] / per_pair[T_RES]
        ok &= ratio <= 2.0
        say(f"  per-pair time, stream T {T} / resident T {T_RES}: {ratio:.2f}  ({'within' if ratio <= 2.0 else 'MISSES'} the 2x condition)")
    return 0 if ok else 1


def _layer_terms(enc):
    nrun = enc.cfg.depth if enc.cfg.n_blocks_run < 0 else enc.cfg.n_blocks_run
    return [max(int(enc.W.layers[l].o_terms), 1) for l in range(nrun)]


def step_forward(say):
    import torch
    from ibloc_amd import vit as V
    for name in ("clip_l14_336_openai", "dinov2_vitb14_518"):
        cfg = V.CONFIGS[name]
        enc = V.VitEncoder(cfg, V.random_weights(cfg, 20))
        T, D = cfg.n_tokens, cfg.dim
        patches = torch.randn((B * (T - 1), cfg.patch_k_pad), device="cuda").to(torch.float16)
        fwd = median_ms(lambda: enc.forward_patches(patches), reps=10, warm=3)
        qkv = torch.randn((B, T, 3 * D), device="cuda").to(torch.float16)
        terms = _layer_terms(enc)
        att = 0.0
        for l, t in enumerate(terms):
            last = l == len(terms) - 1 and not cfg.out_all_tokens
            out = torch.zeros((B, T, t * D), dtype=torch.float16, device="cuda")
            att += median_ms(lambda: V.attention_stream_f16(qkv, cfg.heads, cls_only=last, terms=t, out=out), reps=10, warm=2)
        say(f"  {name} ({T} tokens, plan {enc.precision}): forward of {B} crops {fwd:.2f} ms, its {len(terms)} attention launches "
            f"{att:.2f} ms = {100 * att / fwd:.1f} %")
    return 0


def step_gate(say, name):
    import torch
    from ibloc_amd import vit as V
    from tests import clip_openai_cases as CQ
    from tests.test_gpu_flip_rate import GpuCrops
    cfg = V.CONFIGS[name]
    w = V.random_weights(cfg, 20)
    if cfg.pre_ln:
        w["patch.b"] = np.zeros_like(w["patch.b"])
    wt = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).cuda() for k, v in w.items()}
    u8 = GpuCrops(21).variants(np.random.default_rng(3).integers(0, 100000, size=B))
    ref, passed = None, False
    say(f"  {name} ({cfg.n_tokens} tokens), {B} u8 crops: plan, rel-L2 mean, max, forward of {B} crops")
    for plan in LADDER:
        if plan == "p2;*:3333" and passed:
            break
        spec = V.DEFAULT_PRECISION if plan == "default" else plan
        enc = V.VitEncoder(cfg, w, precision=spec)
        patches, img = enc.preprocess(u8, want_u8=True)
        out = enc.forward_patches(patches).clone()
        if ref is None:
            mean = torch.tensor(enc.recipe.mean, dtype=torch.float32, device="cuda")
            std = torch.tensor(enc.recipe.std, dtype=torch.float32, device="cuda")
            x = (((img.to(torch.float64) * (1 / 255)).to(torch.float32) - mean) / std).permute(0, 3, 1, 2).contiguous()
            ref = torch.cat([torch.from_numpy(CQ.forward(wt, cfg, x[i:i + 8], device="cuda")) for i in range(0, B, 8)]).cuda()
        rel = (torch.linalg.norm(out - ref, dim=1) / torch.linalg.norm(ref, dim=1)).cpu().numpy()
        ms = median_ms(lambda: enc.forward_patches(patches), reps=10, warm=2)
        inside = rel.max() <= 0.95e-3
        passed |= bool(inside)
        say(f"    {plan:52s} {rel.mean():.3e}  {rel.max():.3e}  {ms:8.2f} ms{'   (worst crop >= 5 % inside the gate)' if inside else ''}")
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
            sys.exit("perf_attention_long: no GPU (nothing here is measured without one)")
        step = argv[0]
        sys.exit(step_kernel(say) if step == "kernel" else step_forward(say) if step == "forward" else step_gate(say, step.split(":", 1)[1]))
    steps = argv or ["kernel", "forward"] + [f"gate:{m}" for m in GATE_MODELS]
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
