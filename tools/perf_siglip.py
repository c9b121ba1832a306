#!/usr/bin/env python3
"""GPU: the SigLIP encoders -- which operand-term plan each configuration needs, and what the attention-pooling head costs.

    python tools/perf_siglip.py [--out FILE] [step ...]

steps (default: all, each in a child process of its own under a time limit; the first failure ends the run):
    head            siglip_b16_224, 224 crops, median of 20 (device events, after a warm-up): the trunk forward, the whole head
                    (ibl_probe_head_forward) and the pooling kernel alone (ibl_probe_pool_f32), and the head at batch 7 (one workgroup per
                    crop: 7 of the 256 CUs work in the pooling kernel)
    gate:<model>    embedding rel-L2 per crop against the fp32 restatement on the device over the ladder of operand-term plans
                     on the crops of tests/test_gpu_siglip.py's gate: plan, mean, max, forward time of the gate's batch"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GATE = {"siglip_b16_224": (896, 224), "siglip_b16_256": (224, 224), "siglip_l16_256": (224, 224), "siglip_b16_384": (32, 32),
        "siglip_l16_384": (32, 32)}          # model -> (crops, batch)
LADDER = ("plain", "default", "p2;0:3232;1:2222;2:2211", "p2;0:3232;1:2222;2:2222;3:2211", "p2;0:3232;1:2222;2:2222;3:2222;4:2211",
          "p2;0:3232;1:2222;2:2222;3:2222;4:2222;5:2222;6:2211", "p2;*:2222;0:3232", "p2;*:3333")
LIMITS = {"head": 240, "gate": 420}


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


_WEIGHTS = {}


def _encoder(name, plan=None):
    """the gate's seeded weights (generated once per model) under `plan`"""
    from ibloc_amd import siglip as S
    from ibloc_amd import vit as V
    from tests import siglip_cases as SC
    cfg = V.CONFIGS[name]
    if name not in _WEIGHTS:
        w = V.random_weights(cfg, SC.GATE_WEIGHT_SEED)
        del w["cls"]
        _WEIGHTS[name] = (w, S.random_head_weights(cfg, SC.GATE_HEAD_SEED))
    w, hw = _WEIGHTS[name]
    return cfg, w, hw, S.SiglipEncoder(cfg, w, hw, precision=None if plan == "default" else plan)


def step_head(say):
    import torch
    from ibloc_amd import siglip as S
    cfg, w, hw, enc = _encoder("siglip_b16_224")
    gen = torch.Generator(device="cuda").manual_seed(7)
    say(f"siglip_b16_224 (plan {enc.precision}), median of 20, ms")
    for batch in (224, 7):
        patches = torch.randn((batch * cfg.n_patches, cfg.patch_k_pad), device="cuda", generator=gen).to(torch.float16)
        tokens = enc.trunk.forward_patches(patches)
        trunk = median_ms(lambda: enc.trunk.forward_patches(patches))
        head = median_ms(lambda: enc.head.forward(tokens))
        pooled = torch.empty((batch, cfg.heads, cfg.dim), dtype=torch.float32, device="cuda")
        pool = median_ms(lambda: S.probe_pool(tokens, enc.head.u, want_probs=False, pooled=pooled))
        both = median_ms(lambda: enc.forward_patches(patches))
        say(f"  batch {batch:3d}: trunk forward {trunk:8.3f}   head {head:7.3f} ({100 * head / (trunk + head):.2f} % of trunk + head)   "
            f"pooling kernel alone {pool:7.3f}   trunk + head in one call {both:8.3f}")
    return 0


def step_gate(say, name):
    import torch
    from tests import siglip_cases as SC
    from tests.test_gpu_flip_rate import GpuCrops
    from tests.test_gpu_siglip import _embed_both
    n_crops, batch = GATE[name]
    ids = np.random.default_rng(3).integers(0, 100000, size=n_crops)
    crops = GpuCrops(21).variants(ids)
    say(f"[gate {name}] {n_crops} crops, batch {batch}: plan, mean, max, forward of {batch} crops (ms)")
    ora = None
    for plan in LADDER:
        cfg, w, hw, enc = _encoder(name, plan)
        if ora is None:
            wt = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).cuda() for k, v in w.items()}
            hwt = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).cuda() for k, v in hw.items()}
            hip, ora = _embed_both(enc, wt, hwt, cfg, crops, batch)
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


def main():
    args = sys.argv[1:]
    out = None
    if args[:1] == ["--out"]:
        out, args = args[1], args[2:]
    if args[:1] == ["--child"]:
        import torch
        assert torch.cuda.is_available(), "perf_siglip.py needs a GPU"
        step = args[1]
        f = open(out, "a") if out else None

        def say(s):
            print(s, flush=True)
            if f:
                f.write(s + "\n")
                f.flush()
        return step_head(say) if step == "head" else step_gate(say, step.split(":", 1)[1])
    steps = args or ["head"] + [f"gate:{m}" for m in GATE]
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
