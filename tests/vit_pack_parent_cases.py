"""Case table of tests/test_vit_pack_parent.py and tools/gen_golden_vit_pack_parent.py: what the encoder constructors hand the library --
the descriptor, every field of the weight structs and the bytes behind every pointer -- reduced to sha256.  No device: the constructors
launch nothing, so they run with device="cpu".  tests/golden/vit_pack_parent_digests.json holds the digests of the commit before the weight
packer became `plan_terms` / `pack_top` / `pack_layer`: that change moved no byte, so anything but equality is a defect -- also in a field
no forward reads (a stray `*_terms`, `w_proj_x` under `plain`), which no output digest can see.

Uses only what the earlier commit has: `enc.desc`, `enc.W`, `enc._keep` (DatorHead: `.H`, ProbeHead: `.W` / `.desc`)."""
import contextlib
import ctypes
import hashlib
import os

import numpy as np

from ibloc_amd import dator as D
from ibloc_amd import siglip as SG
from ibloc_amd import vit as V
from tests import vit_stream_cases as SCS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_pack_parent_digests.json")

# (family, plan, kext, fold) of tests/vit_stream_cases.py at n_blocks_run = DEPTH, all tokens and (with a class token) the class rows
STREAM = [(f, p, True, False) for f in SCS.FAMILIES for p in SCS.PLANS] + SCS.EXTRA
TINY = sorted(n for n in V.CONFIGS if n.startswith("tiny_"))
TINY_PLANS = ("plain", "default")


def stream_id(c):
    f, p, kext, fold = c
    return f"{f}-{p}" + ("" if kext else "-kext0") + ("-fold" if fold else "")


def stream_modes(family):
    """all_tokens values the family can run: without a class token there are no class rows to return"""
    return (True, False) if SCS.FAMILIES[family].cls_token else (True,)


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def stream_encoder(case, all_tokens):
    family, plan, kext, fold = case
    _, w, _ = SCS.inputs(family)
    with env("IBL_VIT_RESID_KEXT", "1" if kext else "0"):
        return V.VitEncoder(SCS.run_cfg(family, SCS.DEPTH, all_tokens), w, device="cpu", precision=plan, fold_layerscale=fold)


def tiny_encoder(name, plan):
    cfg = V.CONFIGS[name]
    return V.VitEncoder(cfg, V.random_weights(cfg, 41), device="cpu", precision=None if plan == "default" else plan)


def _sha(data):
    return hashlib.sha256(data).hexdigest()


def struct_fields(s, keep):
    """-> [(field, digest)] of one ctypes struct: an integer or float field by its value, a pointer by the bytes of the kept tensor that
    starts there ("null" for a null pointer; a pointer to nothing that is kept is an error)"""
    by_ptr = {t.data_ptr(): t for t in (keep.values() if isinstance(keep, dict) else keep)}
    out = []
    for name, ctype in s._fields_:
        v = getattr(s, name)
        if ctype is ctypes.c_void_p:
            out.append((name, "null" if not v else _sha(np.ascontiguousarray(by_ptr[v].numpy()).tobytes())))
        elif isinstance(v, ctypes.Array):
            continue                                    # VitWeights.layers: walked by the caller
        else:
            out.append((name, repr(v)))
    return out


def _join(fields):
    return _sha("\n".join(f"{n}={d}" for n, d in fields).encode())


def encoder_digests(enc):
    """-> {"desc", "top", "l0" .. "l<depth-1>", "rest"}: the descriptor's bytes, the fields of `enc.W` outside the layers, each layer
    the configuration has, and the layers it has not (which must stay as ctypes zeroes them)"""
    out = {"desc": _sha(bytes(enc.desc)), "top": _join(struct_fields(enc.W, enc._keep))}
    for l in range(enc.cfg.depth):
        out[f"l{l}"] = _join(struct_fields(enc.W.layers[l], enc._keep))
    out["rest"] = _join([(f"{l}.{n}", d) for l in range(enc.cfg.depth, V.MAX_LAYERS) for n, d in struct_fields(enc.W.layers[l], enc._keep)])
    return out


def stream_group(case):
    out = {}
    for all_tokens in stream_modes(case[0]):
        for k, d in encoder_digests(stream_encoder(case, all_tokens)).items():
            out[f"{'all' if all_tokens else 'cls'}/{k}"] = d
    return out


def tiny_group(name):
    return {f"{plan}/{k}": d for plan in TINY_PLANS for k, d in encoder_digests(tiny_encoder(name, plan)).items()}


def dator_head_group():
    head = D.DatorHead(D.random_head_weights(51), device="cpu")
    return dict(struct_fields(head.H, head._keep))


def probe_head_group():
    cfg = V.CONFIGS["tiny_siglip"]
    head = SG.ProbeHead(cfg, SG.random_head_weights(cfg, 52), device="cpu")
    return {"desc": _sha(bytes(head.desc)), **dict(struct_fields(head.W, head._keep))}


GROUPS = {f"stream/{stream_id(c)}": (lambda c=c: stream_group(c)) for c in STREAM}
GROUPS.update({f"tiny/{n}": (lambda n=n: tiny_group(n)) for n in TINY})
GROUPS.update({"dator_head": dator_head_group, "probe_head": probe_head_group})


def run_group(name):
    """-> {"<group>/<case>": sha256}"""
    return {f"{name}/{k}": d for k, d in GROUPS[name]().items()}
