"""Case table of tests/test_gpu_vit_ragged_parent.py and tools/gen_golden_vit_ragged_parent.py: `forward_ragged` (ibl_vit_forward_ragged,
per-crop patch grids) on seeded weights and pixels, reduced to the sha256 of the output bytes.  tests/golden/vit_ragged_parent_digests.json
holds the digests of the commit before the ragged forward of csrc/vit_ragged.hip was folded into the staged forward of csrc/vit.hip: that
change adds, drops and reorders no launch and changes no operand, so anything but equality is a defect.

The models are tiny_dino (prefix 1) and tiny_dino_reg (prefix 5) of tests/vit_ragged_cases.py -- dim 128, depth 2 -- with its weight and
pixel seeds.  Batches: the mixed grids RC.GRIDS (with prefix 1: 2, 22, 22, 257, 181 and 244 rows -- the attention takes 64 queries per
workgroup, so one crop is shorter than a query block and the last block of the 257-row crop holds a single query), the same batch
reversed, and one crop at 1 x 1 (n_prefix + 1 rows, M = 1 in the class-row GEMMs).  n_blocks_run 0 (the head gathers the class rows
straight from x), 1 (the only block is class-rows-only) and 2 (an every-row block, then the class-rows block).

A group is a function that yields (case name, device tensor); `GROUPS` maps the group's name to it.  The whole output is digested:
(n, dim) class rows or (total_tokens, dim) packed rows, every byte of which the call defines.  Uses only the Python surface the earlier
commit has.  No GEMM shape here depends on the device's CU count."""
import dataclasses
import functools
import os

import torch

from ibloc_amd import vit as V
from tests import vit_ragged_cases as RC
from tests.vit_parent_cases import digest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_ragged_parent_digests.json")

MODELS = {c[0]: c for c in RC.CASES}
# name -> VitEncoder arguments.  kext0: the second weight term of o / fc2 as a launch of its own (w_o_lo / w_fc2_lo)
FORMS = {"plain": dict(precision="plain"), "default": dict(precision=None), "p2-3333": dict(precision="p2;*:3333"),
         "p2-2222-kext0": dict(precision="p2;*:2222", resid_kext=False), "fold": dict(precision=None, fold_layerscale=True)}
BATCHES = {"mixed": slice(None), "reversed": slice(None, None, -1), "one": slice(0, 1)}      # of RC.GRIDS and its pixels


@functools.lru_cache(maxsize=None)
def model(name):
    """-> (cfg, weights, [device pixels per grid of RC.GRIDS])"""
    _, cfg, w, xs = RC.build(MODELS[name])
    return cfg, w, [torch.from_numpy(x).cuda() for x in xs]


def forward(name, form, batch, k, all_tokens, final_ln):
    cfg, w, xs = model(name)
    enc = V.VitEncoder(dataclasses.replace(cfg, n_blocks_run=k, out_all_tokens=all_tokens, final_ln=final_ln), w, **FORMS[form])
    grids = list(RC.GRIDS)[BATCHES[batch]]
    return enc.forward_ragged(enc.patches_from_pixels_ragged(xs[BATCHES[batch]]), grids)


def case_id(k, all_tokens, final_ln):
    return f"{k}-{'all' if all_tokens else 'cls'}-{'ln' if final_ln else 'raw'}"


def cross_group(name):
    """the mixed batch under the default plan: every block count, output mode and final LayerNorm setting"""
    for k in (0, 1, 2):
        for all_tokens in (False, True):
            for final_ln in (True, False):
                yield case_id(k, all_tokens, final_ln), forward(name, "default", "mixed", k, all_tokens, final_ln)


def batches_group(name):
    """the reversed batch and the one-crop batch under the default plan: every block count and output mode"""
    for batch in ("reversed", "one"):
        for k in (0, 1, 2):
            for all_tokens in (False, True):
                yield f"{batch}-{case_id(k, all_tokens, True)}", forward(name, "default", batch, k, all_tokens, True)


def forms_group(name):
    """the remaining plans, the launch-per-term form and folded LayerScale on the mixed batch: two blocks, both output modes"""
    for form in FORMS:
        if form == "default":
            continue
        for all_tokens in (False, True):
            for final_ln in (True, False):
                yield f"{form}-{case_id(2, all_tokens, final_ln)}", forward(name, form, "mixed", 2, all_tokens, final_ln)


GROUPS = {f"{g}/{n}": functools.partial(fn, n) for n in MODELS for g, fn in (("cross", cross_group), ("batches", batches_group), ("forms", forms_group))}


def run_group(name):
    """-> {"<group>/<case>": sha256}"""
    out = {f"{name}/{case}": digest(t) for case, t in GROUPS[name]()}
    torch.cuda.synchronize()
    return out
