"""Case table of tests/test_gpu_features_parent.py and tools/gen_golden_features_parent.py: the neighbourhood kernels and their consumers
through the public calls, on the clouds of tests/feature_cases.py, reduced to the sha256 of the output bytes.
tests/golden/feature_parent_digests.json holds the digests of the commit before csrc/reg_knn.hip was split into knn_select.h,
knn_normal.h, reg_normals.hip, reg_fpfh.hip, reg_colorgrad.hip and reg_radius.hip and before the search kernels that no call can launch
were dropped: neither changed an instruction of a kernel that runs or a launch, so anything but equality is a defect.

A group is (batch, switch): the batch `all` is every cloud of feature_cases.CASES as ONE batch, the other four are the path clouds
(staged tile, tile that cannot stage, sparse-spot fallback, boundary-bin slow path) each ALONE; the switches are the SWITCHES of
tests/test_gpu_features.py.  Per group: normals and FPFH of normals_fpfh_batch; normals, FPFH in resident order, gradients, the centred
norms and the fp16 operand rows of instance_features_batch; the radius-outlier mask; the status word.  For the clouds alone also the
`fallback=` counts of the `[knn]` lines under knn_debug=1, as integers in call order.  Uses only the Python surface the earlier commit
has."""
import hashlib
import os
import tempfile

import numpy as np
import torch

from tests import feature_cases as fc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_parent_digests.json")

SWITCHES = {"default": {}, "knn_noguess": dict(knn_noguess=1), "feat_unfused": dict(feat_unfused=1), "spfh_f64": dict(spfh_f64=1),
            "spfh_qcap": dict(spfh_qcap=8)}          # (tests/test_gpu_features.py SWITCHES: its parent test asserts they are equal)
ALONE = ("uniform", "clump", "sparse", "boundary")
BATCHES = {"all": lambda: [f() for f in fc.CASES.values()]}
BATCHES.update({name: (lambda name=name: [fc.CASES[name]()]) for name in ALONE})
GROUPS = [(b, s) for b in BATCHES for s in SWITCHES]


def group_id(g):
    return f"{g[0]}-{g[1]}"


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


class stderr_text:
    """the bytes written to file descriptor 2 inside the block (launch_knn prints its `[knn]` lines from C) -> .text"""
    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def run_group(ctx, g):
    """-> {"<batch>-<switch>/<output>": sha256 or integer(s)}"""
    from ibloc_amd.registration import CloudBatch, instance_features_batch, normals_fpfh_batch, radius_outlier_batch
    batch, switch = g
    cases = BATCHES[batch]()
    b = CloudBatch.from_numpy([c["pts"] for c in cases], [c["intensity"] for c in cases])
    n = b.n
    ctx.status(clear=True)
    alone = batch != "all"
    with stderr_text() as err:
        with ctx.diag(**SWITCHES[switch], **(dict(knn_debug=1) if alone else {})):
            nrm, fpfh = normals_fpfh_batch(ctx, b, fc.NORMAL[0], fc.NORMAL[1], fc.FEATURE[0], fc.FEATURE[1])
            feat = instance_features_batch(ctx, b, fc.VOXEL, grad_radius=fc.GRAD[0])
            keep = radius_outlier_batch(ctx, b, *fc.OUTLIER)
        torch.cuda.synchronize()
    out = {"a_normals": digest(nrm), "a_fpfh": digest(fpfh), "b_normals": digest(feat.normals[:n]), "b_fpfh": digest(feat.fpfh[:n]),
           "b_grad": digest(feat.grad[:n]), "b_fpfh_norm": digest(feat.fpfh_norm[:n]), "b_fpfh_split": digest(feat.fpfh_split[:n]),
           "keep": digest(keep[:n]), "status": int(ctx.status(clear=True))}
    if alone:
        out["fallback"] = [r["fallback"] for r in fc.parse_knn_debug(err.text)]
    return {f"{group_id(g)}/{k}": v for k, v in out.items()}
