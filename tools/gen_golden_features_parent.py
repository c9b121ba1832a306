#!/usr/bin/env python3
"""GPU, run on the commit BEFORE csrc/reg_knn.hip was split into one file per consumer: the sha256 of the output bytes (and the status
words and fallback counts) of every group of tests/feature_parent_cases.py, which tests/test_gpu_features_parent.py holds the split sources
to.  Uses nothing the earlier commit lacks.  Run it twice: a value that differs between two runs of one build is a kernel that is not
deterministic and has no place in the file.
    python tools/gen_golden_features_parent.py OUT.json    (committed as tests/golden/feature_parent_digests.json)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import feature_parent_cases as PC  # noqa: E402


def main():
    from ibloc_amd.registration import RegContext
    ctx = RegContext(2 << 30)
    out = {}
    for g in PC.GROUPS:
        got = PC.run_group(ctx, g)
        print(PC.group_id(g), len(got), flush=True)
        out.update(got)
    ctx.close()
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("values", len(out))


if __name__ == "__main__":
    main()
