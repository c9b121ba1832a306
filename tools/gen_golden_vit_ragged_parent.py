#!/usr/bin/env python3
"""GPU, run on the commit BEFORE the ragged forward of csrc/vit_ragged.hip was folded into csrc/vit.hip: the sha256 of the output bytes of
every case of tests/vit_ragged_parent_cases.py (forward_ragged over mixed, reversed and one-crop batches, every block count, output mode,
plan and residual-GEMM form), which tests/test_gpu_vit_ragged_parent.py holds the one staged forward to.  Uses nothing the earlier commit
lacks.  Run it twice, as tools/gen_golden_vit_parent.py: a case whose digest differs between two runs of one build is not deterministic
and has no place in the file.
    python tools/gen_golden_vit_ragged_parent.py OUT.json    (committed as tests/golden/vit_ragged_parent_digests.json)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import vit_ragged_parent_cases as PC  # noqa: E402


def main():
    out = {}
    for name in PC.GROUPS:
        got = PC.run_group(name)
        print(name, len(got), flush=True)
        out.update(got)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("cases", len(out))


if __name__ == "__main__":
    main()
