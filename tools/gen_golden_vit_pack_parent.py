#!/usr/bin/env python3
"""CPU, run on the commit BEFORE the weight packer of ibloc_amd/vit.py became `plan_terms` / `pack_top` / `pack_layer`: the sha256 of the
descriptor, of every struct field and of the bytes behind every pointer of every case of tests/vit_pack_parent_cases.py, which
tests/test_vit_pack_parent.py holds the pure packer to.  Uses nothing the earlier commit lacks.  Run it twice: the two files must be
identical.
    python tools/gen_golden_vit_pack_parent.py OUT.json    (committed as tests/golden/vit_pack_parent_digests.json)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import vit_pack_parent_cases as PC  # noqa: E402


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
