"""CPU: the encoder constructors hand the library, byte for byte, what they handed it before the weight packer of ibloc_amd/vit.py became
`plan_terms` / `pack_top` / `pack_layer`: the descriptor, every struct field, the bytes behind every pointer, and null where there was
null.  Cases: tests/vit_pack_parent_cases.py; the digests of the earlier commit: tests/golden/vit_pack_parent_digests.json
(tools/gen_golden_vit_pack_parent.py, run twice there with identical files).  The constructors launch nothing, so they run with
device="cpu".  There is no tolerance: a digest that differs is a field set or left differently, whether or not a forward reads it."""
import functools
import json

import pytest

from tests import vit_pack_parent_cases as PC


@functools.lru_cache(maxsize=None)
def golden():
    with open(PC.GOLDEN) as f:
        return json.load(f)


def test_golden_is_the_case_table():
    owners = {k: [g for g in PC.GROUPS if k.startswith(g + "/")] for k in golden()}
    assert all(len(v) == 1 for v in owners.values()) and {v[0] for v in owners.values()} == set(PC.GROUPS)


@pytest.mark.parametrize("group", list(PC.GROUPS))
def test_packed_bytes_are_the_parents(group):
    want = {k: v for k, v in golden().items() if k.startswith(group + "/")}
    got = PC.run_group(group)
    assert sorted(got) == sorted(want), "the cases of the group are not the cases of the golden file"
    bad = sorted(k for k in got if got[k] != want[k])
    assert not bad, f"{len(bad)} of {len(got)} digests differ from the earlier commit's: {bad}"
