"""-m gpu: `forward_ragged` gives, byte for byte, what it gave when the ragged forward was a second copy of the staged forward in
csrc/vit_ragged.hip.  Cases: tests/vit_ragged_parent_cases.py; the digests of the earlier commit:
tests/golden/vit_ragged_parent_digests.json (tools/gen_golden_vit_ragged_parent.py, run twice there with identical files).  Folding the
two forwards into one added, dropped and reordered no launch and changed no operand, so there is no tolerance: a digest that differs is
a defect."""
import functools
import json

import pytest

from tests import vit_ragged_parent_cases as PC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with open(PC.GOLDEN) as f:
        return json.load(f)


def test_golden_is_the_case_table():
    assert {k.rsplit("/", 1)[0] for k in golden()} == set(PC.GROUPS)


@pytest.mark.parametrize("group", list(PC.GROUPS))
def test_forward_ragged(group):
    """cross: block counts x output modes x final LayerNorm on the mixed batch; batches: the reversed and the one-crop batch; forms: plain,
    p2;*:3333, the launch-per-term form of o / fc2 and folded LayerScale at two blocks"""
    want = {k: v for k, v in golden().items() if k.startswith(group + "/")}
    got = PC.run_group(group)
    assert sorted(got) == sorted(want), "the cases of the group are not the cases of the golden file"
    bad = sorted(k for k in got if got[k] != want[k])
    assert not bad, f"{len(bad)} of {len(got)} outputs differ from the earlier commit's bytes: {bad}"
