"""-m gpu: normals, FPFH, colour gradients, the search operands, radius-outlier masks, status words and fallback counts are, byte for
byte, what they were before csrc/reg_knn.hip was split into knn_select.h, knn_normal.h, reg_normals.hip, reg_fpfh.hip, reg_colorgrad.hip
and reg_radius.hip and the search kernels no call can launch were dropped.  Groups: tests/feature_parent_cases.py; the values of the
earlier commit: tests/golden/feature_parent_digests.json (tools/gen_golden_features_parent.py, run twice there with identical files).
The split changed no instruction of a kernel that runs and no launch, so there is no tolerance: a value that differs is a defect."""
import functools
import json

import pytest

from tests import feature_parent_cases as PC
from tests import test_gpu_features as TF

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with open(PC.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ctx():
    from ibloc_amd.registration import RegContext
    c = RegContext(2 << 30)
    yield c
    c.close()


def test_golden_is_the_case_table():
    assert {k.rsplit("/", 1)[0] for k in golden()} == {PC.group_id(g) for g in PC.GROUPS}
    assert PC.SWITCHES == TF.SWITCHES and set(PC.BATCHES) == {"all", "uniform", "clump", "sparse", "boundary"}


@pytest.mark.parametrize("group", PC.GROUPS, ids=PC.group_id)
def test_outputs_are_the_earlier_commits_bytes(ctx, group):
    want = {k: v for k, v in golden().items() if k.startswith(PC.group_id(group) + "/")}
    got = PC.run_group(ctx, group)
    assert sorted(got) == sorted(want), "the outputs of the group are not those of the golden file"
    for k in sorted(got):
        if not k.endswith(("_normals", "_fpfh", "_grad", "_norm", "_split", "/keep")):
            print(k, got[k], "earlier commit:", want[k])
    bad = sorted(k for k in got if got[k] != want[k])
    assert not bad, f"{len(bad)} of {len(got)} values differ from the earlier commit's: {bad}"
